"""Cases, inputs and the fp64 reference of the conv-attention operator tests (tests/test_conv_attn_cpu.py checks the
reference's own preconditions without a GPU, tests/test_conv_attn_gpu.py holds the kernels against it).

Reference: the fp64 restatement of CrossAttention.forward's attention (attention.py:197-243) on the bf16-rounded operands,
with oracle.ldm_oracle.conv_attn_rows (replace_rows_by_conv_attn, ldm/util.py:701-879) applied per subject string to the
original scores.  `conv_columns` is a second, index-level statement of the same replacement that can also be MUTATED
(taps and shifts transposed, shift sign flipped): the CPU test demands that every case tells the reference from plain
attention and from each mutant by >= 10 bars, so a kernel that ignored or mis-shifted the subject columns cannot pass.
"""
from __future__ import annotations

from functools import lru_cache

import torch

from oracle import ldm_oracle as O

BF16_BAR = 1.5e-2    # max-abs / max|ref| of a bf16 attention operator (tests/test_ops_gpu.py TOL["bf16"])
F32_BAR = 2e-4       # the f32 mode's bar

# (B, Hh, Ww, S, heads, dh, ks, groups): what each is the smallest instance of
ONE_PASS_CASES = [
    (2, 8, 8, 77, 8, 40, 3, 1),     # the workload's key count; subject rows 68..76 inside the last key block
    (1, 6, 10, 70, 8, 40, 3, 1),    # non-square map; N = 60 (partial query block); subject rows 61..69 straddle key row 64
    (2, 8, 8, 77, 8, 80, 2, 2),     # ks = 2 (asymmetric pad 0 / 1); two subject strings
    (1, 5, 7, 96, 5, 80, 4, 2),     # ks = 4; 32 subject rows from key block 2 on; full 96 keys; 5 heads (partial head group); N = 35
    (1, 3, 3, 17, 4, 40, 4, 1),     # a map smaller than the shifts (every column hits the zero fill); one ordinary key
    (2, 16, 16, 77, 8, 40, 3, 3),   # three strings; eight query blocks, so the three-deep Q ring wraps
    (1, 4, 40, 33, 8, 80, 3, 1),    # Ww > 32: vertical neighbours live in other query blocks; subject rows 24..32 straddle key row 32
]
MERGE_ONLY_CASE_DH160 = (2, 8, 8, 77, 8, 160, 3, 1)   # no one-pass kernel at dh 160: flash + subj_scores + merge
MERGE_ONLY_CASE_F32 = (2, 8, 8, 77, 8, 40, 3, 1)      # the f32 mode runs the merge path


def case_id(case):
    return "B{}_{}x{}_S{}_h{}x{}_ks{}_g{}".format(*case)


def _bf16(t):
    return t.to(torch.bfloat16).float()


@lru_cache(maxsize=None)
def inputs(case):
    """q [B, N, C], k / v [B, S, C] (fp32 holding bf16 values) and token_idx (groups x ks^2 key positions, reference order)."""
    B, Hh, Ww, S, heads, dh, ks, groups = case
    g = torch.Generator().manual_seed(1000 * ks + S + dh + Hh)
    N, C, nt = Hh * Ww, heads * dh, ks * ks
    q = torch.randn(B, N, C, generator=g)
    k = torch.randn(B, S, C, generator=g)
    v = torch.randn(B, S, C, generator=g) * 1.5 + 0.2
    pos = torch.randperm(S, generator=g)[:groups * nt].tolist()
    token_idx = tuple(tuple(pos[i * nt:(i + 1) * nt]) for i in range(groups))
    k[:, pos] *= 2
    v[:, pos] *= 2
    return _bf16(q), _bf16(k), _bf16(v), token_idx


def _split(t, heads):
    B, n, C = t.shape
    return t.reshape(B, n, heads, C // heads).permute(0, 2, 1, 3).double()


def _shifted(m, dy, dx):
    """out(y, x) = m(y - dy, x - dx), zero outside the map (last two dims)."""
    Hh, Ww = m.shape[-2:]
    out = torch.zeros_like(m)
    ys, xs = slice(max(dy, 0), Hh + min(dy, 0)), slice(max(dx, 0), Ww + min(dx, 0))
    yr, xr = slice(max(-dy, 0), Hh + min(-dy, 0)), slice(max(-dx, 0), Ww + min(-dx, 0))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[..., ys, xs] = m[..., yr, xr]
    return out


def conv_columns(qh, kh, toks, hw, ks, scale, transpose=False, flip=False):
    """The ks^2 replacement columns [B, H, N, ks^2] of one subject string, stated on indices: A(y, x) = scale / ks^1.5 *
    sum_t q(y + ty - p0, x + tx - p0) . k[tok_t], column j = A shifted by (jy - p0, jx - p0).  transpose: taps and shifts
    with y / x swapped; flip: the shifts negated (the two mutants a wrong kernel would most plausibly compute)."""
    Hh, Ww = hw
    B, H, N, dh = qh.shape
    p0 = 0 if ks == 2 else 1
    A = torch.zeros(B, H, Hh, Ww, dtype=qh.dtype)
    for t in range(ks * ks):
        oy, ox = t // ks - p0, t % ks - p0
        if transpose:
            oy, ox = ox, oy
        qk = torch.einsum("bhnd,bhd->bhn", qh, kh[:, :, toks[t]]).reshape(B, H, Hh, Ww)
        A += _shifted(qk, -oy, -ox)
    A *= scale / ks ** 1.5
    cols = []
    for j in range(ks * ks):
        dy, dx = j // ks - p0, j % ks - p0
        if transpose:
            dy, dx = dx, dy
        if flip:
            dy, dx = -dy, -dx
        cols.append(_shifted(A, dy, dx).reshape(B, H, N))
    return torch.stack(cols, dim=-1)


def _finish(sim, vh):
    B, H, N, _ = sim.shape
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), vh)
    return out.permute(0, 2, 1, 3).reshape(B, N, -1)


@lru_cache(maxsize=None)
def reference(case):
    """fp64 attention output [B, N, C] with the oracle's conv_attn_rows per subject string."""
    B, Hh, Ww, S, heads, dh, ks, groups = case
    q, k, v, token_idx = inputs(case)
    qh, kh, vh = _split(q, heads), _split(k, heads), _split(v, heads)
    scale = dh ** -0.5
    sim = torch.einsum("bhid,bhjd->bhij", qh, kh) * scale
    for toks in token_idx:
        subj = (torch.arange(B).repeat_interleave(ks * ks), torch.tensor(toks).repeat(B))
        sim = O.conv_attn_rows(sim, qh, kh, subj, (Hh, Ww), ks, scale)
    return _finish(sim, vh)


def variant(case, kind):
    """fp64 output of "plain" attention (no replacement) or of conv attention through conv_columns: "exact" (must equal
    `reference`), "transposed", "flipped"."""
    B, Hh, Ww, S, heads, dh, ks, groups = case
    q, k, v, token_idx = inputs(case)
    qh, kh, vh = _split(q, heads), _split(k, heads), _split(v, heads)
    scale = dh ** -0.5
    sim = torch.einsum("bhid,bhjd->bhij", qh, kh) * scale
    if kind != "plain":
        for toks in token_idx:
            sim[..., list(toks)] = conv_columns(qh, kh, toks, (Hh, Ww), ks, scale, transpose=kind == "transposed",
                                                flip=kind == "flipped")
    return _finish(sim, vh)
