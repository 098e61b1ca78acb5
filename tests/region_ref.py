"""Reference restatement of regional prompts (attention couple; adaface_amd/regions.py) for the tests: the operator
in float64, and a context manager under which the oracle's cross-attention follows the one definition every layer shares:

    a_r(p) = mean of m_r over the f x f box of p;  s(p) = sum_r a_r(p);  w_r(p) = a_r(p) / s(p) where s(p) > 0, else (1, 0, ..);
    o(p)   = sum over {r : w_r(p) > 0} of w_r(p) softmax(q_p K_r^T dh^-1/2) V_r        (regions with w_r = 0 selected out)
"""
import contextlib
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from adaface_amd import regions as RG  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402


def region_attention(q, k, v, w, heads, R, scale=None):
    """float64: q [B, Nq, C], k / v [B, R T, C], w [B, R, Nq] (normalised) -> o [B, Nq, C]; w_r = 0 selects region r out."""
    q, k, v, w = q.double(), k.double(), v.double(), w.double()
    B, Nq, C = q.shape
    dh = C // heads
    T = k.shape[1] // R
    scale = dh ** -0.5 if scale is None else scale
    split = lambda t: t.reshape(B, -1, heads, dh).permute(0, 2, 1, 3)
    qh = split(q)
    out = torch.zeros(B, Nq, C, dtype=torch.float64)
    for r in range(R):
        kh, vh = split(k[:, r * T:(r + 1) * T]), split(v[:, r * T:(r + 1) * T])
        sim = torch.einsum("bhid,bhjd->bhij", qh, kh) * scale
        o = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), vh).permute(0, 2, 1, 3).reshape(B, Nq, C)
        wr = w[:, r, :, None]
        out = out + torch.where(wr > 0, wr * o, torch.zeros_like(o))
    return out


@contextlib.contextmanager
def patched(m, R, hw):
    """While active, O.cross_attention follows the definition above for every call that carries a context: m [Bf, R, H, W] the
    weight map of the Bf samples of the forward, hw = (H, W) the latent size; a site with N positions uses f = sqrt(H W / N).
    Self-attention and everything else is the oracle's own arithmetic."""
    pyr = RG.pyramid(m)
    H, W = hw

    def cross_attention(sd, p, x, k_ctx, v_ctx, heads, conv_attn=None):
        if k_ctx is None:
            return original(sd, p, x, k_ctx, v_ctx, heads, conv_attn=conv_attn)
        assert conv_attn is None or conv_attn[2] <= 1, "regions do not combine with conv attention"
        q, k, v = O._lin(sd, p + ".to_q", x), O._lin(sd, p + ".to_k", k_ctx), O._lin(sd, p + ".to_v", v_ctx)
        B, N, C = q.shape
        f = int(round(math.sqrt(H * W / N)))
        lvl = {1: 0, 2: 1, 4: 2, 8: 3}[f]
        w = pyr[lvl].reshape(pyr[lvl].shape[0], R, -1)
        assert w.shape[0] == B and w.shape[2] == N and k.shape[1] % R == 0, (tuple(w.shape), B, N, tuple(k.shape))
        T = k.shape[1] // R
        dh = C // heads
        split = lambda t: t.reshape(B, -1, heads, dh).permute(0, 2, 1, 3)
        qh = split(q)
        out = torch.zeros_like(q)
        for r in range(R):
            kh, vh = split(k[:, r * T:(r + 1) * T]), split(v[:, r * T:(r + 1) * T])
            sim = torch.einsum("bhid,bhjd->bhij", qh, kh) * dh ** -0.5
            o = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), vh).permute(0, 2, 1, 3).reshape(B, N, C)
            wr = w[:, r, :, None].to(o.dtype)
            out = out + torch.where(wr > 0, wr * o, torch.zeros_like(o))
        return O._lin(sd, p + ".to_out.0", out)

    original = O.cross_attention
    O.cross_attention = cross_attention
    try:
        yield
    finally:
        O.cross_attention = original
