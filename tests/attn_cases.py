"""Attention: the hand-written plan table, the fp64 reference with its log-sum-exp, the derived lse bar and the case tables of
tests/test_attn_forms_gpu.py.  A plain helper without fixtures; tests/test_attn_plan_cpu.py checks all of it on the CPU.

The forms are those of Runner::attn_params (csrc/af_model.hip): F1 q | k | v as columns of one [B][N][3C] buffer, F2 k | v as
columns of the cached context [B][S][2C], F3 = F2 with the subject strings' keys dropped and an lse output, F4 = F1 with the
causal mask, F5 a window of the batch.  ops.attention states them through layout / ld_slack / lse / batch_window / drop_keys.
"""
import math
from collections import namedtuple

import torch

LOG2E = 1.0 / math.log(2.0)
SMAX = 96                                    # xs::SMAX: the short-key kernel's key limit
DH_LIST = (8, 16, 32, 40, 64, 80, 128, 160)  # head dims with an instantiation
KNOB_DEFAULT = {"attn_ring": 3, "attn_short": 1}


# ======================================================================================================================
# 1. the plan, written out by hand: (why, knobs, dtype, dh, Nk, ldq, ldk, ldv, ldo, causal, lse, pack) -> kernel
# ======================================================================================================================
PlanRow = namedtuple("PlanRow", "why knobs dtype dh Nk ldq ldk ldv ldo causal lse pack kernel")


def _row(why, kernel, dtype="bf16", dh=40, Nk=77, ld=None, ldk=None, ldv=None, ldo=None, causal=False, lse=False, pack=False,
         ring=3, short=1):
    ld = 8 * dh if ld is None else ld
    ldk = ld if ldk is None else ldk
    return PlanRow(why, {"attn_ring": ring, "attn_short": short}, dtype, dh, Nk, ld, ldk, ldk if ldv is None else ldv,
                   ld if ldo is None else ldo, causal, lse, pack, kernel)


PLAN_ROWS = [
    # ---- the short-key kernel: bf16, pack, knob, no mask, no lse, <= 96 keys, dh 40 / 80
    _row("short: 96 keys, the last count it takes", "short", Nk=96, pack=True),
    _row("short: 97 keys fall to the ring kernel", "ring40", Nk=97, pack=True),
    _row("short dh 80", "short", dh=80, Nk=77, pack=True),
    _row("short dh 80: 97 keys, below the ring threshold: flash", "flash", dh=80, Nk=97, pack=True),
    _row("short: the context's pitch 2C", "short", Nk=77, ld=320, ldk=640, pack=True),
    _row("no pack, no short kernel", "ring40", Nk=77, pack=False),
    _row("knob attn_short off", "ring40", Nk=77, pack=True, short=0),
    _row("knob attn_short off, dh 80", "flash", dh=80, Nk=77, pack=True, short=0),
    _row("causal turns short off (and the ring kernel: it has no mask)", "w4", Nk=77, pack=True, causal=True),
    _row("lse turns short off", "ring40", Nk=68, pack=True, lse=True),
    _row("lse turns short off, dh 80", "flash", dh=80, Nk=68, pack=True, lse=True),
    _row("short: f32 has none", "flash", dtype="f32", Nk=77, pack=True),
    _row("short: fp16 has none", "flash", dtype="f16", Nk=77, pack=True),
    _row("short: dh 160 has none", "flash", dh=160, Nk=77, pack=True),
    _row("short: dh 64 has none", "flash", dh=64, Nk=77, pack=True),
    # ---- ring40: bf16 dh 40, attn_ring bit 0, not causal; else the 128-VGPR build of the flash kernel
    _row("ring40, bits 0 and 1", "ring40", Nk=4096),
    _row("ring40, bit 0 alone", "ring40", Nk=4096, ring=1),
    _row("ring40 with lse", "ring40", Nk=68, lse=True),
    _row("bit 0 off: w4", "w4", Nk=4096, ring=2),
    _row("bit 0 off (bits 1 and 2 on): w4", "w4", Nk=4096, ring=6),
    _row("all bits off: w4", "w4", Nk=300, ring=0),
    _row("causal with the ring knob on: w4", "w4", Nk=200, ring=7, causal=True),
    _row("dh 40 on f32: flash", "flash", dtype="f32", Nk=4096),
    _row("dh 40 on fp16: flash (no w4 build)", "flash", dtype="f16", Nk=4096),
    _row("dh 40 on fp16, ring knob off: flash", "flash", dtype="f16", Nk=4096, ring=0),
    # ---- ring80: bf16 dh 80, bit 1, not causal, >= 256 keys or bit 2
    _row("ring80: 256 keys, the first count it takes", "ring80", dh=80, Nk=256),
    _row("ring80: 255 keys stay on flash", "flash", dh=80, Nk=255),
    _row("ring80: bit 2 takes any key count", "ring80", dh=80, Nk=255, ring=7),
    _row("ring80: bit 2 takes one key", "ring80", dh=80, Nk=1, ring=6),
    _row("ring80: bit 1 off", "flash", dh=80, Nk=1024, ring=1),
    _row("ring80: bit 1 off, bit 2 alone does nothing", "flash", dh=80, Nk=1024, ring=5),
    _row("ring80: bit 0 plays no part", "ring80", dh=80, Nk=1024, ring=2),
    _row("ring80: causal stays on flash", "flash", dh=80, Nk=1024, ring=7, causal=True),
    _row("ring80 with lse", "ring80", dh=80, Nk=300, lse=True),
    _row("dh 80 on f32", "flash", dtype="f32", dh=80, Nk=1024, ring=7),
    _row("dh 80 on fp16", "flash", dtype="f16", dh=80, Nk=1024, ring=7),
    # ---- flash: the rest
    _row("the CLIP tower: dh 64 causal", "flash", dh=64, Nk=77, ld=2304, ldo=768, causal=True),
    _row("the tiny tower: dh 16 causal, f32", "flash", dtype="f32", dh=16, Nk=77, ld=192, ldo=64, causal=True),
    _row("dh 160 self-attention, the qkv pitch", "flash", dh=160, Nk=64, ld=3840, ldo=1280),
    _row("dh 8", "flash", dh=8, Nk=16), _row("dh 32", "flash", dh=32, Nk=50), _row("dh 128", "flash", dh=128, Nk=77),
    # ---- refusals
    _row("a head dim without an instantiation", "refused", dh=48, Nk=77),
    _row("dh 48 on f32", "refused", dtype="f32", dh=48, Nk=77),
    _row("dh 24 even with a pack", "refused", dh=24, Nk=77, pack=True),
    _row("no key", "refused", Nk=0),
    _row("bf16: ldk no multiple of 8", "refused", Nk=77, ld=320, ldk=324),
    _row("bf16: ldk % 8 on the short kernel's way", "refused", Nk=77, ld=320, ldk=644, pack=True),
    _row("fp16: ldk no multiple of 8", "refused", dtype="f16", Nk=77, ld=320, ldk=324),
    _row("f32: ldk a multiple of 4 is enough", "flash", dtype="f32", Nk=77, ld=320, ldk=324),
    _row("f32: ldk no multiple of 4", "refused", dtype="f32", Nk=77, ld=320, ldk=322),
    _row("bf16: ldq no multiple of 8", "refused", Nk=77, ld=324, ldk=320, ldo=320),
    _row("bf16: ldv no multiple of 8", "refused", Nk=77, ld=320, ldv=324),
    _row("ldo no multiple of 4", "refused", Nk=77, ld=320, ldo=322),
    _row("bf16: ldo a multiple of 4 is enough", "ring40", Nk=77, ld=320, ldo=324),
    _row("f32: ldo no multiple of 4", "refused", dtype="f32", Nk=77, ld=320, ldo=322),
]


# ======================================================================================================================
# 2. operands and the fp64 reference
# ======================================================================================================================
def round_to(t, dtype):
    return t.to(torch.bfloat16).float() if dtype == "bf16" else t.to(torch.float16).float() if dtype == "f16" else t.float()


def operands(seed, B, Nq, Nk, heads, dh, dtype):
    """Gaussian q [B, Nq, C], k, v [B, Nk, C] rounded to the storage type, seeded per case"""
    g = torch.Generator().manual_seed(seed)
    C = heads * dh
    q = round_to(torch.randn(B, Nq, C, generator=g), dtype)
    k = round_to(torch.randn(B, Nk, C, generator=g), dtype)
    v = round_to(torch.randn(B, Nk, C, generator=g) * 1.5 + 0.2, dtype)
    return q, k, v


def _heads(t, heads):
    B, N, C = t.shape
    return t.view(B, N, heads, C // heads).transpose(1, 2)


def scores64(q, k, heads, scale):
    """scale * q_i . k_j in fp64, [B, H, Nq, Nk]"""
    return torch.einsum("bhid,bhjd->bhij", _heads(q.double(), heads), _heads(k.double(), heads)) * scale


def ref_attention(q, k, v, heads, scale=None, causal=False, mask=None):
    """(O [B, Nq, C], lse2 [B, H, Nq]) in fp64.  lse2 = logsumexp_j(scale q_i . k_j) / ln 2, the log2 domain AttnParams::lse
    holds.  causal: key j is masked iff j > i.  mask (the CPU test's wrong variants): "ge" masks j >= i instead."""
    B, Nq, C = q.shape
    scale = (C // heads) ** -0.5 if scale is None else scale
    s = scores64(q, k, heads, scale)
    if causal or mask:
        i = torch.arange(Nq).view(-1, 1)
        j = torch.arange(k.shape[1]).view(1, -1)
        s = s.masked_fill((j >= i) if mask == "ge" else (j > i), -math.inf)
    o = torch.einsum("bhij,bhjd->bhid", torch.softmax(s, dim=-1), _heads(v.double(), heads))
    return o.transpose(1, 2).reshape(B, Nq, C), torch.logsumexp(s, dim=-1) * LOG2E


# ======================================================================================================================
# 3. the lse bar, derived (never read off a kernel's output)
# ======================================================================================================================
P_UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}     # rounding unit (half an ulp, relative) of the storage type


def prescaled_q(kernel):
    """ring40 and w4 round q * scale * log2 e to bf16 before the QK^T MFMA (the softmax reference rides in a K slot)"""
    return kernel in ("ring40", "w4")


def p_unit(kernel, dtype, dh):
    """the softmax denominator is summed from P ROUNDED to the storage type where the ones column of the V tile sums it on the
    MFMA: the ring kernels always, the flash kernel on 16-bit storage when dh % 32 != 0 (AttnCfg::ONES); else fp32 P"""
    if dtype == "f32":
        return 0.0
    return P_UNIT[dtype] if kernel in ("ring40", "ring80") or dh % 32 != 0 else 0.0


def lse_bar(q, k, heads, scale, kernel, dtype, lse2):
    """E [B, H, Nq], the per-row error bound of the kernel's lse in log2 units; a test's bar is 2 * E (fp32 accumulation order
    and the hardware exp2 / log2 are not in the derivation).
      max_j delta_ij   delta_ij = 2^-9 scale log2(e) sum_d |q_id| |k_jd|: rounding the pre-scaled Q to bf16 moves component d by
                       <= 2^-9 relative, hence score ij by <= delta_ij, and a log-sum-exp moves by at most the largest move of
                       its arguments (the bound of test_attention_spiky_bf16_dh40); 0 for kernels that keep Q as stored
      log2(1 + u)      every P rounded to the storage type moves by <= u relative, so does their sum
      2e-4 max(1, max |lse2|)   the suite's f32 bar"""
    dh = q.shape[-1] // heads
    E = torch.zeros_like(lse2)
    if prescaled_q(kernel):
        E = E + (torch.einsum("bhid,bhjd->bhij", _heads(q.double().abs(), heads), _heads(k.double().abs(), heads))
                 * (2.0 ** -9 * scale * LOG2E)).amax(-1)
    return E + math.log2(1.0 + p_unit(kernel, dtype, dh)) + 2e-4 * max(1.0, lse2.abs().max().item())


def emulate_lse(q, k, heads, scale, kernel, dtype):
    """The kernels' roundings on the CPU, fp32 sums: the pre-scaled Q rounded to bf16 (ring40, w4), scores in fp32, P = exp2(s -
    row maximum) rounded to the storage type where the denominator is summed from rounded P, lse = maximum + log2(sum)."""
    dh = q.shape[-1] // heads
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    qh, kh = _heads(q.float(), heads), _heads(k.float(), heads)
    if prescaled_q(kernel):
        s = torch.einsum("bhid,bhjd->bhij", round_to(qh * sl2, "bf16"), kh)
    else:
        s = torch.einsum("bhid,bhjd->bhij", qh, kh) * sl2
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    if p_unit(kernel, dtype, dh):
        p = round_to(p, dtype)
    return (m.squeeze(-1) + torch.log2(p.sum(-1))).double()


def wrong_lse(q, k, heads, scale, lse2):
    """three plausible mistakes: the natural-log domain, log2(l) without the running reference, unscaled scores"""
    s = scores64(q, k, heads, scale) * LOG2E
    return {"natural log": lse2 / LOG2E,
            "no running reference": lse2 - s.amax(-1),
            "unscaled scores": torch.logsumexp(scores64(q, k, heads, 1.0), dim=-1) * LOG2E}


# ======================================================================================================================
# 4. the GPU cases (tests/test_attn_forms_gpu.py)
# ======================================================================================================================
Case = namedtuple("Case", "kernel dtype B Nq Nk heads dh knobs note")


def _case(kernel, dtype, B, Nq, Nk, heads, dh, ring=3, short=1, note=""):
    return Case(kernel, dtype, B, Nq, Nk, heads, dh, (("attn_ring", ring), ("attn_short", short)), note)   # (hashable: cache keys)


def case_id(c):
    tag = "-".join(f"{k.split('_')[1]}{v}" for k, v in c.knobs if v != KNOB_DEFAULT[k])
    return f"{c.kernel}-{c.dtype}-B{c.B}-N{c.Nq}-S{c.Nk}-h{c.heads}-d{c.dh}" + (f"-{tag}" if tag else "")


# F1: q | k | v columns of one buffer.  (attn_short is off wherever the DENSE twin of a case, which gets a V^T pack, would
# otherwise take the short-key kernel: the twin has to run the kernel under test.)
F1 = [
    _case("ring40", "bf16", 2, 300, 300, 8, 40, note="H * B % 8 == 0: the XCD remap of ring_coords"),
    _case("ring40", "bf16", 3, 70, 70, 2, 40, short=0, note="H * B % 8 != 0: the plain mapping"),
    _case("w4", "bf16", 2, 300, 300, 8, 40, ring=0),
    _case("ring80", "bf16", 1, 320, 320, 4, 80, note="by its own threshold"),
    _case("ring80", "bf16", 2, 130, 130, 8, 80, ring=7),
    _case("flash", "bf16", 1, 70, 70, 2, 160),
    _case("flash", "f32", 2, 130, 130, 8, 40),
    _case("flash", "f32", 1, 70, 70, 2, 160),
    _case("flash", "f16", 2, 130, 130, 8, 40),
    _case("flash", "f16", 2, 130, 130, 8, 80),
]
# F2: k | v columns of the cached context, S = 77
F2 = [
    _case("short", "bf16", 2, 100, 77, 8, 40),
    _case("short", "bf16", 1, 33, 77, 8, 80),
    _case("short", "bf16", 2, 96, 77, 5, 40, note="the partial head group"),
    _case("ring40", "bf16", 2, 100, 77, 8, 40, short=0),
    _case("w4", "bf16", 2, 100, 77, 8, 40, ring=0, short=0),
    _case("flash", "bf16", 1, 100, 77, 8, 80, short=0),
    _case("flash", "f32", 1, 70, 77, 2, 160),
    _case("flash", "f16", 1, 100, 77, 8, 40),
]
# F3: lse on the context form, S = 77 less one or two ks = 3 subject strings.  (attn_short off: the call WITHOUT lse that O is
# compared with gets a V^T pack and must stay on the same kernel.)
F3 = [
    _case("ring40", "bf16", 2, 100, 77, 8, 40, short=0),
    _case("w4", "bf16", 2, 100, 77, 8, 40, ring=0, short=0),
    _case("flash", "bf16", 2, 100, 77, 8, 80, short=0),
    _case("flash", "bf16", 2, 100, 77, 2, 160),
    _case("flash", "f32", 2, 100, 77, 8, 40),
    _case("flash", "f16", 2, 100, 77, 8, 40),
]
F3_DROP = (9, 18)
# F4: the causal mask on the qkv form
F4 = (
    [_case("flash", dt, 2, 77, 77, 12, 64, note="the tower's own form") for dt in ("f32", "bf16", "f16")]
    + [_case("flash", dt, 2, 77, 77, 4, 16, note="the tiny tower's") for dt in ("f32", "bf16", "f16")]
    + [_case("flash", dt, 1, 300, 300, 2, 64, note="three workgroups per head") for dt in ("f32", "bf16")]
    + [_case("w4", "bf16", 1, 200, 200, 2, 40, ring=7, note="the ring knob is on: the plan must say w4")]
)
# F5: a window of the batch: (case, layout, B, (b0, nb))
F5 = [(c, layout, B, win)
      for c, layout in ((_case("ring40", "bf16", 0, 130, 130, 8, 40), "qkv"), (_case("short", "bf16", 0, 100, 77, 8, 40), "ctx"))
      for B, win in ((4, (1, 2)), (3, (2, 1)))]
# scale = 0.37 dh^-0.5, on the smallest shape of each kernel above: (case, layout)
SCALE_MUL = 0.37
SCALE = [
    (_case("ring40", "bf16", 3, 70, 70, 2, 40), "qkv"),
    (_case("w4", "bf16", 2, 100, 77, 8, 40, ring=0, short=0), "ctx"),
    (_case("flash", "bf16", 1, 100, 77, 8, 80, short=0), "ctx"),
    (_case("flash", "f32", 2, 130, 130, 8, 40), "qkv"),
    (_case("short", "bf16", 2, 100, 77, 8, 40), "ctx"),
]


def seed_of(c, extra=0):
    return 1000 * c.dh + 10 * c.Nq + c.Nk + c.heads + 7 * c.B + extra


def op_form(c, layout, ld_slack=0, lse=False, causal=False, drop_keys=0):
    """What ops.attention builds for a case: the row pitches (ldq, ldk, ldv, ldo) of AttnParams and whether a V^T pack goes with
    it (bf16, no mask, no lse, not the self-attention form, a short-key pack exists for dh and the key count)."""
    C = c.heads * c.dh
    ldq = (3 * C if layout == "qkv" else C) + ld_slack
    ldk = {"dense": C, "qkv": 3 * C, "ctx": 2 * C}[layout] + ld_slack
    pack = (c.dtype == "bf16" and not causal and not lse and layout != "qkv" and c.dh in (40, 80) and c.Nk - drop_keys <= SMAX)
    return {"ldq": ldq, "ldk": ldk, "ldv": ldk, "ldo": C + ld_slack, "vt_pack": pack}
