"""The fp16 compute mode (AF_DTYPE_F16) on the GPU: fp16 storage, v_mfma_f32_32x32x16_f16, fp32 accumulation.

1. Exact operands (tests/exact_operands.py): small integers are exact in fp16 as they are in bf16, so the fp64 reference IS
   the result; every four-wave tile with both stagings, every LDS-halo form and split-K in two and three slices, each asserted
   through af_last_gemm_plan.
2. The eleven-bit probe: operands that fp16 holds and bf16 does not (+-1025).  A path that narrows anything to bf16 fails it.
3. Overflow: beyond +-65504 the stored value is +-inf, as torch.Tensor.half() (no saturating clamp).
4. Gaussian operator parity at TOL["bf16"] / 8 of max|ref|, and at most a quarter of the bf16 kernel's error on the same inputs.
5. Tiny UNet / VAE / CLIP against the reference goldens at the bf16 bars / 8.
6. A 7-step CFG chain on the tiny model against the f32 mode.
7. SD-1.5 widths on a 16 x 16 latent against the f32 mode, with the counters of every bf16-only kernel at zero.
8. fp8 is refused on an fp16 handle.

Where the bars come from: the error of these kernels is operand and output rounding, fp16 carries 11 significant bits against
bf16's 8, so its unit round-off is 2^-3 of bf16's and every stated bf16 bar is divided by 8.  The ratio assertions ask for 4,
not 8: the factor 2 covers what does not scale with the storage type (fp32 summation order, the exponential) and the
extreme-value statistic of a maximum over a finite sample.
"""
import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from oracle import clip_oracle as CO  # noqa: E402  (checkers, never the thing measured)
from oracle import ldm_oracle as O    # noqa: E402

import exact_operands as X            # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ROOT / "tests" / "golden"

BF16_OP_TOL = 1.5e-2                  # tests/test_ops_gpu.py TOL["bf16"]
F16_OP_TOL = BF16_OP_TOL / 8          # 1.875e-3
BF16_MODEL_TOL = 3e-2                 # tests/test_model_gpu.py TOL["bf16"], tests/test_clip_gpu.py TOL["bf16"]
F16_MODEL_TOL = BF16_MODEL_TOL / 8    # 3.75e-3
RATIO = 4.0
AF_ERR_STATE = -4


def _last_plan():
    import ctypes as C
    from adaface_amd import _lib
    t, s, h = C.c_int(), C.c_int(), C.c_int()
    _lib.load().af_last_gemm_plan(C.byref(t), C.byref(s), C.byref(h))
    return t.value, s.value, h.value


def _counts(reset=True):
    from adaface_amd import _lib
    return _lib.plan_counts(reset=reset)


def _dev(t, gpu):
    return None if t is None else t.to(gpu)


def _f16_exact(t):
    return torch.equal(t.to(torch.float32).to(torch.float16).double(), t.double())


def _assert_case_exact_in_f16(c):
    """The precondition of every torch.equal below, on the operands and the fp64 reference alone."""
    for k in ("x", "w", "b", "r", "ref"):
        if c.get(k) is not None:
            assert _f16_exact(c[k]), f"{k} is not exact in float16"
    assert float(c["ref"].abs().max()) < 2048.0


# ======================================================================================================================
# 1. exact operands
# ======================================================================================================================
_conv_case = functools.lru_cache(maxsize=None)(X.conv_case)
_linear_case = functools.lru_cache(maxsize=None)(X.linear_case)

#           B, Cin, H, W, Cout, ks, stride, up, bias, res, carrier
_CONVS = {
    "res64": (2, 64, 8, 8, 64, 3, 1, False, True, True, False),
    "res320": (1, 320, 16, 16, 320, 3, 1, False, True, True, True),      # partial sums pass +-2304: fp16 spacing there is 2
    "down": (1, 128, 8, 8, 64, 3, 2, False, True, False, False),
    "up": (1, 64, 8, 8, 128, 3, 1, True, True, False, False),
    "skip1x1": (2, 1280, 8, 8, 64, 1, 1, False, True, False, True),
    "wide32": (1, 64, 8, 32, 128, 3, 1, False, True, False, False),     # a 32-pixel-wide map: the LDS-halo kernel's other patch shape
}
#           M, K, N, bias, res, carrier
_LINEARS = {
    "ragged": (130, 320, 320, True, True, False),
    "one_tile": (64, 64, 64, True, False, False),
    "deep": (256, 5120, 1280, True, True, True),
}


def _build(kind, name):
    if kind == "conv":
        B, Cin, H, W, Cout, ks, stride, up, bias, res, carrier = _CONVS[name]
        c = _conv_case(B, Cin, H, W, Cout, ks, stride, up, bias, res, seed=Cin + Cout + H + W + ks, storage="bf16", carrier=carrier)
    else:
        M, K, N, bias, res, carrier = _LINEARS[name]
        c = _linear_case(M, K, N, bias, res, seed=M + K + N, storage="bf16", carrier=carrier)
    _assert_case_exact_in_f16(c)
    return c


def _run(gpu, kind, name, c, dtype="f16"):
    from adaface_amd import ops
    if kind == "conv":
        _, _, _, _, _, _, stride, up, _, _, _ = _CONVS[name]
        return ops.conv2d(c["x"].to(gpu), c["w"].to(gpu), _dev(c["b"], gpu), stride=stride, upsample=up, residual=_dev(c["r"], gpu),
                          dtype=dtype)
    return ops.linear(c["x"].to(gpu), c["w"].to(gpu), _dev(c["b"], gpu), _dev(c.get("r"), gpu), dtype=dtype)


# every (tile, staging) pair once, the cases dealt over them so that each case meets the four-wave kernel at least once
_TILE_MATRIX = [
    (0, 0, "conv", "res320"), (0, 1, "linear", "ragged"), (1, 0, "conv", "up"), (1, 1, "conv", "skip1x1"),
    (2, 0, "conv", "down"), (2, 1, "conv", "res320"), (3, 0, "linear", "one_tile"), (3, 1, "conv", "res64"),
    (2, 0, "conv", "res64"), (0, 1, "conv", "skip1x1"), (3, 1, "linear", "ragged"), (1, 0, "conv", "wide32"),
]


@pytest.mark.parametrize("tile,dma,kind,name", _TILE_MATRIX, ids=[f"tile{t}-dma{d}-{n}" for t, d, _, n in _TILE_MATRIX])
def test_exact_fourwave_tiles_f16(gpu, report, knobs, tile, dma, kind, name):
    """conv_gemm_kernel<_Float16, tile, DMA>: the four tiles with register and LDS-DMA staging, on integer operands whose fp64
    reference is exact in fp16 (asserted on the reference): torch.equal over every element."""
    knobs("conv_halo", 0)
    knobs("gemm_tile", tile)
    knobs("gemm_dma", dma)
    knobs("gemm_splitk", 1)
    c = _build(kind, name)
    _counts()
    got = _run(gpu, kind, name, c)
    pc, plan = _counts(), _last_plan()
    assert plan == (tile, 1, 0) and pc[f"tile{tile}"] == 1 and pc["splitk"] == 0 and pc["halo"] == 0, (plan, pc)
    assert pc["tile4"] == pc["tile5"] == pc["rowpanel"] == pc["halo8"] == pc["up_phase4"] == 0, pc
    X.assert_bit_exact(f"f16 exact {kind} {name} tile{tile} dma{dma}", got, c["ref"], plan, report)


@pytest.mark.parametrize("name,tile,tw", [("res320", 0, 16), ("res320", 2, 16), ("wide32", 0, 32), ("wide32", 2, 32)])
def test_exact_halo_forms_f16(gpu, report, knobs, name, tile, tw):
    """conv3x3_halo_kernel<_Float16, {32, 16}, {128, 64}>.  splitk_target 1 keeps the cost model from slicing K, which would
    drop the halo plan."""
    knobs("splitk_target", 1)
    knobs("gemm_tile", tile)
    c = _build("conv", name)
    _counts()
    got = _run(gpu, "conv", name, c)
    pc, plan = _counts(), _last_plan()
    assert plan == (tile, 1, tw) and pc["halo"] == 1 and pc["halo8"] == 0, (plan, pc)
    X.assert_bit_exact(f"f16 exact halo{tw} {name} BN{128 if tile == 0 else 64}", got, c["ref"], plan, report)


@pytest.mark.parametrize("kind,name,slices", [("linear", "deep", 2), ("linear", "deep", 3), ("conv", "skip1x1", 3)])
def test_exact_splitk_f16(gpu, report, knobs, kind, name, slices):
    """K in two and three slices: fp32 slabs and splitk_reduce_kernel<_Float16>; the cancelling carrier's two channels lie in
    different slices."""
    knobs("gemm_splitk", slices)
    c = _build(kind, name)
    _counts()
    got = _run(gpu, kind, name, c)
    pc, plan = _counts(), _last_plan()
    assert plan[0] in (0, 1, 2, 3) and plan[1] == slices and plan[2] == 0 and pc["splitk"] == 1, (plan, pc)
    X.assert_bit_exact(f"f16 exact split-K {slices} {kind} {name}", got, c["ref"], plan, report)


@pytest.mark.parametrize("probe", ["value", "gate"])
@pytest.mark.parametrize("M,K,N", [(70, 64, 256), (130, 320, 1280)])
def test_exact_geglu_probes_f16(gpu, report, probe, M, K, N):
    """The two GEGLU probes of exact_operands on the fp16 kernel, which evaluates gelu_erf_f as the f32 kernels do: for a gate
    >= 8 the erf form returns the gate itself, so the product is exact."""
    from adaface_amd import ops
    build = X.geglu_value_probe if probe == "value" else X.geglu_gate_probe
    c = build(M, K, N, seed=M + K + N, storage="bf16")
    for k in ("x", "w", "b", "ref"):
        assert _f16_exact(c[k]), k
    _counts()
    got = ops.linear(c["x"].to(gpu), c["w"].to(gpu), c["b"].to(gpu), geglu=True, dtype="f16")
    pc, plan = _counts(), _last_plan()
    assert plan[0] in (0, 1) and plan[1] == 1 and plan[2] == 0 and pc["rowpanel"] == 0, (plan, pc)
    X.assert_bit_exact(f"f16 exact geglu {probe} probe [{M},{K}]->{N}", got, c["ref"], plan, report)


# ======================================================================================================================
# 2. the eleven-bit probe
# ======================================================================================================================
ELEVEN_BIT = 1025.0        # 2^10 + 1: an fp16 value, not a bf16 one


@functools.lru_cache(maxsize=None)
def _eleven_bit_case(M, K, N):
    g = torch.Generator().manual_seed(M + K + N)
    d = X.density_for(K)
    x = X.int_tensor((M, K), d, g)
    if K <= 64:
        w = torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1          # dense +-1
    else:
        w = X.int_tensor((N, K), d, g)
    col = torch.randint(0, K, (M,), generator=g)
    sign = torch.randint(0, 2, (M,), generator=g).float() * 2 - 1
    x[torch.arange(M), col] = sign * ELEVEN_BIT                                 # exactly one entry per row
    ref = X.fp64_ref_linear(x, w)
    # preconditions, on the operands and the reference alone
    assert _f16_exact(x) and _f16_exact(w) and _f16_exact(ref)
    assert float(ref.abs().max()) < 2048.0
    not_bf16 = float((ref.float().to(torch.bfloat16).double() != ref).double().mean())
    narrowed = X.fp64_ref_linear(x.to(torch.bfloat16).float(), w)
    changed = float((narrowed != ref).double().mean())
    assert not_bf16 >= 0.4, not_bf16
    assert changed >= 0.4, changed
    return x, w, ref, not_bf16, changed


_ELEVEN = [(130, 64, 64, (10, 13)), (256, 320, 320, (16, 16)), (64, 1280, 128, (8, 8))]


@pytest.mark.parametrize("M,K,N,hw", _ELEVEN)
def test_eleven_bit_probe_linear(gpu, report, M, K, N, hw):
    """x in {-1, 0, 1} with one +-1025 per row, w in {-1, 0, 1}: operands and every result (< 2048) are fp16 values, and at
    least 0.4 of the results are NOT bf16 values.  torch.equal: an operand, accumulator or store narrowed to bf16 fails."""
    from adaface_amd import ops
    x, w, ref, not_bf16, changed = _eleven_bit_case(M, K, N)
    got = ops.linear(x.to(gpu), w.to(gpu), dtype="f16")
    report(f"f16 eleven-bit probe linear [{M},{K}]->{N}: share of outputs not bf16-exact", not_bf16, 1.0, 0.4)
    report(f"f16 eleven-bit probe linear [{M},{K}]->{N}: share changed by narrowing x to bf16", changed, 1.0, 0.4)
    assert torch.equal(got.cpu().double(), ref), int((got.cpu().double() != ref).sum())


@pytest.mark.parametrize("M,K,N,hw", _ELEVEN)
def test_eleven_bit_probe_conv1x1(gpu, M, K, N, hw):
    """The same operands through a 1x1 conv2d (the NCHW -> NHWC converter and the convolution entry)."""
    from adaface_amd import ops
    x, w, ref, _, _ = _eleven_bit_case(M, K, N)
    h, wd = hw
    assert h * wd == M
    xi = x.t().reshape(1, K, h, wd).contiguous()
    got = ops.conv2d(xi.to(gpu), w.reshape(N, K, 1, 1).to(gpu), None, dtype="f16")
    got = got.reshape(N, M).t().cpu().double()
    assert torch.equal(got, ref), int((got != ref).sum())


# ======================================================================================================================
# 3. overflow semantics
# ======================================================================================================================
def test_overflow_becomes_inf_as_torch_half(gpu):
    """Every second row of x is scaled by 4096: its results are 4096 * (an integer sum), beyond 65504 from |sum| >= 16 on.
    Expected: exactly ref.float().half().float() -- +-inf where torch gives inf, the exact value elsewhere."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(16)
    M, K, N = 128, 64, 64
    x = torch.randint(0, 2, (M, K), generator=g).float() * 2 - 1
    w = torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1
    x[::2] *= 4096.0
    ref = X.fp64_ref_linear(x, w)
    assert _f16_exact(x) and _f16_exact(w) and float(X.absbound_linear(x, w).max()) < X.TWO24
    want = ref.float().half().float()
    n_inf = int(torch.isinf(want).sum())
    big = want[::2]
    assert n_inf > 50 and int(torch.isfinite(big).sum()) > 50 and bool((want == float("inf")).any()) and bool((want == float("-inf")).any())
    finite = torch.isfinite(want)
    assert torch.equal(want[finite].double(), ref[finite])                    # inside the range the stored value is exact
    got = ops.linear(x.to(gpu), w.to(gpu), dtype="f16").cpu()
    assert torch.equal(got, want), (int((got != want).sum()), n_inf)


# ======================================================================================================================
# 4. Gaussian operator parity
# ======================================================================================================================
def _q16(t):
    """Inputs rounded to the storage type of the kernel under test, as tests/test_ops_gpu.py's _q does for its modes."""
    return t.to(torch.float16).float()


def _rel_err(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-12
    if not bool(torch.isfinite(got).all()):
        return float("inf"), scale
    return (got - ref).abs().max().item() / scale, scale


def _cmp_pair(report, name, got16, gotbf, ref):
    e16, scale = _rel_err(got16, ref)
    ebf, _ = _rel_err(gotbf, ref)
    report(f"{name} [f16]", e16 * scale, scale, F16_OP_TOL * scale)
    report(f"{name} [bf16, same inputs]", ebf * scale, scale, BF16_OP_TOL * scale)
    report(f"{name} bf16 / f16 error ratio", ebf / max(e16, 1e-30), 1.0, RATIO)
    assert math.isfinite(e16), f"{name}: non-finite fp16 output"
    assert e16 <= F16_OP_TOL, f"{name}: fp16 max abs err {e16:.3e} of max|ref| > {F16_OP_TOL:.3e}"
    assert e16 <= ebf / RATIO, f"{name}: fp16 err {e16:.3e} > bf16 err {ebf:.3e} / {RATIO}"


@pytest.mark.parametrize("B,C,H,W,eps,silu", [(3, 64, 4, 4, 1e-6, False), (2, 1280, 8, 8, 1e-6, False), (1, 128, 96, 80, 1e-6, True),
                                              (2, 640, 32, 32, 1e-5, True)])
def test_groupnorm_f16(gpu, report, B, C, H, W, eps, silu):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(C + H)
    x = _q16(torch.randn(B, C, H, W, generator=g) * 1.7 + 0.4)
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    ref = F.group_norm(x, 32, w, b, eps)
    if silu:
        ref = F.silu(ref)
    run = lambda dt: ops.group_norm(x.to(gpu), w.to(gpu), b.to(gpu), eps=eps, silu=silu, dtype=dt)
    _cmp_pair(report, f"groupnorm C{C} {H}x{W}", run("f16"), run("bf16"), ref)


@pytest.mark.parametrize("rows,C", [(7, 64), (130, 1280), (1024, 640), (8192, 320)])
def test_layernorm_f16(gpu, report, rows, C):
    """(8192 rows of 320: the row-group kernel; the others the one-wave-per-row kernel)"""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(rows + C)
    x = _q16(torch.randn(rows, C, generator=g) * 2.0 + 0.5)
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    ref = F.layer_norm(x, (C,), w, b, 1e-5)
    run = lambda dt: ops.layer_norm(x.to(gpu), w.to(gpu), b.to(gpu), dtype=dt)
    _cmp_pair(report, f"layernorm {rows}x{C}", run("f16"), run("bf16"), ref)


@pytest.mark.parametrize("M,K,N,bias,res", [(2, 320, 1280, True, False), (200, 64, 192, True, False), (333, 128, 4, True, False),
                                            (256, 1280, 1280, True, True)])
def test_linear_f16(gpu, report, M, K, N, bias, res):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(M + K + N)
    x = _q16(torch.randn(M, K, generator=g))
    w = _q16(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) * 0.1 if bias else None
    r = _q16(torch.randn(M, N, generator=g)) if res else None
    ref = F.linear(x, w, b)
    if res:
        ref = ref + r
    run = lambda dt: ops.linear(x.to(gpu), w.to(gpu), _dev(b, gpu), _dev(r, gpu), dtype=dt)
    _cmp_pair(report, f"linear {M}x{K}->{N}", run("f16"), run("bf16"), ref)


@pytest.mark.parametrize("M,d", [(70, 64), (256, 1280), (1024, 640)])
def test_geglu_f16(gpu, report, M, d):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(M + d)
    x = _q16(torch.randn(M, d, generator=g))
    w = _q16(torch.randn(8 * d, d, generator=g) / math.sqrt(d))
    b = torch.randn(8 * d, generator=g) * 0.1
    val, gate = F.linear(x, w, b).chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    run = lambda dt: ops.linear(x.to(gpu), w.to(gpu), b.to(gpu), geglu=True, dtype=dt)
    _cmp_pair(report, f"geglu {M}x{d}", run("f16"), run("bf16"), ref)


@pytest.mark.parametrize("B,Cin,H,W,Cout,ks,stride,up,bias,res", [
    (1, 64, 8, 8, 128, 3, 1, False, False, False),      # tiny-config conv
    (1, 128, 40, 24, 3, 3, 1, False, True, False),      # ragged M, three output channels
    (2, 320, 32, 32, 320, 3, 2, False, True, False),    # Downsample
    (1, 640, 16, 16, 640, 3, 1, True, True, False),     # Upsample (nearest 2x folded into the gather)
    (2, 320, 32, 32, 320, 3, 1, False, True, True),     # ResBlock conv: the LDS-halo kernel
])
def test_conv2d_f16(gpu, report, B, Cin, H, W, Cout, ks, stride, up, bias, res):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(Cin + Cout + H + ks)
    x = _q16(torch.randn(B, Cin, H, W, generator=g))
    w = _q16(torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks))
    b = torch.randn(Cout, generator=g) * 0.1 if bias else None
    xi = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
    ref = F.conv2d(xi, w, b, stride=stride, padding=ks // 2)
    r = _q16(torch.randn(ref.shape, generator=g)) if res else None
    if res:
        ref = ref + r
    run = lambda dt: ops.conv2d(x.to(gpu), w.to(gpu), _dev(b, gpu), stride=stride, upsample=up, residual=_dev(r, gpu), dtype=dt)
    _cmp_pair(report, f"conv{ks}x{ks} {Cin}->{Cout}@{H}x{W} s{stride} up{int(up)}", run("f16"), run("bf16"), ref)


def _ref_attention(q, k, v, heads, causal=False):
    B, N, C = q.shape
    dh = C // heads
    qh = q.view(B, N, heads, dh).transpose(1, 2)
    kh = k.view(B, -1, heads, dh).transpose(1, 2)
    vh = v.view(B, -1, heads, dh).transpose(1, 2)
    sim = torch.einsum("bhid,bhjd->bhij", qh, kh) * dh ** -0.5
    if causal:
        S = kh.shape[2]
        sim = sim.masked_fill(torch.arange(S)[None, :] > torch.arange(N)[:, None], float("-inf"))
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), vh)
    return out.transpose(1, 2).reshape(B, N, C)


@pytest.mark.parametrize("B,Nq,Nk,heads,dh,causal", [
    (3, 70, 64, 2, 40, False), (1, 256, 77, 8, 80, False), (2, 64, 64, 8, 160, False), (2, 77, 77, 4, 64, True),
    (1, 300, 333, 2, 40, False),     # five whole key tiles and a partial sixth
    (1, 100, 50, 2, 32, False),
])
def test_attention_f16(gpu, report, B, Nq, Nk, heads, dh, causal):
    """attn_kernel<_Float16, DH>: the head dims of the UNet (40, 80, 160), the CLIP tower's causal dh 64, partial last key tiles
    (77, 333, 50 keys)."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(Nq + Nk + dh)
    C = heads * dh
    q = _q16(torch.randn(B, Nq, C, generator=g))
    k = _q16(torch.randn(B, Nk, C, generator=g))
    v = _q16(torch.randn(B, Nk, C, generator=g))
    ref = _ref_attention(q, k, v, heads, causal)
    _counts()
    got16 = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype="f16", causal=causal)
    assert _counts()["attn_short"] == 0
    gotbf = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype="bf16", causal=causal)
    _cmp_pair(report, f"attention N{Nq} S{Nk} h{heads} d{dh}{' causal' if causal else ''}", got16, gotbf, ref)


@pytest.mark.parametrize("dh", [64, 40])
def test_attention_spiky_softmax_f16(gpu, report, dh):
    """One key per query far above the rest, from a late tile: the running maximum jumps and the O accumulator is rescaled.
    dh 64 sums the denominator on the VALU, dh 40 through the ones column of the V tile.  q and k are finite fp16 values."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(5)
    B, N, heads = 1, 256, 2
    q = torch.randn(B, N, heads * dh, generator=g)
    k = torch.randn(B, N, heads * dh, generator=g)
    v = torch.randn(B, N, heads * dh, generator=g)
    k[:, 200] = q[:, 17] * 3.0                               # key 200 (4th tile) matches query 17 strongly
    k[:, 70:70 + N // 2] += q[:, :N // 2] * 2.0             # ... and every query of the first half has its own key in a later tile
    q, k, v = _q16(q), _q16(k), _q16(v)
    assert bool(torch.isfinite(q).all() and torch.isfinite(k).all())
    ref = _ref_attention(q, k, v, heads)
    got = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype="f16")
    err, scale = _rel_err(got, ref)
    report(f"attention spiky d{dh} [f16]", err * scale, scale, F16_OP_TOL * scale)
    assert math.isfinite(err) and err <= F16_OP_TOL, err


# ======================================================================================================================
# 5. tiny models against the reference goldens
# ======================================================================================================================
def _unet_kwargs(cfg):
    return dict(in_channels=cfg.in_channels, model_channels=cfg.model_channels, out_channels=cfg.out_channels,
                num_res_blocks=cfg.num_res_blocks, attention_resolutions=cfg.attention_resolutions,
                channel_mult=cfg.channel_mult, num_heads=cfg.num_heads, context_dim=cfg.context_dim,
                transformer_depth=cfg.transformer_depth, n_context_layers=cfg.n_context_layers)


def _vae_kwargs(cfg):
    return dict(ch=cfg.ch, out_ch=cfg.out_ch, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks,
                z_channels=cfg.z_channels, embed_dim=cfg.embed_dim)


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float("inf") if not np.isfinite(got).all() else float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))


def _rms(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


@pytest.fixture(scope="module")
def tiny():
    return dict(np.load(GOLD / "golden_tiny.npz"))


@pytest.mark.parametrize("conv_attn", [False, True])
def test_tiny_unet_f16(gpu, report, tiny, conv_attn):
    """The tiny UNet (plain, and with 3x3 subject-token conv attention) against the reference's eps: max-abs <= 3e-2 / 8 of
    max|eps|, rms at most a quarter of the bf16 forward's, and the twin forward within the same bar."""
    from adaface_amd.engine import Engine
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    cfg = O.TINY_UNET
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=11)
    x = torch.tensor(tiny["tiny_x"], device=gpu)
    t = torch.tensor(tiny["tiny_t"], device=gpu)
    ctx = torch.tensor(tiny["tiny_ctx"], device=gpu)
    ref = tiny["tiny_convattn_eps"] if conv_attn else tiny["tiny_eps"]
    spec = UNetModel._conv_attn_spec(3, {"z": (torch.tensor(tiny["tiny_convattn_idx_b"]), torch.tensor(tiny["tiny_convattn_idx_n"]))})
    out = {}
    for dtype in ("f16", "bf16"):
        eng = Engine(dtype=dtype, unet=_unet_kwargs(cfg))
        assert eng.load_state_dict(sd) == []
        if conv_attn:
            eng.set_conv_attn(*spec)
        eng.set_context(ctx, x.shape[0], layerwise=True)
        _counts()
        eps = eng.unet_forward(x, t)
        pc = _counts()
        assert torch.isfinite(eps).all()
        if dtype == "f16":
            assert pc["tile4"] == pc["tile5"] == pc["halo8"] == pc["rowpanel"] == pc["attn_short"] == pc["xattn_fused"] == 0, pc
            assert pc["conv_attn_short"] == pc["gn_producer"] == pc["ln_consumer"] == pc["ln_producer"] == 0, pc
            assert torch.equal(eps, eng.unet_forward(x, t))          # the cached context, no stale state in the arena
            # the classifier-free-guidance twin: [x; x] with the context of four samples, both halves the golden's
            if conv_attn:
                b_idx, tok = spec[1], spec[2]
                eng.set_conv_attn(3, list(b_idx) + [b + x.shape[0] for b in b_idx], list(tok) + list(tok))
            eng.set_context(torch.cat([ctx, ctx]), 2 * x.shape[0], layerwise=True)
            twin = eng.unet_forward_twin(x, t)
            assert torch.isfinite(twin).all()
            e_twin = _rel(twin.cpu().numpy(), np.concatenate([ref, ref]))
            report(f"tiny_unet twin forward{' + conv attention' if conv_attn else ''} vs reference golden [f16]", e_twin, 1.0, F16_MODEL_TOL)
            assert e_twin <= F16_MODEL_TOL, e_twin
        out[dtype] = eps.cpu().numpy()
        eng.close()
    tag = " + conv attention" if conv_attn else ""
    e16, ebf = _rel(out["f16"], ref), _rel(out["bf16"], ref)
    r16, rbf = _rms(out["f16"], ref), _rms(out["bf16"], ref)
    report(f"tiny_unet{tag} eps vs reference golden [f16]", e16, 1.0, F16_MODEL_TOL)
    report(f"tiny_unet{tag} eps vs reference golden [bf16, same test]", ebf, 1.0, BF16_MODEL_TOL)
    report(f"tiny_unet{tag} eps rms / rms vs reference golden [f16]", r16, 1.0, rbf / RATIO)
    report(f"tiny_unet{tag} eps rms / rms vs reference golden [bf16, same test]", rbf, 1.0, BF16_MODEL_TOL)
    assert e16 <= F16_MODEL_TOL, e16
    assert r16 <= rbf / RATIO, (r16, rbf)


def test_tiny_vae_decoder_f16(gpu, report, tiny):
    from adaface_amd.engine import Engine
    cfg = O.TINY_VAE
    eng = Engine(dtype="f16", vae=_vae_kwargs(cfg))
    eng.load_state_dict(O.synth_state_dict(O.vae_param_shapes(cfg), seed=12))
    img, u8 = eng.vae_decode(torch.tensor(tiny["vae_z"], device=gpu), scale_factor=cfg.scale_factor, want_uint8=True)
    assert torch.isfinite(img).all()
    err = _rel(img.cpu().numpy(), tiny["vae_tiny_img"])
    report("tiny_vae image vs reference golden [f16]", err, 1.0, F16_MODEL_TOL)
    assert err <= F16_MODEL_TOL, err
    d = np.abs(u8.cpu().numpy().astype(int) - O.to_uint8_hwc(torch.tensor(tiny["vae_tiny_img"])).astype(int))
    assert d.max() <= 2, d.max()          # (bf16: 12 of 255 at 3e-2; 3.75e-3 of a [-1, 1] image is half a level)
    eng.close()


def test_tiny_vae_encoder_f16(gpu, report, tiny):
    from adaface_amd.engine import Engine
    cfg = O.TINY_VAE
    eng = Engine(dtype="f16", vae=dict(_vae_kwargs(cfg), encoder=True, in_channels=3))
    eng.load_state_dict(O.synth_state_dict(O.vae_encoder_param_shapes(cfg), seed=13), strict=False)   # encoder side only
    mom = eng.vae_encode(torch.tensor(tiny["vae_enc_x"], device=gpu))
    assert torch.isfinite(mom).all()
    err = _rel(mom.cpu().numpy(), tiny["vae_enc_moments"])
    report("tiny_vae encoder moments vs reference golden [f16]", err, float(np.abs(tiny["vae_enc_moments"]).max()), F16_MODEL_TOL)
    assert mom.shape == tiny["vae_enc_moments"].shape and err <= F16_MODEL_TOL, err
    eng.close()


def test_tiny_clip_tower_f16(gpu, report):
    """The tiny CLIP text tower (causal dh-64... attention, quick-GELU MLP, final LayerNorm) against the transformers golden, at
    tests/test_clip_gpu.py's bf16 bar / 8."""
    from adaface_amd.engine import Engine
    g = dict(np.load(GOLD / "golden_clip.npz"))
    cfg = CO.TINY_CLIP
    sd = O.synth_state_dict(CO.clip_param_shapes(cfg), seed=41)
    eng = Engine(dtype="f16", clip=dict(vocab=cfg.vocab, hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                                        intermediate=cfg.intermediate, max_pos=cfg.max_pos))
    assert eng.load_state_dict(sd) == []
    ids = torch.tensor(g["tiny_ids"], device=gpu)
    emb = eng.clip_embed_tokens(ids)
    ref_emb = CO.clip_embed_tokens(sd, ids.cpu())
    assert _rel(emb.cpu().numpy(), ref_emb.numpy()) < 5e-3 / 8          # (the embedding tables are stored in fp16)
    z = eng.clip_text_forward(emb)
    assert torch.isfinite(z).all()
    err = _rel(z.cpu().numpy(), g["tiny_z"])
    report("clip text tower tiny vs transformers golden [f16]", err, float(np.abs(g["tiny_z"]).max()), F16_MODEL_TOL)
    assert err <= F16_MODEL_TOL, err
    eng.close()


# ======================================================================================================================
# 6. chained, tiny
# ======================================================================================================================
def test_tiny_ddim_chain_f16_vs_f32_mode(gpu, report):
    """The drop-in DDIMSampler on the tiny model, 7 steps with classifier-free guidance: fp16 against the f32 mode of the same
    model.  First-forward eps <= 3.75e-3 of max|eps|; the final latent at most 4 x that measured error (the chain-gain bound
    smoke() states for bf16)."""
    from adaface_amd.configs import tiny_config
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.util import instantiate_from_config
    model = instantiate_from_config(tiny_config()["model"]).eval()
    sd = O.synth_state_dict(O.unet_param_shapes(O.TINY_UNET), seed=11)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith("model.")]
    model = model.to(gpu)
    g = torch.Generator().manual_seed(5)
    B, S = 2, 7
    x_T = torch.randn(B, 4, 16, 16, generator=g).to(gpu)
    c_emb = torch.randn(B * 16, 77, 64, generator=g).to(gpu)
    uc_emb = torch.randn(B * 16, 77, 64, generator=g).to(gpu)
    t0 = torch.full((B,), 801, dtype=torch.long, device=gpu)
    sampler = DDIMSampler(model)
    out = {}
    for mode in ("f32", "fp16"):
        model.set_compute_dtype(mode)
        assert model.model.diffusion_model.compute_dtype == ("f16" if mode == "fp16" else "f32")
        c, uc = model.get_learned_conditioning(c_emb), model.get_learned_conditioning(uc_emb)
        eps = model.apply_model(x_T, t0, c)
        lat, _ = sampler.sample(S=S, conditioning=c, batch_size=B, shape=[4, 16, 16], verbose=False, guidance_scale=[10.0, 4.0],
                                unconditional_conditioning=uc, eta=0.0, x_T=x_T)
        torch.cuda.synchronize()
        assert torch.isfinite(eps).all() and torch.isfinite(lat).all(), mode
        out[mode] = (eps.clone(), lat.clone())
    e1 = (out["fp16"][0] - out["f32"][0]).abs().max().item() / out["f32"][0].abs().max().item()
    ef = (out["fp16"][1] - out["f32"][1]).abs().max().item() / out["f32"][1].abs().max().item()
    report("tiny chain: first-forward eps f16 vs f32 mode", e1, out["f32"][0].abs().max().item(), F16_MODEL_TOL)
    report("tiny chain: final latent after S=7 DDIM steps f16 vs f32 mode", ef, out["f32"][1].abs().max().item(), 4.0 * e1)
    assert 0 < e1 <= F16_MODEL_TOL, e1                              # (0 would mean the mode never switched)
    assert ef <= 4.0 * e1, (ef, e1)


# ======================================================================================================================
# 7. full widths, small map
# ======================================================================================================================
_BF16_ONLY = ("tile4", "tile5", "halo8", "rowpanel", "attn_short", "xattn_fused", "gn_producer", "gn_consumer", "up_phase4", "fp8")


def test_sd15_widths_small_map_f16_vs_f32_mode(gpu, report):
    """SD-1.5 widths, synthetic weights, Bf = 2 on a 16 x 16 latent: fp16 against the f32-mode forward of the same weights and
    inputs.  max-abs <= 3.75e-3 of max|eps|, rms at most a quarter of the bf16 forward's, two forwards bit-identical, and no
    bf16-only kernel launched (the eight-wave tiles, row-panel, short-key and fused cross-attention, GroupNorm fusions, the
    phase-4 upsample, fp8) while the LDS-halo kernel was."""
    from adaface_amd.engine import Engine
    from adaface_amd.synth import synth_weights_into
    cfg = O.SD15_UNET
    g = torch.Generator().manual_seed(160)
    Bf = 2
    x = torch.randn(Bf, 4, 16, 16, generator=g).to(gpu)
    t = torch.tensor([801, 341]).to(gpu)
    ctx = torch.randn(Bf * 16, 77, cfg.context_dim, generator=g).to(gpu)
    out = {}
    for dtype in ("f32", "bf16", "f16"):
        eng = Engine(dtype=dtype, unet=_unet_kwargs(cfg))
        synth_weights_into(eng, O.unet_param_shapes(cfg), seed=42, device=gpu)
        eng.set_context(ctx, Bf, layerwise=True)
        _counts()
        out[dtype] = eng.unet_forward(x, t)
        pc = _counts()
        if dtype == "f16":
            assert all(pc[k] == 0 for k in _BF16_ONLY) and pc["ln_consumer"] == pc["ln_producer"] == 0, pc
            assert pc["halo"] > 0, pc
            assert torch.equal(out["f16"], eng.unet_forward(x, t))
            assert eng._lib.af_fp8_num_sites(eng._h) == 0
        eng.close()
    ref = out["f32"]
    assert torch.isfinite(out["f16"]).all()
    scale = ref.abs().max().item()
    e16 = (out["f16"] - ref).abs().max().item() / scale
    ebf = (out["bf16"] - ref).abs().max().item() / scale
    r16, rbf = _rms(out["f16"].cpu().numpy(), ref.cpu().numpy()), _rms(out["bf16"].cpu().numpy(), ref.cpu().numpy())
    report("sd15 widths 16x16 Bf=2 eps f16 vs f32 mode", e16, scale, F16_MODEL_TOL)
    report("sd15 widths 16x16 Bf=2 eps bf16 vs f32 mode (same test)", ebf, scale, BF16_MODEL_TOL)
    report("sd15 widths 16x16 Bf=2 eps rms / rms f16 vs f32 mode", r16, 1.0, rbf / RATIO)
    report("sd15 widths 16x16 Bf=2 eps rms / rms bf16 vs f32 mode (same test)", rbf, 1.0, BF16_MODEL_TOL)
    assert e16 <= F16_MODEL_TOL, (e16, ebf)
    assert r16 <= rbf / RATIO, (r16, rbf)


def test_sd15_vae_decoder_small_map_f16_vs_f32_mode(gpu, report):
    """The SD-1.5 VAE decoder on an 8 x 8 latent (a 64 x 64 image): fp16 against its f32 mode, 3.75e-3 of max|image|."""
    from adaface_amd.engine import Engine
    from adaface_amd.synth import synth_weights_into
    cfg = O.SD15_VAE
    z = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(88)).to(gpu)
    out = {}
    for dtype in ("f32", "f16"):
        eng = Engine(dtype=dtype, vae=_vae_kwargs(cfg))
        synth_weights_into(eng, O.vae_param_shapes(cfg), seed=22, device=gpu)
        _counts()
        out[dtype] = eng.vae_decode(z, scale_factor=cfg.scale_factor)[0]
        pc = _counts()
        if dtype == "f16":
            assert all(pc[k] == 0 for k in _BF16_ONLY), pc
        eng.close()
    assert torch.isfinite(out["f16"]).all()
    scale = out["f32"].abs().max().item()
    err = (out["f16"] - out["f32"]).abs().max().item() / scale
    report("sd15 VAE decoder 8x8 latent image f16 vs f32 mode", err, scale, F16_MODEL_TOL)
    assert err <= F16_MODEL_TOL, err


# ======================================================================================================================
# 8. refusals
# ======================================================================================================================
def test_fp8_is_refused_on_an_fp16_handle(gpu):
    from adaface_amd import _lib
    from adaface_amd.engine import Engine
    from adaface_amd._lib import stream_ptr
    eng = Engine(dtype="fp16", unet=_unet_kwargs(O.TINY_UNET))
    lib = _lib.load()
    assert lib.af_fp8_num_sites(eng._h) == 0
    for call, what in ((lambda: lib.af_set_fp8(eng._h, 1), "af_set_fp8"), (lambda: lib.af_set_fp8_scope(eng._h, 3), "af_set_fp8_scope"),
                       (lambda: lib.af_fp8_record(eng._h, 1, stream_ptr()), "af_fp8_record")):
        assert call() == AF_ERR_STATE, what
        msg = lib.af_last_error().decode()
        assert what in msg and ("f16" in msg or "fp16" in msg), msg
    assert lib.af_set_fp8(eng._h, 0) == 0           # switching it off is a no-op on every handle
    with pytest.raises(_lib.AfError):
        eng.set_fp8(True)
    eng.close()
