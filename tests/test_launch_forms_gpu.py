"""The conv / GEMM launch forms only the model states, kernel by kernel (ops.conv2d / ops.linear keyword arguments rowbias,
alpha, padding=0, ld_slack -> af_op_conv2d_ex / af_op_linear_ex).

Every other per-kernel test builds one form of ConvGemmParams: alpha 1, no per-sample bias row, pad ks / 2, row pitches equal
to the channel counts.  Runner::conv_params (csrc/af_model.hip) builds others: the time-embedding row on the first 3x3
convolution of every ResBlock, pad 0 with stride 2 (the VAE encoder's bottom / right padding), pitches wider than the channel
count, and alpha != 1 on the VAE attention.  Here each of them meets each kernel the planner can give it.

Sections a-e compare with exact_operands.assert_bit_exact against the fp64 reference over every output element (integer
operands, alpha a power of two: tests/test_exact_operands_cpu.py shows that every plausible mistake changes the reference in
every sample it touches); section f repeats a-d on Gaussian operands at the bars of tests/test_ops_gpu.py and
tests/test_fp16_gpu.py.  Every case asserts which kernel ran.

Pairs the planner can never produce, hence not here: conv_gemm_pp_kernel and the other eight-wave kernels with fp16 or f32
storage (plan_tiled: bf16 only); the bias row on a row-panel, 128 x 160 or four-phase launch (rowpanel_kind / up_phase4_ok
refuse it) and on any linear; bottom / right padding on the LDS-halo and small-map kernels (stride 1, pad 1 only); a tile that
straddles samples on the LDS-halo kernels (their tiles are whole image rows); alpha != 1 on row-panel kinds 2, 3 and 5 (section c
asserts the refusal).  The batched (blockIdx.z) form of the VAE attention: tests/test_vae_attn_gpu.py.
"""
import functools
import math

import pytest
import torch

import exact_operands as X
import test_fp16_gpu as T16
import test_ops_gpu as T

pytestmark = pytest.mark.gpu

_conv_case = functools.lru_cache(maxsize=8)(X.conv_case)
_linear_case = functools.lru_cache(maxsize=4)(X.linear_case)


def _dev(t, gpu):
    return None if t is None else t.to(gpu)


def _counts():
    from adaface_amd import _lib
    return _lib.plan_counts(reset=True)


def _conv(gpu, c, stride=1, dtype="bf16", ld_slack=0):
    from adaface_amd import ops
    return ops.conv2d(c["x"].to(gpu), c["w"].to(gpu), _dev(c["b"], gpu), stride=stride, padding=c.get("pad"), residual=_dev(c["r"], gpu),
                      dtype=dtype, rowbias=_dev(c.get("rb"), gpu), alpha=c.get("alpha", 1.0), ld_slack=ld_slack)


def _linear(gpu, c, dtype="bf16", geglu=False, ld_slack=0, alpha=None):
    from adaface_amd import ops
    return ops.linear(c["x"].to(gpu), c["w"].to(gpu), _dev(c["b"], gpu), _dev(c.get("r"), gpu), geglu=geglu, dtype=dtype,
                      alpha=c.get("alpha", 1.0) if alpha is None else alpha, ld_slack=ld_slack)


def _force(knobs, kernel, tile=0, splitk=1):
    """The knobs tests/test_exact_gpu.py uses to reach each kernel."""
    if kernel == "wave4":          # conv_gemm_kernel
        for k, v in (("gemm_pp", 0), ("conv_halo", 0), ("geglu_rowpanel", 0), ("gemm_m128", 0), ("gemm_tile", tile), ("gemm_splitk", splitk)):
            knobs(k, v)
    elif kernel == "pp":           # conv_gemm_pp_kernel, gathering
        knobs("gemm_pp_minfill", 0)
        knobs("conv_halo8", 0)
        if splitk > 1:
            knobs("gemm_splitk", splitk)
    elif kernel == "halo4":        # conv3x3_halo_kernel
        knobs("gemm_pp", 0)
        knobs("splitk_target", 1)
        knobs("gemm_tile", tile)
    elif kernel == "halo8":        # conv3x3_halo8_kernel
        knobs("gemm_pp_minfill", 0)
        knobs("gemm_splitk", splitk)
    else:                          # conv3x3_s8_kernel: the default planner
        assert kernel in ("s8_4", "s8_1"), kernel


def _assert_kernel(kernel, pc, plan, tile=0, splitk=1, tw=0):
    if kernel == "wave4":
        ok = plan == (tile, splitk, 0) and pc[f"tile{tile}"] == 1 and pc["halo"] == 0 and pc["rowpanel"] == 0
    elif kernel == "pp":
        ok = plan[0] in (4, 5) and plan[1] == splitk and plan[2] == 0 and pc["halo8"] == 0 and pc["rowpanel"] == 0 and pc["up_phase4"] == 0
    elif kernel == "halo4":
        ok = plan == (tile, 1, tw) and pc["halo"] == 1 and pc["halo8"] == 0
    elif kernel == "halo8":
        ok = plan == (5, splitk, 256) and pc["halo8"] == 1
    else:
        ok = plan == (5, 4 if kernel == "s8_4" else 1, 8) and pc["halo8"] == 0 and pc["tile5"] == 1
    assert ok and pc["splitk"] == (1 if plan[1] > 1 else 0), (kernel, plan, pc)


def _id(v):
    if isinstance(v, tuple):
        return "x".join(str(x) for x in v)
    return str(v)


def _params(rows):
    return [pytest.param(*r, id="-".join(_id(v) for v in r)) for r in rows]


# kernel, dtype, (B, Cin, H, W, Cout), tile, halo width, K slices -- 3x3 / stride 1, bias and residual set
_K3 = (
    # conv_gemm_kernel: 144-row samples under 128-row tiles, M = 720 ragged; 64-row samples, two per tile
    [("wave4", dt, (5, 64, 12, 12, 64), 2, 0, 1) for dt in ("bf16", "f32", "f16")]
    + [("wave4", dt, (8, 64, 8, 8, 128), 0, 0, 1) for dt in ("bf16", "f32", "f16")]
    + [("wave4", "bf16", (5, 128, 12, 12, 64), 2, 0, 2)]                     # two K slices: splitk_reduce_kernel applies the row
    # conv_gemm_pp_kernel: 144-row samples under 256-row tiles (the division path, howo_shift = -1), M = 720 = 2 * 256 + 208;
    # 64-row samples, four per tile (the shift path); three K slices + reduce
    + [("pp", "bf16", (5, 64, 12, 12, 160), 5, 0, 1), ("pp", "bf16", (8, 64, 8, 8, 160), 5, 0, 1), ("pp", "bf16", (5, 192, 12, 12, 160), 5, 0, 3)]
    # conv3x3_halo_kernel: a patch = 8 x 16 or 4 x 32 pixels = one whole sample here, so consecutive patches change sample
    + [("halo4", dt, (3, 64, 8, 16, 128), 0, 16, 1) for dt in ("bf16", "f32", "f16")]
    + [("halo4", "bf16", (3, 64, 4, 32, 64), 2, 32, 1)]
    # conv3x3_halo8_kernel: one 16 x 16 image per tile / half a 32 x 16 image; one slice and two (the reduce applies the row)
    + [("halo8", "bf16", (3, 128, 16, 16, 160), 5, 256, 1), ("halo8", "bf16", (3, 128, 16, 16, 160), 5, 256, 2), ("halo8", "bf16", (2, 64, 32, 16, 160), 5, 256, 1)]
    # conv3x3_s8_kernel<4>: 8 x 8 maps, four images per tile, four slices (the reduce applies the row)
    + [("s8_4", "bf16", (8, 256, 8, 8, 160), 5, 8, 4)]
)
_S8_1 = ("s8_1", "bf16", (16, 64, 16, 8, 1280), 5, 8, 1)                     # conv3x3_s8_kernel<1>: section b covers its geometries


def _k3_case(dtype, shape, **kw):
    B, Cin, H, W, Cout = shape
    return _conv_case(B, Cin, H, W, Cout, 3, 1, False, True, True, seed=sum(shape) + 3, storage=dtype, wide=dtype == "f32", **kw)


# ======================================================================================================================
# a. the time-embedding row on every kernel the planner can give a 3x3 convolution that carries one
# ======================================================================================================================
@pytest.mark.parametrize("kernel,dtype,shape,tile,tw,splitk", _params(_K3))
def test_rowbias_on_every_kernel(gpu, report, knobs, kernel, dtype, shape, tile, tw, splitk):
    """y = conv + bias + rowbias[sample] + residual.  The row differs between any two samples of a tile in every column
    (exact_operands.rowbias_rows), so a row taken from the wrong sample fails every output of that sample."""
    _force(knobs, kernel, tile, splitk)
    for carrier in ((False, True) if shape[1] >= 128 else (False,)):
        c = _k3_case(dtype, shape, rowbias=True, carrier=carrier)
        _counts()
        got = _conv(gpu, c, dtype=dtype)
        pc, plan = _counts(), T._last_plan()
        _assert_kernel(kernel, pc, plan, tile, splitk, tw)
        X.assert_bit_exact(f"rowbias {kernel} {shape} [{dtype}] sk{splitk}{' +carrier' if carrier else ''}", got, c["ref"], plan, report)


# ======================================================================================================================
# b. the small-map kernel in one K slice: every tile geometry, with and without the row
# ======================================================================================================================
_S8_MAPS = [   # H, W, B: what a 256-row tile holds
    (16, 8, 16),     # two images
    (8, 16, 16),     # two images
    (4, 16, 32),     # four images
    (32, 8, 8),      # one image
    (64, 8, 4),      # half an image
    (32, 16, 4),     # half an image
]


def _s8_slices(B, Cin, H, W, N):
    """af_conv_s8_slices (csrc/af_conv_s8.hip) restated: 0 = not taken, else the K slices"""
    M = B * H * W
    if M % 256 or N % 80 or Cin % 64 or W < 8 or W > 64 or (W & (W - 1)) or (H & (H - 1)):
        return 0
    R = min(H, 256 // W)
    if 256 % (R * W) or (256 // (R * W)) * (R + 2) * (W + 2) > 448 or (H * W > 256 and H % R) or (H * W) % 32:
        return 0
    if (H, W) == (8, 8):
        return 4 if Cin % 256 == 0 else 0
    return 1 if (M // 256) * (N // 80) >= 128 else 0


_S8_CASES = [(h, w, b, cin) for (h, w, b) in _S8_MAPS for cin in (64, 192)] + [(16, 8, 16, 256)]


@pytest.mark.parametrize("H,W,B,Cin", _S8_CASES, ids=[f"{h}x{w}-B{b}-Cin{c}" for h, w, b, c in _S8_CASES])
def test_small_map_kernel_geometries(gpu, report, H, W, B, Cin):
    """conv3x3_s8_kernel<1> -> 1280 columns on rectangular maps: two and four whole images per tile (each needs its own row),
    one image, half an image (the halo's row offset).  One and three channel chunks; Cin = 256 at 16 x 8 is four chunks in ONE
    slice (only 8 x 8 maps split).  The case without the row is the same launch with rowbias null."""
    N = 1280
    assert _s8_slices(B, Cin, H, W, N) == 1, (B, Cin, H, W)
    for carrier in ((False, True) if Cin >= 128 else (False,)):
        base = X.conv_case(B, Cin, H, W, N, 3, 1, False, True, True, seed=B + Cin + H + 2 * W, carrier=carrier)
        for rowbias in (False, True):
            c = X.add_rowbias(base) if rowbias else base
            _counts()
            got = _conv(gpu, c)
            pc, plan = _counts(), T._last_plan()
            _assert_kernel("s8_1", pc, plan)
            X.assert_bit_exact(f"s8<1> {H}x{W} maps B{B} {Cin}->{N}{' +rowbias' if rowbias else ''}{' +carrier' if carrier else ''}", got,
                               c["ref"], plan, report)


# ======================================================================================================================
# c. alpha
# ======================================================================================================================
_ALPHA_CONVS = [
    ("wave4", "bf16", (2, 64, 12, 12, 64), 2, 0, 1), ("wave4", "f32", (2, 64, 12, 12, 64), 3, 0, 1), ("wave4", "f16", (2, 64, 12, 12, 64), 2, 0, 1),
    ("wave4", "bf16", (2, 128, 12, 12, 64), 2, 0, 2),                        # alpha goes into the slabs, the reduce only adds
    ("pp", "bf16", (5, 64, 12, 12, 160), 5, 0, 1), ("pp", "bf16", (5, 192, 12, 12, 160), 5, 0, 3),
    ("halo4", "bf16", (3, 64, 8, 16, 128), 0, 16, 1), ("halo4", "f32", (3, 64, 4, 32, 64), 2, 32, 1),
    ("halo8", "bf16", (3, 128, 16, 16, 160), 5, 256, 1), ("halo8", "bf16", (3, 128, 16, 16, 160), 5, 256, 2),
    ("s8_4", "bf16", (8, 256, 8, 8, 160), 5, 8, 4), _S8_1,
]


@pytest.mark.parametrize("alpha", X.ALPHAS)
@pytest.mark.parametrize("kernel,dtype,shape,tile,tw,splitk", _params(_ALPHA_CONVS))
def test_alpha_on_every_conv_kernel(gpu, report, knobs, kernel, dtype, shape, tile, tw, splitk, alpha):
    """y = alpha * conv + bias + rowbias + residual with alpha = 0.5 and -2 (exact: powers of two).  A kernel that drops alpha,
    or applies it after the bias, differs in every sample (tests/test_exact_operands_cpu.py)."""
    _force(knobs, kernel, tile, splitk)
    c = _k3_case(dtype, shape, rowbias=True, alpha=alpha, carrier=shape[1] >= 128)
    _counts()
    got = _conv(gpu, c, dtype=dtype)
    pc, plan = _counts(), T._last_plan()
    _assert_kernel(kernel, pc, plan, tile, splitk, tw)
    X.assert_bit_exact(f"alpha {alpha} {kernel} {shape} [{dtype}] sk{splitk}", got, c["ref"], plan, report)


def _query_linear(M, K, N, geglu=False, residual=False):
    from adaface_amd import _lib
    from tests import gemm_plan_cases as G
    return _lib.gemm_plan_query(*G.linear_args(G.BF16, M, K, N, geglu=geglu, residual=residual))[:2]


@pytest.mark.parametrize("alpha", X.ALPHAS)
def test_alpha_on_the_128_row_gemm(gpu, report, alpha):
    """gemm_m128_kernel without LayerNorm statistics takes alpha ([2048, 256] -> 1600: 160 tiles of 128 x 160)."""
    from tests import gemm_plan_cases as G
    M, K, N = 2048, 256, 1600
    assert _query_linear(M, K, N, residual=True)[0] == G.K_M128
    c = _linear_case(M, K, N, True, True, seed=11, carrier=True, alpha=alpha)
    _counts()
    got = _linear(gpu, c)
    pc, plan = _counts(), T._last_plan()
    assert pc["rowpanel"] == 1 and pc["splitk"] == 0, (pc, plan)     # (the 128 x 160 GEMM counts with the row-panel family; K = 256 has no row-panel kernel)
    X.assert_bit_exact(f"alpha {alpha} m128 linear [{M},{K}]->{N}", got, c["ref"], plan, report)


@pytest.mark.parametrize("alpha", X.ALPHAS)
@pytest.mark.parametrize("kernel,M,K,N", [("pp", 700, 128, 192), ("rowpanel", 32868, 320, 128)])
def test_alpha_in_the_geglu_epilogues(gpu, report, knobs, kernel, M, K, N, alpha):
    """(alpha x Wv^T + bv) * gelu(alpha x Wg^T + bg) on the ping-pong 256 x 128 tile and on the row-panel GEGLU kernel (kind 1,
    ragged M): the value probe -- zero gate rows, gate bias 8 / 16 / 32, where every GELU form returns its argument to 1.5e-5."""
    if kernel == "pp":
        knobs("gemm_pp_minfill", 0)
        knobs("geglu_rowpanel", 0)
    c = X.geglu_value_probe(M, K, N, seed=M + K + N, alpha=alpha)
    _counts()
    got = _linear(gpu, c, geglu=True, alpha=alpha)
    pc, plan = _counts(), T._last_plan()
    assert (plan[0] == 4 and plan[2] == 0 and pc["rowpanel"] == 0) if kernel == "pp" else pc["rowpanel"] == 1, (plan, pc)
    X.assert_bit_exact(f"alpha {alpha} geglu value probe {kernel} [{M},{K}]->{N}", got, c["ref"], plan, report)


# M, K, N, the row-panel kind alpha = 1 gets, knobs
_ROWPANEL_ALPHA1 = [
    (32768, 320, 320, 2, ()), (4096, 1280, 1280, 3, (("geglu_rowpanel", 4), ("gemm_m128", 0))), (16384, 640, 1920, 5, (("geglu_rowpanel", 4), ("gemm_m128", 0))),
]


@pytest.mark.parametrize("M,K,N,kind,kn", _ROWPANEL_ALPHA1, ids=[f"kind{c[3]}" for c in _ROWPANEL_ALPHA1])
def test_rowpanel_kernels_without_alpha_are_not_planned_for_it(gpu, report, knobs, M, K, N, kind, kn):
    """The plain row-panel kernels (kinds 2, 3, 5) have no alpha in their epilogue and rowpanel_kind demands alpha == 1: with
    alpha = 0.5 / -2 the plan names a tiled kernel and the result is exact; with alpha = 1 the same shape IS a row-panel launch."""
    from tests import gemm_plan_cases as G
    for k, v in kn:
        knobs(k, v)
    assert _query_linear(M, K, N) == (G.K_ROWPANEL, kind)
    alpha = X.ALPHAS[kind % 2]
    c = X.linear_case(M, K, N, True, False, seed=M + N + kind, alpha=alpha)
    _counts()
    got = _linear(gpu, c)
    pc, plan = _counts(), T._last_plan()
    assert pc["rowpanel"] == 0 and plan[0] in (4, 5), (plan, pc)
    X.assert_bit_exact(f"alpha {alpha} linear [{M},{K}]->{N} off row-panel kind {kind}", got, c["ref"], plan, report)


# ======================================================================================================================
# d. bottom / right padding: 3x3, stride 2, pad 0 on even maps
# ======================================================================================================================
_PAD0 = (
    [("wave4", dt, (2, 128, 16, 16, 128), 0) for dt in ("bf16", "f32", "f16")]
    + [("wave4", dt, (3, 128, 12, 20, 256), 1) for dt in ("bf16", "f32", "f16")]
    + [("wave4", "bf16", (2, 128, 12, 20, 128), 3), ("wave4", "f32", (2, 128, 16, 16, 256), 2)]
    + [("pp", "bf16", (8, 128, 16, 16, 128), 4), ("pp", "bf16", (9, 128, 12, 20, 256), 4), ("pp", "bf16", (8, 128, 16, 16, 256), 4),
       ("pp", "bf16", (9, 128, 12, 20, 128), 4)]
)


@pytest.mark.parametrize("kernel,dtype,shape,tile", _params(_PAD0))
def test_bottom_right_padding(gpu, report, knobs, kernel, dtype, shape, tile):
    """The VAE encoder's Downsample: F.pad(x, (0, 1, 0, 1)) + 3x3 / stride 2 / pad 0, i.e. the gather's last row and column of
    taps read zeros and its first read the map.  Symmetric padding differs in most outputs of every sample."""
    B, Cin, H, W, Cout = shape
    _force(knobs, kernel, tile, 1)
    for carrier in (False, True):
        c = _conv_case(B, Cin, H, W, Cout, 3, 2, False, True, True, seed=sum(shape) + 4, storage=dtype, wide=dtype == "f32", carrier=carrier,
                       rowbias=True, pad=0)
        assert tuple(c["ref"].shape) == (B, Cout, H // 2, W // 2)
        _counts()
        got = _conv(gpu, c, stride=2, dtype=dtype)
        pc, plan = _counts(), T._last_plan()
        _assert_kernel(kernel, pc, plan, tile, 1, 0)
        X.assert_bit_exact(f"pad0 {kernel} {shape} [{dtype}]{' +carrier' if carrier else ''}", got, c["ref"], plan, report)


# ======================================================================================================================
# e. wide rows: ldc / ldo / ldr / ldrb = channels + 8 or + 64
# ======================================================================================================================
def _assert_slack_untouched(name, slack, rows, ld_slack):
    from adaface_amd import ops
    assert tuple(slack.shape) == (rows, ld_slack), (name, tuple(slack.shape))
    bad = (slack != ops.OUTPUT_SENTINEL).nonzero()
    assert bad.numel() == 0, f"{name}: {bad.shape[0]} slack elements of the output rows were written; first (row, slack column): {bad[:8].tolist()}"


# one 3x3 case per kernel of section a (the four-wave kernels in every storage type: their row stores differ in width)
_WIDE_CONVS = [r for r in _K3 if r[2] in ((5, 64, 12, 12, 64), (5, 128, 12, 12, 64), (5, 64, 12, 12, 160), (5, 192, 12, 12, 160),
                                          (3, 64, 8, 16, 128), (3, 128, 16, 16, 160), (8, 256, 8, 8, 160))] + [_S8_1]


@pytest.mark.parametrize("ld_slack", [8, 64])
@pytest.mark.parametrize("kernel,dtype,shape,tile,tw,splitk", _params(_WIDE_CONVS))
def test_wide_rows_conv(gpu, report, knobs, kernel, dtype, shape, tile, tw, splitk, ld_slack):
    """Source, residual, bias row and output with ld_slack extra elements per row: NaN in the operands' slack must not reach the
    result, the sentinel in the output's slack must survive (16-byte row stores and buffer stores are what could overrun), and
    the plan is the kernel the same case gets with ld_slack = 0 (test_rowbias_on_every_kernel)."""
    _force(knobs, kernel, tile, splitk)
    c = _k3_case(dtype, shape, rowbias=True, carrier=False)
    _counts()
    got, slack = _conv(gpu, c, dtype=dtype, ld_slack=ld_slack)
    pc, plan = _counts(), T._last_plan()
    _assert_kernel(kernel, pc, plan, tile, splitk, tw)
    name = f"wide rows +{ld_slack} {kernel} {shape} [{dtype}] sk{splitk}"
    X.assert_bit_exact(name, got, c["ref"], plan, report)
    _assert_slack_untouched(name, slack, c["ref"].numel() // c["ref"].shape[1], ld_slack)


@pytest.mark.parametrize("ld_slack", [8, 64])
@pytest.mark.parametrize("kernel,M,K,N", [("rowpanel", 32768, 320, 320), ("m128", 2048, 256, 1600), ("pp", 1000, 128, 160)])
def test_wide_rows_linear(gpu, report, knobs, kernel, M, K, N, ld_slack):
    """The same for a linear on the plain row-panel kernel (kind 2), the 128 x 160 GEMM and the plain ping-pong kernel (ragged
    M = 1000), bias and residual set.  Every planner rule on pitches is a multiple-of-8 / multiple-of-4 rule, which + 8 and
    + 64 keep: the kernel must be the one ld_slack = 0 gets."""
    from tests import gemm_plan_cases as G
    if kernel == "pp":
        knobs("gemm_pp_minfill", 0)
    want = {"rowpanel": (G.K_ROWPANEL, 2), "m128": (G.K_M128, 0), "pp": (G.K_PP, 0)}[kernel]
    assert _query_linear(M, K, N, residual=True) == want
    c = _linear_case(M, K, N, True, True, seed=M + K + N + 2, carrier=True)
    _counts()
    got, slack = _linear(gpu, c, ld_slack=ld_slack)
    pc, plan = _counts(), T._last_plan()
    assert pc["rowpanel"] == (0 if kernel == "pp" else 1) and pc["splitk"] == 0 and plan[2] == 0 and (kernel != "pp" or plan[0] == 5), (plan, pc)
    name = f"wide rows +{ld_slack} {kernel} linear [{M},{K}]->{N}"
    X.assert_bit_exact(name, got, c["ref"], plan, report)
    _assert_slack_untouched(name, slack, M, ld_slack)


# ======================================================================================================================
# f. Gaussian operands: the non-integer row's rounding, at the project's own bars
# ======================================================================================================================
def _round(t, dtype):
    return t.to(torch.bfloat16).float() if dtype == "bf16" else t.to(torch.float16).float() if dtype == "f16" else t


def _cmp(report, name, got, ref, dtype):
    if dtype != "f16":
        return T._cmp(report, name, got, ref, dtype)
    ref = ref.float()
    scale = ref.abs().max().item() + 1e-12                      # (tests/test_fp16_gpu.py: F16_OP_TOL of max|ref|)
    err = (got.detach().float().cpu() - ref).abs().max().item() / scale
    report(f"{name}[f16]", err * scale, scale, T16.F16_OP_TOL * scale)
    assert math.isfinite(err) and err <= T16.F16_OP_TOL, f"{name}[f16]: max abs err {err:.3e} of max|ref| > {T16.F16_OP_TOL:.3e}"


_GAUSS = [(k, dt, sh, tile, tw, sk, 1, None) for (k, dt, sh, tile, tw, sk) in _K3 + [_S8_1]] + \
         [(k, dt, sh, tile, 0, 1, 2, 0) for (k, dt, sh, tile) in _PAD0]


@pytest.mark.parametrize("kernel,dtype,shape,tile,tw,splitk,stride,pad", _params(_GAUSS))
def test_gaussian_operands(gpu, report, knobs, kernel, dtype, shape, tile, tw, splitk, stride, pad):
    """Every kernel of sections a and d on Gaussian operands with a Gaussian row, against the fp64 reference of the rounded
    operands, at TOL[dtype] of tests/test_ops_gpu.py (fp16: F16_OP_TOL of tests/test_fp16_gpu.py)."""
    from adaface_amd import ops
    B, Cin, H, W, Cout = shape
    _force(knobs, kernel, tile, splitk)
    g = torch.Generator().manual_seed(sum(shape) + stride)
    x = _round(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = _round(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin), dtype)
    b = torch.randn(Cout, generator=g) * 0.1
    rb = _round(torch.randn(B, Cout, generator=g), dtype)
    ho, wo = X.out_hw(H, W, 3, stride, False, pad)
    r = _round(torch.randn(B, Cout, ho, wo, generator=g), dtype)
    ref = X.fp64_ref_conv(x, w, b, r, stride, False, rb, 1.0, pad)
    _counts()
    got = ops.conv2d(x.to(gpu), w.to(gpu), b.to(gpu), stride=stride, padding=pad, residual=r.to(gpu), dtype=dtype, rowbias=rb.to(gpu))
    pc, plan = _counts(), T._last_plan()
    _assert_kernel(kernel, pc, plan, tile, splitk, tw)
    _cmp(report, f"gaussian rowbias {kernel} {shape} s{stride} pad{pad} sk{splitk}", got, ref, dtype)
