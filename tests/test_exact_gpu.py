"""Bit-exact tests of every GEMM / implicit-GEMM convolution kernel variant on integer operands (tests/exact_operands.py).

The other GPU tests bound a kernel at 1.5e-2 of max|reference| on Gaussian operands, or pin it bit for bit to a sibling
kernel.  The first lets one missing product at one output pass (tests/test_exact_operands_cpu.py asserts that); the second
pins a variant to whatever it shares with its sibling.  Here the operands are small integers: every product and every
partial sum of any summation order is an integer below 2^24, exact in an fp32 accumulator, and the result is exact in the
storage type -- so the fp64 CPU reference is what a correct kernel returns and every comparison is torch.equal over every
output element.  No tolerance, no masked element, no skipped case.

Every case asserts which kernel ran (af_last_gemm_plan / the launch counters), as the per-kernel tests of test_ops_gpu.py and
test_fp8_gpu.py do; an exact answer from another kernel does not count.  The shapes are those tests' own parameter lists,
read from their parametrize marks, so the planner conditions are the ones already known to hold.

The cancelling carrier (exact_operands.add_carrier) is a second launch of every case with >= 128 input channels: partial
sums pass through +-2304 (3x3) or +-2048 (one tap) between the first and the last 64-channel chunk, so an accumulator, an LDS
transposition tile or a split-K slab narrower than fp32 loses the small terms and the case fails.

The f32 cases carry about one activation in 64 of +-4097 (13 significant bits): a path that narrows f32 operands to bf16 or
to a 10-bit-mantissa MFMA format fails them.
"""
import functools

import pytest
import torch

import exact_operands as X
import test_fp8_gpu as T8
import test_ops_gpu as T

pytestmark = pytest.mark.gpu


def _cases(fn, first_arg):
    """The argvalues of the parametrize mark of an existing test whose argnames start with `first_arg`."""
    for m in fn.pytestmark:
        if m.name == "parametrize" and str(m.args[0]).startswith(first_arg):
            return [tuple(v) for v in m.args[1]]
    raise LookupError((fn.__name__, first_arg))


def _carriers(cases, k_index):
    """Every case once, and once more with the cancelling carrier where it has >= 128 input channels / K columns."""
    out = []
    for c in cases:
        out.append(pytest.param(*c, False, id="-".join(str(int(v) if isinstance(v, bool) else v) for v in c)))
        if c[k_index] >= 128:
            out.append(pytest.param(*c, True, id="-".join(str(int(v) if isinstance(v, bool) else v) for v in c) + "-carrier"))
    return out


def _dev(t, gpu):
    return None if t is None else t.to(gpu)


def _conv(gpu, c, stride=1, up=False, dtype="bf16"):
    from adaface_amd import ops
    return ops.conv2d(c["x"].to(gpu), c["w"].to(gpu), _dev(c["b"], gpu), stride=stride, upsample=up, residual=_dev(c["r"], gpu),
                      dtype=dtype)


def _linear(gpu, c, dtype="bf16", geglu=False):
    from adaface_amd import ops
    return ops.linear(c["x"].to(gpu), c["w"].to(gpu), _dev(c["b"], gpu), _dev(c.get("r"), gpu), geglu=geglu, dtype=dtype)


def _counts(reset=True):
    from adaface_amd import _lib
    return _lib.plan_counts(reset=reset)


def _tag(carrier):
    return " +carrier" if carrier else ""


# ======================================================================================================================
# A. named bf16 kernels, convolutions
# ======================================================================================================================
@pytest.mark.parametrize("B,Cin,H,W,Cout,ks,stride,up,bias,res,splitk,carrier", _carriers(_cases(T.test_conv2d_pingpong, "B,Cin"), 1))
def test_exact_conv_pingpong(gpu, report, knobs, B, Cin, H, W, Cout, ks, stride, up, bias, res, splitk, carrier):
    """conv_gemm_pp_kernel (eight waves, 256 x {160, 128} tiles; gather, plain 1x1, upsampled, strided, split-K 3 with the reduce
    pass, KT = 1 and 2) forced as test_conv2d_pingpong forces it.  Exact: integer operands, fp32 accumulation below 2^24,
    bf16-representable results."""
    knobs("gemm_pp_minfill", 0)
    knobs("conv_halo8", 0)
    if splitk > 1:
        knobs("gemm_splitk", splitk)
    c = X.conv_case(B, Cin, H, W, Cout, ks, stride, up, bias, res, seed=Cin + Cout + H + ks + 1, carrier=carrier)
    _counts()
    got = _conv(gpu, c, stride, up)
    pc, (tile, sk, halo) = _counts(), T._last_plan()
    assert tile in (4, 5) and halo == 0 and (splitk == 1 or sk == splitk) and pc["halo8"] == 0 and pc["up_phase4"] == 0, (tile, sk, halo, pc)
    assert pc["splitk"] == (1 if sk > 1 else 0), pc
    X.assert_bit_exact(f"exact pp conv{ks}x{ks} {Cin}->{Cout}@{H}x{W} B{B} s{stride} up{int(up)} sk{splitk}{_tag(carrier)}", got, c["ref"],
                       (tile, sk, halo), report)


@pytest.mark.parametrize("B,Cin,H,W,Cout,bias,res,splitk,carrier", _carriers(_cases(T.test_conv2d_halo8, "B,Cin"), 1))
def test_exact_conv_halo8(gpu, report, knobs, B, Cin, H, W, Cout, bias, res, splitk, carrier):
    """conv3x3_halo8_kernel (eight waves, image rows + halo resident in LDS; one, two, five, ten, fifteen chunks, K sliced in
    two and three) against the truth instead of against the gathering kernel it shares its K walk and epilogue with."""
    knobs("gemm_pp_minfill", 0)
    knobs("gemm_splitk", splitk)
    c = X.conv_case(B, Cin, H, W, Cout, 3, 1, False, bias, res, seed=Cin + Cout + H + 11, carrier=carrier)
    _counts()
    got = _conv(gpu, c)
    pc, (tile, sk, halo) = _counts(), T._last_plan()
    assert pc["halo8"] == 1 and tile == 5 and halo == 256 and sk == splitk, (pc, tile, sk, halo)
    X.assert_bit_exact(f"exact halo8 conv3x3 {Cin}->{Cout}@{H}x{W} B{B} sk{splitk}{_tag(carrier)}", got, c["ref"], (tile, sk, halo), report)


@pytest.mark.parametrize("B,Cin,Cout,bias,res,H,carrier", _carriers(_cases(T.test_conv2d_8x8_maps, "B,Cin"), 1))
def test_exact_conv_small_maps(gpu, report, B, Cin, Cout, bias, res, H, carrier):
    """conv3x3_s8_kernel<4> (8 x 8 maps: four images per tile, four K slices summed in slice order) and <1> (16 x 16 maps: one
    slice, direct epilogue) on the default planner.  The deepest K of the suite (23040): keep probability 0.33."""
    c = X.conv_case(B, Cin, H, H, Cout, 3, 1, False, bias, res, seed=B + Cin + Cout, carrier=carrier)
    got = _conv(gpu, c)
    tile, sk, halo = T._last_plan()
    assert tile == 5 and halo == 8 and sk == (4 if H == 8 else 1), (tile, sk, halo)
    X.assert_bit_exact(f"exact s8 conv3x3 {H}x{H} maps {Cin}->{Cout} B{B}{_tag(carrier)}", got, c["ref"], (tile, sk, halo), report)


@pytest.mark.parametrize("B,Cin,H,W,Cout,bias,carrier", _carriers(_cases(T.test_conv2d_up_phase4, "B,Cin"), 1))
def test_exact_conv_up_phase4(gpu, report, B, Cin, H, W, Cout, bias, carrier):
    """The four-phase upsample launch.  Its phase weights are sums of at most four entries of {-1, 0, 1} (carrier: of +-128), exact
    in bf16, so the phased launch must equal interpolate + conv2d exactly (test_conv2d_up_phase4 bounds it at 2e-2)."""
    c = X.conv_case(B, Cin, H, W, Cout, 3, 1, True, bias, False, seed=B + Cin + Cout + H, carrier=carrier)
    _counts()
    got = _conv(gpu, c, 1, True)
    pc, plan = _counts(), T._last_plan()
    assert pc["up_phase4"] == 1 and plan[0] in (4, 5), (pc, plan)
    X.assert_bit_exact(f"exact up-phase4 conv3x3 {Cin}->{Cout}@{H}x{W} B{B}{_tag(carrier)}", got, c["ref"], plan, report)


# the default planner's choice for test_conv2d's shapes: (tile, K slices, halo) by dtype, in the order of that test's list (what
# af_plan_conv_gemm returns with the load-time knobs; a deliberate planner change updates this table, the assertion message
# shows the new plan)
_DEFAULT_CONV_PLANS = {
    "f32": [(2, 4, 0), (2, 1, 32), (2, 10, 0), (2, 11, 0), (0, 8, 0), (3, 1, 0), (2, 4, 0), (0, 2, 0), (0, 16, 0)],
    "bf16": [(2, 4, 0), (2, 1, 32), (2, 5, 0), (2, 5, 0), (0, 8, 0), (3, 1, 0), (2, 2, 0), (1, 1, 0), (0, 16, 0)],
}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("idx", range(9))
def test_exact_conv_default_planner(gpu, report, dtype, idx):
    """test_conv2d's nine shapes where the default planner puts them, in both storage types (f32: the four-wave kernels, wide
    +-4097 activations; bf16: whatever does not fill the chip stays on the four-wave kernels too).  The plan is pinned per
    shape, so a planner change that moves a shape to another kernel shows here and not as silently lost coverage."""
    B, Cin, H, W, Cout, ks, stride, up, bias, res = _cases(T.test_conv2d, "B,Cin")[idx]
    for carrier in ((False, True) if Cin >= 128 else (False,)):
        c = X.conv_case(B, Cin, H, W, Cout, ks, stride, up, bias, res, seed=Cin + Cout + H + ks, storage=dtype, wide=dtype == "f32",
                        carrier=carrier)
        _counts()
        got = _conv(gpu, c, stride, up, dtype)
        pc, plan = _counts(), T._last_plan()
        X.assert_bit_exact(f"exact conv{ks}x{ks} {Cin}->{Cout}@{H}x{W} B{B} s{stride} up{int(up)} [{dtype}]{_tag(carrier)}", got, c["ref"],
                           plan, report)
        assert plan == _DEFAULT_CONV_PLANS[dtype][idx], (dtype, idx, plan, pc)


@pytest.mark.parametrize("B,Cin,C,H,W", [(4, 320, 320, 64, 64), (2, 64, 128, 64, 64)])
def test_exact_conv_gn_producer_epilogue(gpu, report, knobs, B, Cin, C, H, W):
    """ops.conv_gn's first output: the convolution through the epilogue that also sums GroupNorm statistics (the direct,
    wave-private transposition of the eight-wave kernels; halo kernel at 320 channels, 256 x 128 gathering tile at 128)."""
    from adaface_amd import ops
    knobs("gemm_pp_minfill", 0)
    for carrier in ((False, True) if Cin >= 128 else (False,)):
        c = X.conv_case(B, Cin, H, W, C, 3, 1, False, True, False, seed=B + Cin + C + H, carrier=carrier)
        _counts()
        h, _ = ops.conv_gn(c["x"].to(gpu), c["w"].to(gpu), c["b"].to(gpu), torch.ones(C, device=gpu), torch.zeros(C, device=gpu))
        pc, plan = _counts(), T._last_plan()
        assert pc["gn_producer"] == 1 and plan[0] in (4, 5) and plan[1] == 1, (pc, plan)
        X.assert_bit_exact(f"exact conv3x3 + GN-statistics epilogue {Cin}->{C}@{H}x{W} B{B}{_tag(carrier)}", h, c["ref"], plan, report)


# ======================================================================================================================
# B. named bf16 kernels, linears
# ======================================================================================================================
@pytest.mark.parametrize("M,K,N,bias,res,carrier", _carriers(_cases(T.test_linear_m128_tile, "M,K"), 1))
def test_exact_linear_m128(gpu, report, M, K, N, bias, res, carrier):
    """gemm_m128_kernel (row-panel kind 6: 128 x 160 tile, both operands through an LDS-DMA ring) on the default planner, against
    the truth instead of against the kernel it replaced.  Exact: integer operands, every partial sum below 2^24, bf16-exact
    results; K = 5120 is the longest linear of the file."""
    c = X.linear_case(M, K, N, bias, res, seed=M + K + N, carrier=carrier)
    _counts()
    got = _linear(gpu, c)
    pc, plan = _counts(), T._last_plan()
    assert pc["rowpanel"] == 1 and pc["splitk"] == 0, pc
    X.assert_bit_exact(f"exact linear m128 [{M},{K}]->{N}{_tag(carrier)}", got, c["ref"], plan, report)


@pytest.mark.parametrize("M,K,N,bias,res,carrier", _carriers(_cases(T.test_plain_rowpanel, "M,K"), 1))
def test_exact_linear_rowpanel(gpu, report, knobs, M, K, N, bias, res, carrier):
    """The plain row-panel kernels: kind 2 (K = 320), kind 5 (K = 640, N >= 1920) and kind 3 (K = 1280 -> 1280), ragged
    M = 32868 / 16434 / 4196 included -- against the truth, not against the tiled kernel they share the repack and epilogue with."""
    knobs("geglu_rowpanel", 4)
    knobs("gemm_m128", 0)
    c = X.linear_case(M, K, N, bias, res, seed=M + N + 5, carrier=carrier)
    _counts()
    got = _linear(gpu, c)
    pc, plan = _counts(), T._last_plan()
    assert pc["rowpanel"] == 1, pc
    X.assert_bit_exact(f"exact row-panel linear [{M},{K}]->{N}{_tag(carrier)}", got, c["ref"], plan, report)


@pytest.mark.parametrize("M,K,N,bias,res,carrier", _carriers([c[:5] for c in _cases(T.test_linear_pingpong, "M,K") if not c[5]], 1))
def test_exact_linear_pingpong(gpu, report, knobs, M, K, N, bias, res, carrier):
    """The plain (no-gather) 256 x 160 ping-pong kernel on the non-GEGLU shapes of test_linear_pingpong (ragged M = 1000, K = 64:
    one K tile).  Exact for the same reason as the convolutions: integers, fp32 sums below 2^24, bf16-exact results."""
    knobs("gemm_pp_minfill", 0)
    c = X.linear_case(M, K, N, bias, res, seed=M + K + N + 1, carrier=carrier)
    _counts()
    got = _linear(gpu, c)
    pc, (tile, sk, halo) = _counts(), T._last_plan()
    assert tile == 5 and halo == 0 and pc["rowpanel"] == 0, (tile, sk, halo, pc)
    X.assert_bit_exact(f"exact pp linear {M}x{K}->{N}{_tag(carrier)}", got, c["ref"], (tile, sk, halo), report)


# the default planner's choice for test_linear's shapes: ((tile, K slices, halo), row-panel launches) in that test's order
_DEFAULT_LINEAR_PLANS = {
    "f32": [((2, 1, 0), 0), ((3, 1, 0), 0), ((0, 3, 0), 0), ((1, 1, 0), 0), ((0, 5, 0), 0), ((3, 1, 0), 0), ((2, 2, 0), 0), ((3, 1, 0), 0)],
    "bf16": [((2, 1, 0), 0), ((3, 1, 0), 0), ((1, 1, 0), 0), ((1, 1, 0), 0), ((3, 1, 0), 0), ((3, 1, 0), 0), ((2, 2, 0), 0), ((3, 1, 0), 0)],
}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("idx", range(8))
def test_exact_linear_default_planner(gpu, report, dtype, idx):
    """test_linear's eight shapes where the default planner puts them, both storage types (f32 with the wide activations).  Plan
    and row-panel counter pinned per shape."""
    M, K, N, bias, res = _cases(T.test_linear, "M,K")[idx]
    for carrier in ((False, True) if K >= 128 else (False,)):
        c = X.linear_case(M, K, N, bias, res, seed=M + K + N, storage=dtype, wide=dtype == "f32", carrier=carrier)
        _counts()
        got = _linear(gpu, c, dtype)
        pc, plan = _counts(), T._last_plan()
        X.assert_bit_exact(f"exact linear {M}x{K}->{N} [{dtype}]{_tag(carrier)}", got, c["ref"], plan, report)
        assert (plan, pc["rowpanel"]) == _DEFAULT_LINEAR_PLANS[dtype][idx], (dtype, idx, plan, pc)


# ======================================================================================================================
# C. fp8 operands
# ======================================================================================================================
@pytest.mark.parametrize("B,Cin,H,W,Cout,ks,stride,up,bias,res,carrier", _carriers(_cases(T8.test_conv2d_fp8_kernel, "B,Cin"), 1))
def test_exact_conv_fp8(gpu, report, knobs, B, Cin, H, W, Cout, ks, stride, up, bias, res, carrier):
    """The fp8-operand ping-pong kernel.  Operands in {-1, 0, 1}: x * 2^3 and w * 2^8 (the row scale of a row whose largest
    entry is 1) are exact in e4m3, bias and residual are integers, so quantisation changes nothing and the bf16 output equals the
    fp64 reference.  The carrier keeps this: x = 2 -> 16, and a row holding +-128 (+-1024) scales by 2^1 (2^-2), which leaves
    its +-1 entries at 2 (0.25), all e4m3 values -- asserted below with test_fp8_gpu's own _quant_x / _quant_w."""
    from adaface_amd import ops
    knobs("gemm_pp_minfill", 0)
    c = X.conv_case(B, Cin, H, W, Cout, ks, stride, up, bias, res, seed=Cin + Cout + H + ks + 7, storage="fp8", carrier=carrier)
    assert torch.equal(T8._quant_x(c["x"]), c["x"]) and torch.equal(T8._quant_w(c["w"]), c["w"])      # precondition 1 for e4m3
    _counts()
    got = ops.conv2d_fp8(c["x"].to(gpu), c["w"].to(gpu), _dev(c["b"], gpu), stride=stride, upsample=up, residual=_dev(c["r"], gpu))
    pc, plan = _counts(), T._last_plan()
    assert pc["fp8"] == 1 and plan[0] in (4, 5), (pc, plan)
    X.assert_bit_exact(f"exact fp8 conv{ks}x{ks} {Cin}->{Cout}@{H}x{W} B{B} s{stride}{_tag(carrier)}", got, c["ref"], plan, report)


# ======================================================================================================================
# D. the four-wave family, forced: conv_gemm_kernel<{bf16, float}, {128x128, 64x128, 128x64, 64x64}, DMA on / off> and
#    launch_halo<{bf16, float}, {32, 16}, {128, 64}>
# ======================================================================================================================
_conv_case = functools.lru_cache(maxsize=4)(X.conv_case)
_linear_case = functools.lru_cache(maxsize=4)(X.linear_case)

_FOURWAVE = [   # kind, shape, K slices
    ("conv", (2, 64, 32, 32, 160, 3, 2, False, True, False), 1),      # strided 3x3
    ("conv", (1, 128, 40, 24, 3, 3, 1, False, True, False), 1),       # ragged M and N = 3 (padded to 4)
    ("linear", (333, 128, 4, True, False), 1),                        # ragged linear
    ("linear", (200, 64, 192, True, False), 1),                       # short K: one (bf16) or two (f32) K tiles
    ("conv", (2, 1280, 8, 8, 1280, 3, 1, False, True, True), 1),      # deep K, one slice
    ("conv", (2, 1280, 8, 8, 1280, 3, 1, False, True, True), 3),      # deep K in three slices + splitk_reduce_kernel
]


def _fourwave_run(gpu, report, knobs, dtype, kind, shape, splitk, tile, dma, groupm=None):
    knobs("gemm_pp", 0)
    knobs("conv_halo", 0)
    knobs("geglu_rowpanel", 0)
    knobs("gemm_m128", 0)
    knobs("gemm_tile", tile)
    knobs("gemm_dma", dma)
    knobs("gemm_splitk", splitk)
    if groupm is not None:
        knobs("gemm_groupm", groupm)
    kdim = shape[1]
    for carrier in ((False, True) if kdim >= 128 else (False,)):
        if kind == "conv":
            B, Cin, H, W, Cout, ks, stride, up, bias, res = shape
            c = _conv_case(*shape, seed=sum(int(v) for v in shape), storage=dtype, wide=dtype == "f32", carrier=carrier)
            _counts()
            got = _conv(gpu, c, stride, up, dtype)
        else:
            c = _linear_case(*shape, seed=sum(int(v) for v in shape), storage=dtype, wide=dtype == "f32", carrier=carrier)
            _counts()
            got = _linear(gpu, c, dtype)
        pc, plan = _counts(), T._last_plan()
        assert plan == (tile, splitk, 0) and pc[f"tile{tile}"] == 1 and pc["rowpanel"] == 0 and pc["halo"] == 0 and \
            pc["splitk"] == (1 if splitk > 1 else 0), (plan, pc)
        X.assert_bit_exact(f"exact four-wave {kind} {shape} [{dtype}] tile{tile} dma{dma} sk{splitk} gm{groupm}{_tag(carrier)}", got,
                           c["ref"], plan, report)


def _fourwave_matrix():
    """Every instantiation once: storage type x tile x staging, the six cases dealt round-robin (shifted by three for bf16) so
    that each storage type meets every case, the three-slice one included.  (The full 16 x 6 matrix was thinned to this: the
    file's wall time is dominated by the fp64 references of sections A-C and E, which are not thinned.)"""
    out = []
    for di, dtype in enumerate(("f32", "bf16")):
        for tile in range(4):
            for dma in (0, 1):
                kind, shape, splitk = _FOURWAVE[(2 * tile + dma + 3 * di) % len(_FOURWAVE)]
                out.append(pytest.param(dtype, tile, dma, kind, shape, splitk,
                                        id=f"{dtype}-tile{tile}-dma{dma}-{kind}-" + "x".join(str(int(v)) for v in shape) + f"-sk{splitk}"))
    return out


@pytest.mark.parametrize("dtype,tile,dma,kind,shape,splitk", _fourwave_matrix())
def test_exact_fourwave_gemm(gpu, report, knobs, dtype, tile, dma, kind, shape, splitk):
    """conv_gemm_kernel: all sixteen instantiations (storage type x tile x LDS-DMA or register staging), each once, over a strided
    3x3, a ragged convolution with three output channels, a ragged and a short-K linear and a deep-K convolution in one and in
    three K slices (splitk_reduce_kernel for both storage types).  No other test forces these kernels, yet the whole f32 parity
    mode and every bf16 launch that does not fill the chip run on them."""
    _fourwave_run(gpu, report, knobs, dtype, kind, shape, splitk, tile, dma)


@pytest.mark.parametrize("groupm", [1, 4])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_exact_fourwave_gemm_grouped_tile_order(gpu, report, knobs, dtype, groupm):
    """The grouped tile order (gemm_groupm 1 and 4) on the 64 x 64 tile of the strided 3x3: 32 x 3 tiles, so groups of four rows
    of tiles are whole and the order really changes."""
    _fourwave_run(gpu, report, knobs, dtype, "conv", _FOURWAVE[0][1], 1, 3, 0, groupm)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tile,shape,tw", [
    (0, (2, 320, 32, 32, 320, 3, 1, False, True, True), 32), (2, (2, 320, 32, 32, 320, 3, 1, False, True, True), 32),
    (0, (1, 64, 24, 16, 128, 3, 1, False, True, False), 16), (2, (1, 64, 24, 16, 128, 3, 1, False, True, False), 16),
    (2, (1, 64, 24, 16, 4, 3, 1, False, True, False), 16),
])
def test_exact_fourwave_halo(gpu, report, knobs, tile, shape, tw, dtype):
    """conv3x3_halo_kernel (four waves, 128-pixel patches with their halo in LDS): patch width 32 and 16, 128 and 64 columns
    (gemm_tile 0 / 2), both storage types -- the eight launch_halo instantiations -- and four output channels on the 64-column one.  splitk_target 1
    keeps the cost model from slicing K, which would drop the halo plan."""
    knobs("gemm_pp", 0)
    knobs("splitk_target", 1)
    knobs("gemm_tile", tile)
    B, Cin, H, W, Cout, ks, stride, up, bias, res = shape
    for carrier in ((False, True) if Cin >= 128 else (False,)):
        c = _conv_case(*shape, seed=sum(int(v) for v in shape), storage=dtype, wide=dtype == "f32", carrier=carrier)
        _counts()
        got = _conv(gpu, c, dtype=dtype)
        pc, plan = _counts(), T._last_plan()
        assert plan[2] in (16, 32) and plan == (tile, 1, tw) and pc["halo"] == 1 and pc["halo8"] == 0, (plan, pc)
        X.assert_bit_exact(f"exact four-wave halo{tw} {Cin}->{Cout}@{H}x{W} B{B} [{dtype}] BN{128 if tile == 0 else 64}{_tag(carrier)}", got,
                           c["ref"], plan, report)


@pytest.mark.parametrize("knob,expect", [(1, (3, 1, 0)), (0, (0, 2, 0))])
def test_exact_small_m_tile64_plan(gpu, report, knobs, knob, expect):
    """[1024, 1280] -> 1280 in bf16: the small_m_tile64 plan (64 x 64 tiles in ONE K slice) and, with the knob off, what the cost
    model picks instead (128 x 128 tiles over two K slices + reduce)."""
    knobs("gemm_pp", 0)
    knobs("geglu_rowpanel", 0)
    knobs("gemm_m128", 0)
    knobs("small_m_tile64", knob)
    for carrier in (False, True):
        c = _linear_case(1024, 1280, 1280, True, True, seed=11, carrier=carrier)
        _counts()
        got = _linear(gpu, c)
        pc, plan = _counts(), T._last_plan()
        assert plan == expect and pc["rowpanel"] == 0, (plan, pc)
        X.assert_bit_exact(f"exact linear 1024x1280->1280 small_m_tile64={knob}{_tag(carrier)}", got, c["ref"], plan, report)


# ======================================================================================================================
# E. GEGLU: two probes that need no tolerance (exact_operands.geglu_value_probe / geglu_gate_probe)
# ======================================================================================================================
_GEGLU = (
    [("pp", (M, K, N), "bf16") for (M, K, N, b, r, gg) in _cases(T.test_linear_pingpong, "M,K") if gg]
    + [("rowpanel", (M, K, N), "bf16") for (M, K, N, b) in _cases(T.test_geglu_rowpanel, "M,K")]
    + [("fourwave", (M, d, 4 * d), dt) for (M, d) in _cases(T.test_geglu, "M,d") for dt in ("bf16", "f32")]
)


@pytest.mark.parametrize("probe", ["value", "gate"])
@pytest.mark.parametrize("kernel,shape,dtype", _GEGLU)
def test_exact_geglu_probes(gpu, report, knobs, kernel, shape, dtype, probe):
    """GEGLU on the ping-pong 256 x 128 tile (tile 4), the row-panel GEGLU kernels (kinds 1 and 4, K = 320 / 640, ragged M) and
    the four-wave kernel with 128 columns in bf16 and f32.  gelu is not exact, but for a gate >= 8 every form the kernels use
    returns g (1 + d), |d| <= 1.5e-5 (the f32 form: g), far inside half a bf16 ulp -- tests/test_exact_operands_cpu.py derives
    that from the formulas.  Value probe: zero gate rows, gate bias 8 / 16 / 32 -> (x Wv^T + bv) * g_n.  Gate probe: zero value
    rows, value bias +-1 / +-2, non-negative integer gate operands -> v_n * g with every g an integer >= 8."""
    M, K, N = shape
    if kernel == "pp":
        knobs("gemm_pp_minfill", 0)
    elif kernel == "fourwave":
        knobs("gemm_pp", 0)
        knobs("geglu_rowpanel", 0)
    build = X.geglu_value_probe if probe == "value" else X.geglu_gate_probe
    kw = {"wide": True} if (probe == "value" and dtype == "f32") else {}
    c = build(M, K, N, seed=M + K + N, storage=dtype, **kw)
    _counts()
    got = _linear(gpu, c, dtype, geglu=True)
    pc, plan = _counts(), T._last_plan()
    if kernel == "pp":
        assert plan[0] == 4 and plan[2] == 0 and pc["rowpanel"] == 0, (plan, pc)
    elif kernel == "rowpanel":
        assert pc["rowpanel"] == 1, (plan, pc)
    else:
        assert plan[0] in (0, 1) and plan[1] == 1 and plan[2] == 0 and pc["rowpanel"] == 0, (plan, pc)
    X.assert_bit_exact(f"exact geglu {probe} probe {kernel} [{M},{K}]->{N} [{dtype}]", got, c["ref"], plan, report)
