"""GPU parity of every hot-path operator against the torch fp32 CPU op the reference calls.

Each HIP kernel is reached through the C ABI (af_op_*).  Two storage/MFMA modes:
  f32  : parity mode (f32 MFMA, exact fp32 products) — tolerance 2e-4 of the output scale
  bf16 : throughput mode (bf16 MFMA, fp32 accumulate)  — tolerance 1.5e-2 of the output scale (observed <= 7.7e-3)
Tolerances are relative to max|reference| and are stated here, not tuned per case.
"""
import math

import numpy as np

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-4, "bf16": 1.5e-2}   # bf16: largest observed over all cases 7.7e-3 (gpurun_out/parity_report.txt)


def _cmp(report, name, got, ref, dtype, tol_scale=1.0):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-12
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs().max().item() if finite else float("inf")
    tol = TOL[dtype] * tol_scale
    report(f"{name}[{dtype}]", err, scale, tol * scale)
    assert finite, f"{name}[{dtype}]: non-finite output"
    assert err <= tol * scale, f"{name}[{dtype}]: max abs err {err:.3e} > {tol:.1e} * {scale:.3e}"


def _q(t, dtype):
    """Round inputs to the kernel's storage type so the comparison isolates kernel arithmetic."""
    return t.to(torch.bfloat16).float() if dtype == "bf16" else t


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,C,H,W,eps,silu", [
    (2, 320, 64, 64, 1e-5, True), (2, 640, 32, 32, 1e-5, True), (1, 960, 64, 64, 1e-5, True),
    (2, 1280, 8, 8, 1e-6, False), (1, 2560, 16, 16, 1e-5, True), (1, 1920, 32, 32, 1e-5, True),
    (1, 128, 96, 80, 1e-6, True), (3, 64, 4, 4, 1e-6, False), (1, 512, 128, 128, 1e-6, True),
])
def test_groupnorm(gpu, report, dtype, B, C, H, W, eps, silu):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(C + H)
    x = _q(torch.randn(B, C, H, W, generator=g) * 1.7 + 0.4, dtype)
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    ref = F.group_norm(x, 32, w, b, eps)
    if silu:
        ref = F.silu(ref)
    got = ops.group_norm(x.to(gpu), w.to(gpu), b.to(gpu), eps=eps, silu=silu, dtype=dtype)
    _cmp(report, f"groupnorm C{C} {H}x{W}", got, ref, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows,C", [(4096, 320), (1024, 640), (256, 1280), (7, 64), (130, 1280)])
def test_layernorm(gpu, report, dtype, rows, C):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(rows + C)
    x = _q(torch.randn(rows, C, generator=g) * 2.0 + 0.5, dtype)
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    ref = F.layer_norm(x, (C,), w, b, 1e-5)
    got = ops.layer_norm(x.to(gpu), w.to(gpu), b.to(gpu), dtype=dtype)
    _cmp(report, f"layernorm {rows}x{C}", got, ref, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M,K,N,bias,res", [
    (4096, 320, 320, True, True), (1024, 640, 640, False, False), (77 * 2, 768, 1280, False, False),
    (2, 320, 1280, True, False), (256, 1280, 1280, True, True), (200, 64, 192, True, False),
    (4096, 1280, 320, True, True), (333, 128, 4, True, False),
])
def test_linear(gpu, report, dtype, M, K, N, bias, res):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(M + K + N)
    x = _q(torch.randn(M, K, generator=g), dtype)
    w = _q(torch.randn(N, K, generator=g) / math.sqrt(K), dtype)
    b = torch.randn(N, generator=g) * 0.1 if bias else None
    r = _q(torch.randn(M, N, generator=g), dtype) if res else None
    ref = F.linear(x, w, b)
    if res:
        ref = ref + r
    got = ops.linear(x.to(gpu), w.to(gpu), None if b is None else b.to(gpu), None if r is None else r.to(gpu),
                     dtype=dtype)
    _cmp(report, f"linear {M}x{K}->{N}", got, ref, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M,d", [(4096, 320), (1024, 640), (256, 1280), (70, 64)])
def test_geglu(gpu, report, dtype, M, d):
    """FeedForward's GEGLU projection (attention.py:32-45): Linear(d, 8d) -> value * gelu(gate)."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(M + d)
    x = _q(torch.randn(M, d, generator=g), dtype)
    w = _q(torch.randn(8 * d, d, generator=g) / math.sqrt(d), dtype)
    b = torch.randn(8 * d, generator=g) * 0.1
    val, gate = F.linear(x, w, b).chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    got = ops.linear(x.to(gpu), w.to(gpu), b.to(gpu), geglu=True, dtype=dtype)
    _cmp(report, f"geglu {M}x{d}", got, ref, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,Cin,H,W,Cout,ks,stride,up,bias,res", [
    (2, 320, 32, 32, 320, 3, 1, False, True, True),     # ResBlock conv
    (1, 4, 64, 64, 320, 3, 1, False, True, False),      # input_blocks.0
    (1, 320, 64, 64, 4, 3, 1, False, True, False),      # out conv
    (2, 320, 32, 32, 320, 3, 2, False, True, False),    # Downsample
    (1, 640, 16, 16, 640, 3, 1, True, True, False),     # Upsample (nearest 2x folded in)
    (2, 960, 16, 16, 640, 1, 1, False, True, False),    # skip_connection 1x1
    (1, 128, 40, 24, 3, 3, 1, False, True, False),      # VAE conv_out, ragged M
    (1, 64, 8, 8, 128, 3, 1, False, False, False),      # tiny-config conv
    (2, 1280, 8, 8, 1280, 3, 1, False, True, True),     # deep-K small-M
])
def test_conv2d(gpu, report, dtype, B, Cin, H, W, Cout, ks, stride, up, bias, res):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(Cin + Cout + H + ks)
    x = _q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = _q(torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks), dtype)
    b = torch.randn(Cout, generator=g) * 0.1 if bias else None
    xi = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
    ref = F.conv2d(xi, w, b, stride=stride, padding=ks // 2)
    r = _q(torch.randn(ref.shape, generator=g), dtype) if res else None
    if res:
        ref = ref + r
    got = ops.conv2d(x.to(gpu), w.to(gpu), None if b is None else b.to(gpu), stride=stride, upsample=up,
                     residual=None if r is None else r.to(gpu), dtype=dtype)
    _cmp(report, f"conv{ks}x{ks} {Cin}->{Cout}@{H}x{W} s{stride} up{int(up)}", got, ref, dtype)


def _last_plan():
    import ctypes as C
    from adaface_amd import _lib
    t, s, h = C.c_int(), C.c_int(), C.c_int()
    _lib.load().af_last_gemm_plan(C.byref(t), C.byref(s), C.byref(h))
    return t.value, s.value, h.value


# one smallest launch per AfGemmKernel value: (what runs, knob, the launch as ops.* takes it).  conv: B, Cin, H, W, Cout, ks, stride, up;
# linear: M, K, N, residual
_PLAN_QUERY_LAUNCHES = [
    ("four-wave", None, "bf16", "linear", (333, 128, 4, False)),
    ("four-wave halo", None, "f32", "conv", (1, 4, 64, 64, 320, 3, 1, False)),
    ("ping-pong", ("gemm_pp_minfill", 0), "bf16", "linear", (512, 64, 160, False)),
    ("eight-wave halo", ("gemm_pp_minfill", 0), "bf16", "conv", (1, 64, 64, 64, 160, 3, 1, False)),
    ("small-map", None, "bf16", "conv", (4, 256, 8, 8, 80, 3, 1, False)),
    ("four-phase upsample", None, "bf16", "conv", (4, 128, 16, 16, 320, 3, 1, True)),
    ("row-panel", None, "bf16", "linear", (32768, 320, 320, True)),
    ("m128", None, "bf16", "linear", (4096, 1280, 1280, False)),
    ("ping-pong fp8", ("gemm_pp_minfill", 0), "bf16", "conv_fp8", (2, 64, 32, 32, 160, 3, 2, False)),
]


@pytest.mark.parametrize("kernel,knob,dtype,op,shape", _PLAN_QUERY_LAUNCHES, ids=[c[0] for c in _PLAN_QUERY_LAUNCHES])
def test_plan_query_matches_launch(gpu, knobs, kernel, knob, dtype, op, shape):
    """af_gemm_plan_query (host only; tests/test_gemm_plan_cpu.py pins it against the golden table) describes what a real
    launch does: for one smallest shape per kernel, af_last_gemm_plan and the launch counters after the op equal what the
    query says for the same integers."""
    from adaface_amd import _lib, ops
    from tests import gemm_plan_cases as G
    want_kernel = {"four-wave": G.K_WAVE4, "four-wave halo": G.K_HALO4, "ping-pong": G.K_PP, "eight-wave halo": G.K_HALO8,
                   "small-map": G.K_S8, "four-phase upsample": G.K_UP_PHASE4, "row-panel": G.K_ROWPANEL, "m128": G.K_M128,
                   "ping-pong fp8": G.K_PP_FP8}[kernel]
    if knob:
        knobs(*knob)
    dt = {"bf16": G.BF16, "f32": G.F32}[dtype]
    g = torch.Generator().manual_seed(3)
    if op == "linear":
        M, K, N, res = shape
        args = G.linear_args(dt, M, K, N, residual=res)
        x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
        run = lambda: ops.linear(x.to(gpu), w.to(gpu), None, torch.randn(M, N, generator=g).to(gpu) if res else None, dtype=dtype)  # noqa: E731
    else:
        B, Cin, H, W, Cout, ks, stride, up = shape
        args = G.conv_fp8_args(B, Cin, H, W, Cout, ks, stride, up) if op == "conv_fp8" else G.conv_args(dt, B, Cin, H, W, Cout, ks, stride, up)
        x, w = torch.randn(B, Cin, H, W, generator=g), torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks)
        if op == "conv_fp8":
            run = lambda: ops.conv2d_fp8(x.to(gpu), w.to(gpu), None, stride=stride, upsample=up)  # noqa: E731
        else:
            run = lambda: ops.conv2d(x.to(gpu), w.to(gpu), None, stride=stride, upsample=up, dtype=dtype)  # noqa: E731
    k, rowpanel, tile, splitk, halo, _, ws_bytes = _lib.gemm_plan_query(*args)
    assert k == want_kernel and (rowpanel == 2) == (kernel == "row-panel"), (k, rowpanel)
    assert (ws_bytes > 0) == (splitk > 1)
    want = dict.fromkeys(["halo", "splitk", "ln_consumer", "ln_producer", "fp8", "halo8", "rowpanel", "up_phase4", "gn_producer"]
                         + [f"tile{i}" for i in range(6)], 0)
    if k in (G.K_PP_FP8, G.K_UP_PHASE4):
        want["fp8" if k == G.K_PP_FP8 else "up_phase4"] = 1          # (not counted under a tile)
    else:
        want["halo" if k == G.K_HALO4 else f"tile{tile}"] = 1
        want["halo8"] = int(k == G.K_HALO8)
        want["rowpanel"] = int(k in (G.K_ROWPANEL, G.K_M128))
    want["splitk"] = int(splitk > 1)
    _lib.plan_counts(reset=True)
    out = run()
    torch.cuda.synchronize()
    pc = _lib.plan_counts(reset=True)
    assert torch.isfinite(out).all()
    assert _last_plan() == (tile, splitk, halo), (_last_plan(), (tile, splitk, halo))
    assert {n: pc[n] for n in want} == want, (pc, want)


@pytest.mark.parametrize("B,Cin,H,W,Cout,ks,stride,up,bias,res,splitk", [
    (2, 320, 32, 32, 320, 3, 1, False, True, True, 1),    # gather, 2 N tiles of 160, residual
    (1, 128, 24, 24, 160, 3, 1, False, True, False, 1),   # M = 576: ragged last M tile (rows >= M read as zero)
    (2, 64, 32, 32, 160, 3, 2, False, True, False, 1),    # stride 2, K = 9 tiles of one tap each
    (1, 128, 16, 16, 320, 3, 1, True, False, True, 1),    # nearest-2x upsample folded into the gather
    (2, 960, 16, 16, 640, 1, 1, False, True, False, 1),   # 1x1: plain-GEMM variant (no gather)
    (2, 1280, 16, 16, 1280, 3, 1, False, True, True, 3),  # split-K slabs + reduce (60 tiles per slice)
    (1, 256, 32, 32, 256, 3, 1, False, True, False, 1),   # VAE width: N % 128 == 0 only -> 256x128 tile
    (2, 64, 16, 16, 160, 3, 1, False, True, False, 1),    # one K tile per tap (KT = 9)
    (2, 64, 16, 16, 160, 1, 1, False, True, False, 1),    # KT = 1: prologue-only pipeline
    (2, 128, 16, 16, 160, 1, 1, False, True, False, 1),   # KT = 2
])
def test_conv2d_pingpong(gpu, report, knobs, B, Cin, H, W, Cout, ks, stride, up, bias, res, splitk):
    """The eight-wave 256x{160,128} ping-pong kernel (conv_gemm_pp_kernel), forced regardless of grid fill."""
    from adaface_amd import ops
    knobs("gemm_pp_minfill", 0)
    knobs("conv_halo8", 0)      # the gathering kernel (the LDS-halo variant has its own test below)
    if splitk > 1:
        knobs("gemm_splitk", splitk)
    dtype = "bf16"
    g = torch.Generator().manual_seed(Cin + Cout + H + ks + 1)
    x = _q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = _q(torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks), dtype)
    b = torch.randn(Cout, generator=g) * 0.1 if bias else None
    xi = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
    ref = F.conv2d(xi, w, b, stride=stride, padding=ks // 2)
    r = _q(torch.randn(ref.shape, generator=g), dtype) if res else None
    if res:
        ref = ref + r
    got = ops.conv2d(x.to(gpu), w.to(gpu), None if b is None else b.to(gpu), stride=stride, upsample=up,
                     residual=None if r is None else r.to(gpu), dtype=dtype)
    tile, sk, halo = _last_plan()
    assert tile in (4, 5) and halo == 0 and (splitk == 1 or sk == splitk), (tile, sk, halo)  # planner may slice K itself
    _cmp(report, f"pp conv{ks}x{ks} {Cin}->{Cout}@{H}x{W} s{stride} up{int(up)} sk{splitk}", got, ref, dtype)


@pytest.mark.parametrize("B,Cin,H,W,Cout,bias", [
    (4, 128, 16, 16, 320, True),      # 1024 stored pixels per phase: the smallest the launcher takes; two N tiles of 160
    (2, 64, 32, 64, 128, False),      # non-square power-of-two map, the 256 x 128 tile (VAE widths), one channel chunk
    (16, 640, 32, 32, 640, True),     # UNet output block 8: [16, 640, 32, 32] -> 64 x 64
    (1, 192, 32, 32, 160, True),      # three channel chunks, one sample
])
def test_conv2d_up_phase4(gpu, report, knobs, B, Cin, H, W, Cout, bias):
    """Upsample (nearest 2x) + 3x3 convolution as four 2x2 phase convolutions on the stored map (ConvGemmParams::W_up4):
    against torch's interpolate + conv2d on the same bf16 operands, and against the nine-tap gathering kernel -- the two differ
    only by the bf16 rounding of the pre-summed weights (and the summation order)."""
    from adaface_amd import _lib, ops
    dtype = "bf16"
    g = torch.Generator().manual_seed(B + Cin + Cout + H)
    x = _q(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = _q(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9), dtype)
    b = torch.randn(Cout, generator=g) * 0.1 if bias else None
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    args = (x.to(gpu), w.to(gpu), None if b is None else b.to(gpu))
    _lib.plan_counts(reset=True)
    got = ops.conv2d(*args, upsample=True, dtype=dtype)
    assert _lib.plan_counts(reset=True)["up_phase4"] == 1
    _cmp(report, f"up-phase4 conv3x3 {Cin}->{Cout}@{H}x{W}->{2 * H}x{2 * W}", got, ref, dtype)
    knobs("conv_up_phase4", 0)
    nine = ops.conv2d(*args, upsample=True, dtype=dtype)
    assert _lib.plan_counts(reset=True)["up_phase4"] == 0
    scale = ref.abs().max().item()
    assert (got.cpu() - nine.cpu()).abs().max().item() <= 2e-2 * scale
    # borders: the first / last output rows and columns see the zero padding through different phases
    for sl in (np.s_[..., 0, :], np.s_[..., -1, :], np.s_[..., :, 0], np.s_[..., :, -1]):
        assert torch.allclose(got.cpu()[sl], ref[sl], atol=2e-2 * scale, rtol=0)


@pytest.mark.parametrize("B,Cin,C,H,W,res", [
    (4, 320, 320, 64, 64, False),      # ResBlock conv1 at the 64x64 level: LDS-halo kernel, 10 channels per group
    (16, 640, 640, 32, 32, True),      # conv2 + residual at 32x32: 20 channels per group
    (16, 128, 1280, 16, 16, False),    # 40 channels per group (two groups per wave), 4 slabs per sample
    (2, 64, 128, 64, 64, False),       # VAE width: the 256 x 128 tile, 4 channels per group
    (1, 128, 512, 128, 128, True),     # 256 slabs per sample: more than the apply kernel folds -> gn_finalize_kernel
])
def test_conv_gn_producer_stats(gpu, report, knobs, B, Cin, C, H, W, res):
    """GroupNorm statistics summed in the producer convolution's epilogue (ConvGemmParams::gn_stats_out): the GroupNorm of
    the convolution's stored (bf16) output against torch.group_norm of that same tensor, and bit for bit the convolution
    output against the launch without the statistics pass."""
    from adaface_amd import _lib, ops
    knobs("gemm_pp_minfill", 0)
    if H == 16:
        # (round 4: at Bf = 16 the 16 x 16 maps run on conv3x3_s8_kernel, which leaves no statistics -- their GroupNorm is the
        # single-launch small-map kernel, which needs none; the producer epilogue of the halo kernel is still what smaller batches
        # on these maps take, and is exercised here with that kernel forced)
        knobs("conv_halo8", 1)
    g = torch.Generator().manual_seed(B + Cin + C + H)
    x = _q(torch.randn(B, Cin, H, W, generator=g), "bf16")
    w = _q(torch.randn(C, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin), "bf16")
    b = torch.randn(C, generator=g) * 0.3
    r = _q(torch.randn(B, C, H, W, generator=g), "bf16") if res else None
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    _lib.plan_counts(reset=True)
    h, y = ops.conv_gn(x.to(gpu), w.to(gpu), b.to(gpu), gamma.to(gpu), beta.to(gpu), eps=1e-5, silu=True,
                       residual=None if r is None else r.to(gpu))
    assert _lib.plan_counts(reset=True)["gn_producer"] == 1
    plain = ops.conv2d(x.to(gpu), w.to(gpu), b.to(gpu), residual=None if r is None else r.to(gpu), dtype="bf16")
    assert _lib.plan_counts(reset=True)["gn_producer"] == 0
    assert torch.equal(h, plain)
    ref = F.silu(F.group_norm(h.cpu(), 32, gamma, beta, 1e-5))
    _cmp(report, f"conv3x3+GN producer stats {Cin}->{C}@{H}x{W}", y, ref, "bf16")
    ref2 = ops.group_norm(h, gamma.to(gpu), beta.to(gpu), eps=1e-5, silu=True, dtype="bf16")   # stand-alone statistics pass
    assert (y - ref2).abs().max().item() <= 2e-2 * ref.abs().max().item()


def test_conv_gn_producer_refuses_sliced_k(gpu):
    """A convolution whose plan slices K (few output tiles: the slabs are summed by the reduce kernel, not by an epilogue
    that sees whole outputs) has no statistics producer: the operator says so instead of writing partial sums of partial
    sums, and the model keeps the stand-alone statistics pass for such layers (af_conv_gn_stats_ok)."""
    from adaface_amd import ops
    from adaface_amd._lib import AfError
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1280, 8, 8, generator=g).to(gpu)
    w = (torch.randn(1280, 1280, 3, 3, generator=g) / 100).to(gpu)
    ones = torch.ones(1280, device=gpu)
    with pytest.raises(AfError):
        ops.conv_gn(x, w, None, ones, ones * 0)


@pytest.mark.parametrize("M,K,N,bias,res", [(4096, 1280, 1280, True, True), (4096, 1280, 1280, False, False), (4096, 5120, 1280, True, True),
                                            (2048, 1280, 1280, True, False), (8192, 640, 640, True, True), (4096, 256, 1600, True, False),
                                            (4096, 1280, 3840, False, False), (16384, 640, 640, True, True), (16384, 320, 640, False, False)])
def test_linear_m128_tile(gpu, report, knobs, M, K, N, bias, res):
    """gemm_m128_kernel (128 x 160 tile, both operands through an LDS-DMA ring): the few-row plain GEMMs of the 16x16 level,
    against torch and against the kernel it replaces (knob gemm_m128 = 0) on the same operands; 20 repeated launches must be
    bit-identical (the kernel's first version stored a register the next instruction had rewritten, a few launches in a hundred:
    scripts/check_isa_hazards.py)."""
    from adaface_amd import _lib, ops
    g = torch.Generator().manual_seed(M + K + N)
    x = _q(torch.randn(M, K, generator=g), "bf16")
    w = _q(torch.randn(N, K, generator=g) / math.sqrt(K), "bf16")
    b = torch.randn(N, generator=g) if bias else None
    r = _q(torch.randn(M, N, generator=g), "bf16") if res else None
    ref = torch.nn.functional.linear(x, w, b)
    if res:
        ref = ref + r
    args = (x.to(gpu), w.to(gpu), None if b is None else b.to(gpu), None if r is None else r.to(gpu))
    _lib.plan_counts(reset=True)
    got = ops.linear(*args, dtype="bf16")
    pc1 = _lib.plan_counts(reset=True)
    knobs("gemm_m128", 0)
    old = ops.linear(*args, dtype="bf16")
    pc0 = _lib.plan_counts(reset=True)
    assert pc1["rowpanel"] == 1 and pc1["splitk"] == 0, pc1          # (the m128 launch is counted with the row-panel family)
    _cmp(report, f"linear m128 [{M},{K}]->{N}", got, ref, "bf16")
    _cmp(report, f"linear m128 vs previous kernel [{M},{K}]->{N}", got, old, "bf16")
    again = ops.linear(*args, dtype="bf16")
    knobs("gemm_m128", 1)
    assert torch.equal(again, old)
    for _ in range(20):
        assert torch.equal(ops.linear(*args, dtype="bf16"), got)


@pytest.mark.parametrize("B,C,H,W,N", [(8, 320, 64, 64, 320), (9, 320, 64, 64, 960)])
def test_groupnorm_in_rowpanel_prologue(gpu, report, knobs, B, C, H, W, N):
    """SpatialTransformer.norm + proj_in with the GroupNorm applied in the row-panel GEMM's prologue (ConvGemmParams::gn_ab):
    the rows it normalises in registers are bit for bit what gn_apply_kernel would have stored, so -- the un-fused launch
    running on the same kernel -- the two outputs are IDENTICAL.  Both against torch.  (The K = 640 form of round 3 measured
    slower than the tiled kernel + the GroupNorm pass and left the product in round 4.)"""
    from adaface_amd import _lib, ops
    g = torch.Generator().manual_seed(B + C + N)
    x = _q(torch.randn(B, C, H, W, generator=g) * 1.3 + 0.5 * torch.randn(B, C, 1, 1, generator=g), "bf16")
    gamma = torch.randn(C, generator=g) * 0.2 + 1.0
    beta = torch.randn(C, generator=g) * 0.2
    w = torch.randn(N, C, generator=g) / math.sqrt(C)
    b = torch.randn(N, generator=g) * 0.1
    _lib.plan_counts(reset=True)
    plain, fused = ops.gn_conv1x1(x.to(gpu), gamma.to(gpu), beta.to(gpu), w.to(gpu), b.to(gpu), eps=1e-6)
    assert _lib.plan_counts(reset=True)["gn_consumer"] == 1
    ref = torch.nn.functional.conv2d(torch.nn.functional.group_norm(x, 32, gamma, beta, 1e-6), _q(w, "bf16").view(N, C, 1, 1), b)
    _cmp(report, f"groupnorm in row-panel prologue B{B} C{C} {H}x{W} N{N} (fused)", fused, ref, "bf16")
    _cmp(report, f"groupnorm + GEMM (plain) B{B} C{C} {H}x{W} N{N}", plain, ref, "bf16")
    if C == 320:
        assert torch.equal(plain, fused)
    else:
        _cmp(report, f"groupnorm in row-panel prologue vs plain C{C}", fused, plain, "bf16")


@pytest.mark.parametrize("M,K,N,bias", [(32768, 320, 1280, True), (32868, 320, 640, False), (65536, 320, 1280, True),
                                        (16384, 640, 2560, True), (16434, 640, 192, False), (32768, 640, 2560, False)])
def test_geglu_rowpanel(gpu, report, knobs, M, K, N, bias):
    """GEGLU over K = 320 / 640 on the row-panel kernel (activation rows resident in registers, weight tiles streaming across
    all column tiles) against torch and against the tiled eight-wave kernel on the same inputs (same K order: bit-identical).
    M = 32868 leaves a last workgroup with 100 of its 256 rows (stores of the missing rows go out of range); K = 640 is the
    16-rows-per-wave form whose column tiles are split over two workgroups per panel at 16384 rows (N = 192: three tiles, no split)."""
    from adaface_amd import _lib, ops
    g = torch.Generator().manual_seed(M + N)
    x = _q(torch.randn(M, K, generator=g), "bf16")
    w = _q(torch.randn(2 * N, K, generator=g) / math.sqrt(K), "bf16")
    b = torch.randn(2 * N, generator=g) * 0.1 if bias else None
    ref = F.linear(x, w, b)
    val, gate = ref.chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    args = (x.to(gpu), w.to(gpu), None if b is None else b.to(gpu))
    _lib.plan_counts(reset=True)
    got = ops.linear(*args, geglu=True, dtype="bf16")
    assert _lib.plan_counts(reset=True)["rowpanel"] == 1
    _cmp(report, f"row-panel geglu [{M},{K}]->{N}", got, ref, "bf16")
    knobs("geglu_rowpanel", 0)
    tiled = ops.linear(*args, geglu=True, dtype="bf16")
    assert _lib.plan_counts(reset=True)["rowpanel"] == 0
    assert torch.equal(got, tiled), (got - tiled).abs().max().item()


@pytest.mark.parametrize("M,K,N,bias,res", [(32768, 320, 320, True, True), (32868, 320, 960, False, False), (65536, 320, 320, True, False),
                                            (16384, 640, 1920, True, False), (16434, 640, 2400, False, False),
                                            (4096, 1280, 1280, True, True), (4196, 1280, 1280, False, False)])
def test_plain_rowpanel(gpu, report, knobs, M, K, N, bias, res):
    """The row-panel kernel on the non-GEGLU K = 320 GEMMs (160-column tiles, residual added in the accumulator layout) and
    on the K = 640 q / k / v projection (N >= 1920; 2400 = 15 tiles, an odd count that stays on one workgroup per panel):
    against torch and, bit for bit, against the tiled eight-wave kernel."""
    from adaface_amd import _lib, ops
    knobs("geglu_rowpanel", 4)
    knobs("gemm_m128", 0)                  # (the [4096, 1280] -> 1280 shape is the 128 x 160 kernel's by default: test_linear_m128_tile)
    g = torch.Generator().manual_seed(M + N + 5)
    x = _q(torch.randn(M, K, generator=g), "bf16")
    w = _q(torch.randn(N, K, generator=g) / math.sqrt(K), "bf16")
    b = torch.randn(N, generator=g) * 0.1 if bias else None
    r = _q(torch.randn(M, N, generator=g), "bf16") if res else None
    ref = F.linear(x, w, b)
    if res:
        ref = ref + r
    args = (x.to(gpu), w.to(gpu), None if b is None else b.to(gpu), None if r is None else r.to(gpu))
    _lib.plan_counts(reset=True)
    got = ops.linear(*args, dtype="bf16")
    assert _lib.plan_counts(reset=True)["rowpanel"] == 1
    _cmp(report, f"row-panel linear [{M},{K}]->{N}", got, ref, "bf16")
    knobs("geglu_rowpanel", 1)
    tiled = ops.linear(*args, dtype="bf16")
    assert _lib.plan_counts(reset=True)["rowpanel"] == 0
    assert torch.equal(got, tiled), (got - tiled).abs().max().item()


@pytest.mark.parametrize("B,Cin,Cout,bias,res,H", [
    (16, 1280, 1280, True, True, 8),     # the 8x8-level ResBlock convolution at the benchmark batch: 4 row tiles x 16 column tiles x 4 slices
    (16, 2560, 1280, True, False, 8),    # the skip-concatenated input: ten chunks per slice
    (4, 256, 80, False, True, 8),        # one row tile, one column tile, ONE chunk per slice (the next chunk's halo pieces are all dead)
    (8, 512, 160, True, False, 8),       # two chunks per slice: both halo buffers
    (16, 1280, 1280, True, True, 16),    # 16x16 maps: one image x 80 columns per tile, ONE K slice, direct epilogue (bias + residual)
    (16, 640, 1280, True, False, 16),    # ten chunks
    (8, 192, 1280, False, True, 16),     # 128 tiles (the least the kernel takes), three chunks
])
def test_conv2d_8x8_maps(gpu, report, knobs, B, Cin, Cout, bias, res, H):
    """conv3x3_s8_kernel (3x3 / stride 1 on 8 x 8 maps: tiles of four whole images x 80 columns over four K slices, the images'
    halos resident in LDS; on 16 x 16 maps: one image x 80 columns per tile in ONE K slice) against torch, against the kernel it
    replaces (knob conv_halo8 bit 1 off), run to run bit-identical (slabs summed in slice order)."""
    from adaface_amd import _lib, ops
    g = torch.Generator().manual_seed(B + Cin + Cout)
    x = _q(torch.randn(B, Cin, H, H, generator=g), "bf16")
    w = _q(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin), "bf16")
    b = torch.randn(Cout, generator=g) if bias else None
    r = _q(torch.randn(B, Cout, H, H, generator=g), "bf16") if res else None
    ref = F.conv2d(x, w, b, padding=1) + (r if res else 0)
    run = lambda: ops.conv2d(x.to(gpu), w.to(gpu), b.to(gpu) if bias else None, residual=r.to(gpu) if res else None, dtype="bf16")
    got = run()
    tile, sk, halo = _last_plan()
    assert tile == 5 and halo == 8 and sk == (4 if H == 8 else 1), (tile, sk, halo)
    _cmp(report, f"conv3x3 {H}x{H} maps {Cin}->{Cout} B{B}", got, ref, "bf16")
    for _ in range(5):
        assert torch.equal(run(), got)
    knobs("conv_halo8", 1)
    old = run()
    assert _last_plan()[2] != 8
    d = (got - old).abs().max().item()
    sc = ref.abs().max().item()
    report(f"conv3x3 {H}x{H} maps vs the round-3 kernel {Cin}->{Cout} B{B}[bf16]", d, sc, 2 * TOL["bf16"] * sc)
    assert d <= 2 * TOL["bf16"] * sc


@pytest.mark.parametrize("B,Cin,H,W,Cout,bias,res,splitk", [
    (2, 320, 64, 64, 320, True, True, 1),      # the dominant ResBlock conv: 4-row tiles of a 64-wide image, 5 chunks (odd K)
    (1, 64, 64, 64, 160, True, False, 1),      # one chunk: the prologue's halo only
    (2, 128, 32, 32, 320, False, True, 1),     # 8-row tiles, 2 chunks (even number of steps)
    (4, 640, 16, 16, 160, True, False, 1),     # one image per tile
    (1, 960, 32, 32, 320, True, True, 1),      # 15 chunks
    (2, 1280, 16, 16, 1280, True, True, 2),    # K sliced into two runs of 10 chunks + reduce
    (3, 192, 64, 64, 160, True, False, 3),     # three slices of one chunk each
])
def test_conv2d_halo8(gpu, report, knobs, B, Cin, H, W, Cout, bias, res, splitk):
    """The eight-wave LDS-halo 3x3 kernel (conv3x3_halo8_kernel) against torch AND against the gathering kernel on the same
    inputs: both walk K as (channel chunk, tap) with the same tiles, so their bf16 results agree bit for bit."""
    from adaface_amd import _lib, ops
    knobs("gemm_pp_minfill", 0)
    knobs("gemm_splitk", splitk)          # the same K slices for both kernels (the planner would slice some of these)
    g = torch.Generator().manual_seed(Cin + Cout + H + 11)
    x = _q(torch.randn(B, Cin, H, W, generator=g), "bf16")
    w = _q(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9), "bf16")
    b = torch.randn(Cout, generator=g) * 0.1 if bias else None
    ref = F.conv2d(x, w, b, padding=1)
    r = _q(torch.randn(ref.shape, generator=g), "bf16") if res else None
    if res:
        ref = ref + r
    args = (x.to(gpu), w.to(gpu), None if b is None else b.to(gpu))
    kw = dict(residual=None if r is None else r.to(gpu), dtype="bf16")
    _lib.plan_counts(reset=True)
    got = ops.conv2d(*args, **kw)
    pc = _lib.plan_counts(reset=True)
    tile, sk, halo = _last_plan()
    assert pc["halo8"] == 1 and tile == 5 and halo == 256 and sk == splitk, (pc, tile, sk, halo)
    _cmp(report, f"halo8 conv3x3 {Cin}->{Cout}@{H}x{W} B{B} sk{splitk}", got, ref, "bf16")
    knobs("conv_halo8", 0)
    gathered = ops.conv2d(*args, **kw)
    assert _lib.plan_counts(reset=True)["halo8"] == 0
    assert torch.equal(got, gathered), (got - gathered).abs().max().item()


@pytest.mark.parametrize("M,K,N,bias,res,geglu", [
    (4096, 320, 320, True, True, False), (1000, 640, 1920, False, False, False), (4096, 1280, 320, True, True, False),
    (512, 64, 160, True, False, False), (4096, 320, 1280, True, False, True), (700, 640, 2560, True, False, True),
    (1024, 1280, 5120, False, False, True),
])
def test_linear_pingpong(gpu, report, knobs, M, K, N, bias, res, geglu):
    """Linear / GEGLU through the ping-pong kernel (GEGLU: 256x128 tile, value|gate interleaved in 16-row groups)."""
    from adaface_amd import ops
    knobs("gemm_pp_minfill", 0)
    dtype = "bf16"
    g = torch.Generator().manual_seed(M + K + N + 1)
    x = _q(torch.randn(M, K, generator=g), dtype)
    rows = 2 * N if geglu else N
    w = _q(torch.randn(rows, K, generator=g) / math.sqrt(K), dtype)
    b = torch.randn(rows, generator=g) * 0.1 if bias else None
    r = _q(torch.randn(M, N, generator=g), dtype) if res else None
    ref = F.linear(x, w, b)
    if geglu:
        val, gate = ref.chunk(2, dim=-1)
        ref = val * F.gelu(gate)
    if res:
        ref = ref + r
    got = ops.linear(x.to(gpu), w.to(gpu), None if b is None else b.to(gpu), None if r is None else r.to(gpu),
                     geglu=geglu, dtype=dtype)
    tile, sk, halo = _last_plan()
    assert tile == (4 if geglu else 5) and halo == 0, (tile, sk, halo)
    _cmp(report, f"pp linear {M}x{K}->{N}{' geglu' if geglu else ''}", got, ref, dtype)


def _ref_attention(q, k, v, heads):
    B, N, C = q.shape
    dh = C // heads
    qh = q.view(B, N, heads, dh).transpose(1, 2)
    kh = k.view(B, -1, heads, dh).transpose(1, 2)
    vh = v.view(B, -1, heads, dh).transpose(1, 2)
    sim = torch.einsum("bhid,bhjd->bhij", qh, kh) * dh ** -0.5
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), vh)
    return out.transpose(1, 2).reshape(B, N, C)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,Nq,Nk,heads,dh", [
    (1, 1024, 1024, 8, 40), (1, 256, 256, 8, 80), (2, 64, 64, 8, 160), (2, 1024, 77, 8, 40),
    (1, 256, 77, 8, 160), (1, 64, 77, 8, 160), (1, 100, 50, 2, 32), (1, 16, 16, 8, 8), (2, 4, 77, 8, 16),
    (1, 300, 300, 2, 64), (1, 256, 77, 2, 128),
])
def test_attention(gpu, report, dtype, B, Nq, Nk, heads, dh):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(Nq + Nk + dh)
    C = heads * dh
    q = _q(torch.randn(B, Nq, C, generator=g), dtype)
    k = _q(torch.randn(B, Nk, C, generator=g), dtype)
    v = _q(torch.randn(B, Nk, C, generator=g), dtype)
    ref = _ref_attention(q, k, v, heads)
    got = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype=dtype)
    _cmp(report, f"attention N{Nq} S{Nk} h{heads} d{dh}", got, ref, dtype)


def test_attention_spiky_softmax(gpu, report):
    """Online-softmax rescale path: one key dominates from a late tile (forces the running max to jump)."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(5)
    B, N, heads, dh = 1, 256, 2, 64
    q = torch.randn(B, N, heads * dh, generator=g)
    k = torch.randn(B, N, heads * dh, generator=g)
    v = torch.randn(B, N, heads * dh, generator=g)
    k[:, 200] = q[:, 17] * 3.0  # key 200 (4th tile) matches query 17 strongly
    ref = _ref_attention(q, k, v, heads)
    got = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype="f32")
    _cmp(report, "attention spiky", got, ref, "f32")


def test_timestep_embedding(gpu, report):
    from adaface_amd import ops
    t = torch.tensor([981, 1, 500, 21], dtype=torch.long)
    dim, half = 320, 160
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    ref = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    got = ops.timestep_embedding(t.to(gpu), dim, dtype="f32")
    _cmp(report, "timestep_embedding", got, ref, "f32", tol_scale=0.5)


def test_ddim_step(gpu, report):
    from adaface_amd import ops
    g = torch.Generator().manual_seed(9)
    x, ec, eu = (torch.randn(2, 4, 64, 64, generator=g) for _ in range(3))
    a_t, a_prev, gs = 0.3521, 0.4012, 7.5
    e = eu + gs * (ec - eu)
    pred = (x - math.sqrt(1 - a_t) * e) / math.sqrt(a_t)
    ref = math.sqrt(a_prev) * pred + math.sqrt(1 - a_prev) * e
    xp, p0 = ops.ddim_step(x.to(gpu), ec.to(gpu), eu.to(gpu), gs, a_t, a_prev, math.sqrt(1 - a_t))
    _cmp(report, "ddim x_prev", xp, ref, "f32", tol_scale=0.05)
    _cmp(report, "ddim pred_x0", p0, pred, "f32", tol_scale=0.05)


def test_lincomb(gpu, report):
    """The PLMS multistep combinations (plms.py:236-249) and the uncond-first CFG combine (plms.py:199)."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(10)
    e = [torch.randn(2, 4, 33, 31, generator=g) for _ in range(4)]  # odd size: exercises the vector tail
    d = [t.to(gpu) for t in e]
    ref4 = (55 * e[0] - 59 * e[1] + 37 * e[2] - 9 * e[3]) / 24
    _cmp(report, "lincomb AB4", ops.lincomb([(d[0], 55 / 24), (d[1], -59 / 24), (d[2], 37 / 24), (d[3], -9 / 24)]), ref4,
         "f32", tol_scale=0.05)
    _cmp(report, "lincomb AB2", ops.lincomb([(d[0], 1.5), (d[1], -0.5)]), (3 * e[0] - e[1]) / 2, "f32", tol_scale=0.05)
    _cmp(report, "lincomb cfg", ops.lincomb([(d[0], 3.0), (d[1], 0.0)], cfg=True), e[1] + 3.0 * (e[0] - e[1]), "f32",
         tol_scale=0.05)


def test_to_uint8(gpu):
    """Byte output is asserted EXACTLY: the kernel restates the reference's fp32 op order, clamp((x + 1) / 2, 0, 1)
    (stable_txt2img.py:715) then 255. * x truncated by astype(uint8) (:764-765); values landing exactly on a byte
    boundary and far outside [-1, 1] are in the input on purpose."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(3)
    img = torch.randn(2, 3, 32, 48, generator=g)
    edge = torch.tensor([-1.0, 1.0, -3.0, 3.0, 0.0, -0.0, 2.0 / 255 * 127 - 1.0, 1.0 - 2.0 ** -23, -1.0 + 2.0 ** -23,
                         254.0 / 255 * 2 - 1, 0.5, -0.5])
    img.view(-1)[: edge.numel()] = edge
    k = torch.arange(256, dtype=torch.float32)            # x with 255 * clamp((x + 1) / 2) at / next to integer k
    img.view(-1)[100:356] = k / 255.0 * 2.0 - 1.0
    img.view(-1)[400:656] = torch.nextafter(k / 255.0 * 2.0 - 1.0, torch.tensor(-4.0))
    ref = (255.0 * torch.clamp((img + 1.0) / 2.0, min=0.0, max=1.0).permute(0, 2, 3, 1).numpy()).astype("uint8")
    got = ops.to_uint8(img.to(gpu)).cpu().numpy()
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert (got == ref).all(), int((got != ref).sum())


@pytest.mark.parametrize("dh", [40, 80])
@pytest.mark.parametrize("ring", [1, 0])
@pytest.mark.parametrize("spike", [6.0, 24.0])
def test_attention_spiky_bf16_dh40(gpu, report, knobs, ring, spike, dh):
    """bf16 dh = 40 / 80 kernels (the 64x64- and 32x32-level attention).  Their softmax reference rides in a spare K slot of the QK^T
    MFMA.  The eight-wave ring kernel (ring = 1) takes it from the FIRST key tile only and repeats a query block with the
    running-reference loop when a later score overflows exp2 (more than 2^127 above it); the four-wave kernel (ring = 0)
    moves the reference when a score rises more than 2^24 above it.  A key in a LATE tile aligned with one query and
    `spike` times longer forces those rare branches: spike 6 -> +55 in the log2 domain (reference move in the four-wave
    kernel, large-but-finite P in the ring kernel), spike 24 -> +220 (overflow -> repeat in the ring kernel).  Queries
    that do not see the spike take the common path in the same launch."""
    from adaface_amd import ops
    knobs("attn_ring", 3 * ring)
    g = torch.Generator().manual_seed(6)
    B, N, heads = 1, 512, 8
    q = _q(torch.randn(B, N, heads * dh, generator=g), "bf16")
    k = _q(torch.randn(B, N, heads * dh, generator=g), "bf16")
    v = _q(torch.randn(B, N, heads * dh, generator=g), "bf16")
    k[:, 330] = _q(q[:, 17] * spike, "bf16")     # key 330 = 6th tile
    k[:, 470] = _q(q[:, 300] * spike, "bf16")    # query 300 sits in another 256-query block / wave than query 17
    ref = _ref_attention(q, k, v, heads)
    sim = torch.einsum("bid,bjd->bij", q[..., :dh], k[..., :dh]) * dh ** -0.5 * math.log2(math.e)
    gap = (sim[0, 17, 330] - sim[0, 17, :64].max()).item()
    assert gap > (140.0 if spike > 20 else 24.0), gap     # the branch condition really is met
    got = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype="bf16")
    assert torch.isfinite(got).all()
    if spike <= 8:
        _cmp(report, f"attention spiky dh{dh} ring{ring} spike{spike:g}", got, ref, "bf16")
    else:
        # The kernels round the pre-scaled Q (q * scale * log2 e) to bf16: component d of a query moves by <= 2^-9 relative, so
        # the score against key j moves by <= delta_ij = 2^-9 * scale * log2(e) * sum_d |q_id| |k_jd| units of the log2
        # domain -- tenths of a unit against the spiked keys (|k| = 24 |q|), whatever the score itself is.  To first order
        # that moves row i of the output by <= E_i = ln 2 * sum_j p_ij delta_ij max_d |v_jd - o_id|.  The bar is PER ROW:
        # the normal bf16 bar plus that row's own bound (no global loosening); the emulation of exactly this rounding on
        # the CPU stays below 0.55 E_i on every row.
        sl2 = dh ** -0.5 * math.log2(math.e)
        qh = q.view(B, N, heads, dh).transpose(1, 2)
        kh = k.view(B, N, heads, dh).transpose(1, 2)
        vh = v.view(B, N, heads, dh).transpose(1, 2)
        pr = torch.softmax(torch.einsum("bhid,bhjd->bhij", qh, kh) * dh ** -0.5, dim=-1)
        oh = torch.einsum("bhij,bhjd->bhid", pr, vh)
        delta = torch.einsum("bhid,bhjd->bhij", qh.abs(), kh.abs()) * sl2 * 2.0 ** -9
        dv = (vh.unsqueeze(2) - oh.unsqueeze(3)).abs().amax(-1)
        E = math.log(2.0) * (pr * delta * dv).sum(-1)                                      # [B, H, N]
        scale = ref.abs().max().item()
        err = (got.cpu() - ref).abs().view(B, N, heads, dh).amax(-1).transpose(1, 2)      # [B, H, N]
        bar = TOL["bf16"] * scale + E
        worst = (err / bar).max().item()
        report(f"attention spiky dh{dh} ring{ring} spike{spike:g}: worst row error / (bf16 bar + the row's Q-rounding bound)[bf16]",
               worst, 1.0, 1.0)
        report(f"attention spiky dh{dh} ring{ring} spike{spike:g}: rows whose bound is below the bf16 bar[bf16]",
               (err * (E < TOL["bf16"] * scale)).max().item(), scale, 2.0 * TOL["bf16"] * scale)
        assert (E > TOL["bf16"] * scale).float().mean().item() < 0.25      # the loosened rows are a minority
        assert worst <= 1.0, worst
    # the two spiked queries on their own: their output is essentially v[330] / v[470]
    assert (got[0, 17].cpu() - ref[0, 17]).abs().max() <= 1.5e-2 * ref.abs().max()
    assert (got[0, 300].cpu() - ref[0, 300]).abs().max() <= 1.5e-2 * ref.abs().max()


@pytest.mark.parametrize("dh", [40, 80])
@pytest.mark.parametrize("B,Nq,Nk,heads", [(2, 300, 333, 8), (1, 256, 77, 8), (3, 70, 64, 2), (1, 1024, 1, 8), (2, 513, 129, 4)])
def test_attention_dh40_ring_shapes(gpu, report, knobs, B, Nq, Nk, heads, dh):
    """Ragged shapes through the ring kernel (dh 40, and dh 80 forced onto it for short key lists too): partial query
    blocks, partial / single key tiles, one key."""
    from adaface_amd import ops
    knobs("attn_ring", 7)
    g = torch.Generator().manual_seed(Nq + Nk)
    C = heads * dh
    q = _q(torch.randn(B, Nq, C, generator=g), "bf16")
    k = _q(torch.randn(B, Nk, C, generator=g), "bf16")
    v = _q(torch.randn(B, Nk, C, generator=g), "bf16")
    ref = _ref_attention(q, k, v, heads)
    got = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype="bf16")
    _cmp(report, f"attention ring N{Nq} S{Nk} h{heads} d{dh}", got, ref, "bf16")


@pytest.mark.parametrize("B,Nq,Nk,heads,dh", [
    (2, 4096, 77, 8, 40),      # the 64x64-level cross-attention: 8 query blocks per wave
    (3, 1024, 77, 8, 80),      # the 32x32 level
    (1, 1000, 77, 8, 40),      # ragged last query block (1000 = 31 * 32 + 8)
    (2, 96, 96, 5, 40),        # a full key list, a partial head group (heads 4 of 5 and 1 of 5 in two workgroups)
    (1, 33, 1, 4, 80),         # one key: softmax weight 1
    (2, 256, 68, 8, 80),       # conv attention leaves S - 9 keys to the flash part; 68 keys here on the short kernel
    (1, 64, 33, 8, 40),        # one key in the second key block
])
def test_attention_short_keys_register_resident(gpu, report, knobs, B, Nq, Nk, heads, dh):
    """xs::xattn_short_kernel (cross-attention over <= 96 keys with K / V^T fragments resident in registers) against
    torch, and against the flash kernel it replaces on the same inputs (knob attn_short = 0); the launch counter proves
    which one ran."""
    from adaface_amd import _lib, ops
    g = torch.Generator().manual_seed(Nq + 3 * Nk + dh)
    C = heads * dh
    q = _q(torch.randn(B, Nq, C, generator=g), "bf16")
    k = _q(torch.randn(B, Nk, C, generator=g), "bf16")
    v = _q(torch.randn(B, Nk, C, generator=g) * 1.5 + 0.2, "bf16")
    ref = _ref_attention(q, k, v, heads)
    _lib.plan_counts(reset=True)
    got = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype="bf16", nan_guard=True)
    assert _lib.plan_counts(reset=True)["attn_short"] == 1
    _cmp(report, f"attention short-key N{Nq} S{Nk} h{heads} d{dh}", got, ref, "bf16")
    knobs("attn_short", 0)
    flash = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype="bf16")
    assert _lib.plan_counts(reset=True)["attn_short"] == 0
    d = (got - flash).abs().max().item()
    report(f"attention short-key vs flash kernel N{Nq} S{Nk} d{dh}[bf16]", d, ref.abs().max().item(), 2 * TOL["bf16"] * ref.abs().max().item())
    assert d <= 2 * TOL["bf16"] * ref.abs().max().item()


@pytest.mark.parametrize("B,N,S", [(2, 4096, 77), (3, 1024, 80), (1, 256, 65), (2, 512, 72), (1, 768, 79)])
def test_cross_attention_layer_in_one_kernel(gpu, report, B, N, S):
    """xf::xattn_fused_kernel -- x + to_out(softmax(to_q(LayerNorm(x)) K^T / sqrt(dh)) V) of a 64x64-level BasicTransformerBlock
    (attention.py:172-257, 279) in ONE launch -- against the torch restatement of those lines on the same bf16-rounded operands,
    and against the three launches it replaces (LayerNorm + to_q, short-key attention, to_out + residual through the op-level
    entry points).  Key counts 65 .. 80 (the kernel takes 64 < S <= 80 -- the text encoder's 77 -- so that all masking happens in
    the last key block of 16; other counts stay on the three launches), several samples per launch (the K / V pack is per sample).  Also the LayerNorm partial sums the kernel leaves for
    norm3's consumer: sum and sum of squares of the rows it stored."""
    from adaface_amd import _lib, ops
    g = torch.Generator().manual_seed(B * 1000 + N + S)
    C, heads, dh = 320, 8, 40
    x = _q(torch.randn(B, N, C, generator=g) * 1.4 + 0.3 * torch.randn(B, N, 1, generator=g), "bf16")
    gamma = torch.randn(C, generator=g) * 0.2 + 1.0
    beta = torch.randn(C, generator=g) * 0.2
    wq = _q(torch.randn(C, C, generator=g) / math.sqrt(C), "bf16")
    wo = _q(torch.randn(C, C, generator=g) / math.sqrt(C), "bf16")
    bo = torch.randn(C, generator=g) * 0.1
    kv = _q(torch.randn(B, S, 2 * C, generator=g) * torch.tensor([1.0] * C + [1.5] * C), "bf16")
    k, v = kv[..., :C], kv[..., C:]
    # reference (fp32): attention.py:279 x + attn2(norm2(x), context); :190 q = to_q(x); :197-243 softmax(q k^T scale) v; :245 to_out
    ln = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    q = ln @ wq.t()
    o = _ref_attention(q, k, v, heads)
    ref = x + o @ wo.t() + bo
    _lib.plan_counts(reset=True)
    got, parts = ops.xattn_fused(x.to(gpu), gamma.to(gpu), beta.to(gpu), wq.to(gpu), kv.to(gpu), wo.to(gpu), bo.to(gpu))
    assert _lib.plan_counts(reset=True)["xattn_fused"] == 1
    _cmp(report, f"cross-attention layer fused B{B} N{N} S{S}", got, ref, "bf16")
    # bit-identical run to run (a first version read S^T accumulators from inline asm a few cycles early on the younger wave of
    # a SIMD: the row maximum, hence the bf16 rounding of P, moved by an ulp from launch to launch)
    for _ in range(6):
        again, _p = ops.xattn_fused(x.to(gpu), gamma.to(gpu), beta.to(gpu), wq.to(gpu), kv.to(gpu), wo.to(gpu), bo.to(gpu))
        assert torch.equal(again, got)
    # the three launches: LayerNorm -> to_q, attention (short-key kernel), to_out + residual
    lnq = ops.layer_norm(x.reshape(B * N, C).to(gpu), gamma.to(gpu), beta.to(gpu), dtype="bf16")
    qq = ops.linear(lnq, wq.to(gpu), None, None, dtype="bf16").reshape(B, N, C)
    oo = ops.attention(qq, k.contiguous().to(gpu), v.contiguous().to(gpu), heads, dtype="bf16")
    plain = ops.linear(oo.reshape(B * N, C), wo.to(gpu), bo.to(gpu), x.reshape(B * N, C).to(gpu), dtype="bf16").reshape(B, N, C)
    _cmp(report, f"cross-attention layer three launches B{B} N{N} S{S}", plain, ref, "bf16")
    d = (got - plain).abs().max().item()
    sc = ref.abs().max().item()
    report(f"cross-attention layer fused vs three launches B{B} N{N} S{S}[bf16]", d, sc, 2 * TOL["bf16"] * sc)
    assert d <= 2 * TOL["bf16"] * sc
    # LayerNorm partial sums of the STORED (bf16) rows: parts 0 / 2 = columns 0-159 / 160-319, parts 1 / 3 zero
    st = got.reshape(B * N, C).double()
    assert float(parts[1].abs().max()) == 0.0 and float(parts[3].abs().max()) == 0.0
    for part, lo in ((0, 0), (2, 160)):
        s1, s2 = st[:, lo:lo + 160].sum(dim=1), (st[:, lo:lo + 160] ** 2).sum(dim=1)
        assert torch.allclose(parts[part][:, 0].double(), s1, rtol=1e-4, atol=1e-3)
        assert torch.allclose(parts[part][:, 1].double(), s2, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("B,Nq,Nk,heads", [(16, 1024, 1024, 8), (2, 300, 333, 8), (1, 513, 129, 4), (3, 70, 64, 2)])
def test_attention_dh80_ring_bit_identical(gpu, knobs, B, Nq, Nk, heads):
    """The dh-80 ring kernel (four-wave workgroups sharing LDS-DMA-staged K / V tiles, round 4) runs the same online softmax,
    MFMA for MFMA, as the four-wave register-staged kernel it replaces at the 32x32 level: outputs are equal BIT FOR BIT, at
    the benchmark shape and on ragged ones (so the bf16 forward, and every bar measured on it, does not move)."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(B + Nq + Nk)
    C = heads * 80
    q = _q(torch.randn(B, Nq, C, generator=g) * 1.3, "bf16").to(gpu)
    k = _q(torch.randn(B, Nk, C, generator=g) * 1.3, "bf16").to(gpu)
    v = _q(torch.randn(B, Nk, C, generator=g), "bf16").to(gpu)
    knobs("attn_ring", 7)
    new = ops.attention(q, k, v, heads, dtype="bf16")
    knobs("attn_ring", 1)
    old = ops.attention(q, k, v, heads, dtype="bf16")
    assert torch.isfinite(new).all()
    assert torch.equal(new, old), (new.float() - old.float()).abs().max().item()


@pytest.mark.parametrize("dh,Nk", [(40, 77), (40, 129), (80, 129), (80, 300)])
def test_attention_dh40_ring_nan_guard(gpu, report, knobs, dh, Nk):
    """the ring kernel zero-fills rows >= Nk of the last key tile through the buffer range check.  K and V are
    placed in front of 128 rows of NaNs (af_op_attention flag bit 1): a kernel that really read those rows would turn
    0 * NaN into NaN in O (finite garbage there is invisible: P is 0).  One run, finite and matching."""
    from adaface_amd import ops
    knobs("attn_ring", 7)       # (dh 80: the ring kernel for fewer than 256 keys too)
    g = torch.Generator().manual_seed(1000 + Nk)
    B, Nq, heads = 2, 512, 8
    C = heads * dh
    q = _q(torch.randn(B, Nq, C, generator=g), "bf16")
    k = _q(torch.randn(B, Nk, C, generator=g), "bf16")
    v = _q(torch.randn(B, Nk, C, generator=g), "bf16")
    ref = _ref_attention(q, k, v, heads)
    got = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, dtype="bf16", nan_guard=True)
    assert torch.isfinite(got).all(), "ring kernel read K/V rows past Nk"
    _cmp(report, f"attention ring nan-guard d{dh} S{Nk}", got, ref, "bf16")


# ---------------------------------------------------------------------------------------------------------------
# Size-independent properties at the benchmark's full SD-1.5 shapes (Bf = 16), where a CPU reference of the whole
# tensor would take minutes: linearity of the convolution, invariance of attention to the key order, invariance of
# GroupNorm to an affine change of its input, bitwise run-to-run determinism.  bf16 kernels, fp32 comparisons.
# ---------------------------------------------------------------------------------------------------------------
def test_fullsize_conv_linearity_and_determinism(gpu, report):
    """conv3x3 320->320 at 64x64, batch 16 (M = 65536: two rounds of the 256x160 ping-pong tile):
    conv(a*x + b*y) == a*conv(x) + b*conv(y) up to bf16 rounding of inputs / outputs, and two runs are bit-identical."""
    from adaface_amd import ops
    g = torch.Generator(device=gpu).manual_seed(1)
    x = torch.randn(16, 320, 64, 64, generator=g, device=gpu).bfloat16().float()
    y = torch.randn(16, 320, 64, 64, generator=g, device=gpu).bfloat16().float()
    w = (torch.randn(320, 320, 3, 3, generator=g, device=gpu) / math.sqrt(320 * 9)).bfloat16().float()
    cx = ops.conv2d(x, w, dtype="bf16")
    assert _last_plan()[0] == 5
    assert torch.equal(cx, ops.conv2d(x, w, dtype="bf16"))
    cy = ops.conv2d(y, w, dtype="bf16")
    z = (2.0 * x - 0.5 * y)                  # exactly representable combinations stay bf16-exact only approximately:
    cz = ops.conv2d(z, w, dtype="bf16")      # z is re-rounded to bf16 at the boundary, so compare at bf16 tolerance
    ref = 2.0 * cx - 0.5 * cy
    _cmp(report, "fullsize conv linearity 320->320@64 B16", cz, ref, "bf16")
    # one output pixel against a direct fp64 evaluation (zero-padded border pixel and an interior one)
    for (b, oy, ox) in ((3, 0, 0), (15, 63, 17), (7, 31, 40)):
        patch = F.pad(x[b:b + 1].double(), (1, 1, 1, 1))[:, :, oy:oy + 3, ox:ox + 3]
        direct = (patch * w.double()).sum(dim=(1, 2, 3))
        assert (cx[b, :, oy, ox].double() - direct).abs().max() < 3e-2 * direct.abs().max()


def test_fullsize_attention_key_permutation_invariance(gpu, report):
    """Self-attention at the 64x64 level (N = S = 4096, 8 heads of 40): softmax(q k^T) v does not depend on the order of
    the keys -- the property the conv-attention path relies on when it moves the subject's keys to the end."""
    from adaface_amd import ops
    g = torch.Generator(device=gpu).manual_seed(2)
    q = torch.randn(2, 4096, 320, generator=g, device=gpu)
    k = torch.randn(2, 4096, 320, generator=g, device=gpu)
    v = torch.randn(2, 4096, 320, generator=g, device=gpu)
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(3)).to(gpu)
    a = ops.attention(q, k, v, heads=8, dtype="bf16")
    b = ops.attention(q, k[:, perm].contiguous(), v[:, perm].contiguous(), heads=8, dtype="bf16")
    assert torch.equal(a, ops.attention(q, k, v, heads=8, dtype="bf16"))            # deterministic
    _cmp(report, "fullsize attention key-permutation invariance N4096 d40", b, a, "bf16")
    rows = a.view(2, 4096, 8, 40)
    assert torch.isfinite(rows).all()
    # convexity: every output is a convex combination of the values of its head
    vmax = v.view(2, 4096, 8, 40).amax(dim=1, keepdim=True)
    vmin = v.view(2, 4096, 8, 40).amin(dim=1, keepdim=True)
    assert (rows <= vmax + 0.05).all() and (rows >= vmin - 0.05).all()


def test_fullsize_groupnorm_affine_invariance(gpu, report):
    """GroupNorm(32) at C = 320, 64x64, batch 16: GN(a*x + b) == GN(x) for a > 0 (per-sample statistics)."""
    from adaface_amd import ops
    g = torch.Generator(device=gpu).manual_seed(4)
    x = torch.randn(16, 320, 64, 64, generator=g, device=gpu)
    w = torch.randn(320, generator=g, device=gpu) * 0.3 + 1.0
    b = torch.randn(320, generator=g, device=gpu) * 0.2
    y0 = ops.group_norm(x, w, b, eps=1e-5, silu=True, dtype="f32")
    y1 = ops.group_norm(3.0 * x + 0.75, w, b, eps=1e-5, silu=True, dtype="f32")
    assert torch.equal(y0, ops.group_norm(x, w, b, eps=1e-5, silu=True, dtype="f32"))
    _cmp(report, "fullsize groupnorm affine invariance C320@64 B16", y1, y0, "f32", tol_scale=5.0)


# ---------------------------------------------------------------------------------------------------------------
# The same operators against outputs of the REFERENCE's own modules (tests/golden/gen_golden.py imports
# ldm.modules.attention / openaimodel on CPU; weights are regenerated from tests/golden/opgold.py): SURVEY.md §8c (1).
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ops_vs_reference_module_goldens(gpu, report, dtype):
    import sys
    from pathlib import Path
    import numpy as np
    from adaface_amd import ops
    gold_dir = Path(__file__).resolve().parent / "golden"
    sys.path.insert(0, str(gold_dir))
    from opgold import module_params as mp
    g = dict(np.load(gold_dir / "golden_tiny.npz"))
    D = lambda t: t.to(gpu)
    G = lambda k: torch.tensor(g[k])

    def chk(name, got, key, scale=1.0):
        _cmp(report, f"refmod {name}", got, G(key), dtype, tol_scale=scale)

    w = mp("gn32")
    chk("GroupNorm32+SiLU", ops.group_norm(D(G("op_gn_x")), D(w["weight"]), D(w["bias"]), eps=1e-5, silu=True, dtype=dtype), "op_gn32_silu")
    w = mp("normalize")
    chk("Normalize eps1e-6", ops.group_norm(D(G("op_gn_x")), D(w["weight"]), D(w["bias"]), eps=1e-6, silu=False, dtype=dtype), "op_normalize")
    w = mp("ln")
    chk("LayerNorm", ops.layer_norm(D(G("op_ln_x")), D(w["weight"]), D(w["bias"]), dtype=dtype), "op_ln")
    w = mp("ff")
    h = ops.linear(D(G("op_ln_x")), D(w["net.0.proj.weight"]), D(w["net.0.proj.bias"]), geglu=True, dtype=dtype)
    chk("FeedForward GEGLU", ops.linear(h, D(w["net.2.weight"]), D(w["net.2.bias"]), dtype=dtype), "op_ff_geglu", 2.0)
    w = mp("attn_self")
    x = D(G("op_attn_self_x"))
    q, k, v = (ops.linear(x, D(w[f"to_{n}.weight"]), dtype=dtype) for n in "qkv")
    a = ops.attention(q, k, v, heads=8, dtype=dtype)
    chk("CrossAttention self N64 dh160", ops.linear(a, D(w["to_out.0.weight"]), D(w["to_out.0.bias"]), dtype=dtype), "op_attn_self", 2.0)
    w = mp("attn_cross")
    x, c = D(G("op_attn_cross_x")), D(G("op_attn_cross_ctx"))
    q = ops.linear(x, D(w["to_q.weight"]), dtype=dtype)
    k, v = ops.linear(c, D(w["to_k.weight"]), dtype=dtype), ops.linear(c, D(w["to_v.weight"]), dtype=dtype)
    a = ops.attention(q, k, v, heads=4, dtype=dtype)
    chk("CrossAttention cross S77", ops.linear(a, D(w["to_out.0.weight"]), D(w["to_out.0.bias"]), dtype=dtype), "op_attn_cross", 2.0)
    x = D(G("op_res_x"))
    w = mp("down")
    chk("Downsample conv3x3 s2", ops.conv2d(x, D(w["op.weight"]), D(w["op.bias"]), stride=2, dtype=dtype), "op_downsample")
    w = mp("up")
    chk("Upsample nearest2x+conv3x3", ops.conv2d(x, D(w["conv.weight"]), D(w["conv.bias"]), upsample=True, dtype=dtype), "op_upsample")
    # ResBlock (openaimodel.py:259-279) assembled from the operator entry points
    for name, key in (("res_same", "op_resblock_same"), ("res_widen", "op_resblock_widen")):
        w = mp(name)
        emb = F.linear(F.silu(G("op_res_emb")), w["emb_layers.1.weight"], w["emb_layers.1.bias"])   # [2, Cout] (tiny, host)
        h = ops.group_norm(x, D(w["in_layers.0.weight"]), D(w["in_layers.0.bias"]), eps=1e-5, silu=True, dtype=dtype)
        h = ops.conv2d(h, D(w["in_layers.2.weight"]), D(w["in_layers.2.bias"]), dtype=dtype) + D(emb)[:, :, None, None]
        h = ops.group_norm(h, D(w["out_layers.0.weight"]), D(w["out_layers.0.bias"]), eps=1e-5, silu=True, dtype=dtype)
        skip = x if "skip_connection.weight" not in w else ops.conv2d(x, D(w["skip_connection.weight"]), D(w["skip_connection.bias"]), dtype=dtype)
        chk(f"ResBlock {name}", ops.conv2d(h, D(w["out_layers.3.weight"]), D(w["out_layers.3.bias"]), residual=skip, dtype=dtype), key, 2.0)
