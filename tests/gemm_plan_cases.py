"""The launches whose plans tests/golden/gemm_plans.npz records (tests/test_gemm_plan_cpu.py, scripts/dump_gemm_plans.py).

A case is the argument tuple of af_gemm_plan_query -- ARGS below -- plus a knob setting (index into KNOBS).  `linear_args` /
`conv_args` build the integers the way af_op_linear / af_op_conv2d build their ConvGemmParams, so the GPU test can ask the
query about the very launch an op makes.  `cases()` is deterministic: the table and the test walk the same list.

What the product of the listed values leaves out, and why:
  * the LayerNorm and consumer-GroupNorm flags go with bf16 only: the launcher refuses them on the other storage types;
  * `gn_stats_out` goes with bf16 only, and with Cout % 32 == 0 (32 groups): same reason;
  * fp8 goes with bf16, Cin % 64 == 0 and no upsampling (the op's own preconditions);
  * the one-at-a-time knob settings and the "no workspace" launcher run on every KNOB_STRIDE-th default case (and on every
    anchor), not on all of them: 15 settings times the full list would be 400 000 rows.
"""
from itertools import product

ARGS = ("dtype", "M", "N", "K", "cin_pad", "ks", "stride", "pad", "up", "Hs", "Ws", "Ho", "Wo", "ldc", "ldo", "gn_hw", "gn_cpg", "flags")
OUTS = ("kernel", "rowpanel", "tile", "splitk", "halo_tw", "group_m", "ws_bytes")
BF16, F32, F16 = 0, 1, 2
GEGLU, RESIDUAL, ROWBIAS, LN_CONSUMER, LN_PRODUCER, GN_AB, GN_STATS_OUT, FP8, PHASE_WEIGHTS, WORKSPACE = (1 << i for i in range(10))
# AfGemmKernel
K_NONE, K_WAVE4, K_HALO4, K_PP, K_PP_FP8, K_HALO8, K_S8, K_UP_PHASE4, K_ROWPANEL, K_M128 = range(10)

# index 0 = the load-time defaults; "no_workspace" is not a knob: it clears the WORKSPACE flag
KNOBS = [None, ("gemm_pp", 0), ("gemm_pp_minfill", 0), ("conv_halo", 0), ("conv_halo8", 0), ("conv_halo8", 1), ("conv_halo8", 7),
         ("geglu_rowpanel", 0), ("geglu_rowpanel", 4), ("gemm_m128", 0), ("small_m_tile64", 0), ("conv_up_phase4", 0),
         ("gemm_tile", 1), ("gemm_splitk", 3), "no_workspace"]
KNOB_STRIDE = 110


def _rup(a, b):
    return (a + b - 1) // b * b


def _bk(dtype):
    return 32 if dtype == F32 else 64


def linear_args(dtype, M, K, N, geglu=False, residual=False, flags=0, gn_hw=0):
    """af_op_linear: [M, K] x [N (GEGLU: 2 N), K]^T, the rows as one 1 x M map"""
    kp, no4 = _rup(K, _bk(dtype)), _rup(N, 4)
    fl = flags | WORKSPACE | (GEGLU if geglu else 0) | (RESIDUAL if residual else 0)
    return (dtype, M, 2 * N if geglu else no4, kp, kp, 1, 1, 0, 0, 1, M, 1, M, kp, no4, gn_hw, 0, fl)


def conv_args(dtype, B, Cin, H, W, Cout, ks, stride=1, up=False, residual=False, flags=0, phase_weights=None):
    """af_op_conv2d (pad ks / 2); phase_weights None = as the op does (bf16, upsampled 3x3, whole 64-channel chunks)"""
    cin_pad, co4, pad, up = _rup(Cin, _bk(dtype)), _rup(Cout, 4), ks // 2, int(bool(up))
    Ho, Wo = ((H << up) + 2 * pad - ks) // stride + 1, ((W << up) + 2 * pad - ks) // stride + 1
    if phase_weights is None:
        phase_weights = bool(up) and ks == 3 and dtype == BF16 and cin_pad % 64 == 0
    fl = flags | WORKSPACE | (RESIDUAL if residual else 0) | (PHASE_WEIGHTS if phase_weights else 0)
    gn_cpg = Cout // 32 if flags & GN_STATS_OUT else 0
    return (dtype, B * Ho * Wo, co4, ks * ks * cin_pad, cin_pad, ks, stride, pad, up, H, W, Ho, Wo, cin_pad, co4, 0, gn_cpg, fl)


def conv_fp8_args(B, Cin, H, W, Cout, ks, stride=1, up=False, residual=False):
    """af_op_conv2d_fp8: e4m3 operands, K padded to 128 (the twin's layout)"""
    a = list(conv_args(BF16, B, Cin, H, W, Cout, ks, stride, up, residual, FP8, phase_weights=False))
    a[3] = _rup(ks * ks * Cin, 128)
    return tuple(a)


LIN_M = (2, 154, 256, 512, 1000, 1024, 4096, 4196, 8192, 16384, 16434, 32768, 32868, 65536)
LIN_K = (64, 128, 320, 640, 768, 1280, 2560, 5120)
LIN_N = (4, 160, 192, 320, 640, 960, 1280, 1920, 2560, 3840, 5120, 10240)
CONV_B = (1, 2, 4, 8, 16)
# every Cin of {4, 64, 128, 192, 256, 320, 512, 640, 960, 1280, 1920, 2560} and every Cout of {3 (stored as 4), 80, 128, 160, 320,
# 640, 1280} at least once, on the pairings the networks and the existing GPU tests use
CONV_CH = ((4, 320), (64, 128), (64, 160), (128, 3), (128, 320), (192, 160), (256, 80), (320, 4), (320, 320), (320, 640), (512, 128),
           (640, 640), (640, 1280), (960, 640), (1280, 1280), (1920, 1280), (2560, 1280))
CONV_MAPS = ((8, 8), (16, 16), (32, 32), (64, 64), (40, 24), (32, 64))
CONV_KINDS = ((3, 1, False, None), (3, 2, False, None), (3, 1, True, True), (3, 1, True, False), (1, 1, False, None))   # ks, stride, up, phase weights


def _linears():
    for dtype, M, K, N in product((BF16, F32, F16), LIN_M, LIN_K, LIN_N):
        yield linear_args(dtype, M, K, N)
        yield linear_args(dtype, M, K, N, residual=True)
        if N % 64 == 0:
            yield linear_args(dtype, M, K, N, geglu=True)
        if dtype == BF16:
            yield linear_args(dtype, M, K, N, flags=LN_CONSUMER)
            yield linear_args(dtype, M, K, N, flags=LN_PRODUCER)
            for hw in (1024, 4096):
                if M % hw == 0:
                    yield linear_args(dtype, M, K, N, flags=GN_AB, gn_hw=hw)


def _convs():
    for dtype, B, (Cin, Cout), (H, W), (ks, stride, up, pw) in product((BF16, F32, F16), CONV_B, CONV_CH, CONV_MAPS, CONV_KINDS):
        if pw and not (dtype == BF16 and Cin % 64 == 0):
            continue                                     # (no phase weights exist there: the "without" case covers it)
        yield conv_args(dtype, B, Cin, H, W, Cout, ks, stride, up, phase_weights=pw)
        if dtype == BF16 and Cout % 32 == 0:
            yield conv_args(dtype, B, Cin, H, W, Cout, ks, stride, up, flags=GN_STATS_OUT, phase_weights=pw)
        if dtype == BF16 and Cin % 64 == 0 and not up:
            yield conv_fp8_args(B, Cin, H, W, Cout, ks, stride)


def anchors():
    """(name, args, knob index, expected {field: value}) of the shapes whose plans the GPU tests pin"""
    conv9 = [(2, 320, 32, 32, 320, 3, 1, False, True), (1, 4, 64, 64, 320, 3, 1, False, False), (1, 320, 64, 64, 4, 3, 1, False, False),
             (2, 320, 32, 32, 320, 3, 2, False, False), (1, 640, 16, 16, 640, 3, 1, True, False), (2, 960, 16, 16, 640, 1, 1, False, False),
             (1, 128, 40, 24, 3, 3, 1, False, False), (1, 64, 8, 8, 128, 3, 1, False, False), (2, 1280, 8, 8, 1280, 3, 1, False, True)]
    conv_plans = {F32: [(2, 4, 0), (2, 1, 32), (2, 10, 0), (2, 11, 0), (0, 8, 0), (3, 1, 0), (2, 4, 0), (0, 2, 0), (0, 16, 0)],
                  BF16: [(2, 4, 0), (2, 1, 32), (2, 5, 0), (2, 5, 0), (0, 8, 0), (3, 1, 0), (2, 2, 0), (1, 1, 0), (0, 16, 0)]}
    lin8 = [(4096, 320, 320, True), (1024, 640, 640, False), (154, 768, 1280, False), (2, 320, 1280, False), (256, 1280, 1280, True),
            (200, 64, 192, False), (4096, 1280, 320, True), (333, 128, 4, False)]
    lin_plans = {F32: [(2, 1, 0), (3, 1, 0), (0, 3, 0), (1, 1, 0), (0, 5, 0), (3, 1, 0), (2, 2, 0), (3, 1, 0)],
                 BF16: [(2, 1, 0), (3, 1, 0), (1, 1, 0), (1, 1, 0), (3, 1, 0), (3, 1, 0), (2, 2, 0), (3, 1, 0)]}
    out = [
        ("linear 4096x1280->1280", linear_args(BF16, 4096, 1280, 1280), 0, dict(kernel=K_M128, splitk=1)),
        ("geglu 32768x320->1280", linear_args(BF16, 32768, 320, 1280, geglu=True), 0, dict(kernel=K_ROWPANEL, rowpanel=1)),
        ("linear 32768x320->320 +res", linear_args(BF16, 32768, 320, 320, residual=True), 0, dict(kernel=K_ROWPANEL, rowpanel=2)),
        ("conv3x3 16x1280->1280@8x8", conv_args(BF16, 16, 1280, 8, 8, 1280, 3), 0, dict(kernel=K_S8, halo_tw=8, splitk=4)),
        ("conv3x3 16x1280->1280@16x16", conv_args(BF16, 16, 1280, 16, 16, 1280, 3), 0, dict(kernel=K_S8, halo_tw=8, splitk=1)),
        ("conv3x3 up 4x128->320@16x16", conv_args(BF16, 4, 128, 16, 16, 320, 3, up=True), 0, dict(kernel=K_UP_PHASE4)),
    ]
    for dtype in (F32, BF16):
        for i, (B, Cin, H, W, Cout, ks, stride, up, res) in enumerate(conv9):
            t, s, h = conv_plans[dtype][i]
            out.append((f"test_conv2d[{i}] dtype {dtype}", conv_args(dtype, B, Cin, H, W, Cout, ks, stride, up, res), 0, dict(tile=t, splitk=s, halo_tw=h)))
        for i, (M, K, N, res) in enumerate(lin8):
            t, s, h = lin_plans[dtype][i]
            out.append((f"test_linear[{i}] dtype {dtype}", linear_args(dtype, M, K, N, residual=res), 0,
                        dict(tile=t, splitk=s, halo_tw=h, rowpanel=0)))
    return out


# one smallest launch per kernel value the product above does not reach at the load-time knobs (from the GPU tests that force them)
EXTRA = [
    (conv_args(BF16, 1, 64, 64, 64, 160, 3), 2),                   # eight-wave halo, gemm_pp_minfill = 0 (test_conv2d_halo8)
    (linear_args(BF16, 512, 64, 160), 2),                          # ping-pong, gemm_pp_minfill = 0 (test_linear_pingpong)
    (conv_args(BF16, 4, 256, 8, 8, 80, 3, residual=True), 0),      # small-map kernel, one tile (test_conv2d_8x8_maps)
    (linear_args(BF16, 333, 128, 4), 0),                           # four-wave
    (conv_args(F32, 1, 4, 64, 64, 320, 3), 0),                     # four-wave halo
]


def cases():
    """[(args, knob index)], deterministic"""
    base = [(a, 0) for a in _linears()] + [(a, 0) for a in _convs()]
    anch = [(a, k) for _, a, k, _ in anchors()]
    out = base + anch + list(EXTRA)
    sub = base[::KNOB_STRIDE] + anch
    for ki in range(1, len(KNOBS)):
        for a, _ in sub:
            if KNOBS[ki] == "no_workspace":
                a = a[:-1] + (a[-1] & ~WORKSPACE,)
            out.append((a, ki))
    return out


def run(case_list):
    """the plans of `case_list` as rows of 7 integers, through af_gemm_plan_query; knobs restored afterwards"""
    from adaface_amd import _lib
    rows, cur = [], 0
    try:
        for a, ki in case_list:
            if ki != cur:
                _lib.reset_knobs()
                if isinstance(KNOBS[ki], tuple):
                    _lib.set_knob(*KNOBS[ki])
                cur = ki
            rows.append(_lib.gemm_plan_query(*a))
    finally:
        _lib.reset_knobs()
    return rows
