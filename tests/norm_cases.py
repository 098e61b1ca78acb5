"""The GroupNorm / LayerNorm shapes of tests/test_norm_plan_cpu.py and tests/test_norm_gpu.py, each with the branch of
af_norm.hip it is there for and the launch plan it must get -- written out by hand from the thresholds, never computed here,
so that a threshold that moves shows up as a case whose plan changed (af_norm_plan_query, `_lib.norm_plan_query`).

GroupNorm(32), storage element e (bf16 / f16: 8 per 16-byte vector, f32: 4), cpg = C / 32 channels per group:
  small     gn_small_kernel when cpg is whole vectors and HW * (cpg / e) <= 2560 items (knob gn_small, default on)
  chunked   P = 4 pixels per chunk, doubled while P < 64 and chunks * B > 1024, then doubled while chunks > 1024;
            fold (the apply pass combines the partial sums) at <= 64 chunks, else gn_finalize_kernel, whose unrolled loop
            takes 64 chunks per trip and whose remainder loop takes the rest;
            wide = more than 256 vectors per pixel (C / e > 256): the statistics pass's one-thread-per-column loop
LayerNorm: refused unless C is whole vectors and at most 320 of them; row-group kernel (8 lanes per row on 16-bit storage, 16
on f32; 32 / 16 rows per workgroup) when the vectors divide by the lanes, at most 10 per lane, and rows / rows-per-workgroup
>= 256; else one wave per row (4 rows per workgroup, ceil(vectors / 64) per lane).
"""
from collections import namedtuple

ALL = ("f32", "bf16", "f16")
H16 = ("bf16", "f16")

# plan: (kernel, P, nchunk, npart, wide) as norm_plan_query reports it
GnCase = namedtuple("GnCase", "shape dtypes plan nosmall why")   # shape (B, C, H, W); nosmall: the plan under gn_small = 0
SMALL = ("small", 0, 0, 0, False)
REFUSED = ("refused", 0, 0, 0, False)


def _chunked(kernel, P, nchunk, wide=False):
    return (kernel, P, nchunk, nchunk, wide)


def _by(**kw):
    """a plan that differs by dtype: {"f32": ..., "bf16": ..., "f16": ...} (h16 = both 16-bit types)"""
    out = {}
    for k, v in kw.items():
        for d in (H16 if k == "h16" else (k,)):
            out[d] = v
    return out


GN_CASES = [
    # ---- chunked path: ragged last chunks, the finalize remainder loop, the chunking loops
    GnCase((2, 320, 9, 29), ALL, _chunked("finalize", 4, 66), None,
           "HW 261 = 65 * 4 + 1: last chunk of 1 pixel; 66 chunks: gn_finalize runs its remainder loop only; 40 / 80 vectors per "
           "pixel do not divide 256; two samples"),
    GnCase((1, 64, 67, 5), ALL, _chunked("finalize", 4, 84), None,
           "HW 335 = 83 * 4 + 3: 84 chunks, one trip of the unrolled finalize loop then the remainder; 2 channels per group: a "
           "16-byte vector spans 2 (f32) or 4 (16-bit) groups"),
    GnCase((1, 32, 7, 9), ALL, _chunked("fold", 4, 16), None, "HW 63 = 15 * 4 + 3: 16 chunks, folded combine; one channel per group"),
    GnCase((1, 64, 1, 1), ALL, _chunked("fold", 4, 1), None, "one pixel, one chunk"),
    GnCase((48, 64, 10, 10), ALL, _chunked("fold", 8, 13), None, "25 * 48 chunks > 1024: the batch pushes P to 8; HW 100 = 12 * 8 + 4"),
    GnCase((32, 64, 36, 36), ALL, _chunked("fold", 64, 21), None,
           "the batch pushes P to its cap of 64 (41 * 32 chunks > 1024 at P = 32); HW 1296 = 20 * 64 + 16"),
    GnCase((1, 32, 260, 257), ALL, _chunked("finalize", 128, 523), None,
           "HW 66820: 1045 chunks at P = 64 > 1024, the per-sample cap loop doubles P to 128; 523 chunks = 8 * 64 + 11, last of 4 pixels"),
    GnCase((2, 1280, 9, 29), ("f32",), _chunked("finalize", 4, 66, wide=True), None,
           "f32: 320 vectors per pixel (wide statistics loop), 2610 items > 2560 so not small; ragged chunk, finalize remainder"),
    GnCase((1, 2560, 9, 29), H16, _chunked("finalize", 4, 66, wide=True), None,
           "16-bit: 320 vectors per pixel (wide statistics loop), 2610 items > 2560 so not small; ragged chunk, finalize remainder"),
    # ---- small kernel, and the same shapes on the chunked path under gn_small = 0
    GnCase((1, 256, 3, 3), ALL, SMALL, _chunked("fold", 4, 3), "9 (16-bit) / 18 (f32) items: one partly filled wave"),
    GnCase((2, 256, 5, 7), ALL, SMALL, _chunked("fold", 4, 9), "35 / 70 items: partly filled waves, two samples"),
    GnCase((1, 256, 33, 31), ALL, SMALL, _chunked("finalize", 4, 256), "1023 / 2046 items: a last register slot one item short"),
    GnCase((1, 1280, 9, 7), ALL, SMALL,
           _by(f32=_chunked("fold", 4, 16, wide=True), h16=_chunked("fold", 4, 16)), "odd map, 5 / 10 vectors per pixel of a group"),
    GnCase((1, 2560, 7, 9), ALL, SMALL, _chunked("fold", 4, 16, wide=True), "10 / 20 vectors per pixel of a group"),
    GnCase((1, 256, 16, 20), ALL, SMALL, _chunked("finalize", 4, 80), "320 / 640 items"),
    GnCase((1, 256, 16, 21), ALL, SMALL, _chunked("finalize", 4, 84), "336 / 672 items"),
    # ---- the small kernel's limit of 2560 items, both sides, per element size
    GnCase((1, 256, 32, 40), ("f32",), SMALL, _chunked("finalize", 4, 320), "f32: exactly 2560 items"),
    GnCase((1, 256, 21, 61), ("f32",), _chunked("finalize", 4, 321), None, "f32: 2562 items, the smallest map past the limit; HW 1281 = 320 * 4 + 1"),
    GnCase((1, 256, 40, 64), H16, SMALL, _chunked("finalize", 4, 640), "16-bit: exactly 2560 items"),
    GnCase((1, 256, 13, 197), H16, _chunked("finalize", 4, 641), None, "16-bit: 2561 items, the smallest map past the limit; HW 2561 = 640 * 4 + 1"),
    # ---- refusals
    GnCase((1, 48, 4, 4), ALL, REFUSED, None, "C % 32 != 0"),
    GnCase((1, 2592, 4, 4), ALL, REFUSED, None, "C = 81 * 32 > 2560"),
]

# plan: (kernel, vectors per lane, rows per workgroup)
LnCase = namedtuple("LnCase", "rows C dtypes plan why")
LN_REFUSED = ("refused", 0, 0)

LN_CASES = [
    LnCase(8197, 320, H16, ("rowgroup", 5, 32), "row-group, last workgroup of 5 live rows"),
    LnCase(4099, 320, ("f32",), ("rowgroup", 5, 16), "row-group, last workgroup of 3 live rows"),
    LnCase(8200, 640, H16, ("rowgroup", 10, 32), "row-group at its limit of 10 vectors per lane, 8 live rows in the last workgroup"),
    LnCase(8200, 640, ("f32",), ("rowgroup", 10, 16), "row-group at its limit of 10 vectors per lane, 8 live rows in the last workgroup"),
    LnCase(8195, 64, H16, ("rowgroup", 1, 32), "row-group, one vector per lane, 3 live rows in the last workgroup"),
    LnCase(8195, 64, ("f32",), ("rowgroup", 1, 16), "row-group, one vector per lane, 3 live rows in the last workgroup"),
    LnCase(8191, 320, H16, ("wave_row", 1, 4), "255 workgroups' worth of rows: one row below the row-group threshold"),
    LnCase(4095, 320, ("f32",), ("wave_row", 2, 4), "255 workgroups' worth of rows: one row below the row-group threshold"),
    LnCase(8200, 328, ("bf16",), ("wave_row", 1, 4), "41 vectors do not divide by 8 lanes: wave per row at a row-group row count"),
    LnCase(8200, 704, ("bf16",), ("wave_row", 2, 4), "88 vectors = 11 per lane > 10: wave per row at a row-group row count"),
    LnCase(5, 2560, ("bf16",), ("wave_row", 5, 4), "320 vectors: the widest row a wave holds; 5 rows: a last workgroup of one wave"),
    LnCase(16, 2568, ("bf16",), LN_REFUSED, "321 vectors > 64 * 5"),
    LnCase(16, 36, ("bf16",), LN_REFUSED, "36 elements are no whole number of 16-byte vectors"),
]

# The norm shapes of the older GPU tests and the kernel each reaches per dtype (kernel name only): a threshold change shows
# here which of those tests moved to another kernel.  (test name, dtype, (B, C, H, W), kernel)
_OPS_GN = [((2, 320, 64, 64), "finalize", "finalize"), ((2, 640, 32, 32), "finalize", "finalize"), ((1, 960, 64, 64), "finalize", "finalize"),
           ((2, 1280, 8, 8), "small", "small"), ((1, 2560, 16, 16), "fold", "small"), ((1, 1920, 32, 32), "finalize", "finalize"),
           ((1, 128, 96, 80), "finalize", "finalize"), ((3, 64, 4, 4), "fold", "fold"), ((1, 512, 128, 128), "finalize", "finalize")]
_F16_GN = [((3, 64, 4, 4), "fold"), ((2, 1280, 8, 8), "small"), ((1, 128, 96, 80), "finalize"), ((2, 640, 32, 32), "finalize")]
_FP8_GN = [((2, 320, 64, 64), "finalize"), ((2, 1280, 8, 8), "small"), ((1, 640, 32, 32), "finalize"), ((1, 2560, 16, 16), "small")]
SUITE_GN = (
    [("test_ops_gpu::test_groupnorm", "f32", s, kf) for s, kf, _ in _OPS_GN]
    + [("test_ops_gpu::test_groupnorm", "bf16", s, kb) for s, _, kb in _OPS_GN]
    + [("test_ops_gpu::test_fullsize_groupnorm_affine_invariance", "f32", (16, 320, 64, 64), "fold")]
    + [("test_fp16_gpu::test_groupnorm_f16", d, s, k) for s, k in _F16_GN for d in H16]
    + [("test_fp8_gpu::test_groupnorm_fp8_output", "bf16", s, k) for s, k in _FP8_GN]
    + [("test_fp8_gpu::test_groupnorm_fp8_output", "bf16", (2, 320, 9, 29), "finalize"),
       ("test_fp8_gpu::test_groupnorm_fp8_output", "bf16", (2, 256, 5, 7), "small")]
    + [("test_fp8_calib_gpu::test_groupnorm_fp8_record", "bf16", s, k) for s, k in _FP8_GN]
)
# (test name, dtype, (rows, C), kernel)
_OPS_LN = [((4096, 320), "rowgroup", "wave_row"), ((1024, 640), "wave_row", "wave_row"), ((256, 1280), "wave_row", "wave_row"),
           ((7, 64), "wave_row", "wave_row"), ((130, 1280), "wave_row", "wave_row")]
_F16_LN = [((7, 64), "wave_row"), ((130, 1280), "wave_row"), ((1024, 640), "wave_row"), ((8192, 320), "rowgroup")]
_FP8_LN = [((4096, 320), "wave_row"), ((1024, 640), "wave_row"), ((256, 1280), "wave_row"), ((130, 1280), "wave_row")]
SUITE_LN = (
    [("test_ops_gpu::test_layernorm", "f32", s, kf) for s, kf, _ in _OPS_LN]
    + [("test_ops_gpu::test_layernorm", "bf16", s, kb) for s, _, kb in _OPS_LN]
    + [("test_ops_gpu::fused cross-attention helper", "bf16", (8192, 320), "rowgroup")]
    + [("test_fp16_gpu::test_layernorm_f16", d, s, k) for s, k in _F16_LN for d in H16]
    + [("test_fp8_gpu::test_layernorm_fp8_output", "bf16", s, k) for s, k in _FP8_LN]
    + [("test_fp8_gpu::test_layernorm_fp8_output", "bf16", (8197, 320), "rowgroup")]
    + [("test_fp8_calib_gpu::test_layernorm_fp8_record", "bf16", s, k) for s, k in _FP8_LN + [((8192, 320), "rowgroup"), ((8200, 640), "rowgroup")]]
)


def gn_plan(case, dtype, nosmall=False):
    """the hand-written plan of `case` in `dtype` as norm_plan_query's dict"""
    p = case.nosmall if nosmall else case.plan
    if isinstance(p, dict):
        p = p[dtype]
    return dict(zip(("kernel", "P", "nchunk", "npart", "wide"), p))


def ln_plan(case):
    return dict(zip(("kernel", "nv", "rows_per_block"), case.plan))


def gn_params():
    """(case, dtype, nosmall) of every GroupNorm launch the table describes"""
    out = []
    for c in GN_CASES:
        for d in c.dtypes:
            out.append((c, d, False))
            if c.nosmall is not None:
                out.append((c, d, True))
    return out


def gn_id(p):
    c, d, nosmall = p
    return "x".join(map(str, c.shape)) + f"-{d}" + ("-nosmall" if nosmall else "")


def ln_params():
    return [(c, d) for c in LN_CASES for d in c.dtypes]


def ln_id(p):
    c, d = p
    return f"{c.rows}x{c.C}-{d}"
