"""The norm launch plan (af_plan_groupnorm / af_plan_layernorm through af_norm_plan_query: host code, no GPU) against the plans
tests/norm_cases.py writes out by hand, and the coverage that table is there for: every kernel of both plans, both sides of
every threshold, the finalize remainder loop, ragged last chunks on both chunked paths.  The launchers follow the same plan
(tests/test_norm_gpu.py runs it), so this is what tells which kernel a GPU test of a norm covered."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests import norm_cases as N  # noqa: E402


@pytest.fixture
def lib():
    from adaface_amd import _lib
    _lib.load()
    _lib.reset_knobs()
    yield _lib
    _lib.reset_knobs()


def _gn(lib, case, dtype, nosmall=False, pre_npart=0):
    B, C, H, W = case.shape
    lib.set_knob("gn_small", 0 if nosmall else 1)
    return lib.norm_plan_query("groupnorm", dtype, B=B, HW=H * W, C=C, pre_npart=pre_npart)


@pytest.mark.parametrize("p", N.gn_params(), ids=N.gn_id)
def test_groupnorm_plan_is_the_hand_written_one(lib, p):
    case, dtype, nosmall = p
    assert _gn(lib, case, dtype, nosmall) == N.gn_plan(case, dtype, nosmall), case.why


@pytest.mark.parametrize("p", N.ln_params(), ids=N.ln_id)
def test_layernorm_plan_is_the_hand_written_one(lib, p):
    case, dtype = p
    assert lib.norm_plan_query("layernorm", dtype, rows=case.rows, C=case.C) == N.ln_plan(case), case.why


def test_knob_off_moves_only_small_cases(lib):
    """gn_small = 0 changes the plan of exactly the cases the table marks as small"""
    for case in N.GN_CASES:
        for d in case.dtypes:
            on, off = _gn(lib, case, d), _gn(lib, case, d, nosmall=True)
            assert (on != off) == (case.nosmall is not None), (case.shape, d)
            assert (on["kernel"] == "small") == (case.nosmall is not None), (case.shape, d)


def test_table_reaches_every_kernel_and_both_sides_of_every_threshold(lib):
    gn = [(c, d, ns, _gn(lib, c, d, ns)) for c, d, ns in N.gn_params()]
    ln = [(c, d, lib.norm_plan_query("layernorm", d, rows=c.rows, C=c.C)) for c, d in N.ln_params()]
    assert {p["kernel"] for *_, p in gn} == set(lib.GN_KERNELS)
    assert {p["kernel"] for *_, p in ln} == set(lib.LN_KERNELS)

    def tail(c, p):
        return (c.shape[2] * c.shape[3]) % p["P"]
    fin = [(c, p) for c, _, _, p in gn if p["kernel"] == "finalize"]
    fold = [(c, p) for c, _, _, p in gn if p["kernel"] == "fold"]
    # gn_finalize_kernel: the remainder loop alone (< 57 chunks past none), the unrolled loop then the remainder, the unrolled loop alone
    assert any(p["nchunk"] % 64 != 0 and p["nchunk"] < 128 for _, p in fin)
    assert any(p["nchunk"] % 64 != 0 and p["nchunk"] > 128 for _, p in fin)
    assert any(p["nchunk"] % 64 == 0 for _, p in fin)
    # ragged last chunk on both chunked paths, and a whole one
    assert any(tail(c, p) for c, p in fin) and any(tail(c, p) for c, p in fold)
    assert any(tail(c, p) == 0 for c, p in fin + fold)
    # fold / finalize: 64 chunks is the last fold (the full-size case of the older suite), the table has both sides
    assert max(p["npart"] for _, p in fold) <= 64 < min(p["npart"] for _, p in fin)
    # the chunking loops: P untouched, raised by the batch, at the batch loop's cap, raised by the per-sample cap
    assert {4, 8, 64, 128} <= {p["P"] for _, p in fin + fold}
    # the wide statistics loop on and off, on both chunked paths
    assert {p["wide"] for _, p in fin} == {True, False} == {p["wide"] for _, p in fold}
    # the small kernel's 2560 items: at the limit and one map past it, per element size
    for d, at, past in (("f32", 1280, 1281), ("bf16", 2560, 2561), ("f16", 2560, 2561)):
        k = {c.shape[2] * c.shape[3]: p["kernel"] for c, dd, ns, p in gn if dd == d and not ns and c.shape[1] == 256}
        assert k[at] == "small" and k[past] == "finalize", (d, k)
    # refusals: C % 32 and C > 2560; one channel count just inside
    assert {c.shape[1] for c, _, _, p in gn if p["kernel"] == "refused"} == {48, 2592}
    assert any(c.shape[1] == 2560 and p["kernel"] != "refused" for c, _, _, p in gn)

    # LayerNorm: both sides of the row threshold per element size, of the 10 vectors per lane, of the lane-group divisibility,
    # of the 320 vectors a wave holds
    by = {(c.rows, c.C, d): p for c, d, p in ln}
    for d, lo, hi in (("bf16", 8191, 8197), ("f16", 8191, 8197), ("f32", 4095, 4099)):
        assert by[(lo, 320, d)]["kernel"] == "wave_row" and by[(hi, 320, d)]["kernel"] == "rowgroup"
    assert by[(8200, 640, "bf16")] == {"kernel": "rowgroup", "nv": 10, "rows_per_block": 32}
    assert by[(8200, 704, "bf16")]["kernel"] == "wave_row" and by[(8200, 328, "bf16")]["kernel"] == "wave_row"
    assert {p["nv"] for *_, p in ln if p["kernel"] == "rowgroup"} == {1, 5, 10}
    assert by[(5, 2560, "bf16")]["kernel"] == "wave_row" and by[(16, 2568, "bf16")]["kernel"] == "refused"
    # every row-group case has a ragged last workgroup
    assert all(c.rows % p["rows_per_block"] for c, _, p in ln if p["kernel"] == "rowgroup")


def test_exact_thresholds(lib):
    """the thresholds themselves, one step either side (shapes no GPU test needs to run)"""
    q = lib.norm_plan_query
    assert q("groupnorm", "bf16", B=1, HW=256, C=320)["kernel"] == "fold"          # 64 chunks
    assert q("groupnorm", "bf16", B=1, HW=257, C=320)["kernel"] == "finalize"      # 65
    assert q("groupnorm", "bf16", B=1, HW=4096, C=320)["P"] == 4                   # 1024 chunks: not yet doubled
    assert q("groupnorm", "bf16", B=1, HW=4097, C=320)["P"] == 8
    assert q("groupnorm", "bf16", B=1, HW=65536, C=32)["P"] == 64                  # 1024 chunks at the cap of the batch loop
    assert q("groupnorm", "bf16", B=1, HW=65537, C=32)["P"] == 128
    assert not q("groupnorm", "bf16", B=1, HW=400, C=2048)["wide"]                 # 256 vectors per pixel
    assert q("groupnorm", "f32", B=1, HW=700, C=1056)["wide"]                      # 264
    assert q("layernorm", "bf16", rows=8192, C=320)["kernel"] == "rowgroup"
    assert q("layernorm", "f32", rows=4096, C=320)["kernel"] == "rowgroup"
    assert q("layernorm", "f16", rows=8192, C=320) == q("layernorm", "bf16", rows=8192, C=320)


def test_producer_statistics_replace_the_chunk_count(lib):
    """pre_npart (a producer convolution's partial sums): no statistics pass, fold / finalize by that count, chunks unchanged"""
    q = lib.norm_plan_query
    assert q("groupnorm", "bf16", B=2, HW=4096, C=320, pre_npart=64) == {"kernel": "fold", "P": 8, "nchunk": 512, "npart": 64, "wide": False}
    assert q("groupnorm", "bf16", B=2, HW=16384, C=320, pre_npart=256)["kernel"] == "finalize"
    assert not q("groupnorm", "bf16", B=1, HW=4096, C=2560, pre_npart=64)["wide"] and q("groupnorm", "bf16", B=1, HW=4096, C=2560)["wide"]
    assert q("groupnorm", "bf16", B=2, HW=64, C=1280, pre_npart=1)["kernel"] == "small"   # the small kernel sums for itself


@pytest.mark.parametrize("name,dtype,shape,kernel", N.SUITE_GN, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_kernel_of_each_groupnorm_shape_in_the_older_tests(lib, name, dtype, shape, kernel):
    B, C, H, W = shape
    assert lib.norm_plan_query("groupnorm", dtype, B=B, HW=H * W, C=C)["kernel"] == kernel, name


@pytest.mark.parametrize("name,dtype,shape,kernel", N.SUITE_LN, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_kernel_of_each_layernorm_shape_in_the_older_tests(lib, name, dtype, shape, kernel):
    assert lib.norm_plan_query("layernorm", dtype, rows=shape[0], C=shape[1])["kernel"] == kernel, name


def test_query_rejects_bad_arguments(lib):
    out = (lib.C.c_int64 * 5)()
    for args in ((2, 0, 1, 16, 64, 0), (0, 7, 1, 16, 64, 0), (0, 0, 1, -1, 64, 0), (0, 0, 1, 1 << 31, 64, 0)):
        with pytest.raises(lib.AfError):
            lib.check(lib.load().af_norm_plan_query(*args, out), "af_norm_plan_query")
