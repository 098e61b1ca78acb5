"""The checks that make tests/test_ln_fold_gpu.py mean something before it runs (no GPU): the stage bounds of
tests/ln_fold_ref.py are achievable -- a CPU emulation of the chain with the kernels' arithmetic stays inside every one of them
on every case's inputs -- and discriminating -- each of eight mistakes a kernel could make leaves the bound of ITS stage on a
stated share of rows or columns; the input conditions the bounds lean on hold; the cases reach the kernels they name; and the
operator's refusals, which come before the device is touched."""
import ctypes as C
import math
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests import gemm_plan_cases as G  # noqa: E402
from tests import ln_fold_ref as R  # noqa: E402
from tests.test_ops_gpu import TOL  # noqa: E402

CPU_M = 224   # rows of the CPU cases: 32 of the sigma = 0.05 rows, 14 groups of 16 rows
NAMES = sorted(R.CHAINS)
KERNEL_NAME = {G.K_PP: "pp", G.K_ROWPANEL: "rowpanel", G.K_M128: "m128"}
TILED_KNOBS = (("geglu_rowpanel", 0), ("gemm_m128", 0))


@pytest.fixture
def lib():
    from adaface_amd import _lib
    _lib.load()
    _lib.reset_knobs()
    yield _lib
    _lib.reset_knobs()


def _layout(name):
    return R.LAYOUT_OF[R.EXPECT[name][0][0]]


def planned(lib, name):
    """((kernel name, row-panel kind) of the producer, of the folded consumer) from af_gemm_plan_query at the current knobs"""
    M, Kp, Cn, N, _, res, geglu = R.CHAINS[name]
    p = lib.gemm_plan_query(*G.linear_args(G.BF16, M, Kp, Cn, residual=res, flags=G.LN_PRODUCER))
    c = lib.gemm_plan_query(*G.linear_args(G.BF16, M, Cn, N, geglu=geglu, flags=G.LN_CONSUMER))
    assert p[3] == 1 and c[3] == 1, (p, c)   # one K slice each
    return (KERNEL_NAME.get(p[0], p[0]), p[1]), (KERNEL_NAME.get(c[0], c[0]), c[1])


@pytest.mark.parametrize("name", NAMES)
def test_cases_reach_the_kernels_they_name(lib, name):
    assert planned(lib, name) == R.EXPECT[name]
    for k, v in TILED_KNOBS:
        lib.set_knob(k, v)
    assert planned(lib, name) == (("pp", 0), ("pp", 0))


def test_cases_cover_every_kernel_family_on_both_sides():
    prod = {R.EXPECT[n][0] for n in NAMES}
    cons = {R.EXPECT[n][1] for n in NAMES}
    assert prod == {("rowpanel", 2), ("pp", 0), ("m128", 0)}
    assert cons == {("rowpanel", 1), ("rowpanel", 2), ("rowpanel", 4), ("rowpanel", 5), ("m128", 0)}
    assert any(R.CHAINS[n][0] % 256 for n in NAMES)   # a ragged last panel


@pytest.mark.parametrize("name", NAMES)
def test_input_conditions(name):
    c = R.named_case(name, M=CPU_M)
    for k in ("a", "wp", "res", "wc"):
        assert c[k] is None or torch.equal(R.rb(c[k]), c[k]), f"{k} is not bf16-representable"
    ic = R.input_conditions(c)
    assert ic["ratio"] <= R.RATIO_CAP, ic                      # the cancellation the S3 bound scales with
    assert 1.5 <= ic["offset"] <= 2.5 and ic["offset_mean"] >= 0.5, ic   # row means up to 2 sigma: mu * colsum matters
    assert abs(ic["small_rows"] - 1 / 7) < 1e-9, ic            # every 7th row
    assert ic["eps_share"] >= 1e-3, ic                         # eps is at least 1e-3 of var + eps on some row
    g, b = c["gamma"], c["beta"]
    assert 0.1 < float(g.std()) < 0.3 and abs(float(g.mean()) - 1) < 0.05 and 0.1 < float(b.std()) < 0.3


@pytest.mark.parametrize("name", NAMES)
def test_emulation_stays_inside_every_bound(name):
    c = R.named_case(name, M=CPU_M)
    for layout in {_layout(name), "slab80"}:
        f = R.check_chain(c, R.emulate(c, layout), layout)
        assert f["wf_equal"], f
        for s in R.STAGES:
            assert f[s] <= 1.0, (layout, s, f)
        assert f["e_folded"] < TOL["bf16"] and f["e_plain"] < TOL["bf16"], f
        assert f["gate_max"] <= R.GATE_RANGE, f


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_a_mistake_leaves_the_bound_of_its_stage(variant):
    stage, floor = R.VARIANT_STAGE[variant]
    names = [n for n in NAMES if R.CHAINS[n][6]] if variant == "geglu_unpermuted" else NAMES
    for name in names[:2] + names[-2:]:
        c = R.named_case(name, M=CPU_M)
        layout = _layout(name)
        good = R.share_outside(c, R.emulate(c, layout), layout, stage)
        bad = R.share_outside(c, R.emulate(c, layout, variant), layout, stage)
        assert good == 0.0, (name, stage, good)
        assert bad >= floor, (name, variant, stage, bad)


def test_gelu_formula_allowance_is_the_measured_one():
    err, at = R.measure_gelu_fit()
    assert 0.99 * R.GELU_FIT_ERR <= err <= 1.001 * R.GELU_FIT_ERR, (err, at)
    x = torch.linspace(-R.GATE_RANGE, R.GATE_RANGE, 2 ** 20 + 1, dtype=torch.float64)
    slope = 0.5 * (1 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    assert float(slope.abs().max()) <= R.GELU_LIPSCHITZ


def _refusal(lib, dtype, M, Kp, Cn, N, geglu=0, parts_n=0):
    """af_op_ln_chain on null tensors: a refusal comes back before anything is allocated or launched"""
    plans = (C.c_int * 10)()
    rc = lib.load().af_op_ln_chain(dtype, *([None] * 6), 1e-5, None, None, M, Kp, Cn, N, geglu, parts_n, 20, 256, *([None] * 8),
                                   plans, None)
    return rc, lib.load().af_last_error().decode()


def test_operator_refuses_before_it_touches_the_device(lib):
    M, Kp, Cn, N = R.REFUSED
    rc, msg = _refusal(lib, G.BF16, M, Kp, Cn, N)
    assert rc == -1 and "plans no LayerNorm epilogue" in msg and "producer" in msg, (rc, msg)
    rc, msg = _refusal(lib, G.BF16, 4096, 320, 320, 960)       # too few rows for any eight-wave kernel
    assert rc == -1 and "plans no LayerNorm epilogue" in msg, (rc, msg)
    M, Kp, Cn, N = R.CHAINS["64_rp_bias_res__n960"][:4]
    for dtype in (G.F32, G.F16):                               # the launcher refuses LayerNorm flags on these
        rc, msg = _refusal(lib, dtype, M, Kp, Cn, N)
        assert rc == -1 and "bf16" in msg, (rc, msg)
    rc, msg = _refusal(lib, G.BF16, M, Kp, Cn, N, parts_n=8)   # the producer writes 4 slabs
    assert rc == -1 and "writes 4 statistics slabs" in msg and "handed 8" in msg, (rc, msg)
    rc, msg = _refusal(lib, G.BF16, M, Kp, Cn, N + 1)
    assert rc == -1, (rc, msg)
