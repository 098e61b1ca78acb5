"""The conv / linear planner against the table its predecessor wrote (tests/golden/gemm_plans.npz): af_gemm_plan_query is host
code, so every decision -- kernel, row-panel kind, tile, K slices, halo, tile order, workspace -- is checked without a GPU.  The
table was dumped (scripts/dump_gemm_plans.py) from the decision chain as the launcher used to walk it by hand, before the plan
named its kernel; a planner change that moves a launch shows here as the case and both plans."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests import gemm_plan_cases as G  # noqa: E402


@pytest.fixture(scope="module")
def table():
    d = np.load(ROOT / "tests" / "golden" / "gemm_plans.npz")
    return d["args"], d["knob"], d["plans"]


def _show(args, knob, plan):
    return f"{dict(zip(G.ARGS, args))} knob {G.KNOBS[knob]}: {dict(zip(G.OUTS, plan))}"


def test_plans_match_the_golden_table(table):
    args, knob, plans = table
    cs = G.cases()
    assert 0 < len(cs) < 30000 and len(cs) == len(plans)
    assert [tuple(r) for r in args.tolist()] == [c[0] for c in cs] and knob.tolist() == [c[1] for c in cs], "case list and table differ"
    got = G.run(cs)
    bad = [i for i, (g, w) in enumerate(zip(got, plans.tolist())) if list(g) != w]
    for i in bad[:20]:
        print(f"case {i} {_show(cs[i][0], cs[i][1], plans[i].tolist())}\n  now: {dict(zip(G.OUTS, got[i]))}")
    assert not bad, f"{len(bad)} of {len(cs)} plans differ from the table (first 20 printed)"


def test_table_reaches_every_kernel_and_rowpanel_kind(table):
    _, _, plans = table
    assert set(plans[:, 0].tolist()) == set(range(10))          # every AfGemmKernel value
    assert set(plans[:, 1].tolist()) == {0, 1, 2, 3, 4, 5}
    # the sub-kind belongs to row-panel launches only, sliced K to kernels that can reduce it
    assert ((plans[:, 1] != 0) == (plans[:, 0] == G.K_ROWPANEL)).all()
    assert (plans[np.isin(plans[:, 0], (G.K_ROWPANEL, G.K_M128, G.K_UP_PHASE4, G.K_HALO4)), 3] == 1).all()
    assert ((plans[:, 6] != 0) == (plans[:, 3] > 1)).all()


def test_table_carries_the_plans_the_gpu_tests_pin(table):
    args, knob, plans = table
    index = {(tuple(a), k): i for i, (a, k) in enumerate(zip(args.tolist(), knob.tolist()))}
    for name, a, k, want in G.anchors():
        row = dict(zip(G.OUTS, plans[index[(a, k)]].tolist()))
        assert {f: row[f] for f in want} == want, (name, row)
