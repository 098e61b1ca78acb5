"""CPU test of the samplers' host loops: every case of tests/golden/gen_sampler_traces.py (each sampler x the opt-in features,
their combinations and their refusals, on a stub model with the step kernels replaced by recording host functions) must give
the record -- model calls with their keywords and leg order, the ops' scalars, the three logs, the error a refusal raises --
that the commit named in tests/golden/sampler_traces.json gave."""
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import gen_sampler_traces as GT  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return json.loads(GT.TRACES.read_text())


def test_the_matrix_is_the_recorded_one(golden):
    assert len(golden["commit"]) == 40
    assert list(golden["cases"]) == GT.case_names()
    # what the matrix is there for: every sampler runs, refuses, and takes each branch of the model-call decision
    entries = {n: {r[0] for r in c["trace"]} for n, c in golden["cases"].items()}
    for s in GT.SAMPLERS:
        assert {"single", "twin"} <= entries[f"{s}:cfg"] | entries[f"{s}:no_uncond"]
        assert "pag" in entries[f"{s}:pag_adaptive"] and "single on [x; x]" in entries[f"{s}:no_twin_entry"]
        assert "error" in golden["cases"][f"{s}:refuse_sag_pag"] and golden["cases"][f"{s}:refuse_sag_pag"]["trace"] == []
    assert "sag_degrade" in entries["plms:sag_cfg"] and "tgate" in str(golden["cases"]["dpm:tgate_3"]["trace"])


@pytest.mark.parametrize("name", GT.case_names())
def test_case_reproduces_the_recorded_trace(golden, name):
    want, got = golden["cases"][name], GT.run_case(name)
    assert got.get("error") == want.get("error")
    for k, (w, g) in enumerate(zip(want["trace"], got["trace"])):
        assert g == w, f"{name}: record {k} of the trace"
    assert got == want
