#!/usr/bin/env python
"""Write tests/golden/gemm_plans.npz: the plan of every launch of tests/gemm_plan_cases.py as the built library decides it.

    python scripts/dump_gemm_plans.py [--out FILE]

Host only (af_gemm_plan_query touches no device).  tests/test_gemm_plan_cpu.py compares the library with this table row by
row; regenerate it only for a deliberate planner change, and read the diff of the plans that moved.
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests import gemm_plan_cases as G  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "tests" / "golden" / "gemm_plans.npz")
    a = ap.parse_args()
    cs = G.cases()
    args = np.array([c[0] for c in cs], dtype=np.int64)
    knob = np.array([c[1] for c in cs], dtype=np.int16)
    plans = np.array(G.run(cs), dtype=np.int64)
    np.savez_compressed(a.out, args=args, knob=knob, plans=plans)
    print(f"{len(cs)} cases -> {a.out} ({a.out.stat().st_size} bytes); kernels seen: {sorted(set(plans[:, 0].tolist()))}, "
          f"row-panel kinds: {sorted(set(plans[:, 1].tolist()))}")
