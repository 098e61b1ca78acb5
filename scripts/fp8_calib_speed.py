#!/usr/bin/env python
"""Does a calibrated fp8 forward cost what the fixed-scale one costs?  (Same kernels, other constants: shown, not assumed.)

SD-1.5 UNet, synthetic weights, the benchmark's CFG batch (af_unet_forward_twin, Bf = 16, 64x64 latents) in fp8 mode.  One
process, after warm-up: rounds of [N forwards with every shift at 3 | N forwards with calibrated shifts], alternating, HIP
events around each block of N.  Prints one JSON line: ms per forward per round and mode, medians, and the spread (max - min
over the rounds) of each mode.

    python scripts/fp8_calib_speed.py                     # this tree: fixed and calibrated
    python scripts/fp8_calib_speed.py --root OTHER_TREE   # another checkout's package + library (e.g. the parent commit,
                                                          # which has no calibration): its fixed mode only
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", type=str, default=str(Path(__file__).resolve().parents[1]), help="tree whose adaface_amd is timed")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--forwards", type=int, default=20, help="forwards per timed block (>= 20)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None, help="also append the JSON line to this file")
    opt = ap.parse_args()
    sys.path.insert(0, opt.root)
    import torch
    from adaface_amd.engine import Engine
    from adaface_amd.synth import synth_context, synth_weights_into

    dev = torch.device("cuda", 0)
    unet = dict(in_channels=4, model_channels=320, out_channels=4, num_res_blocks=2, attention_resolutions=[4, 2, 1],
                channel_mult=[1, 2, 4, 4], num_heads=8, context_dim=768, transformer_depth=1)
    eng = Engine(dtype="bf16", unet=unet)
    synth_weights_into(eng, eng.tensor_table(), seed=51, device=dev)
    g = torch.Generator().manual_seed(52)
    x = torch.randn(8, 4, 64, 64, generator=g).to(dev)
    t = torch.full((8,), 501, dtype=torch.long, device=dev)
    ctx = torch.cat([synth_context(8, seed=100, device=dev), synth_context(8, seed=101, device=dev, shared=True)])
    eng.set_context(ctx, 16, layerwise=True)
    eng.set_fp8(True)
    out = torch.empty(16, 4, 64, 64, device=dev)
    fwd = lambda: eng.unet_forward_twin(x, t, out)   # noqa: E731
    modes = {"fixed": None}
    if hasattr(eng, "calibrate_fp8"):
        cal = eng.calibrate_fp8(fwd, passes=2, headroom=1)
        modes["calibrated"] = {n: s for n, (_, s, _) in cal.items()}
        eng.set_fp8_shifts(None)
    for _ in range(opt.warmup):
        fwd()
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    for _ in range(opt.rounds):
        for m, shifts in modes.items():
            if len(modes) > 1:
                eng.set_fp8_shifts(shifts)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(opt.forwards):
                fwd()
            e1.record()
            e1.synchronize()
            ms[m].append(e0.elapsed_time(e1) / opt.forwards)
    res = {"what": "fp8 twin forward Bf=16, ms per forward", "root": opt.root, "forwards_per_block": opt.forwards,
           "rounds": {m: [round(v, 4) for v in vs] for m, vs in ms.items()},
           "median": {m: round(statistics.median(vs), 4) for m, vs in ms.items()},
           "spread": {m: round(max(vs) - min(vs), 4) for m, vs in ms.items()}}
    if "calibrated" in modes:
        res["shifts"] = sorted(set(modes["calibrated"].values()))
    line = json.dumps(res)
    print(line)
    if opt.out:
        with open(opt.out, "a") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
