#!/usr/bin/env python
"""What seed-stable noise and the DPM-Solver++(2M) SDE step cost, at BASELINE config 1's shape: batch 8, 4 x 64 x 64 latents
(n = 131072 fp32 elements), SD-1.5 with synthetic weights for the sampler runs.

    (a) per-launch time, HIP events, best of --reps: one event pair around ONE launch, and one pair around --burst back-to-back
        launches divided by their number (as scripts/dpm_solver_mode.py measures af_dpmpp_step):
          af_dpmpp_sde_step with in-kernel noise (ONE launch),
          torch.randn + af_dpmpp_sde_step(noise_dev) (TWO launches, the form without a noise source),
          af_dpmpp_step (the deterministic step),
          af_philox_randn beside torch.randn for the same tensor.
    (b) bf16: wall time of DPMSolverSampler.sample at S = --dpm-steps, SDE (PhiloxNoise) against the deterministic solver.
Synthetic weights: nothing here says anything about image quality.

    python scripts/philox_noise_mode.py [--out profiles/philox_noise_<commit>.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--dpm-steps", dest="dpm_steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--burst", type=int, default=200)
ap.add_argument("--no-sampler", dest="sampler", action="store_false", help="(a) only: do not build the SD-1.5 model")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib, ops  # noqa: E402
from adaface_amd.noise import PhiloxNoise  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B, SD = args.batch, args.dpm_steps
say(f"Seed-stable noise and the DPM-Solver++(2M) SDE step at config 1's shape: batch {B}, 4 x 64 x 64 latents")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

# ---------------------------------------------------------------- (a) the kernels -----------------------------------
lib = _lib.load()
per = 4 * 64 * 64
n = B * per
g = torch.Generator().manual_seed(1)
x = torch.randn(n, generator=g).to(dev)
e = torch.randn(2 * n, generator=g).to(dev)
hist, out0, out1, z = (torch.empty(n, device=dev) for _ in range(4))
hist.normal_()
P, sp = _lib.ptr, _lib.stream_ptr()
co = [float(v) for v in ops.dpmpp_coeffs(0.30, 0.36, 0.12)]
cs = [float(v) for v in ops.dpmpp_sde_coeffs(0.30, 0.36, 0.12)]


def sde_fused():
    lib.af_dpmpp_sde_step(P(x), P(e[:n]), P(e[n:]), P(hist), n, 7.5, cs[0], cs[1], cs[2], cs[3], cs[5], cs[6], P(out0), P(out1), cs[4],
                          None, per, None, 0, 42, 3, sp)


def sde_two_launches():
    torch.randn(n, device=dev, out=z)
    lib.af_dpmpp_sde_step(P(x), P(e[:n]), P(e[n:]), P(hist), n, 7.5, cs[0], cs[1], cs[2], cs[3], cs[5], cs[6], P(out0), P(out1), cs[4],
                          P(z), per, None, 0, 0, 0, sp)


def deterministic():
    lib.af_dpmpp_step(P(x), P(e[:n]), P(e[n:]), P(hist), n, 7.5, co[0], co[1], co[2], co[3], co[4], co[5], P(out0), P(out1), sp)


def philox_randn():
    lib.af_philox_randn(P(z), B, per, None, 0, 42, 1, 3, sp)


def torch_randn():
    torch.randn(n, device=dev, out=z)


def bracket(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / count


FNS = ((sde_fused, "af_dpmpp_sde_step, in-kernel noise", 1, 6), (sde_two_launches, "torch.randn + af_dpmpp_sde_step(noise_dev)", 2, 8),
       (deterministic, "af_dpmpp_step", 1, 6), (philox_randn, "af_philox_randn", 1, 1), (torch_randn, "torch.randn", 1, 1))
for fn, *_ in FNS:
    for _ in range(20):
        fn()
torch.cuda.synchronize()
empty = lib.af_prof_event_overhead_us(sp, 64)
single = {fn.__name__: min(bracket(fn, 1) for _ in range(args.reps * 8)) for fn, *_ in FNS}
burst = {fn.__name__: [] for fn, *_ in FNS}
for _ in range(args.reps):                       # alternating, so a clock or neighbour drift hits all of them
    for fn, *_ in FNS:
        burst[fn.__name__].append(bracket(fn, args.burst))
say(f"(a) at n = {n} fp32 elements (HIP events; an empty event pair measures {empty:.2f} us)")
for fn, name, launches, streams in FNS:
    k = fn.__name__
    say(f"    {name:44s} one call per event pair, best of {args.reps * 8}: {single[k]:6.2f} us ({single[k] - empty:6.2f} us less the empty "
        f"pair);  {args.burst} calls per pair, best of {args.reps}: {min(burst[k]):6.2f} us per call  ({launches} launch{'es' if launches > 1 else ''}, "
        f"{streams} streams = {streams * n * 4 / 1e6:.2f} MB)")
say("    caveats: for the single-launch calls both figures are bounds on kernels of a few microseconds, not execution times.  One call")
say("    per pair adds the dispatch and the events' own cost (the empty pair measures only part of it); many calls per pair run at")
say("    the rate the host can enqueue them (ctypes, or torch's dispatcher for torch.randn).  A kernel time proper needs a kernel trace.")
say()

# ---------------------------------------------------------------- (b) the sampler ------------------------------------
if args.sampler:
    from adaface_amd.synth import synth_context  # noqa: E402
    from bench import build_model  # noqa: E402
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402
    model = build_model(dev, "bf16")
    g = torch.Generator().manual_seed(42)
    x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
    c = model.get_learned_conditioning(synth_context(B, seed=100, device=dev))
    uc = model.get_learned_conditioning(synth_context(B, seed=101, device=dev, shared=True))
    RUNS = (("deterministic (dpmsolver++)", {}), ("SDE, PhiloxNoise in-kernel", dict(algorithm="sde-dpmsolver++", noise_source=PhiloxNoise(42))),
            ("SDE, torch.randn + noise_dev", dict(algorithm="sde-dpmsolver++")))

    def run(kw):
        t0 = time.perf_counter()
        lat, _ = DPMSolverSampler(model).sample(S=SD, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False,
                                                guidance_scale=[10.0, 4.0], unconditional_conditioning=uc, x_T=x_T, skip_type="logSNR", **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(lat).all()
        return time.perf_counter() - t0

    for _, kw in RUNS:
        run(kw)
    wall = {name: [] for name, _ in RUNS}
    for _ in range(args.reps):
        for name, kw in RUNS:
            wall[name].append(run(kw))
    say(f"(b) bf16, batch {B}, S = {SD} logSNR: wall time of one sample() call (host clock to device synchronise, best of {args.reps}, "
        "runs alternating; no VAE decode)")
    for name, _ in RUNS:
        t = min(wall[name])
        say(f"    {name:32s} {1e3 * t:8.1f} ms   {B / t:6.2f} latents/s")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
