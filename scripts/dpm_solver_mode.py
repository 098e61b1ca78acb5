#!/usr/bin/env python
"""What the DPM-Solver++(2M) sampler costs and how it behaves in the compute modes, at BASELINE config 1's shape: SD-1.5 with
synthetic weights (as bench.py builds them), batch 8 -> CFG batch Bf = 16, 64x64 latents, annealed guidance [10, 4].

    (a) per-launch time of af_dpmpp_step (guidance + history + x0 write: six streams) beside af_ddim_step (guidance + pred_x0:
        five streams) at n = 8*4*64*64, HIP events, best of --reps: one event pair around ONE launch (less what an empty pair
        measures), and one pair around --burst back-to-back launches divided by their number.
    (b) bf16: wall time of DPMSolverSampler.sample at S = --dpm-steps on both grids beside DDIMSampler.sample at S = --steps
        (host clock around a call that ends in a device synchronise, best of --reps after one warm-up call).
    (c) the final latent's deviation in the bf16 and fp16 modes from the f32 mode of the same sampler and grid, as max-abs / max
        and rms / rms, beside DDIM's at the same S.
Synthetic weights: nothing here says anything about image quality at 20 steps.

    python scripts/dpm_solver_mode.py [--out profiles/dpm_solver_<commit>.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50, help="DDIM steps of the benchmark, for (b)")
ap.add_argument("--dpm-steps", dest="dpm_steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--burst", type=int, default=200)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib, ops  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402
from ldm.models.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B, S, SD = args.batch, args.steps, args.dpm_steps
say(f"DPM-Solver++(2M) at config 1's shape: SD-1.5 synthetic weights, Bf = {2 * B}, 64x64 latents, guidance [10, 4]")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

# ---------------------------------------------------------------- (a) the step kernels ------------------------------
lib = _lib.load()
n = B * 4 * 64 * 64
g = torch.Generator().manual_seed(1)
x = torch.randn(n, generator=g).to(dev)
e = torch.randn(2 * n, generator=g).to(dev)
hist, out0, out1 = (torch.empty(n, device=dev) for _ in range(3))
hist.normal_()
P, sp = _lib.ptr, _lib.stream_ptr()
co = [float(v) for v in ops.dpmpp_coeffs(0.30, 0.36, 0.12)]


def launch_dpmpp():
    lib.af_dpmpp_step(P(x), P(e[:n]), P(e[n:]), P(hist), n, 7.5, co[0], co[1], co[2], co[3], co[4], co[5], P(out0), P(out1), sp)


def launch_ddim():
    lib.af_ddim_step(P(x), P(e[:n]), P(e[n:]), None, n, 7.5, 0.30, 0.36, 0.7 ** 0.5, 0.0, 1.0, P(out0), P(out1), sp)


def bracket(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / count


for fn in (launch_dpmpp, launch_ddim):
    for _ in range(20):
        fn()
torch.cuda.synchronize()
empty = lib.af_prof_event_overhead_us(sp, 64)
single = {fn.__name__: min(bracket(fn, 1) for _ in range(args.reps * 8)) for fn in (launch_dpmpp, launch_ddim)}
burst = {"launch_dpmpp": [], "launch_ddim": []}
for _ in range(args.reps):                       # alternating, so a clock or neighbour drift hits both
    for fn in (launch_dpmpp, launch_ddim):
        burst[fn.__name__].append(bracket(fn, args.burst))
say(f"(a) step kernels at n = {n} fp32 elements (HIP events; an empty event pair measures {empty:.2f} us)")
for name, fn, streams in (("af_dpmpp_step", "launch_dpmpp", 6), ("af_ddim_step", "launch_ddim", 5)):
    say(f"    {name:14s} one launch per event pair, best of {args.reps * 8}: {single[fn]:6.2f} us ({single[fn] - empty:6.2f} us less the empty pair);"
        f"  {args.burst} launches per pair, best of {args.reps}: {min(burst[fn]):6.2f} us per launch"
        f"  ({streams} streams = {streams * n * 4 / 1e6:.2f} MB)")
say("    caveats: both figures are bounds on a kernel of about a microsecond, not its execution time.  One launch per pair adds the")
say("    dispatch and the events' own cost (the empty pair measures only part of it); many launches per pair run at the rate the")
say("    host can enqueue them through ctypes, which is slower than the kernel.  A kernel time proper needs a kernel trace.")
say()

# ---------------------------------------------------------------- (b), (c) the samplers -----------------------------
model = build_model(dev, "f32")
unet = model.model.diffusion_model
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
c_emb = synth_context(B, seed=100, device=dev)
uc_emb = synth_context(B, seed=101, device=dev, shared=True)
RUNS = (("DDIM", SD, {}), ("DPM-Solver++ time_uniform", SD, dict(skip_type="time_uniform")),
        ("DPM-Solver++ logSNR", SD, dict(skip_type="logSNR")))


def run(name, steps, kw, c, uc):
    cls = DDIMSampler if name == "DDIM" else DPMSolverSampler
    t0 = time.perf_counter()
    lat, _ = cls(model).sample(S=steps, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False, guidance_scale=[10.0, 4.0],
                               unconditional_conditioning=uc, eta=0.0, x_T=x_T, **kw)
    torch.cuda.synchronize()
    return lat.clone(), time.perf_counter() - t0


lat, wall = {}, {}
for mode in ("f32", "bf16", "fp16"):
    unet.set_compute_dtype("f32" if mode != "f32" else "bf16")       # a fresh engine in `mode`
    model.set_compute_dtype(mode)
    c, uc = model.get_learned_conditioning(c_emb), model.get_learned_conditioning(uc_emb)
    for name, steps, kw in RUNS:
        lat[name, mode], _ = run(name, steps, kw, c, uc)
        assert torch.isfinite(lat[name, mode]).all(), (name, mode)
    if mode == "bf16":
        for name, steps, kw in RUNS + (("DDIM", S, {}),):
            wall[name, steps] = min(run(name, steps, kw, c, uc)[1] for _ in range(args.reps))

say(f"(b) bf16, batch {B}: wall time of one sample() call (host clock to device synchronise, best of {args.reps}; no VAE decode)")
base = wall["DDIM", S]
for (name, steps), t in wall.items():
    say(f"    {name:28s} S = {steps:3d}: {1e3 * t:8.1f} ms   {B / t:6.2f} latents/s   {base / t:5.2f} x the rate of DDIM S = {S}")
say()


def dev_of(a, ref):
    d = (a - ref).double()
    return d.abs().max().item() / ref.abs().max().item(), (d.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


say(f"(c) final latent at S = {SD}: deviation from the f32 mode of the same sampler and grid      max-abs / max|.|    rms / rms")
for name, _, _ in RUNS:
    for mode in ("bf16", "fp16"):
        m, r = dev_of(lat[name, mode], lat[name, "f32"])
        say(f"    {name:28s} {mode:5s} {m:10.3e}      {r:10.3e}")
m, r = dev_of(lat["DPM-Solver++ logSNR", "f32"], lat["DDIM", "f32"])
say(f"    (two different solvers, f32: DPM-Solver++ logSNR against DDIM at S = {SD}: {m:.3e} / {r:.3e}; synthetic weights, no quality claim)")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
