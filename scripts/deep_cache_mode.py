#!/usr/bin/env python
"""What DeepCache (af_unet_forward_cached) saves at BASELINE config 1's shape: SD-1.5 with synthetic weights (as
bench.py builds them), batch 8 -> CFG twin batch Bf = 16, 64x64 latents, bf16, annealed guidance [10, 4].

    (a) for depth k in 1, 2, 3: the time of one full forward (af_unet_forward_twin), of one refresh forward and of one reuse
        forward (host clock around --burst forwards that end in a device synchronise, best of --reps rounds, the three
        alternating within a round), and what each launches: conv / GEMM launches (the plan counters) and all kernel launches
        (the profiler's brackets, in a forward of their own).
    (b) wall time of one sample() call without DeepCache and with interval N in 2, 3, 5 (depth --depth): DDIMSampler at
        S = --steps and DPMSolverSampler (time_uniform) at S = --dpm-steps; and the final latent's rms deviation from the
        uncached run of the same sampler.
The deviation is measured on SYNTHETIC random weights, where a reuse step is no closer to the full forward than the previous
step's eps is: it says nothing about image quality.

    python scripts/deep_cache_mode.py [--out profiles/deep_cache_<commit>.txt]
"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50, help="DDIM steps of the benchmark")
ap.add_argument("--dpm-steps", dest="dpm_steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--depth", type=int, default=2, help="depth of the sampler runs in (b)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--burst", type=int, default=10)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402
from ldm.models.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B = args.batch
say(f"DeepCache at config 1's shape: SD-1.5 synthetic weights, bf16, twin Bf = {2 * B}, 64x64 latents, guidance [10, 4]")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

model = build_model(dev, "bf16")
unet = model.model.diffusion_model
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
c = model.get_learned_conditioning(synth_context(B, seed=100, device=dev))
uc = model.get_learned_conditioning(synth_context(B, seed=101, device=dev, shared=True))
lib = _lib.load()

# ---------------------------------------------------------------- (a) one forward ------------------------------------
# one sampler step sets the engine's context for the twin batch exactly as a run does
DDIMSampler(model).sample(S=1, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False, guidance_scale=[10.0, 4.0],
                          unconditional_conditioning=uc, eta=0.0, x_T=x_T)
eng = unet.engine(dev)
t = torch.full((B,), 500, dtype=torch.long, device=dev)
out = torch.empty(2 * B, 4, 64, 64, device=dev)


def conv_gemm(pc):
    return sum(pc[f"tile{i}"] for i in range(6)) + pc["halo"] + pc["fp8"] + pc["up_phase4"]


def all_launches(fn):
    lib.af_prof_reset()
    lib.af_prof_set_stride(1)
    lib.af_prof_enable(0x3ff)
    fn()
    torch.cuda.synchronize()
    lib.af_prof_enable(0)
    n = 10
    ms, la, fl, by = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)()
    lib.af_prof_collect(n, ms, la, fl, by)
    return int(sum(la))


def burst(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.burst):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.burst


say(f"(a) one U-Net forward (host clock around {args.burst} forwards to a device synchronise, best of {args.reps} alternating rounds)")
say("    depth   forward    time [ms]   conv/GEMM launches   all kernel launches")
for k in (1, 2, 3):
    fns = (("full", lambda: eng.unet_forward_twin(x_T, t, out)),
           ("refresh", lambda: eng.unet_forward_cached(x_T, t, depth=k, mode="refresh", twin=True, out=out)),
           ("reuse", lambda: eng.unet_forward_cached(x_T, t, depth=k, mode="reuse", twin=True, out=out)))
    best = {name: 1e9 for name, _ in fns}
    for name, fn in fns:                      # warm every shape (the reuse after its refresh)
        fn()
    for _ in range(args.reps):
        for name, fn in fns:
            best[name] = min(best[name], burst(fn))
    for name, fn in fns:
        _lib.plan_counts(reset=True)
        fn()
        torch.cuda.synchronize()
        n_gemm = conv_gemm(_lib.plan_counts(reset=True))
        say(f"    k = {k}   {name:8s} {1e3 * best[name]:9.3f}   {n_gemm:10d}   {all_launches(fn):14d}")
        if name == "refresh":                # (the profiled refresh is what the reuse rows read)
            fn()
say()


# ---------------------------------------------------------------- (b) the samplers -----------------------------------
def run(cls, steps, interval, **kw):
    s = cls(model)
    t0 = time.perf_counter()
    lat, _ = s.sample(S=steps, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False, guidance_scale=[10.0, 4.0],
                      unconditional_conditioning=uc, eta=0.0, x_T=x_T, deep_cache_interval=interval, deep_cache_depth=args.depth, **kw)
    torch.cuda.synchronize()
    return lat.clone(), time.perf_counter() - t0, s.deep_cache_log


def rms_dev(a, ref):
    return ((a - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


say(f"(b) one sample() call, batch {B}, depth k = {args.depth} (host clock to a device synchronise, best of {args.reps} after a warm-up call;")
say("    no VAE decode).  rms: the final latent against the uncached run of the same sampler, SYNTHETIC weights -- no quality claim")
for name, cls, steps, kw in (("DDIM", DDIMSampler, args.steps, {}), ("DPM-Solver++(2M)", DPMSolverSampler, args.dpm_steps, {})):
    ref, base = None, None
    for interval in (None, 2, 3, 5):
        lat, _, log = run(cls, steps, interval, **kw)
        wall = min(run(cls, steps, interval, **kw)[1] for _ in range(args.reps))
        assert torch.isfinite(lat).all(), (name, interval)
        if interval is None:
            ref, base = lat, wall
        say(f"    {name:17s} S = {steps:3d}  N = {str(interval):4s}: {1e3 * wall:8.1f} ms   {B / wall:6.2f} latents/s   {base / wall:5.2f} x uncached"
            f"   full forwards {log.count('full') + log.count('refresh'):3d} of {len(log):3d}   rms {rms_dev(lat, ref):.3e}")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
