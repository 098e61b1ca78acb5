#!/usr/bin/env python
"""What T-GATE (af_tgate_set) saves at BASELINE config 1's shape: SD-1.5 with synthetic weights (as bench.py
builds them), batch 8 -> CFG twin batch Bf = 16, 64x64 latents, bf16, annealed guidance [10, 4].

    (a) the time of one forward -- the twin forward (Bf = 16), the capture forward (twin), the plain forward of B = 8 and the
        replay forward of B = 8 -- host clock around --burst forwards that end in a device synchronise, the four alternating
        within a round, best and worst of --reps rounds (the worst minus the best is the run-to-run spread of that number);
        and what each launches: conv / GEMM launches, attention launches (the plan counters), all kernel launches (the
        profiler's brackets, in a forward of its own).
    (b) the add kernel's own time in a capture and in a replay forward (the profiler's event pairs around every launch of its
        class, in forwards of their own).
    (c) wall time of one sample() call for g in off, n / 2, n / 3: DDIMSampler at S = --steps and DPMSolverSampler
        (time_uniform) at S = --dpm-steps, each without DeepCache and with --deep-cache N; and the final latent's rms deviation
        from the ungated run of the same sampler and DeepCache setting.
    (d) the same deviation on an f32-mode model at batch --dev-batch (no timing): the change T-GATE itself makes, without
        bf16's rounding in it.
The deviations are measured on SYNTHETIC random weights, where cross-attention outputs do not converge as a trained model's
do: they say nothing about image quality, which is the paper's claim and not this script's.

    python scripts/tgate_mode.py [--out profiles/tgate_<commit>.txt]
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
ap.add_argument("--deep-cache", dest="deep_cache", type=int, default=3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--burst", type=int, default=10)
ap.add_argument("--dev-batch", dest="dev_batch", type=int, default=2, help="batch of the f32-mode deviation runs; 0 = skip (d)")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402
from ldm.models.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402

N_CLS = 23                                   # AF_K_COUNT (af_common.h)
K_TGATE = 22                                 # AF_K_TGATE_ADD
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B = args.batch
say(f"T-GATE at config 1's shape: SD-1.5 synthetic weights, bf16, twin Bf = {2 * B} / single leg B = {B}, 64x64 latents, guidance [10, 4]")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

model = build_model(dev, "bf16")
unet = model.model.diffusion_model
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
c = model.get_learned_conditioning(synth_context(B, seed=100, device=dev))
uc = model.get_learned_conditioning(synth_context(B, seed=101, device=dev, shared=True))
lib = _lib.load()
eng = unet.engine(dev)
t = torch.full((B,), 500, dtype=torch.long, device=dev)
out2, out1 = torch.empty(2 * B, 4, 64, 64, device=dev), torch.empty(B, 4, 64, 64, device=dev)
ctx2 = torch.cat([c[0], uc[0]]) if isinstance(c, tuple) else torch.cat([c, uc])
ctx1 = c[0] if isinstance(c, tuple) else c
layerwise = bool(c[2]["use_layerwise_context"]) if isinstance(c, tuple) else False


def conv_gemm(pc):
    return sum(pc[f"tile{i}"] for i in range(6)) + pc["halo"] + pc["fp8"] + pc["up_phase4"]


def attn(pc):
    return sum(v for k, v in pc.items() if k.startswith("attn_")) + pc["xattn_fused"] + pc["conv_attn_short"]


def profiled(fn, mask):
    lib.af_prof_reset()
    lib.af_prof_set_stride(1)
    lib.af_prof_enable(mask)
    fn()
    torch.cuda.synchronize()
    lib.af_prof_enable(0)
    ms, la, fl, by = (C.c_double * N_CLS)(), (C.c_int64 * N_CLS)(), (C.c_double * N_CLS)(), (C.c_double * N_CLS)()
    lib.af_prof_collect(N_CLS, ms, la, fl, by)
    return list(ms), list(la)


def burst(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.burst):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.burst


# ---------------------------------------------------------------- (a) one forward ------------------------------------
# the twin forms run on the context of 2 B samples, the plain forward on that of B; a replay needs none.  The context set is
# outside the timed window, as it is outside a sampler's steps (it is hoisted per run).
def set2():
    eng.set_context(ctx2, 2 * B, layerwise=layerwise)


def set1():
    eng.set_context(ctx1, B, layerwise=layerwise)


fns = (("twin   Bf=%d" % (2 * B), set2, lambda: eng.unet_forward_twin(x_T, t, out2)),
       ("capture (twin)", set2, lambda: eng.unet_forward_twin(x_T, t, out2, tgate="capture")),
       ("plain  B=%d" % B, set1, lambda: eng.unet_forward(x_T, t, out1)),
       ("replay B=%d" % B, None, lambda: eng.unet_forward(x_T, t, out1, tgate="replay")))
best = {name: 1e9 for name, _, _ in fns}
worst = {name: 0.0 for name, _, _ in fns}
for name, pre, fn in fns:                     # warm every shape (the replay after its capture)
    if pre:
        pre()
    fn()
for _ in range(args.reps):
    for name, pre, fn in fns:
        if pre:
            pre()
        fn()
        v = burst(fn)
        best[name], worst[name] = min(best[name], v), max(worst[name], v)
say(f"(a) one U-Net forward (host clock around {args.burst} forwards to a device synchronise, {args.reps} alternating rounds)")
say("    forward           best [ms]  worst [ms]   conv/GEMM launches   attention launches   all kernel launches")
for name, pre, fn in fns:
    if pre:
        pre()
    fn()
    _lib.plan_counts(reset=True)
    fn()
    torch.cuda.synchronize()
    pc = _lib.plan_counts(reset=True)
    n_all = int(sum(profiled(fn, (1 << N_CLS) - 1)[1]))
    say(f"    {name:16s} {1e3 * best[name]:9.3f}  {1e3 * worst[name]:9.3f}   {conv_gemm(pc):10d}   {attn(pc):16d}   {n_all:16d}")
pl, rp, tw = "plain  B=%d" % B, "replay B=%d" % B, "twin   Bf=%d" % (2 * B)
say(f"    replay / plain: {best[rp] / best[pl]:.3f} (best / best); spread of the plain forward {1e3 * (worst[pl] - best[pl]):.3f} ms, "
    f"of the replay {1e3 * (worst[rp] - best[rp]):.3f} ms, difference {1e3 * (best[pl] - best[rp]):.3f} ms")
say(f"    replay / twin: {best[rp] / best[tw]:.3f}")
say()

# ---------------------------------------------------------------- (b) the kernel -------------------------------------
say("(b) tgate_add_kernel in one forward (event pairs around every launch of its class)")
set2()
ms, la = profiled(lambda: eng.unet_forward_twin(x_T, t, out2, tgate="capture"), 1 << K_TGATE)
say(f"    capture: {la[K_TGATE]:3d} launches, {1e3 * ms[K_TGATE]:8.1f} us in all")
ms, la = profiled(lambda: eng.unet_forward(x_T, t, out1, tgate="replay"), 1 << K_TGATE)
say(f"    replay:  {la[K_TGATE]:3d} launches, {1e3 * ms[K_TGATE]:8.1f} us in all")
say()


# ---------------------------------------------------------------- (c) the samplers -----------------------------------
def run(mdl, cls, steps, gate, interval, cc, ucc, xT):
    s = cls(mdl)
    t0 = time.perf_counter()
    lat, _ = s.sample(S=steps, conditioning=cc, batch_size=xT.shape[0], shape=[4, 64, 64], verbose=False,
                      guidance_scale=[10.0, 4.0], unconditional_conditioning=ucc, eta=0.0, x_T=xT, tgate_step=gate,
                      deep_cache_interval=interval, deep_cache_depth=2)
    torch.cuda.synchronize()
    return lat.clone(), time.perf_counter() - t0, s


def rms_dev(a, ref):
    return ((a - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


say(f"(c) one sample() call, batch {B} (host clock to a device synchronise, best of {args.reps} after a warm-up call; no VAE decode).")
say("    rms: the final latent against the ungated run of the same sampler and DeepCache setting, SYNTHETIC weights -- no quality claim")
for name, cls, steps in (("DDIM", DDIMSampler, args.steps), ("DPM-Solver++(2M)", DPMSolverSampler, args.dpm_steps)):
    for interval in (None, args.deep_cache):
        ref, base = None, None
        for gate in (None, steps // 2, steps // 3):
            lat, _, s = run(model, cls, steps, gate, interval, c, uc, x_T)
            wall = min(run(model, cls, steps, gate, interval, c, uc, x_T)[1] for _ in range(args.reps))
            assert torch.isfinite(lat).all(), (name, gate, interval)
            if gate is None:
                ref, base = lat, wall
            full = s.deep_cache_log.count("full") + s.deep_cache_log.count("refresh")
            say(f"    {name:17s} S = {steps:3d}  deep_cache {str(interval):4s}  g = {str(gate):4s}: {1e3 * wall:8.1f} ms   {B / wall:6.2f} latents/s"
                f"   {wall / base:5.3f} x ungated   replay steps {s.tgate_log.count('replay'):3d} of {len(s.tgate_log):3d}"
                f"   full forwards {full:3d}   rms {rms_dev(lat, ref):.3e}")
say()

# ---------------------------------------------------------------- (d) f32-mode deviation -----------------------------
if args.dev_batch > 0:
    del model, unet, eng
    torch.cuda.empty_cache()
    Bd = args.dev_batch
    m32 = build_model(dev, "f32")
    c32 = m32.get_learned_conditioning(synth_context(Bd, seed=100, device=dev))
    uc32 = m32.get_learned_conditioning(synth_context(Bd, seed=101, device=dev, shared=True))
    say(f"(d) f32 mode, batch {Bd}: rms deviation of the final latent from the ungated run (SYNTHETIC weights -- no quality claim)")
    for name, cls, steps in (("DDIM", DDIMSampler, args.steps), ("DPM-Solver++(2M)", DPMSolverSampler, args.dpm_steps)):
        ref = run(m32, cls, steps, None, None, c32, uc32, x_T[:Bd])[0]
        for gate in (steps // 2, steps // 3):
            lat = run(m32, cls, steps, gate, None, c32, uc32, x_T[:Bd])[0]
            say(f"    {name:17s} S = {steps:3d}  g = {gate:3d}: rms {rms_dev(lat, ref):.3e}")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
