#!/usr/bin/env python
"""What ControlNet (af_unet_set_control) costs at BASELINE config 1's shape: SD-1.5 with synthetic weights (as
bench.py builds them) plus a synthetic ControlNet, batch 8 -> CFG twin batch Bf = 16, 64x64 latents, 512x512 hint, bf16.

    (a) the time of one twin U-Net forward with control off, with residuals for both legs attached and with cond_only residuals
        attached (the add launch is the only difference); host clock around --burst forwards that end in a device synchronise,
        alternating within a round, best and worst of --reps rounds (worst minus best is the run-to-run spread).
    (b) the control forward alone, on Bf = 16 (both legs) and on B = 8 (cond_only), the same way; and the hint network, once.
    (c) the add kernel: its one launch with 13 segments beside 13 launches of itself with one segment each, on the residuals
        and concatenation-shaped buffers of the forward (the profiler's event pairs around every launch of its class).
    (d) a DeepCache reuse step of depth --depth: the truncated control forward and the U-Net's reuse step with its 2-segment add.
    (e) wall time of one sample() call (DDIM at S = --steps) with control off / both legs / cond_only / both legs under
        --deep-cache N.

    python scripts/controlnet_mode.py [--out profiles/controlnet_<commit>.txt]
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
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--deep-cache", dest="deep_cache", type=int, default=3)
ap.add_argument("--depth", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--burst", type=int, default=10)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib, layout, ops  # noqa: E402
from adaface_amd.ldm.modules.diffusionmodules.controlnet import SD15_CONTROLNET, ControlNet  # noqa: E402
from adaface_amd.synth import synth_context, synth_controlnet_state_dict, synth_hint  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402

N_CLS = 24                                   # AF_K_COUNT (af_common.h)
K_ADD = 23                                   # AF_K_CONTROL_ADD
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B = args.batch
say(f"ControlNet at config 1's shape: SD-1.5 synthetic weights, bf16, twin Bf = {2 * B}, 64x64 latents, one 512x512 hint")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

model = build_model(dev, "bf16")
unet = model.model.diffusion_model
net = ControlNet(**SD15_CONTROLNET)
net.load_control_state_dict(synth_controlnet_state_dict(layout.controlnet_param_shapes(**net._layout_kwargs()), seed=4321))
net = net.to(dev).set_compute_dtype("bf16")
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
hint = synth_hint(1, 46, 512, 512).to(dev)
c = model.get_learned_conditioning(synth_context(B, seed=100, device=dev))
uc = model.get_learned_conditioning(synth_context(B, seed=101, device=dev, shared=True))
lib = _lib.load()
eng, ceng = unet.engine(dev), net.engine(dev)
t = torch.full((B,), 500, dtype=torch.long, device=dev)
x2, t2 = torch.cat([x_T, x_T]), torch.cat([t, t])
out2 = torch.empty(2 * B, 4, 64, 64, device=dev)
ctx2 = torch.cat([c[0], uc[0]]) if isinstance(c, tuple) else torch.cat([c, uc])
ctx1 = c[0] if isinstance(c, tuple) else c
layerwise = bool(c[2]["use_layerwise_context"]) if isinstance(c, tuple) else False
scales = [1.0] * 13


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


def rounds(fns):
    best = {name: 1e9 for name, _, _ in fns}
    worst = {name: 0.0 for name, _, _ in fns}
    for name, pre, fn in fns:
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
    return best, worst


# ---------------------------------------------------------------- the hint, the residuals ------------------------------
torch.cuda.synchronize()
t0 = time.perf_counter()
ceng.control_set_hint(hint)
torch.cuda.synchronize()
first_hint = time.perf_counter() - t0
t0 = time.perf_counter()
ceng.control_set_hint(hint)
torch.cuda.synchronize()
hint_ms = time.perf_counter() - t0
ceng.set_context(ctx2, 2 * B, layerwise=layerwise)
flat2 = ceng.control_forward(x2, t2)
ceng.set_context(ctx1, B, layerwise=layerwise)
flat1 = ceng.control_forward(x_T, t)
eng.set_context(ctx2, 2 * B, layerwise=layerwise)


def off():
    eng.set_control(None)


def both():
    eng.set_control(flat2, scales, source=ceng, shape=(2 * B, 64, 64))


def cond():
    eng.set_control(flat1, scales, cond_only=True, source=ceng, shape=(B, 64, 64))


fwd = lambda: eng.unet_forward_twin(x_T, t, out2)
fns = (("control off", off, fwd), ("both legs", both, fwd), ("cond_only", cond, fwd))
best, worst = rounds(fns)
say(f"(a) one twin U-Net forward, Bf = {2 * B} (host clock around {args.burst} forwards to a device synchronise, {args.reps} alternating rounds)")
say("    residuals attached    best [ms]  worst [ms]")
for name, _, _ in fns:
    say(f"    {name:18s} {1e3 * best[name]:11.3f}  {1e3 * worst[name]:9.3f}")
say(f"    spread of the uncontrolled forward {1e3 * (worst['control off'] - best['control off']):.3f} ms; both legs - off "
    f"{1e3 * (best['both legs'] - best['control off']):.3f} ms, cond_only - off {1e3 * (best['cond_only'] - best['control off']):.3f} ms")
twin_ms = best["control off"]
off()
say()

# ---------------------------------------------------------------- (b) the control forward -----------------------------
buf2, buf1 = torch.empty_like(flat2), torch.empty_like(flat1)
fns = ((f"control Bf={2 * B}", lambda: ceng.set_context(ctx2, 2 * B, layerwise=layerwise), lambda: ceng.control_forward(x2, t2, out=buf2)),
       (f"control B={B}", lambda: ceng.set_context(ctx1, B, layerwise=layerwise), lambda: ceng.control_forward(x_T, t, out=buf1)))
cbest, cworst = rounds(fns)
say("(b) the control forward alone (13 residuals), the same clock")
for name, _, _ in fns:
    say(f"    {name:18s} {1e3 * cbest[name]:11.3f}  {1e3 * cworst[name]:9.3f}   {cbest[name] / twin_ms:5.3f} x the twin U-Net forward")
say(f"    hint network (1 x 3 x 512 x 512 -> 1 x 64 x 64 x 320), once per hint: {1e3 * hint_ms:.3f} ms (first call with its arena: {1e3 * first_hint:.3f} ms)")
say()

# ---------------------------------------------------------------- (c) the add kernel ----------------------------------
plan = eng.control_plan(64, 64)
srcs = [r.reshape(2 * B, -1, r.shape[-1]) for r in ceng.control_residuals(flat2, 2 * B, 64, 64)]
cats = [torch.zeros(2 * B, hh * ww, 2 * cc, device=dev, dtype=torch.bfloat16) for cc, hh, ww, _ in plan]
dsts = [cat[:, :, cc:] for cat, (cc, _, _, _) in zip(cats, plan)]
ops.control_add(dsts, srcs, scales)
one = min(profiled(lambda: ops.control_add(dsts, srcs, scales), 1 << K_ADD)[0][K_ADD] for _ in range(args.reps))
many = min(profiled(lambda: [ops.control_add([d], [s], [1.0]) for d, s in zip(dsts, srcs)], 1 << K_ADD)[0][K_ADD] for _ in range(args.reps))
nbytes = 3 * sum(s.numel() for s in srcs) * 2
say(f"(c) control_add_kernel on the {len(srcs)} residuals of Bf = {2 * B} into the skip halves of concatenation-shaped buffers ({nbytes / 1e6:.1f} MB moved)")
say(f"    one launch, 13 segments:   {1e3 * one:8.1f} us   ({nbytes / one / 1e9:.2f} TB/s)")
say(f"    13 launches, 1 segment:    {1e3 * many:8.1f} us in all (kernel time only: the 12 launch gaps are not in it)")
t_one = burst(lambda: ops.control_add(dsts, srcs, scales))
t_many = burst(lambda: [ops.control_add([d], [s], [1.0]) for d, s in zip(dsts, srcs)])
say(f"    host clock, {args.burst} back to back: one launch {1e6 * t_one:.1f} us per call, 13 launches {1e6 * t_many:.1f} us per set")
del cats, dsts, srcs
say()

# ---------------------------------------------------------------- (d) DeepCache reuse ---------------------------------
k = args.depth
ceng.set_context(ctx2, 2 * B, layerwise=layerwise)
both()
eng.unet_forward_cached(x_T, t, depth=k, mode="refresh", twin=True, out=out2)
flat_k = ceng.control_forward(x2, t2, n_blocks=k)
bufk = torch.empty_like(flat_k)


def reuse_on():
    eng.set_control(flat_k, scales[:k], source=ceng, shape=(2 * B, 64, 64))


fns = ((f"control, {k} blocks", None, lambda: ceng.control_forward(x2, t2, n_blocks=k, out=bufk)),
       ("reuse, controlled", reuse_on, lambda: eng.unet_forward_cached(x_T, t, depth=k, mode="reuse", twin=True, out=out2)))
dbest, dworst = rounds(fns)
say(f"(d) a DeepCache reuse step of depth {k}, Bf = {2 * B}")
for name, _, _ in fns:
    say(f"    {name:18s} {1e3 * dbest[name]:11.3f}  {1e3 * dworst[name]:9.3f}")
off()
eng.unet_cache_invalidate()
say()


# ---------------------------------------------------------------- (e) sample() ----------------------------------------
def run(setting, interval):
    if setting is None:
        unet.set_control(None)
    else:
        unet.set_control(net, hint, cond_only=(setting == "cond_only"))
    s = DDIMSampler(model)
    kw = {} if interval is None else dict(deep_cache_interval=interval, deep_cache_depth=k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lat, _ = s.sample(S=args.steps, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False, guidance_scale=[10.0, 4.0],
                      unconditional_conditioning=uc, eta=0.0, x_T=x_T, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(lat).all(), (setting, interval)
    return time.perf_counter() - t0


say(f"(e) one DDIM sample() call, S = {args.steps}, batch {B} (host clock to a device synchronise, best of {args.reps} after a warm-up call; no VAE decode)")
base = None
for setting, interval in ((None, None), ("both", None), ("cond_only", None), (None, args.deep_cache), ("both", args.deep_cache)):
    run(setting, interval)
    wall = min(run(setting, interval) for _ in range(args.reps))
    if setting is None and interval is None:
        base = wall
    say(f"    control {str(setting):10s} deep_cache {str(interval):4s}: {1e3 * wall:8.1f} ms   {B / wall:6.2f} latents/s   {wall / base:5.3f} x the uncontrolled run")
unet.set_control(None)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
