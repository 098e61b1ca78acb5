#!/usr/bin/env python
"""What regional prompts (af_set_regions) cost at BASELINE config 1's shape: SD-1.5 with synthetic weights (as
bench.py builds them), batch 8 -> CFG twin batch Bf = 16, 64x64 latents, bf16, for R - 1 = 2, 3, 4 vertical strips plus the base
prompt at weight 0.2 (unconditional legs (1, 0, ..)).

    (a) the time of one twin forward -- plain (one prompt of 77 keys), regions on the fused kernel, regions by composition (knob
        region_fused = 0) -- host clock around --burst forwards that end in a device synchronise, alternating within a round,
        best and worst of --reps rounds; and what each launches: attention launches (plan counters + fused region launches),
        conv / GEMM launches.
    (b) the fused kernel's time per site level (the profiler's event pairs around every launch, classes 25 + level) and the
        combine kernel's in the composition, in forwards of their own.
    (c) wall time of one DDIM sample() call, --steps steps: plain, regions fused, regions by composition.

    python scripts/region_mode.py [--out profiles/region_<commit>.txt]
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
ap.add_argument("--steps", type=int, default=20, help="DDIM steps of (c)")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--burst", type=int, default=5)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib  # noqa: E402
from adaface_amd import regions as RG  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402

N_CLS = 30                                   # AF_K_COUNT (af_common.h)
K_REGION, K_COMBINE = 25, 29                 # AF_K_REGION_ATTN (+ level), AF_K_REGION_COMBINE
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B = args.batch
say(f"regional prompts at config 1's shape: SD-1.5 synthetic weights, bf16, twin Bf = {2 * B}, 64x64 latents, vertical strips + base 0.2")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

model = build_model(dev, "bf16")
unet = model.model.diffusion_model
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
lib = _lib.load()
eng = unet.engine(dev)
t = torch.full((B,), 500, dtype=torch.long, device=dev)
out2 = torch.empty(2 * B, 4, 64, 64, device=dev)


def cond(seed, shared=False):
    return synth_context(B, seed=seed, device=dev, shared=shared)


c0, uc0 = cond(100), cond(101, shared=True)
probe = model.get_learned_conditioning(c0)
layerwise = bool(probe[2]["use_layerwise_context"]) if isinstance(probe, tuple) else False
ten = lambda c: c


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


def setup(n_strips):
    """(context of the 2 B samples, weights or None) for n_strips regions (0 = plain)"""
    if n_strips == 0:
        return torch.cat([ten(c0), ten(uc0)]), None
    regs = [ten(cond(110 + i)) for i in range(n_strips)]
    ctx = RG.concat_contexts([ten(c0)] + regs, ten(uc0))
    masks = RG.masks_from_boxes([(i / n_strips, 0.0, (i + 1) / n_strips, 1.0, 1.0) for i in range(n_strips)], 64, 64)
    return ctx, RG.build_weights(masks, 0.2, B, 2).to(dev)


fwd = lambda: eng.unet_forward_twin(x_T, t, out2)
say(f"(a) one twin U-Net forward (host clock around {args.burst} forwards to a device synchronise, {args.reps} rounds), and (b) kernels")
say("    forward                      best [ms]  worst [ms]   attention launches (fused region)   conv/GEMM launches")
for n_strips in (0, 2, 3, 4):
    ctx, w = setup(n_strips)
    for fused in ((1,) if n_strips == 0 else (1, 0)):
        _lib.set_knob("region_fused", fused)
        eng.set_context(ctx, 2 * B, layerwise=layerwise)
        eng.set_regions(w)
        fwd()
        best, worst = 1e9, 0.0
        for _ in range(args.reps):
            v = burst(fwd)
            best, worst = min(best, v), max(worst, v)
        _lib.plan_counts(reset=True)
        n0 = lib.af_region_attn_launches()
        fwd()
        torch.cuda.synchronize()
        pc = _lib.plan_counts(reset=True)
        nf = lib.af_region_attn_launches() - n0
        name = "plain, 77 keys" if n_strips == 0 else f"R = {n_strips + 1} {'fused' if fused else 'composition'}"
        say(f"    {name:26s} {1e3 * best:9.3f}  {1e3 * worst:9.3f}   {attn(pc) + nf:10d} ({nf:3d})   {conv_gemm(pc):26d}")
        if n_strips:
            ms, la = profiled(fwd, ((1 << 5) - 1) << K_REGION)
            if fused:
                say("        region_attn_kernel by level: " + ", ".join(
                    f"f = {1 << l}: {la[K_REGION + l]} launches {1e3 * ms[K_REGION + l]:.1f} us" for l in range(4)))
            else:
                say(f"        region_combine_kernel: {la[K_COMBINE]} launches {1e3 * ms[K_COMBINE]:.1f} us in all")
        eng.set_regions(None)
_lib.reset_knobs()
say()


def run(cc, ucc, weights, fused):
    _lib.set_knob("region_fused", fused)
    model.set_regions(weights)
    try:
        t0 = time.perf_counter()
        lat, _ = DDIMSampler(model).sample(S=args.steps, conditioning=cc, batch_size=B, shape=[4, 64, 64], verbose=False,
                                           guidance_scale=[10.0, 4.0], unconditional_conditioning=ucc, eta=0.0, x_T=x_T)
        torch.cuda.synchronize()
        assert torch.isfinite(lat).all()
        return time.perf_counter() - t0
    finally:
        model.set_regions(None)
        _lib.reset_knobs()


if True:
    say(f"(c) one DDIM sample() call, batch {B}, S = {args.steps} (host clock to a device synchronise, best of {args.reps} after a warm-up call)")
    for n_strips in (0, 2, 3, 4):
        ctx, w = setup(n_strips)
        cc, ucc = ctx[: ctx.shape[0] // 2].contiguous(), ctx[ctx.shape[0] // 2:].contiguous()
        cc, ucc = model.get_learned_conditioning(cc), model.get_learned_conditioning(ucc)
        for fused in ((1,) if n_strips == 0 else (1, 0)):
            run(cc, ucc, None if w is None else w.cpu(), fused)
            wall = min(run(cc, ucc, None if w is None else w.cpu(), fused) for _ in range(args.reps))
            name = "plain, 77 keys" if n_strips == 0 else f"R = {n_strips + 1} {'fused' if fused else 'composition'}"
            say(f"    {name:26s} {1e3 * wall:9.1f} ms   {B / wall:6.2f} latents/s")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
