#!/usr/bin/env python
"""What img2img by strength and inpainting (af_noise_blend) cost at BASELINE config 1's shape: SD-1.5 with
synthetic weights (as bench.py builds them), batch 8, 64x64 latents, bf16.

    (a) the blend in front of a sampler step: the fused launch (noise generated in the kernel, and noise read from a tensor)
        beside the torch composition it replaces -- noise (af_philox_randn, or torch.randn), q_sample (three element-wise
        launches) and img_orig * mask + (1. - mask) * img (four more).  Host clock around --burst calls that end in a device
        synchronise, alternating within a round, best and worst of --reps rounds; the kernel's own time from the profiler's
        event pairs; launch counts as counted (the fused call) and as torch issues them (the composition).
    (b) the results are the same bits (the claim the timings are about).
    (c) wall time of one sample() call (DDIM at S = --steps): txt2img, inpainting with the composition, inpainting with the
        fused blend, img2img at strength 0.5 (expected near half the steps' time), and one VAE encode of the batch.

    python scripts/inpaint_mode.py [--out profiles/inpaint_<commit>.txt]
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--burst", type=int, default=200)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib, img2img, ops  # noqa: E402
from adaface_amd.noise import STREAM_QSAMPLE, PhiloxNoise  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402

N_CLS = 25                                   # AF_K_COUNT (af_common.h)
K_BLEND = 24                                 # AF_K_NOISE_BLEND
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B = args.batch
say(f"img2img / inpainting at config 1's shape: SD-1.5 synthetic weights, bf16, batch {B}, 64x64 latents")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

model = build_model(dev, "bf16")
lib = _lib.load()
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
img = (torch.rand(B, 3, 512, 512, generator=g) * 2.0 - 1.0).to(dev)
repaint = torch.zeros(B, 1, 512, 512)
repaint[:, :, 128:384, 128:384] = 1.0                      # the middle quarter of the image is repainted
keep = img2img.repaint_to_keep(repaint).to(dev)
c = model.get_learned_conditioning(synth_context(B, seed=100, device=dev))
uc = model.get_learned_conditioning(synth_context(B, seed=101, device=dev, shared=True))
src = PhiloxNoise(42)
t_int = 500
ts = torch.full((B,), t_int, dtype=torch.long, device=dev)
sa, s1 = float(model.sqrt_alphas_cumprod[t_int]), float(model.sqrt_one_minus_alphas_cumprod[t_int])


def burst(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.burst):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.burst


def rounds(fns):
    best = {name: 1e9 for name, _ in fns}
    worst = {name: 0.0 for name, _ in fns}
    for _, fn in fns:
        fn()
    for _ in range(args.reps):
        for name, fn in fns:
            v = burst(fn)
            best[name], worst[name] = min(best[name], v), max(worst[name], v)
    return best, worst


# ---------------------------------------------------------------- one VAE encode ---------------------------------------
img2img.encode_image(model, img)
torch.cuda.synchronize()
t0 = time.perf_counter()
x0 = img2img.encode_image(model, img)
torch.cuda.synchronize()
encode_s = time.perf_counter() - t0


# ---------------------------------------------------------------- (a) the blend ----------------------------------------
def comp_philox():
    img_orig = model.q_sample(x0, ts, noise=src.randn(x0.shape, STREAM_QSAMPLE, 3, dev))
    return img_orig * keep + (1. - keep) * x_T


def comp_torch():
    return model.q_sample(x0, ts) * keep + (1. - keep) * x_T


def fused_philox():
    return ops.noise_blend(x_T, x0, keep, sa, s1, seed=src.seed, step=3)


z = src.randn(x0.shape, STREAM_QSAMPLE, 3, dev)


def fused_noise():
    return ops.noise_blend(x_T, x0, keep, sa, s1, noise=z)


def fused_randn():
    return ops.noise_blend(x_T, x0, keep, sa, s1, noise=torch.randn_like(x0))


def torch_launches(fn):
    """Device kernels one call issues, from torch's own profiler (the count only; its timings are not used)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
               and "Memset" not in e.name)


def kernel_us(fn):
    lib.af_prof_reset()
    lib.af_prof_set_stride(1)
    lib.af_prof_enable(1 << K_BLEND)
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    lib.af_prof_enable(0)
    ms, la, fl, by = (C.c_double * N_CLS)(), (C.c_int64 * N_CLS)(), (C.c_double * N_CLS)(), (C.c_double * N_CLS)()
    lib.af_prof_collect(N_CLS, ms, la, fl, by)
    return 1e3 * ms[K_BLEND] / max(la[K_BLEND], 1), by[K_BLEND] / max(la[K_BLEND], 1)


fns = (("composition, Philox noise", comp_philox), ("fused, noise in the kernel", fused_philox),
       ("composition, torch.randn", comp_torch), ("fused, torch.randn tensor", fused_randn), ("fused, noise tensor given", fused_noise))
best, worst = rounds(fns)
counts = {}
for name, fn in fns:
    try:
        counts[name] = torch_launches(fn)
    except Exception as e:       # (the count is a convenience: the timings stand without it)
        counts[name] = f"n/a ({type(e).__name__})"
say(f"(a) the blend in front of one sampler step, [{B}, 4, 64, 64] fp32 latents, keep mask [{B}, 1, 64, 64] "
    f"(host clock around {args.burst} calls to a device synchronise, {args.reps} alternating rounds)")
say("    form                          best [us]  worst [us]  device launches per call")
for name, _ in fns:
    say(f"    {name:28s} {1e6 * best[name]:10.1f}  {1e6 * worst[name]:10.1f}  {counts[name]}")
before = _lib.noise_blend_launches()
fused_philox()
say(f"    af_noise_blend launches counted for one fused call: {_lib.noise_blend_launches() - before}")
for name, fn in (("noise in the kernel", fused_philox), ("noise tensor given", fused_noise)):
    us, nbytes = kernel_us(fn)
    say(f"    noise_blend_kernel, {name}: {us:.1f} us per launch between event pairs ({nbytes / 1e6:.2f} MB moved; at this size the "
        f"launch, not the bandwidth, is what is timed)")
say(f"    fused / composition: Philox {best['fused, noise in the kernel'] / best['composition, Philox noise']:.3f}, "
    f"torch.randn {best['fused, torch.randn tensor'] / best['composition, torch.randn']:.3f}")
say()

# ---------------------------------------------------------------- (b) the same bits ------------------------------------
same = torch.equal(fused_philox(), comp_philox()) and torch.equal(fused_noise(), comp_philox())
say(f"(b) fused == composition, bit for bit: {same}")
assert same
say()


# ---------------------------------------------------------------- (c) sample() -----------------------------------------
def run(**kw):
    s = DDIMSampler(model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lat, _ = s.sample(S=args.steps, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False, guidance_scale=[10.0, 4.0],
                      unconditional_conditioning=uc, eta=0.0, x_T=x_T, noise_source=PhiloxNoise(42), **kw)
    if kw.get("fused_blend"):
        lat = img2img.finish(lat, x0, keep)
    torch.cuda.synchronize()
    assert torch.isfinite(lat).all(), kw
    return time.perf_counter() - t0


say(f"(c) one DDIM sample() call, S = {args.steps}, batch {B} (host clock to a device synchronise, best / worst of {args.reps} after a "
    f"warm-up call; no VAE decode)")
cases = (("txt2img", {}), ("inpaint, torch composition", dict(mask=keep, x0=x0)),
         ("inpaint, fused blend + finish", dict(mask=keep, x0=x0, fused_blend=True)),
         ("img2img, strength 0.5", dict(x0=x0, strength=0.5)),
         ("inpaint, strength 0.5, fused", dict(mask=keep, x0=x0, strength=0.5, fused_blend=True)))
for _, kw in cases:
    run(**kw)
walls = {name: [] for name, _ in cases}
for _ in range(args.reps):
    for name, kw in cases:
        walls[name].append(run(**kw))
base = min(walls["txt2img"])
for name, _ in cases:
    w = walls[name]
    say(f"    {name:32s} {1e3 * min(w):8.1f} / {1e3 * max(w):8.1f} ms   {min(w) / base:5.3f} x txt2img")
say(f"    one VAE encode of the batch (8 x 3 x 512 x 512 -> x0), once per run: {1e3 * encode_s:.1f} ms")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
