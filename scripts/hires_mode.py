#!/usr/bin/env python
"""What the hires fix (adaface_amd/hires.py, af_resample2d) costs: SD-1.5 with synthetic weights (as bench.py builds
them), bf16, batch --batch, 512 x 512 -> 768 x 768.

    (a) the resampling kernel alone, between HIP events around --burst back-to-back calls, beside F.interpolate on the device:
        [8, 4, 64, 64] -> 96 x 96 bilinear (the `latent` upscaler) and [8, 3, 512, 512] -> 768 x 768 bicubic (`pixel-bicubic`);
        launches per call as the library counts them; the largest difference between the two.
    (b) hires.two_pass with the `latent` upscaler, DDIM S = --steps, strength 0.7: pass one's sample() at 64 x 64 latents, the
        upscale, and pass two's sample() at 96 x 96, each to a device synchronise (host clock, best of --reps after a warm-up).
    (c) what a pixel upscaler adds: decode_first_stage at 512 x 512, the resampling, encode_image at 768 x 768.

    python scripts/hires_mode.py [--out profiles/hires_<commit>.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--burst", type=int, default=20)
ap.add_argument("--skip-samplers", dest="skip_samplers", action="store_true")
ap.add_argument("--skip-pixel", dest="skip_pixel", action="store_true")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import hires, img2img, ops  # noqa: E402
from adaface_amd.noise import PhiloxNoise  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def between_events(fn):
    """us per call: HIP events around --burst back-to-back calls, best of --reps"""
    fn()
    best = float("inf")
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.burst):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, 1e3 * e0.elapsed_time(e1) / args.burst)
    return best


def wall(fn):
    """(result, seconds): host clock around one call that ends in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


B = args.batch
say(f"Hires fix 512 x 512 -> 768 x 768: SD-1.5 synthetic weights, bf16, batch {B}")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

# ---------------------------------------------------------------- (a) the kernel -------------------------------------
g = torch.Generator().manual_seed(42)
say(f"(a) the resampling kernel alone (us per call: HIP events around {args.burst} back-to-back calls, best of {args.reps}) beside")
say("    F.interpolate(align_corners=False) on the device; launches per call counted by the library")
say("    case                                         kernel [us]   torch [us]   launches   GB/s (kernel)   max |kernel - torch|")
for shape, size, mode in (((8, 4, 64, 64), (96, 96), "bilinear"), ((8, 3, 512, 512), (768, 768), "bicubic")):
    x = torch.randn(*shape, generator=g).to(dev)
    y = torch.empty(shape[0], shape[1], *size, device=dev)
    n0 = ops.resample2d_launches()
    ops.resample2d(x, size, mode, out=y)
    n1 = ops.resample2d_launches()
    ref = F.interpolate(x, size=size, mode=mode, align_corners=False)
    diff = float((y - ref).abs().max())
    t_k = between_events(lambda: ops.resample2d(x, size, mode, out=y))
    t_t = between_events(lambda: F.interpolate(x, size=size, mode=mode, align_corners=False))
    gbs = 4.0 * (x.numel() + y.numel()) / (t_k * 1e-6) / 1e9          # the bytes the op must move: read x once, write y once
    say(f"    {str(list(shape)):18s} -> {size[0]} x {size[1]} {mode:9s} {t_k:10.1f}   {t_t:10.1f}   {n1 - n0:8d}   {gbs:13.1f}   {diff:.3e}")
say()

if not (args.skip_samplers and args.skip_pixel):
    from bench import build_model  # noqa: E402
    from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402
    model = build_model(dev, "bf16")
    c = model.get_learned_conditioning(synth_context(B, seed=100, device=dev))
    uc = model.get_learned_conditioning(synth_context(B, seed=101, device=dev, shared=True))

# ---------------------------------------------------------------- (b) the two passes ---------------------------------
lat1 = None
if not args.skip_samplers:
    S = args.steps
    first = dict(S=S, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False, guidance_scale=[10.0, 4.0],
                 unconditional_conditioning=uc, eta=0.0, noise_source=PhiloxNoise(42))
    second = hires.second_kwargs(first)
    sampler = DDIMSampler(model)
    times = {"pass one": [], "upscale": [], "pass two": []}
    for rep in range(args.reps + 1):                        # (the first round is the warm-up of both sizes)
        (lat1, _), t1 = wall(lambda: sampler.sample(**first))
        up, tu = wall(lambda: hires.upscale_latent(model, lat1, (96, 96), "latent"))
        (lat2, _), t2 = wall(lambda: sampler.sample(**second, shape=[4, 96, 96], x0=up, strength=0.7, x_T=None))
        assert torch.isfinite(lat2).all() and tuple(lat2.shape) == (B, 4, 96, 96)
        if rep:
            for k, v in (("pass one", t1), ("upscale", tu), ("pass two", t2)):
                times[k].append(v)
    say(f"(b) hires.two_pass by its parts, DDIM S = {S}, guidance [10, 4], upscaler latent, strength 0.7 (host clock to a device")
    say(f"    synchronise, best of {args.reps} after a warm-up round; no VAE decode)")
    say(f"    pass one  sample() at 64 x 64 latents, {S} steps:          {1e3 * min(times['pass one']):9.1f} ms")
    say(f"    upscale   ops.resample2d 64 x 64 -> 96 x 96 bilinear:      {1e3 * min(times['upscale']):9.3f} ms")
    say(f"    pass two  sample() at 96 x 96 latents, {int(S * 0.7)} of {S} steps:    {1e3 * min(times['pass two']):9.1f} ms")
    say(f"    pass two / pass one per step: {(min(times['pass two']) / int(S * 0.7)) / (min(times['pass one']) / S):.2f} x")
    say()

# ---------------------------------------------------------------- (c) a pixel upscaler -------------------------------
if not args.skip_pixel:
    if lat1 is None:
        lat1 = torch.randn(B, 4, 64, 64, generator=g).to(dev)
    try:
        best = {"decode": float("inf"), "resample": float("inf"), "encode": float("inf")}
        for rep in range(args.reps + 1):
            img, td = wall(lambda: model.decode_first_stage(lat1).float().contiguous())
            up, tr = wall(lambda: ops.resample2d(img, (768, 768), "bicubic").clamp_(-1.0, 1.0))
            x0, te = wall(lambda: img2img.encode_image(model, up))
            if rep:
                best = {"decode": min(best["decode"], td), "resample": min(best["resample"], tr), "encode": min(best["encode"], te)}
        assert tuple(x0.shape) == (B, 4, 96, 96) and torch.isfinite(x0).all()
        say(f"(c) the pixel-bicubic upscaler by its parts, batch {B} (host clock to a device synchronise, best of {args.reps} after a warm-up)")
        say(f"    decode_first_stage [{B}, 4, 64, 64] -> 512 x 512:           {1e3 * best['decode']:9.1f} ms")
        say(f"    ops.resample2d 512 x 512 -> 768 x 768 bicubic + clamp:    {1e3 * best['resample']:9.3f} ms")
        say(f"    encode_image 768 x 768 -> [{B}, 4, 96, 96]:                 {1e3 * best['encode']:9.1f} ms")
    except torch.OutOfMemoryError as e:
        say(f"(c) the pixel upscaler at batch {B}: UNMEASURED, out of memory ({str(e).splitlines()[0]})")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
