"""Hires fix: a first pass at the model's native size, an upscale of its result, and a second img2img pass at the target
size.  Not part of the reference; opt-in.

    size = target_size(h_lat, w_lat, scale=1.5)                    # the second pass's latent sides, multiples of 8
    second = second_kwargs(first, steps=20)                        # pass one's sampler arguments with the derived noise source
    lat2, lat1 = two_pass(sampler, first, second, size, "latent", strength=0.7)

SD-1.5 composes well near 512 x 512 only; asked directly for 768 or 1024 it repeats subjects.  The second pass starts from the
upscaled composition noised to `strength` of the schedule (sample(x0=, strength=), ldm/models/diffusion/blend.py), so it adds
detail at the target size and keeps the composition.

This file is host logic only: the resampling is ops.resample2d (csrc/af_resample.hip), one launch per call; the pixel
upscalers go through the first stage's decoder and encoder.
"""
from __future__ import annotations

import torch

from . import ops

# upscaler -> (space, resampling mode).  "latent*" resample the latent itself (the "Latent" upscalers of the common front
# ends); "pixel-*" decode, resample the image, clamp to [-1, 1] and encode (the posterior's mode)
UPSCALERS = ("latent", "latent-bicubic", "latent-nearest", "pixel-bicubic", "pixel-lanczos")
_MODES = {"latent": ("latent", "bilinear"), "latent-bicubic": ("latent", "bicubic"), "latent-nearest": ("latent", "nearest-exact"),
          "pixel-bicubic": ("pixel", "bicubic"), "pixel-lanczos": ("pixel", "lanczos3")}
MAX_SCALE = 4.0


def _round8(v: float) -> int:
    return int(v / 8.0 + 0.5) * 8


def target_size(h_lat, w_lat, scale=None, size=None):
    """The second pass's latent sides (h, w) from the first pass's: by `scale` in (1, 4], or an explicit latent `size` (h, w);
    not both.  Each side is rounded to the nearest multiple of 8 (halves up) and must end no smaller than the first pass's."""
    h_lat, w_lat = int(h_lat), int(w_lat)
    if h_lat < 1 or w_lat < 1:
        raise ValueError(f"hires: first-pass latent sides {h_lat} x {w_lat}")
    if (scale is None) == (size is None):
        raise ValueError("hires: give a scale or a size (one of them)")
    if scale is not None:
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not (1.0 < float(scale) <= MAX_SCALE):
            raise ValueError(f"hires: scale {scale!r} (a number in (1, {MAX_SCALE:g}])")
        h, w = _round8(h_lat * float(scale)), _round8(w_lat * float(scale))
    else:
        if len(size) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in size):
            raise ValueError(f"hires: size {size!r} (two positive integers, the latent sides)")
        h, w = _round8(size[0]), _round8(size[1])
    if h < h_lat or w < w_lat:
        raise ValueError(f"hires: target latent {h} x {w} is smaller than the first pass's {h_lat} x {w_lat} (upscaling only)")
    return h, w


@torch.no_grad()
def upscale_latent(model, latent, size, upscaler="latent"):
    """The clean latent of pass two, [B, C, size[0], size[1]] fp32, from pass one's result `latent`."""
    if upscaler not in _MODES:
        raise ValueError(f"hires: upscaler {upscaler!r} (one of {', '.join(UPSCALERS)})")
    space, mode = _MODES[upscaler]
    h, w = int(size[0]), int(size[1])
    latent = latent.to(torch.float32).contiguous()
    if space == "latent":
        return ops.resample2d(latent, (h, w), mode)
    from . import img2img
    img = model.decode_first_stage(latent).to(torch.float32).contiguous()
    f = img.shape[2] // latent.shape[2]
    up = ops.resample2d(img, (h * f, w * f), mode).clamp_(-1.0, 1.0)
    return img2img.encode_image(model, up)


def second_kwargs(first: dict, steps=None) -> dict:
    """Pass two's sampler arguments from pass one's: the same sampler settings, S = steps if given, and a PhiloxNoise source
    replaced by its derive("hires"), so that pass two's start, step and blend noise are uncorrelated with pass one's and still a
    pure function of (seed, global sample index).  shape, x_T, x0 and strength are two_pass's to set."""
    second = {k: v for k, v in first.items() if k not in ("shape", "x_T", "x0", "strength", "mask")}
    if steps:
        second["S"] = int(steps)
    src = second.get("noise_source")
    if src is not None:
        second["noise_source"] = src.derive("hires")
    return second


def two_pass(sampler, first: dict, second: dict, size, upscaler="latent", strength=0.7, noise=None):
    """sampler.sample(**first); upscale_latent of its result to the latent `size`; sampler.sample(**second, shape=, x0=, strength=,
    x_T=noise).  Returns (latent2, latent1).  noise: the N(0, 1) tensor added to the upscaled latent, or None: the sampler's own
    (second's noise_source, else torch.randn).  Resolution-bound model state (regions, a ControlNet hint, a hybrid model's concat
    condition) is the caller's to clear."""
    for name, kw in (("first", first), ("second", second)):
        bad = [k for k in ("mask", "x0") if kw.get(k) is not None]
        if bad:
            raise NotImplementedError(f"hires: {name} carries {', '.join(k + '=' for k in bad)}: the passes are txt2img and the "
                                      "img2img of its upscaled result, neither takes an image or a mask of its own")
    bad = [k for k in ("shape", "strength", "x_T") if k in second]
    if bad:
        raise ValueError(f"hires: second carries {', '.join(k + '=' for k in bad)}, which two_pass sets itself")
    latent1, _ = sampler.sample(**first)
    up = upscale_latent(sampler.model, latent1, size, upscaler)
    latent2, _ = sampler.sample(**second, shape=[int(up.shape[1]), int(size[0]), int(size[1])], x0=up, strength=strength, x_T=noise)
    return latent2, latent1
