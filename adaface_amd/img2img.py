"""img2img by strength and inpainting: the front end.  Not part of the reference; opt-in.

    x0   = encode_image(model, img)                      # the clean latent of an image in [-1, 1]
    keep = repaint_to_keep(repaint)                      # image-resolution repaint mask (1 = repaint) -> latent keep mask
    lat, _ = sampler.sample(..., x0=x0, mask=keep, strength=0.75, fused_blend=True)
    lat  = finish(lat, x0, keep)                         # the kept region is x0 itself, without the last step's noise

img2img is the same call without mask=.  A hybrid model (the 9-channel sd-v1-5-inpainting U-Net) also takes
model.set_concat_cond(concat_cond(model, img, repaint)) before the run.  The samplers' side is
ldm/models/diffusion/blend.py, the arithmetic af_noise_blend (csrc/af_inpaint.hip); what runs once per run (mask preparation)
is torch.
"""
from __future__ import annotations

import torch

from . import ops
from .noise import STREAM_QSAMPLE

# the posterior's noise, when encode_image is asked to sample with a PhiloxNoise: stream 2 at the last step of the keying
# contract (step < 2^24), which no sampler loop reaches -- the blends draw from stream 2 at their loop index
POSTERIOR_STEP = (1 << 24) - 1


def _binary(repaint):
    if repaint.dim() != 4 or repaint.shape[1] != 1:
        raise ValueError(f"repaint mask: [B, 1, H, W] in [0, 1] expected, got {tuple(repaint.shape)}")
    return (repaint > 0.5).to(torch.float32)


def repaint_to_keep(repaint, f=8):
    """Image-resolution repaint mask [B, 1, H, W] in [0, 1] (1 = repaint) -> latent keep mask [B, 1, H / f, W / f] =
    1 - maxpool_f(repaint > 0.5): a latent cell with any repainted pixel is repainted."""
    rb = _binary(repaint)
    if rb.shape[2] % f or rb.shape[3] % f:
        raise ValueError(f"repaint mask: sides {tuple(rb.shape[2:])} must be multiples of {f}")
    return 1.0 - torch.nn.functional.max_pool2d(rb, kernel_size=f, stride=f)


@torch.no_grad()
def encode_image(model, img, noise_source=None):
    """x0 of an image [B, 3, H, W] in [-1, 1]: the mode of the first stage's posterior times model.scale_factor.
    noise_source: None = the mode; a tensor = the posterior sampled with it as its N(0, 1) noise; a PhiloxNoise = sampled with
    that source's stream 2 at step POSTERIOR_STEP (ids as the source's)."""
    post = model.encode_first_stage(img.to(model.device, torch.float32))
    if noise_source is None:
        return model.get_first_stage_encoding(post.mode())
    if isinstance(noise_source, torch.Tensor):
        noise = noise_source.to(model.device, torch.float32)
    else:
        noise = noise_source.randn(post.mean.shape, STREAM_QSAMPLE, POSTERIOR_STEP, model.device)
    return post.sample(noise=noise, scale=model.scale_factor)


@torch.no_grad()
def concat_cond(model, img, repaint, f=8):
    """The condition a hybrid model concatenates onto its latent, [B, 1 + z, H / f, W / f]: the latent-resolution repaint
    mask (1 = repaint; max-pooled as repaint_to_keep) and the encoding of the image with the repainted pixels blanked."""
    rb = _binary(repaint).to(img.device)
    small = 1.0 - repaint_to_keep(rb, f)
    masked = encode_image(model, img * (1.0 - rb))
    return torch.cat([small.to(masked.device), masked], dim=1)


def finish(latent, x0, keep):
    """The clean final blend, one launch: x0 * keep + (1 - keep) * latent.  The loop's last blend is at the smallest
    timestep's noise level, which leaves that noise in the kept region; this puts x0 itself there."""
    return ops.noise_blend(latent, x0, keep, 1.0, 0.0)


def pick_shard(items, n_samples: int, lo: int, hi: int, what="--img2img"):
    """This rank's items of a list given as one for all samples or one per GLOBAL sample index: [lo, hi) of the latter, the
    single one hi - lo times of the former."""
    items = list(items)
    if len(items) == 1:
        return items * (hi - lo)
    if len(items) != n_samples:
        raise ValueError(f"{what}: one, or one per sample ({n_samples}), got {len(items)}")
    return items[lo:hi]


def load_image(path, h, w):
    """RGB, resized to h x w, [-1, 1], [1, 3, h, w]."""
    import numpy as np
    from PIL import Image
    a = np.array(Image.open(path).convert("RGB").resize((w, h), resample=Image.LANCZOS)).astype(np.float32) / 255.0
    return 2.0 * torch.from_numpy(a[None].transpose(0, 3, 1, 2)).clamp(0.0, 1.0) - 1.0


def load_mask(path, h, w):
    """Greyscale, resized to h x w, [0, 1] (white = repaint), [1, 1, h, w]."""
    import numpy as np
    from PIL import Image
    a = np.array(Image.open(path).convert("L").resize((w, h), resample=Image.BILINEAR)).astype(np.float32) / 255.0
    return torch.from_numpy(a[None, None]).clamp(0.0, 1.0)


def load_batch(paths, n_samples, lo, hi, h, w, loader, what):
    """[hi - lo, C, h, w]: this rank's images (pick_shard), each file read once."""
    mine = pick_shard(paths, n_samples, lo, hi, what)
    read = {p: loader(p, h, w) for p in dict.fromkeys(mine)}
    return torch.cat([read[p] for p in mine])


def ckpt_in_channels(path):
    """The input channels of the U-Net in a checkpoint file (conv_in's weight), or None when it has no such tensor."""
    key = "model.diffusion_model.input_blocks.0.0.weight"
    if path.endswith(".safetensors"):
        from safetensors import safe_open
        with safe_open(path, framework="pt", device="cpu") as f:
            return int(f.get_slice(key).get_shape()[1]) if key in f.keys() else None
    sd = torch.load(path, map_location="cpu", weights_only=True)
    sd = sd.get("state_dict", sd)
    return int(sd[key].shape[1]) if key in sd else None


def select_hybrid(config, ckpt=None):
    """Make `config` (the dict / OmegaConf of load_config or sd15_config) a hybrid model's when its U-Net, or the checkpoint's,
    has more input than output channels: in_channels from the checkpoint, conditioning_key "hybrid".  Returns whether it is."""
    model = config.model if hasattr(config, "model") else config["model"]
    params = model["params"]
    unet = params["unet_config"]["params"]
    cin = ckpt_in_channels(ckpt) if ckpt else None
    if cin is not None and cin != unet["in_channels"]:
        unet["in_channels"] = cin
    if unet["in_channels"] > unet["out_channels"]:
        params["conditioning_key"] = "hybrid"
    return params.get("conditioning_key", None) == "hybrid"
