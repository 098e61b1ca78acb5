"""img2img by strength and the fused inpainting blend for this package's samplers.  Not part of the reference;
both opt-in (strength=None, fused_blend=False leave every call of a run as it is).

strength (SDEdit: Meng et al., "SDEdit: Guided Image Synthesis and Editing with Stochastic Differential Equations", ICLR
2022): a run on the ascending grid ts executes its n smallest timesteps ts[:n], largest first, from the clean latent x0
noised to ts[n - 1] -- the noise level and the first executed step agree (DDIMSampler.decode, the reference's img2img tail,
is one step off).  n = min(len(ts), max(1, int(len(ts) * strength))).

fused_blend: the blend in front of a step, q_sample(x0, t) * mask + (1 - mask) * img, as ONE launch (ops.noise_blend) with
the bits of that composition.  With a noise_source its noise is generated inside the launch (stream 2, step = the loop index).

The four sampler loops share two functions of this file: initial_latent, the latent a run starts from (by strength, x_T, the
noise source's start code or torch.randn), and step_blend, the blend in front of a step (fused, or the reference's torch ops).

This file is host logic only: the arithmetic is af_noise_blend's (csrc/af_inpaint.hip).
"""
from __future__ import annotations

import torch

from adaface_amd import ops
from adaface_amd.noise import STREAM_QSAMPLE, STREAM_XT


def strength_steps(n_grid: int, strength) -> int:
    """The number of executed steps of a run by strength on a grid of n_grid timesteps.  Host only."""
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not (0. < float(strength) <= 1.):
        raise ValueError(f"strength: {strength!r} (None = off, or a number in (0, 1])")
    n_grid = int(n_grid)
    if n_grid < 1:
        raise ValueError(f"strength: a grid of {n_grid} timesteps")
    return min(n_grid, max(1, int(n_grid * float(strength))))


def strength_timesteps(ts, strength):
    """ts[:n], the timesteps a run by strength executes (ascending, as ts)."""
    return ts[:strength_steps(len(ts), strength)]


def check_strength(strength, x0, **off):
    """strength needs the clean latent x0, and none of the loop methods' own timestep selections (off: name -> must be falsy)."""
    if strength is None:
        return
    strength_steps(1, strength)
    if x0 is None:
        raise ValueError("strength: needs x0, the clean latent to start from (adaface_amd.img2img.encode_image)")
    bad = [k for k, v in off.items() if v is not None and v is not False]
    if bad:
        raise NotImplementedError(f"strength with {', '.join(bad)}: the run by strength selects its own timesteps")


class QTable:
    """The two fp32 tables q_sample reads, on the host: one copy per run instead of a device read per step."""

    def __init__(self, model):
        self.sa = model.sqrt_alphas_cumprod.detach().float().cpu()
        self.s1 = model.sqrt_one_minus_alphas_cumprod.detach().float().cpu()

    def __call__(self, t: int):
        return float(self.sa[int(t)]), float(self.s1[int(t)])


def _key(noise_source, b, device):
    if noise_source is None:
        return dict()
    ids_dev, first_id = noise_source.ids_device(b, device)
    return dict(seed=noise_source.seed, sample_ids=ids_dev, first_id=first_id)


def start_code(model, x0, t: int, x_T=None, noise_source=None):
    """The start of a run by strength: x0 noised to timestep t in one launch.  The noise is x_T if given (read as z, not as a
    latent), else the source's stream 0 at step 0 -- the start code the same seed draws for txt2img -- else torch.randn."""
    sa, s1 = QTable(model)(t)
    if x_T is not None:
        return ops.noise_blend(None, x0, None, sa, s1, noise=x_T)
    if noise_source is None:
        return ops.noise_blend(None, x0, None, sa, s1, noise=torch.randn_like(x0))
    return ops.noise_blend(None, x0, None, sa, s1, stream=STREAM_XT, step=0, **_key(noise_source, x0.shape[0], x0.device))


class FusedBlend:
    """One run's fused blend: blend(img, t, i) = q_sample(x0, t) * mask + (1 - mask) * img at loop index i, one launch."""

    def __init__(self, model, mask, x0, noise_source=None):
        assert x0 is not None
        self.mask, self.x0, self.noise_source = mask, x0, noise_source
        self.table = QTable(model)
        self.key = _key(noise_source, x0.shape[0], x0.device)

    def __call__(self, img, t: int, i: int):
        sa, s1 = self.table(t)
        if self.noise_source is None:
            return ops.noise_blend(img, self.x0, self.mask, sa, s1, noise=torch.randn_like(self.x0))
        return ops.noise_blend(img, self.x0, self.mask, sa, s1, stream=STREAM_QSAMPLE, step=i, **self.key)


def initial_latent(model, shape, x_T, noise_source, strength, x0, t_first, device):
    """The latent a run starts from: by strength, x0 noised to t_first (start_code); else x_T if given; else the start code of
    the noise source (stream 0, step 0), or torch.randn on the device without one."""
    if strength is not None:
        return start_code(model, x0, t_first, x_T, noise_source)
    if x_T is not None:
        return x_T
    if noise_source is None:
        return torch.randn(shape, device=device)
    return noise_source.randn(shape, STREAM_XT, 0, device)


def step_blend(model, mask, x0, noise_source=None, fused_blend=False):
    """One run's blend in front of a step, blend(img, ts, t, i) at loop index i with the timestep as the tensor ts [B] and as
    the host integer t: None without a mask; the FusedBlend launch; or the reference's q_sample(x0, ts) * mask + (1 - mask) * img
    in torch, its noise the source's stream 2 at step i, or q_sample's own torch.randn_like without a source."""
    if mask is None:
        return None
    assert x0 is not None
    if fused_blend:
        fused = FusedBlend(model, mask, x0, noise_source)
        return lambda img, ts, t, i: fused(img, t, i)

    def blend(img, ts, t, i):
        if noise_source is None:
            img_orig = model.q_sample(x0, ts)
        else:
            img_orig = model.q_sample(x0, ts, noise=noise_source.randn(x0.shape, STREAM_QSAMPLE, i, ts.device))
        return img_orig * mask + (1. - mask) * img
    return blend
