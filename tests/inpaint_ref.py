"""Restatements for the img2img / inpainting tests (not a test module).

  * strength_n / executed: the strength -> n -> ts[:n] arithmetic, stated once more from the definition.
  * blend_torch: the torch composition af_noise_blend replaces, op by op as LatentDiffusion.q_sample and the samplers' blend
    line evaluate it (each torch op is one fp32 rounding).
  * ddim_strength_ref / plms_strength_ref: a run by strength on the CPU oracle.  The oracle's own ddim_sample / plms_sample
    run on the grid of the executed timesteps: with make_ddim_timesteps answering ts[:n], their per-index tables
    (alphas = acp[ts[:n]], alphas_prev = [acp[0]] + acp[ts[:n-1]]) are the first n rows of the full run's, the guidance is
    annealed over n steps and PLMS starts an empty eps history -- which is what a run by strength is.  The start is the
    oracle's q_sample of x0 at ts[n - 1].
"""
from __future__ import annotations

import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from oracle import ldm_oracle as O  # noqa: E402


def strength_n(n_grid: int, strength: float) -> int:
    return min(n_grid, max(1, int(n_grid * strength)))


def executed(ts, strength):
    """The timesteps a run by strength executes, in the order they are taken (largest first)."""
    ts = np.asarray(ts)
    return [int(t) for t in ts[:strength_n(len(ts), strength)][::-1]]


def blend_torch(x, x0, keep, sa, s1, z):
    """q_sample then the blend line, with sa / s1 fp32 scalars broadcast as extract_into_tensor's [B, 1, 1, 1] tensors are."""
    dev = x0.device
    sa_t = torch.full((x0.shape[0],) + (1,) * (x0.dim() - 1), float(np.float32(sa)), device=dev, dtype=torch.float32)
    s1_t = torch.full_like(sa_t, float(np.float32(s1)))
    q = sa_t * x0 if z is None else sa_t * x0 + s1_t * z
    if keep is None:
        return q
    return q * keep + (1. - keep) * x


@contextmanager
def _oracle_grid(sub):
    orig = O.make_ddim_timesteps
    O.make_ddim_timesteps = lambda *a, **k: np.asarray(sub)
    try:
        yield
    finally:
        O.make_ddim_timesteps = orig


def _start(schedule, S, strength, x0, z):
    ts = O.make_ddim_timesteps(S, schedule["alphas_cumprod"].shape[0])
    sub = ts[:strength_n(len(ts), strength)]
    t = torch.full((x0.shape[0],), int(sub[-1]), dtype=torch.long)
    return sub, O.q_sample(schedule, x0, t, z)


def ddim_strength_ref(apply_model, schedule, S, strength, x0, z, cond, uncond, guidance=(10.0, 4.0), mask=None, q_noise=None):
    """(latent, executed timesteps ascending).  mask / q_noise: the blend in front of each executed step, q_noise[i] at loop
    index i.  Needs n >= 2 (the oracle anneals the guidance over n - 1 intervals)."""
    sub, start = _start(schedule, S, strength, x0, z)
    with _oracle_grid(sub), torch.no_grad():
        kw = {} if mask is None else dict(mask=mask, x0=x0, q_noise=q_noise)
        return O.ddim_sample(apply_model, schedule, S, start, cond, uncond, guidance_scale=guidance, **kw), sub


def plms_strength_ref(apply_model, schedule, S, strength, x0, z, cond, uncond, guidance=3.0):
    sub, start = _start(schedule, S, strength, x0, z)
    with _oracle_grid(sub), torch.no_grad():
        return O.plms_sample(apply_model, schedule, S, start, cond, uncond, guidance_scale=guidance), sub
