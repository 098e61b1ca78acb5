"""Perturbed-attention guidance (Ahn et al., ECCV 2024; the SD-1.5 PAG pipelines of diffusers) and guidance rescale (Lin et
al., WACV 2024, section 3.4; `guidance_rescale` of diffusers) for this package's samplers.  Not part of the reference; opt-in.

One helper serves DDIMSampler, PLMSSampler and DPMSolverSampler: it makes the model call of a step -- the three-leg forward
(cond, uncond, perturbed) with PAG, the twin forward with rescale alone -- and combines the predictions in one af_guidance
launch,

    e = e_u + w (e_c - e_u) + s_t (e_c - e_p),   s_t = max(pag_scale - pag_adaptive_scale (1000 - t), 0),
    e <- e (phi f + 1 - phi),                    f = std(e_c) / std(e) per sample,

and the sampler's own step kernel then takes e as its eps_cond with eps_uncond None.  With pag_scale = 0 and
guidance_rescale = 0 the samplers never come here and make the calls they always made.
"""
from __future__ import annotations

from adaface_amd import ops
from adaface_amd.engine import pag_scale_at

import torch


def check_args(pag_scale=0., pag_adaptive_scale=0., guidance_rescale=0.):
    """The three settings as floats; ValueError for a negative scale or a rescale outside [0, 1]."""
    vals = []
    for name, v in (("pag_scale", pag_scale), ("pag_adaptive_scale", pag_adaptive_scale), ("guidance_rescale", guidance_rescale)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not float(v) >= 0.0:
            raise ValueError(f"{name}: {v!r} (a number >= 0)")
        vals.append(float(v))
    if vals[2] > 1.0:
        raise ValueError(f"guidance_rescale: {guidance_rescale!r} (a number in [0, 1])")
    return tuple(vals)


def is_on(pag_scale=0., guidance_rescale=0.) -> bool:
    return bool(pag_scale) or bool(guidance_rescale)


def check_model(model, unconditional_conditioning, pag_scale):
    """What PAG needs before the first step: an unconditional conditioning, a model with the three-leg entry point, and layers
    given to set_pag."""
    if not pag_scale:
        return
    if unconditional_conditioning is None:
        raise ValueError("pag_scale > 0 needs an unconditional_conditioning: the combine is e_u + w (e_c - e_u) + s (e_c - e_p)")
    if not hasattr(model, "apply_model_cfg_pag"):
        raise ValueError("pag_scale > 0: the model has no apply_model_cfg_pag (perturbed-attention guidance needs the HIP U-Net)")
    if not getattr(model, "pag", ()):
        raise ValueError("pag_scale > 0: no PAG layer is set on the model (model.set_pag(('mid',)))")


def twin_condition(sampler, c, uc):
    """(cond, uncond) concatenated cond FIRST -- the order apply_model_cfg_twin / apply_model_cfg_pag take, whatever the
    sampler's own order (PLMS puts uncond first) -- once per sampling run."""
    key = (id(c), id(uc))
    cache = getattr(sampler, "_guided_twin_cache", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    if isinstance(c, tuple):
        c_c, c_in_c, extra_info = c
        c_u, c_in_u, _ = uc
        twin = (torch.cat([c_c, c_u]), sum([list(c_in_c), list(c_in_u)], []), extra_info)
    else:
        twin = torch.cat([c, uc])
    sampler._guided_twin_cache = (key, twin, c, uc)   # (c / uc kept alive so that the ids stay unique)
    return twin


def guided_eps(sampler, x, t, c, uc, guidance_scale, timestep, pag_scale=0., pag_adaptive_scale=0., guidance_rescale=0.,
               deep_cache_run=None, loop_index=0):
    """The combined, rescaled eps [B] of one model call at (x, t).  timestep: t as a host integer (the adaptive PAG scale is
    computed on the host, as diffusers does).  deep_cache_run / loop_index: the run's DeepCacheRun and the step's loop index;
    the call form it gets carries the leg count.  Appends (legs, s_t) to sampler.guidance_log."""
    model = sampler.model
    b = x.shape[0]
    log = getattr(sampler, "guidance_log", None)
    if log is None:
        log = sampler.guidance_log = []
    if pag_scale:
        check_model(model, uc, pag_scale)
        s_t = pag_scale_at(timestep, pag_scale, pag_adaptive_scale)
        dc = None if deep_cache_run is None else deep_cache_run.step(loop_index, (3, b, x.shape[2], x.shape[3]))
        twin = twin_condition(sampler, c, uc)
        e = model.apply_model_cfg_pag(x, t, twin) if dc is None else model.apply_model_cfg_pag(x, t, twin, deep_cache=dc)
        log.append((3, s_t))
        return ops.guidance(e[:b], e[b:2 * b], e[2 * b:], guidance_scale, s_t, guidance_rescale)
    if uc is None or guidance_scale == 1.:
        # rescale alone without guidance: e = e_c and f = 1, nothing to combine
        dc = None if deep_cache_run is None else deep_cache_run.step(loop_index, (1, b, x.shape[2], x.shape[3]))
        log.append((1, 0.0))
        return model.apply_model(x, t, c) if dc is None else model.apply_model(x, t, c, deep_cache=dc)
    dc = None if deep_cache_run is None else deep_cache_run.step(loop_index, (2, b, x.shape[2], x.shape[3]))
    twin = twin_condition(sampler, c, uc)
    if dc is not None:
        e = model.apply_model_cfg_twin(x, t, twin, deep_cache=dc)
    elif hasattr(model, "apply_model_cfg_twin"):
        e = model.apply_model_cfg_twin(x, t, twin)
    else:
        e = model.apply_model(torch.cat([x] * 2), torch.cat([t] * 2), twin)
    log.append((2, 0.0))
    return ops.guidance(e[:b], e[b:], None, guidance_scale, 0.0, guidance_rescale)
