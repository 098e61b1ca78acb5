"""Where a sampler step's model call is decided: one ModelCalls per sampling run, built by every loop
(ddim_sampling, DDIMSampler.decode, plms_sampling, dpm_solver_sampling, lcm_sampling) before its first step.  It validates the
opt-in settings once, owns the run's DeepCacheRun / TGateRun and its guidance log, concatenates the (cond, uncond) pair once per
order, and eps() makes each step's call:

    T-GATE capture / replay   the step's usual form with deep_cache= and tgate=; a replay is one leg          -> (e_c, e_u | None)
    SAG                       guidance.sag_eps: the usual call with the capture on, one degraded leg, combine   -> (e, None)
    PAG or rescale            apply_model_cfg_pag (three legs) or the twin / single call, then ops.guidance     -> (e, None)
    single leg                apply_model(x, t, cond): no uncond, or guidance 1                                 -> (e_c, None)
    twin                      apply_model_cfg_twin(x, t, [cond; uncond])                                        -> (e_c, e_u)

(the two guided branches are guidance.guided_eps, entered with the run as calls=, which makes its forwards through call() below)
and the sampler's step kernel makes the CFG combine of (e_c, e_u).  deep_cache= reaches a model only on a step of an active
DeepCacheRun and tgate= only in a capture or replay phase (other models do not take the keywords); a model without
apply_model_cfg_twin gets apply_model on [x; x].  Host logic only.
"""
from __future__ import annotations

import torch

from adaface_amd.ldm.models.diffusion import guidance as G
from adaface_amd.ldm.models.diffusion.deep_cache import DeepCacheRun
from adaface_amd.ldm.models.diffusion.tgate import TGateRun, refuse_guided


class ModelCalls:
    """One sampling run's model calls.  twin_order: the leg order of the unguided twin call, "cond_first" (the reference's DDIM
    order) or "uncond_first" (its PLMS order); every guided call is cond first.  stepped: which of the two per-run schedules this
    sampler's loop has ("deep_cache", "tgate"): those are built, stepped once per model call / loop step, and their logs
    published as sampler.deep_cache_log / sampler.tgate_log.  log: the list guided calls are recorded in; None: a fresh one.
    Either way it is sampler.guidance_log from here on."""

    def __init__(self, sampler, cond, uncond, total_steps, deep_cache_interval=None, deep_cache_depth=2, pag_scale=0.,
                 pag_adaptive_scale=0., guidance_rescale=0., tgate_step=None, sag_scale=0., sag_blur_sigma=1.0,
                 twin_order="cond_first", stepped=("deep_cache", "tgate"), log=None):
        self.sampler, self.model, self.cond, self.uncond, self.twin_order = sampler, sampler.model, cond, uncond, twin_order
        self.pag_scale, self.pag_adaptive_scale, self.guidance_rescale = G.check_args(pag_scale, pag_adaptive_scale, guidance_rescale)
        G.check_model(self.model, uncond, self.pag_scale)
        refuse_guided(tgate_step, self.pag_scale, self.guidance_rescale)
        self.sag_scale, self.sag_blur_sigma = 0., 1.0
        if sag_scale != 0. or sag_blur_sigma != 1.0:
            self.sag_scale, self.sag_blur_sigma = G.check_sag_args(sag_scale, sag_blur_sigma)
            G.refuse_sag(self.model, self.sag_scale, self.pag_scale, self.guidance_rescale, tgate_step, deep_cache_interval)
        self.guided = G.is_on(self.pag_scale, self.guidance_rescale, self.sag_scale)
        self.log = sampler.guidance_log = [] if log is None else log      # (legs, PAG or SAG scale) per guided model call
        self.dc_run = self.tg_run = None
        if "deep_cache" in stepped:
            self.dc_run = DeepCacheRun(self.model, total_steps, deep_cache_interval, deep_cache_depth)
            sampler.deep_cache_log = self.dc_run.log
        if "tgate" in stepped:
            self.tg_run = TGateRun(self.model, total_steps, tgate_step)
            sampler.tgate_log = self.tg_run.log
        self._twins = {}
        if self.sag_scale:      # alphas_cumprod as host doubles, read once per run (no device read per step)
            self.acp = self.model.alphas_cumprod.detach().double().cpu().numpy()

    @classmethod
    def bare(cls, sampler, cond, uncond, twin_order="cond_first"):
        """The run of a p_sample_* call made outside a loop: no opt-ins, the sampler's guidance_log left as it is.  Kept on the
        sampler while cond and uncond are the same objects, so a caller's own loop concatenates the pair once."""
        calls = getattr(sampler, "_bare_calls", None)
        if calls is None or calls.model is not sampler.model or calls.cond is not cond or calls.uncond is not uncond:
            calls = sampler._bare_calls = cls(sampler, cond, uncond, 1, twin_order=twin_order, stepped=(),
                                              log=getattr(sampler, "guidance_log", None))
        return calls

    def twin(self, order="cond_first"):
        """The run's (cond, uncond) concatenated in `order`, built once per order; the run holds cond and uncond themselves."""
        if order not in self._twins:
            a, b = (self.cond, self.uncond) if order == "cond_first" else (self.uncond, self.cond)
            if isinstance(a, tuple):      # (c, c_in, extra_info): the cond's extra_info in either order
                self._twins[order] = (torch.cat([a[0], b[0]]), list(a[1]) + list(b[1]), self.cond[2])
            else:
                self._twins[order] = torch.cat([a, b])
        return self._twins[order]

    def call(self, x, t, legs, order="cond_first", **kw):
        """One forward on 1, 2 or 3 legs; kw: deep_cache= / tgate=, only when set.  Two legs without keywords on a model
        without the twin entry point: [x; x] through apply_model."""
        if legs == 1:
            return self.model.apply_model(x, t, self.cond, **kw)
        if legs == 3:
            return self.model.apply_model_cfg_pag(x, t, self.twin(), **kw)
        if kw or hasattr(self.model, "apply_model_cfg_twin"):
            # [x; x] without the concatenation: the UNet computes its context-independent prefix once (af_unet_forward_twin)
            return self.model.apply_model_cfg_twin(x, t, self.twin(order), **kw)
        return self.model.apply_model(torch.cat([x] * 2), torch.cat([t] * 2), self.twin(order))

    def eps(self, x, t, i, timestep, guidance_scale):
        """(e_c, e_u) of the model call at (x, t) of loop index i; e_u None: e_c is final, the step kernel combines nothing.
        timestep: t as a host integer (None: read from t where a guided call needs it)."""
        b = x.shape[0]
        single = self.uncond is None or guidance_scale == 1.
        phase = None if self.tg_run is None else self.tg_run.step(i)
        if self.guided:
            e = G.guided_eps(self.sampler, x, t, self.cond, self.uncond, guidance_scale, timestep, loop_index=i, calls=self)
            return e, None
        single = single or phase == "replay"      # (T-GATE: one leg from the gate on)
        form = (not single, b, x.shape[2], x.shape[3])
        dc = None if self.dc_run is None else self.dc_run.step(i, form if self.tg_run is None else self.tg_run.form(form, phase))
        kw = dict(deep_cache=dc, tgate=phase) if phase is not None else {} if dc is None else dict(deep_cache=dc)
        if single:
            return self.call(x, t, 1, **kw), None
        e = self.call(x, t, 2, self.twin_order, **kw)
        return (e[:b], e[b:]) if self.twin_order == "cond_first" else (e[b:], e[:b])
