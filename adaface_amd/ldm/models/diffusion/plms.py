"""Drop-in for ldm.models.diffusion.plms.PLMSSampler (reference plms.py:11-253), the `--plms` alternative of
scripts/stable_txt2img.py.  Same constructor / sample / plms_sampling / p_sample_plms signatures.  Note the
reference's quirks, kept: classifier-free guidance concatenates (UNCOND, COND) — the opposite order of the DDIM
sampler (plms.py:193-199) — takes `unconditional_guidance_scale` (a scalar, no annealing), and eta must be 0.
All tensor arithmetic runs in HIP kernels (af_lincomb, af_ddim_step); the sampler itself is host logic.  The model calls
are the run's ModelCalls' (model_calls.py, twin_order="uncond_first"); the combine of the unguided twin call and the second
call of the first step at t_next are this sampler's own.
"""
from __future__ import annotations

import numpy as np
import torch

from adaface_amd import ops
from adaface_amd.ldm.models.diffusion.blend import check_strength, initial_latent, step_blend, strength_timesteps
from adaface_amd.ldm.models.diffusion.model_calls import ModelCalls
from adaface_amd.ldm.modules.diffusionmodules.util import (make_ddim_sampling_parameters, make_ddim_timesteps,
                                                            noise_like)


class PLMSSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor) and attr.device != self.model.device:
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize, num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        acp = self.model.alphas_cumprod.detach().float().cpu()
        assert acp.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        to_dev = lambda x: x.clone().detach().to(torch.float32).to(self.model.device)
        self.register_buffer('betas', to_dev(self.model.betas))
        self.register_buffer('alphas_cumprod', to_dev(self.model.alphas_cumprod))
        self.register_buffer('alphas_cumprod_prev', to_dev(self.model.alphas_cumprod_prev))
        self.register_buffer('sqrt_one_minus_alphas_cumprod', to_dev(np.sqrt(1. - acp)))
        sig, a, a_prev = make_ddim_sampling_parameters(alphacums=acp, ddim_timesteps=self.ddim_timesteps, eta=ddim_eta,
                                                       verbose=verbose)
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = sig, a, a_prev
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1. - a)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, deep_cache_interval=None, deep_cache_depth=2, pag_scale=0.,
               pag_adaptive_scale=0., guidance_rescale=0., tgate_step=None, noise_source=None, strength=None,
               fused_blend=False, sag_scale=0., sag_blur_sigma=1.0, **kwargs):
        """plms.py:71-117.  pag_scale / pag_adaptive_scale / guidance_rescale (not in the reference): perturbed-attention
        guidance and guidance rescale on every model call of the run, see guidance.py.  noise_source (not in the reference):
        an adaface_amd.noise.PhiloxNoise for the start code (stream 0) and the blend's q_sample noise (stream 2) -- nothing
        else: the eta = 0 update has no noise of its own.  strength / fused_blend (not in the reference): img2img by strength
        and the one-launch inpainting blend, as DDIMSampler.sample (blend.py); a run by strength starts an eps history of its
        own, so its first executed step is the two-call one.  sag_scale / sag_blur_sigma (not in the reference):
        self-attention guidance on every model call of the run, as DDIMSampler.sample (guidance.py)."""
        from adaface_amd.ldm.models.diffusion.deep_cache import is_off
        check_strength(strength, x0)
        if not is_off(deep_cache_interval):
            raise NotImplementedError("deep_cache_interval with the PLMS sampler: it calls the model twice in its first step and "
                                      "extrapolates from an eps history (use DDIMSampler or DPMSolverSampler)")
        if tgate_step not in (None, 0) or isinstance(tgate_step, bool):
            raise NotImplementedError("tgate_step with the PLMS sampler: its eps history mixes predictions from before and after "
                                      "the gate, which T-GATE does not define (use DDIMSampler or DPMSolverSampler)")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        return self.plms_sampling(conditioning, (batch_size, C, H, W), callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, pag_scale=pag_scale,
                                  pag_adaptive_scale=pag_adaptive_scale, guidance_rescale=guidance_rescale,
                                  noise_source=noise_source, strength=strength, fused_blend=fused_blend,
                                  sag_scale=sag_scale, sag_blur_sigma=sag_blur_sigma)

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, pag_scale=0., pag_adaptive_scale=0., guidance_rescale=0.,
                      noise_source=None, strength=None, fused_blend=False, sag_scale=0., sag_blur_sigma=1.0):
        """plms.py:119-173.  noise_source / strength / fused_blend: as sample(); with strength, x_T is the noise added to x0."""
        check_strength(strength, x0, timesteps=timesteps)
        if ddim_use_original_steps:
            raise NotImplementedError("ddim_use_original_steps is not used by txt2img")
        device = self.model.betas.device
        b = shape[0]
        if strength is not None:
            timesteps = strength_timesteps(self.ddim_timesteps, strength)
        elif timesteps is None:
            timesteps = self.ddim_timesteps
        else:
            subset_end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1
            timesteps = self.ddim_timesteps[:subset_end]
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        calls = ModelCalls(self, cond, unconditional_conditioning, total_steps, pag_scale=pag_scale,
                           pag_adaptive_scale=pag_adaptive_scale, guidance_rescale=guidance_rescale, sag_scale=sag_scale,
                           sag_blur_sigma=sag_blur_sigma, twin_order="uncond_first", stepped=())
        img = initial_latent(self.model, shape, x_T, noise_source, strength, x0,
                             None if strength is None else int(timesteps[-1]), device)
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        old_eps = []
        blend = step_blend(self.model, mask, x0, noise_source, fused_blend)
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            ts_next = torch.full((b,), int(time_range[min(i + 1, len(time_range) - 1)]), device=device, dtype=torch.long)
            if blend is not None:
                img = blend(img, ts, int(step), i)
            img, pred_x0, e_t = self.p_sample_plms(img, cond, ts, index=index, quantize_denoised=quantize_denoised,
                                                   temperature=temperature, noise_dropout=noise_dropout,
                                                   score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
                                                   unconditional_guidance_scale=unconditional_guidance_scale,
                                                   unconditional_conditioning=unconditional_conditioning,
                                                   old_eps=old_eps, t_next=ts_next,
                                                   timesteps=(int(step), int(time_range[min(i + 1, len(time_range) - 1)])),
                                                   calls=calls)
            old_eps.append(e_t)
            if len(old_eps) >= 4:
                old_eps.pop(0)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        return img, intermediates

    @torch.no_grad()
    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, old_eps=None, t_next=None,
                      timesteps=None, calls=None):
        """plms.py:175-253.  calls: the loop's ModelCalls (model_calls.py), which makes every model call of the step with the
        run's guidance settings; None: one made here from c and unconditional_conditioning without any, the reference's calls.
        timesteps: (t, t_next) as host integers (None: read from the tensors where needed)."""
        if quantize_denoised or score_corrector is not None or use_original_steps:
            raise NotImplementedError("quantize_denoised / score_corrector / use_original_steps are not on the txt2img path")
        f32 = lambda v: float(np.float32(float(v)))
        if calls is None:
            calls = ModelCalls.bare(self, c, unconditional_conditioning, "uncond_first")

        def get_model_output(xx, tt):
            th = None if timesteps is None else timesteps[0 if tt is t else 1]
            e_c, e_u = calls.eps(xx, tt, 0, th, unconditional_guidance_scale)
            if e_u is None:
                return e_c
            return ops.lincomb([(e_c, unconditional_guidance_scale), (e_u, 0.0)], cfg=True)  # e_u + g (e_c - e_u)

        def get_x_prev_and_pred_x0(e, idx):
            # one noise_like draw per call, as the reference (plms.py:236), so the device generator advances
            # identically even when sigma_t = 0 (eta = 0) makes the term vanish
            sigma_t = f32(self.ddim_sigmas[idx])
            noise = noise_like(x.shape, x.device, repeat_noise)
            if noise_dropout > 0.:
                noise = torch.nn.functional.dropout(noise, p=noise_dropout)
            return ops.ddim_step(x, e, None, 1.0, f32(self.ddim_alphas[idx]), f32(self.ddim_alphas_prev[idx]),
                                 f32(self.ddim_sqrt_one_minus_alphas[idx]), sigma_t,
                                 None if sigma_t == 0. else noise, temperature)

        e_t = get_model_output(x, t)
        if len(old_eps) == 0:        # pseudo improved Euler (2nd order)
            x_prev, _ = get_x_prev_and_pred_x0(e_t, index)
            e_t_next = get_model_output(x_prev, t_next)
            e_t_prime = ops.lincomb([(e_t, 0.5), (e_t_next, 0.5)])
        elif len(old_eps) == 1:      # 2nd-order Adams-Bashforth
            e_t_prime = ops.lincomb([(e_t, 3 / 2), (old_eps[-1], -1 / 2)])
        elif len(old_eps) == 2:      # 3rd order
            e_t_prime = ops.lincomb([(e_t, 23 / 12), (old_eps[-1], -16 / 12), (old_eps[-2], 5 / 12)])
        else:                        # 4th order
            e_t_prime = ops.lincomb([(e_t, 55 / 24), (old_eps[-1], -59 / 24), (old_eps[-2], 37 / 24), (old_eps[-3], -9 / 24)])
        x_prev, pred_x0 = get_x_prev_and_pred_x0(e_t_prime, index)
        return x_prev, pred_x0, e_t
