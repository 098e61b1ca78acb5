"""Drop-in for ldm.models.diffusion.ddim.DDIMSampler (reference ddim.py:12-350).

Same constructor, method names and keyword arguments.  Differences are confined to what
makes it MI355X-native and device-agnostic:
  * register_buffer does not force "cuda" (the reference does, ddim.py:22-26);
  * the CFG combine and the x_{t-1} update are ONE fused HIP kernel (af_ddim_step);
  * the (cond, uncond) context pair is concatenated once per sample() call, not once per
    step, so the UNet's hoisted cross-attention K/V stay cached across the 50 steps; which entry point of the model a
    step calls, with which keywords, is decided by the run's ModelCalls (model_calls.py);
  * a scalar guidance_scale means "no annealing" instead of the reference's
    UnboundLocalError (ddim.py:169-173);
  * deep_cache_interval= / deep_cache_depth= (opt-in, not in the reference): DeepCache, see deep_cache.py;
  * pag_scale= / pag_adaptive_scale= / guidance_rescale= (opt-in, not in the reference): perturbed-attention guidance and
    guidance rescale, see guidance.py.  All zero: the calls below are the calls made without them.
  * strength= / fused_blend= (opt-in, not in the reference): img2img by strength and the one-launch inpainting blend, see
    blend.py.  None / False: the calls below are the calls made without them.
"""
from __future__ import annotations

import numpy as np
import torch

from adaface_amd import ops
from adaface_amd.ldm.models.diffusion.blend import check_strength, initial_latent, step_blend, strength_timesteps
from adaface_amd.ldm.models.diffusion.model_calls import ModelCalls
from adaface_amd.ldm.modules.diffusionmodules.util import (extract_into_tensor, make_ddim_sampling_parameters,
                                                           make_ddim_timesteps, noise_like)
from adaface_amd.noise import STREAM_STEP


def _check_noise_source(noise_source, noise_dropout):
    if noise_source is not None and noise_dropout > 0.:
        raise NotImplementedError("noise_dropout with a noise_source: the dropout mask would come from torch's generator, and "
                                  "the result would again depend on the batch split")


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.deep_cache_log = []      # "full" / "refresh" / "reuse" per step of the last run
        self.tgate_log = []           # None / "capture" / "replay" per step of the last run

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor) and attr.device != self.model.device:
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        """ddim.py:28-68."""
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize, num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        alphas_cumprod = self.model.alphas_cumprod
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        to_torch = lambda x: x.clone().detach().to(torch.float32).to(self.model.device)
        acp_cpu = alphas_cumprod.detach().float().cpu()

        self.register_buffer('betas', to_torch(self.model.betas))
        self.register_buffer('alphas_cumprod', to_torch(alphas_cumprod))
        self.register_buffer('alphas_cumprod_prev', to_torch(self.model.alphas_cumprod_prev))
        self.register_buffer('sqrt_alphas_cumprod', to_torch(np.sqrt(acp_cpu)))
        self.register_buffer('sqrt_one_minus_alphas_cumprod', to_torch(np.sqrt(1. - acp_cpu)))
        self.register_buffer('log_one_minus_alphas_cumprod', to_torch(np.log(1. - acp_cpu)))
        self.register_buffer('sqrt_recip_alphas_cumprod', to_torch(np.sqrt(1. / acp_cpu)))
        self.register_buffer('sqrt_recipm1_alphas_cumprod', to_torch(np.sqrt(1. / acp_cpu - 1)))

        ddim_sigmas, ddim_alphas, ddim_alphas_prev = make_ddim_sampling_parameters(
            alphacums=acp_cpu, ddim_timesteps=self.ddim_timesteps, eta=ddim_eta, verbose=verbose)
        # the per-step scalars stay on the host: each is read once per step as a kernel argument
        self.ddim_sigmas = ddim_sigmas
        self.ddim_alphas = ddim_alphas
        self.ddim_alphas_prev = ddim_alphas_prev
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1. - ddim_alphas)
        acp_prev = self.model.alphas_cumprod_prev.detach().float().cpu()
        self.ddim_sigmas_for_original_num_steps = ddim_eta * torch.sqrt(
            (1 - acp_prev) / (1 - acp_cpu) * (1 - acp_cpu / acp_prev))

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, guidance_scale=1.,
               unconditional_conditioning=None, noise_source=None, deep_cache_interval=None, deep_cache_depth=2,
               pag_scale=0., pag_adaptive_scale=0., guidance_rescale=0., tgate_step=None, strength=None, fused_blend=False,
               sag_scale=0., sag_blur_sigma=1.0, **kwargs):
        """ddim.py:71-132.  noise_source: None = the reference's generators (torch.randn on the device); an
        adaface_amd.noise.PhiloxNoise = every draw of the loop keyed by (seed, global sample id, stream, step).
        deep_cache_interval: None or 1 = off; N >= 2 = the full U-Net on loop indices i % N == 0 only, or an explicit
        sequence of those indices (with 0); between them the outermost deep_cache_depth blocks run on the kept deep feature.
        pag_scale / pag_adaptive_scale: perturbed-attention guidance on the layers given to model.set_pag, every step a
        three-leg forward; guidance_rescale in [0, 1]: the combined prediction rescaled towards the conditional one's standard
        deviation (guidance.py).
        tgate_step: None or 0 = off; g in 1 .. S - 1 = T-GATE (tgate.py): loop index g - 1 also keeps the cross-attention
        outputs, from loop index g on the U-Net runs on one leg with them and without guidance.
        strength: None = off; a number in (0, 1] (needs x0) = img2img, the run executes the n = max(1, int(len * strength))
        smallest of the grid's timesteps from x0 noised to the largest of them (blend.py); S in the other arguments' rules
        above is then n.  fused_blend: the blend of mask= / x0= in front of each step as one launch with the same bits.
        sag_scale / sag_blur_sigma: self-attention guidance (guidance.py): every step also runs one single-leg forward on the
        input blurred where the middle block's self-attention looks; not with pag_scale, guidance_rescale, tgate_step or
        deep_cache_interval."""
        _check_noise_source(noise_source, noise_dropout)
        check_strength(strength, x0)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print(f'Data shape for DDIM sampling is {size}, eta {eta}')
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature,
                                  score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                                  log_every_t=log_every_t, guidance_scale=guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, verbose=verbose,
                                  noise_source=noise_source, deep_cache_interval=deep_cache_interval,
                                  deep_cache_depth=deep_cache_depth, pag_scale=pag_scale, pag_adaptive_scale=pag_adaptive_scale,
                                  guidance_rescale=guidance_rescale, tgate_step=tgate_step, strength=strength,
                                  fused_blend=fused_blend, sag_scale=sag_scale, sag_blur_sigma=sag_blur_sigma, **kwargs)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      guidance_scale=1., unconditional_conditioning=None, verbose=False, noise_source=None,
                      deep_cache_interval=None, deep_cache_depth=2, pag_scale=0., pag_adaptive_scale=0., guidance_rescale=0.,
                      tgate_step=None, strength=None, fused_blend=False, sag_scale=0., sag_blur_sigma=1.0, **kwargs):
        """ddim.py:135-220: the S-iteration loop with annealed guidance (:169-180,215-218).  With a noise_source the start
        code (x_T None) is its stream 0, the blend's q_sample noise its stream 2 and the step noise its stream 1, each at
        step = the loop index.  strength / fused_blend: as sample(); with strength, x_T is the noise added to x0."""
        check_strength(strength, x0, timesteps=timesteps, ddim_use_original_steps=ddim_use_original_steps)
        _check_noise_source(noise_source, noise_dropout)
        device = self.model.betas.device
        b = shape[0]
        if strength is not None:
            # the n smallest timesteps of the grid; the per-index tables are read by index < n, as in a full run
            timesteps = strength_timesteps(self.ddim_timesteps, strength)
        elif timesteps is None:
            timesteps = self.ddpm_num_timesteps if ddim_use_original_steps else self.ddim_timesteps
        elif not ddim_use_original_steps:
            subset_end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1
            timesteps = self.ddim_timesteps[:subset_end]
        time_range = reversed(range(0, timesteps)) if ddim_use_original_steps else np.flip(timesteps)
        total_steps = timesteps if ddim_use_original_steps else timesteps.shape[0]
        calls = ModelCalls(self, cond, unconditional_conditioning, total_steps, deep_cache_interval, deep_cache_depth, pag_scale,
                           pag_adaptive_scale, guidance_rescale, tgate_step, sag_scale, sag_blur_sigma)
        img = initial_latent(self.model, shape, x_T, noise_source, strength, x0,
                             None if strength is None else int(timesteps[-1]), device)
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        if verbose:
            print(f"Running DDIM Sampling with {total_steps} timesteps")

        if isinstance(guidance_scale, (list, tuple)):
            max_guide_scale, min_guide_scale = guidance_scale
        else:
            max_guide_scale = min_guide_scale = guidance_scale
        max_guide_anneal_steps = total_steps - 1
        delta = (max_guide_scale - min_guide_scale) / max_guide_anneal_steps if max_guide_anneal_steps > 0 else 0.
        guide_scale = max_guide_scale
        blend = step_blend(self.model, mask, x0, noise_source, fused_blend)

        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            if blend is not None:
                img = blend(img, ts, int(step), i)
            img, pred_x0 = self.p_sample_ddim(img, cond, ts, index=index, use_original_steps=ddim_use_original_steps,
                                              quantize_denoised=quantize_denoised, temperature=temperature,
                                              noise_dropout=noise_dropout, score_corrector=score_corrector,
                                              corrector_kwargs=corrector_kwargs, guidance_scale=guide_scale,
                                              unconditional_conditioning=unconditional_conditioning,
                                              noise_source=noise_source, noise_step=i, timestep=int(step), calls=calls)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
            guide_scale = guide_scale - delta if i <= max_guide_anneal_steps else 1
        return img, intermediates

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      guidance_scale=1., unconditional_conditioning=None, noise_source=None, noise_step=0, timestep=None,
                      calls=None):
        """ddim.py:222-296.  noise_source: the step noise is its stream 1 at step noise_step (the loop index) instead of
        torch.randn; repeat_noise then gives every sample the first sample's id.  calls: the loop's ModelCalls
        (model_calls.py), which makes this step's model call from noise_step -- with the run's DeepCache, T-GATE and guidance
        settings -- for the update below to take; None: one made here from c and unconditional_conditioning without any of
        them, the reference's call.  timestep: t as a host integer (None: read from t where needed)."""
        _check_noise_source(noise_source, noise_dropout)
        b, device = x.shape[0], x.device
        if calls is None:
            calls = ModelCalls.bare(self, c, unconditional_conditioning)
        e_c, e_u = calls.eps(x, t, noise_step, timestep, guidance_scale)

        alphas = self.model.alphas_cumprod if use_original_steps else self.ddim_alphas
        alphas_prev = self.model.alphas_cumprod_prev if use_original_steps else self.ddim_alphas_prev
        sqrt_one_minus_alphas = self.model.sqrt_one_minus_alphas_cumprod if use_original_steps else self.ddim_sqrt_one_minus_alphas
        sigmas = self.ddim_sigmas_for_original_num_steps if use_original_steps else self.ddim_sigmas
        # the reference materialises each scalar through torch.full(...) => fp32 (ddim.py:273-276)
        f32 = lambda v: float(np.float32(float(v)))
        sigma_t = f32(sigmas[index])
        # drawn every step like the reference (ddim.py:286) so the generator state advances identically,
        # even though sigma_t = 0 (eta = 0) makes the term vanish
        if noise_source is None:
            noise = noise_like(x.shape, device, repeat_noise)
            if noise_dropout > 0.:
                noise = torch.nn.functional.dropout(noise, p=noise_dropout)
            if sigma_t == 0.:
                noise = None
        elif sigma_t == 0.:
            noise = None        # a keyed draw advances no generator state: nothing to draw where the term vanishes
        else:
            src = noise_source.repeated(b) if repeat_noise else noise_source
            noise = src.randn(x.shape, STREAM_STEP, noise_step, device)
        if score_corrector is not None:
            # ddim.py:262-264: the corrector sees the COMBINED score; combine first (af_lincomb, the kernel's own CFG form),
            # then hand its result to the update as a plain eps
            assert self.model.parameterization == "eps"
            e_t = e_c if e_u is None else ops.lincomb([(e_c, guidance_scale), (e_u, 0.0)], cfg=True)
            e_c, e_u = score_corrector.modify_score(self.model, e_t, x, t, c, **(corrector_kwargs or {})), None
        x_prev, pred_x0 = ops.ddim_step(x, e_c, e_u, guidance_scale, f32(alphas[index]), f32(alphas_prev[index]),
                                        f32(sqrt_one_minus_alphas[index]), sigma_t, noise, temperature)
        if quantize_denoised:
            # ddim.py:281-282,293: x_prev is rebuilt around the quantised pred_x0 (a VQ first stage; AutoencoderKL has no
            # `quantize`, and the reference raises AttributeError there as this does).  x_prev - sqrt(a_prev) pred_x0 is the
            # dir_xt + noise term the fused kernel already formed, so only the pred_x0 term is swapped (fp32 scalars as the
            # reference's torch.full(...) materialises them)
            q, _, *_ = self.model.first_stage_model.quantize(pred_x0)
            sa = float(np.sqrt(np.float32(f32(alphas_prev[index]))))
            x_prev = ops.lincomb([(x_prev, 1.0), (pred_x0, -sa), (q, sa)])
            pred_x0 = q
        return x_prev, pred_x0

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """ddim.py:299-312."""
        if use_original_steps:
            sqrt_alphas_cumprod = self.sqrt_alphas_cumprod
            sqrt_one_minus_alphas_cumprod = self.sqrt_one_minus_alphas_cumprod
        else:
            sqrt_alphas_cumprod = torch.sqrt(self.ddim_alphas).to(x0.device)
            sqrt_one_minus_alphas_cumprod = torch.as_tensor(self.ddim_sqrt_one_minus_alphas).to(x0.device)
        if noise is None:
            noise = torch.randn_like(x0)
        return (extract_into_tensor(sqrt_alphas_cumprod, t, x0.shape) * x0 +
                extract_into_tensor(sqrt_one_minus_alphas_cumprod, t, x0.shape) * noise)

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, deep_cache_interval=None, deep_cache_depth=2, pag_scale=0., pag_adaptive_scale=0.,
               guidance_rescale=0.):
        """ddim.py:315-350 (img2img tail): anneals guidance from `guidance_scale` to min(2, guidance_scale).
        deep_cache_interval / deep_cache_depth / pag_scale / pag_adaptive_scale / guidance_rescale: as sample()."""
        timesteps = np.arange(self.ddpm_num_timesteps) if use_original_steps else self.ddim_timesteps
        timesteps = timesteps[:t_start]
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        calls = ModelCalls(self, cond, unconditional_conditioning, total_steps, deep_cache_interval, deep_cache_depth, pag_scale,
                           pag_adaptive_scale, guidance_rescale, stepped=("deep_cache",))
        max_g = guidance_scale
        min_g = min(2.0, max_g)
        delta = (max_g - min_g) / (total_steps - 1) if total_steps > 1 else 0.
        g = max_g
        x_dec = x_latent
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            ts = torch.full((x_latent.shape[0],), int(step), device=x_latent.device, dtype=torch.long)
            x_dec, _ = self.p_sample_ddim(x_dec, cond, ts, index=index, use_original_steps=use_original_steps,
                                          guidance_scale=g, unconditional_conditioning=unconditional_conditioning,
                                          noise_step=i, timestep=int(step), calls=calls)
            g = g - delta
        return x_dec
