"""Inference subset of ldm.models.diffusion.ddpm (reference ddpm.py): the pieces of
LatentDiffusion the denoising path touches — model assembly from the yaml config
(ddpm.py:714-813), register_schedule (:244-296), apply_model (:2192-2297),
DiffusionWrapper.forward (:5477-5516), decode_first_stage (:1251-1308), ema_scope (:310-323),
q_sample (:478-482).  ~4.5k lines of training losses are out of scope.

The text side: cond_stage_model = the FrozenCLIPEmbedder drop-in (CLIP text tower on the HIP kernels),
embedding_manager = the inference subset of EmbeddingManager.  get_learned_conditioning takes prompts (needs a tokenizer,
whose vocabulary files do not exist offline), token-id tensors, or a pre-computed static prompt embedding.
"""
from __future__ import annotations

from contextlib import contextmanager
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from adaface_amd.ldm.modules.diffusionmodules.util import extract_into_tensor, make_beta_schedule
from adaface_amd.ldm.util import instantiate_from_config


class DiffusionWrapper(nn.Module):
    """ddpm.py:5477-5516: routes (x, t, c_crossattn=[(emb, prompts, extra_info)]) to the UNet.  conditioning_key "hybrid"
    (the sd-v1-5-inpainting checkpoint: a 9-channel conv_in) also concatenates c_concat onto x along the channels."""

    def __init__(self, diff_model_config, conditioning_key):
        super().__init__()
        self.diffusion_model = instantiate_from_config(diff_model_config)
        self.conditioning_key = conditioning_key
        if conditioning_key not in (None, "crossattn", "hybrid"):
            raise NotImplementedError(f"conditioning_key '{conditioning_key}' is not used by SD-v1 txt2img / inpainting")

    def forward(self, x, t, c_concat: list = None, c_crossattn: list = None, cfg_twin: bool = False, deep_cache=None,
                cfg_pag: bool = False, tgate=None):
        if self.conditioning_key is None:
            raise NotImplementedError("unconditional UNet is not on the path")
        if self.conditioning_key == "hybrid":
            # ddpm.py:5503-5506: unet(cat([x] + c_concat, 1), t, context=cat(c_crossattn, 1)).  Under cfg_twin / cfg_pag x and
            # c_concat are those of ONE leg, so the legs still share one concatenated x
            if not c_concat:
                raise ValueError("conditioning_key 'hybrid' needs c_concat (LatentDiffusion.set_concat_cond, or the dict form)")
            x = torch.cat([x] + [c.to(x.device, x.dtype) for c in c_concat], dim=1)
            want = getattr(self.diffusion_model, "in_channels", x.shape[1])
            if x.shape[1] != want:
                raise ValueError(f"hybrid conditioning: x and c_concat have {x.shape[1]} channels together, the U-Net takes {want}")
            if len(c_crossattn) > 1:
                if not all(isinstance(c, torch.Tensor) for c in c_crossattn):
                    raise NotImplementedError("hybrid conditioning: several c_crossattn entries must be plain tensors")
                c_crossattn = [torch.cat(list(c_crossattn), dim=1)]
        if tgate is not None:         # T-GATE capture / replay step (UNetModel.forward); None: the calls below, unchanged
            c0 = c_crossattn[0]
            c_static_emb, c_in, extra_info = c0 if isinstance(c0, tuple) else (c0, None, None)
            return self.diffusion_model(x, t, context=c_static_emb, context_in=c_in, extra_info=extra_info,
                                        cfg_twin=bool(cfg_twin), cfg_pag=bool(cfg_pag), deep_cache=deep_cache, tgate=tgate)
        c0 = c_crossattn[0]
        if isinstance(c0, tuple):
            c_static_emb, c_in, extra_info = c0
        else:
            c_static_emb, c_in, extra_info = c0, None, None
        if cfg_pag:                   # the three-leg call of perturbed-attention guidance (UNetModel.forward)
            return self.diffusion_model(x, t, context=c_static_emb, context_in=c_in, extra_info=extra_info, cfg_pag=True,
                                        deep_cache=deep_cache)
        if deep_cache is not None:    # DeepCache refresh / reuse step (UNetModel.forward); None: the calls below, unchanged
            return self.diffusion_model(x, t, context=c_static_emb, context_in=c_in, extra_info=extra_info,
                                        cfg_twin=bool(cfg_twin), deep_cache=deep_cache)
        if cfg_twin:
            return self.diffusion_model(x, t, context=c_static_emb, context_in=c_in, extra_info=extra_info, cfg_twin=True)
        return self.diffusion_model(x, t, context=c_static_emb, context_in=c_in, extra_info=extra_info)


class DDPM(nn.Module):
    """Schedule buffers + UNet wrapper (ddpm.py:73-296), inference arguments only."""

    def __init__(self, unet_config, timesteps=1000, beta_schedule="linear", linear_start=1e-4, linear_end=2e-2,
                 cosine_s=8e-3, given_betas=None, conditioning_key=None, parameterization="eps", use_ema=True,
                 first_stage_key="image", image_size=256, channels=3, log_every_t=100, v_posterior=0.,
                 use_layerwise_embedding=False, **ignored_training_kwargs):
        super().__init__()
        assert parameterization in ("eps", "x0")
        self.parameterization = parameterization
        self.first_stage_key = first_stage_key
        self.image_size = image_size
        self.channels = channels
        self.log_every_t = log_every_t
        self.use_layerwise_embedding = use_layerwise_embedding
        self.N_CA_LAYERS = 16 if use_layerwise_embedding else 1
        self.use_ema = False  # LitEma is training-only; the inference config sets use_ema False (yaml:18)
        self.v_posterior = v_posterior
        self.model = DiffusionWrapper(unet_config, conditioning_key)
        self.register_schedule(given_betas=given_betas, beta_schedule=beta_schedule, timesteps=timesteps,
                               linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)

    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        """ddpm.py:244-296: numpy fp64 tables stored as fp32 buffers."""
        betas = given_betas if given_betas is not None else make_beta_schedule(
            beta_schedule, timesteps, linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)
        alphas = 1. - betas
        alphas_cumprod = np.cumprod(alphas, axis=0)
        alphas_cumprod_prev = np.append(1., alphas_cumprod[:-1])
        self.num_timesteps = int(betas.shape[0])
        self.linear_start, self.linear_end = linear_start, linear_end
        to_torch = partial(torch.tensor, dtype=torch.float32)
        self.register_buffer('betas', to_torch(betas))
        self.register_buffer('alphas_cumprod', to_torch(alphas_cumprod))
        self.register_buffer('alphas_cumprod_prev', to_torch(alphas_cumprod_prev))
        self.register_buffer('sqrt_alphas_cumprod', to_torch(np.sqrt(alphas_cumprod)))
        self.register_buffer('sqrt_one_minus_alphas_cumprod', to_torch(np.sqrt(1. - alphas_cumprod)))
        self.register_buffer('sqrt_recip_alphas_cumprod', to_torch(np.sqrt(1. / alphas_cumprod)))
        self.register_buffer('sqrt_recipm1_alphas_cumprod', to_torch(np.sqrt(1. / alphas_cumprod - 1)))

    @property
    def device(self):
        return self.betas.device

    @contextmanager
    def ema_scope(self, context=None):
        yield None  # use_ema is False at inference (ddpm.py:310-323 is then a no-op)

    def q_sample(self, x_start, t, noise=None):
        """ddpm.py:478-482."""
        noise = torch.randn_like(x_start) if noise is None else noise
        return (extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start +
                extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)


class LatentDiffusion(DDPM):
    """ddpm.py:712-5396, inference subset."""
    supports_tgate = True         # apply_model / apply_model_cfg_twin take tgate= (samplers: tgate.py)
    supports_deep_cache = True    # apply_model / apply_model_cfg_twin take deep_cache= (samplers: deep_cache.py)

    def __init__(self, first_stage_config, cond_stage_config=None, personalization_config=None,
                 num_timesteps_cond=None, cond_stage_key="image", cond_stage_trainable=False, concat_mode=True,
                 cond_stage_forward=None, conditioning_key=None, scale_factor=1.0, scale_by_std=False,
                 *args, **kwargs):
        if conditioning_key is None:
            conditioning_key = 'concat' if concat_mode else 'crossattn'
        unet_config = kwargs.pop("unet_config")
        kwargs.pop("ckpt_path", None)
        kwargs.pop("ignore_keys", None)
        super().__init__(unet_config, conditioning_key=conditioning_key, *args, **kwargs)
        self.cond_stage_key = cond_stage_key
        self.cond_stage_trainable = cond_stage_trainable
        self.scale_factor = scale_factor
        self.first_stage_model = instantiate_from_config(first_stage_config).eval()
        # ddpm.py:808-813, 860-880: the conditioning producer.  Constructed like the reference does so that the
        # `cond_stage_model.*` entries of an SD checkpoint load; its HIP engine is only created on first use.
        self.cond_stage_config = cond_stage_config
        self.personalization_config = personalization_config
        self.cond_stage_forward = cond_stage_forward
        self.cond_stage_model = None
        if isinstance(cond_stage_config, dict) and "target" in cond_stage_config:
            self.cond_stage_model = instantiate_from_config(cond_stage_config).eval()
        self.embedding_manager = None
        if self.cond_stage_model is not None:
            from adaface_amd.ldm.modules.embedding_manager import EmbeddingManager
            if isinstance(personalization_config, dict) and "target" in personalization_config:
                pc = dict(personalization_config.get("params", None) or {})
                pc.pop("embedding_manager_ckpt", None)
                self.embedding_manager = EmbeddingManager(self.cond_stage_model, **pc)
            else:
                self.embedding_manager = EmbeddingManager(self.cond_stage_model, subject_strings=[])
        self.compel_cfg_weight_level_range = None
        self.apply_compel_cfg_prob = 0
        self.empty_context = None
        self._concat_cond = None      # set_concat_cond (hybrid models)

    # ---- conditioning ------------------------------------------------------------------------
    def get_learned_conditioning(self, cond_in, zs_clip_features=None, zs_id_embs=None,
                                 zs_out_id_embs_scale_range=(1.0, 1.0), randomize_clip_weights=False,
                                 apply_arc2face_inverse_embs=False, apply_arc2face_embs=False, embman_iter_type=None):
        """ddpm.py:962-1076.  Accepts a pre-computed static prompt embedding tensor [B*16,77,768] (or
        [B,77,768], replicated over the 16 layers like embedding_manager.py:1342-1353) and wraps it into the
        (emb, prompts, extra_info) tuple the sampler and the UNet expect (ddpm.py:1056-1069)."""
        if isinstance(cond_in, torch.Tensor) and cond_in.is_floating_point():
            emb = cond_in
            if self.use_layerwise_embedding and emb.dim() == 3 and emb.shape[0] % self.N_CA_LAYERS != 0:
                raise ValueError("layerwise embedding must have batch divisible by 16")
            prompts = [""] * (emb.shape[0] // (self.N_CA_LAYERS if self.use_layerwise_embedding else 1))
            extra_info = {'use_layerwise_context': self.use_layerwise_embedding, 'use_conv_attn_kernel_size': -1,
                          'placeholder2indices': None, 'prompt_emb_mask': None, 'is_training': False,
                          'compel_cfg_weight_level_range': None, 'apply_compel_cfg_prob': 0,
                          'empty_context': self.empty_context, 'capture_distill_attn': False}
            return (emb, prompts, extra_info)
        # prompts (list of str) or token ids (int64 [B, 77]): the reference's flow, ddpm.py:966-1069
        if apply_arc2face_inverse_embs or apply_arc2face_embs:
            raise NotImplementedError("apply_arc2face_(inverse_)embs replace the prompt embeddings in training-time iterations "
                                      "(ddpm.py:1010-1053): not part of the inference path")
        if zs_clip_features is not None or zs_id_embs is not None:          # ddpm.py:992-999
            if not getattr(self.embedding_manager, "do_zero_shot", False):
                raise NotImplementedError("zero-shot identity conditioning needs an EmbeddingManager built with do_zero_shot=True "
                                          "(plus the Arc2Face encoder and SubjBasisGenerator weights, absent offline)")
            self.embedding_manager.set_zs_image_features(zs_clip_features, zs_id_embs, zs_out_id_embs_scale_range)
        if self.cond_stage_model is None:
            raise RuntimeError("this LatentDiffusion was built without a cond_stage_config: pass an embedding tensor")
        self.cond_stage_model.device = self.device
        if self.empty_context is not None:
            self.empty_context = self.empty_context.to(self.device)
        if randomize_clip_weights:
            self.cond_stage_model.sample_last_layers_skip_weights()
        self.embedding_manager.set_curr_iter_type(embman_iter_type or 'recon_iter')
        static_prompt_embedding = self.cond_stage_model.encode(cond_in, embedding_manager=self.embedding_manager)
        import copy
        extra_info = {'use_layerwise_context': self.use_layerwise_embedding,
                      'use_conv_attn_kernel_size': self.embedding_manager.use_conv_attn_kernel_size,
                      'placeholder2indices': copy.copy(self.embedding_manager.placeholder2indices),
                      'prompt_emb_mask': copy.copy(self.embedding_manager.prompt_emb_mask),
                      'is_training': self.embedding_manager.training,
                      'compel_cfg_weight_level_range': self.compel_cfg_weight_level_range,
                      'apply_compel_cfg_prob': self.apply_compel_cfg_prob,
                      'empty_context': self.empty_context,
                      'capture_distill_attn': False}
        prompts = list(cond_in) if not isinstance(cond_in, torch.Tensor) else [""] * cond_in.shape[0]
        return (static_prompt_embedding, prompts, extra_info)

    @staticmethod
    def layerwise_repeat(emb, n_layers=16):
        """[B,T,D] -> [B*16,T,D] with the layer copies adjacent per instance (embedding_manager.py:1342-1353)."""
        B, T, D = emb.shape
        return emb.unsqueeze(1).expand(B, n_layers, T, D).reshape(B * n_layers, T, D).contiguous()

    # ---- denoiser ----------------------------------------------------------------------------
    def set_concat_cond(self, c_concat):
        """The channels a hybrid model (conditioning_key "hybrid": the 9-channel inpainting U-Net) concatenates onto x_noisy
        in every apply_model / apply_model_cfg_twin / apply_model_cfg_pag whose condition carries no c_concat of its own:
        [1 or B, Cc, H, W] (adaface_amd.img2img.concat_cond), or None to clear.  The samplers stay unaware of it.  Not a
        reference method."""
        if self.model.conditioning_key != "hybrid":
            raise ValueError(f"set_concat_cond: conditioning_key is {self.model.conditioning_key!r}; only a 'hybrid' model "
                             "concatenates a condition onto its input")
        if c_concat is not None:
            unet = self.model.diffusion_model
            want = unet.in_channels - unet.out_channels
            if not isinstance(c_concat, torch.Tensor) or c_concat.dim() != 4 or c_concat.shape[1] != want:
                raise ValueError(f"set_concat_cond: a tensor [1 or B, {want}, H, W] is needed")
        self._concat_cond = c_concat
        return self

    def _with_concat(self, cond: dict, x_noisy):
        """cond with the stored c_concat (hybrid models, when cond has none), fitted to x_noisy's batch."""
        if self.model.conditioning_key != "hybrid" or "c_concat" in cond:
            return cond
        cc = self._concat_cond
        if cc is None:
            raise ValueError("a hybrid model needs its concatenated condition: set_concat_cond, or cond = {c_concat, c_crossattn}")
        B = x_noisy.shape[0]
        if cc.shape[0] != B:
            if B % cc.shape[0] != 0:
                raise ValueError(f"set_concat_cond: {cc.shape[0]} samples for a batch of {B}")
            cc = cc.repeat(B // cc.shape[0], 1, 1, 1)     # (a batch [x; x] takes [cc; cc])
        if tuple(cc.shape[2:]) != tuple(x_noisy.shape[2:]):
            raise ValueError(f"set_concat_cond: the condition is {tuple(cc.shape[2:])}, the latent {tuple(x_noisy.shape[2:])}")
        return dict(cond, c_concat=[cc])

    def apply_model(self, x_noisy, t, cond, return_ids=False, deep_cache=None, tgate=None):
        """ddpm.py:2192-2297 (the split_input_params patch mode is never active: SURVEY.md §8a a6).
        deep_cache (not in the reference): None, ("refresh", k) or ("reuse", k), see UNetModel.forward.
        tgate (not in the reference): None, "capture" or "replay" (T-GATE, tgate.py), see UNetModel.forward."""
        if not isinstance(cond, dict):
            if not isinstance(cond, list):
                cond = [cond]
            key = 'c_concat' if self.model.conditioning_key == 'concat' else 'c_crossattn'
            cond = {key: cond}
        cond = self._with_concat(cond, x_noisy)
        if tgate is not None:
            x_recon = self.model(x_noisy, t, deep_cache=deep_cache, tgate=tgate, **cond)
        else:
            x_recon = self.model(x_noisy, t, **cond) if deep_cache is None else self.model(x_noisy, t, deep_cache=deep_cache, **cond)
        if isinstance(x_recon, tuple) and not return_ids:
            return x_recon[0]
        return x_recon

    def apply_model_cfg_twin(self, x_noisy, t, cond_twin, deep_cache=None, tgate=None):
        """apply_model(torch.cat([x] * 2), torch.cat([t] * 2), cond_twin) -- the classifier-free-guidance call of
        p_sample_ddim / p_sample_plms (ddim.py:236-247) -- without the concatenation: `cond_twin` is the condition of the
        2B samples (cond first), x_noisy / t those of one half.  Returns eps of the 2B samples.  Not a reference method: the
        drop-in samplers use it when the model has it, and fall back to apply_model on the concatenated batch otherwise."""
        cond = cond_twin
        if not isinstance(cond, dict):
            if not isinstance(cond, list):
                cond = [cond]
            cond = {'c_crossattn': cond}
        if 'c_crossattn' in cond:
            cond = self._with_concat(cond, x_noisy)
        if tgate is not None:         # (T-GATE capture on the twin form: the kept outputs are the means over the two legs)
            if 'c_crossattn' not in cond:
                raise NotImplementedError("apply_model_cfg_twin: T-GATE needs a cross-attention condition")
            return self.model(x_noisy, t, cfg_twin=True, deep_cache=deep_cache, tgate=tgate, **cond)
        if 'c_crossattn' not in cond:
            return self.apply_model(torch.cat([x_noisy] * 2), torch.cat([t] * 2), cond_twin)
        if deep_cache is not None:
            return self.model(x_noisy, t, cfg_twin=True, deep_cache=deep_cache, **cond)
        return self.model(x_noisy, t, cfg_twin=True, **cond)

    def apply_model_cfg_pag(self, x_noisy, t, cond_twin, deep_cache=None):
        """The three-leg call of perturbed-attention guidance, beside apply_model_cfg_twin and with its arguments: `cond_twin`
        is the condition of 2B samples (cond FIRST), x_noisy / t those of one leg.  Returns eps of 3B samples, legs (cond,
        uncond, perturbed): the third leg is the first with the identity as the attention map of the self-attention layers
        given to set_pag.  Not a reference method."""
        cond = cond_twin
        if not isinstance(cond, dict):
            if not isinstance(cond, list):
                cond = [cond]
            cond = {'c_crossattn': cond}
        if 'c_crossattn' not in cond:
            raise NotImplementedError("apply_model_cfg_pag: perturbed-attention guidance needs a cross-attention condition")
        cond = self._with_concat(cond, x_noisy)
        if deep_cache is not None:
            return self.model(x_noisy, t, cfg_pag=True, deep_cache=deep_cache, **cond)
        return self.model(x_noisy, t, cfg_pag=True, **cond)

    # ---- decoder -----------------------------------------------------------------------------
    @torch.no_grad()
    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False):
        """ddpm.py:1251-1308: z / scale_factor -> first_stage_model.decode; the division is folded into
        the NCHW->NHWC conversion kernel at the head of the HIP decoder."""
        if predict_cids:
            raise NotImplementedError("VQ codebook ids are not used by the KL autoencoder")
        return self.first_stage_model.decode(z, scale_factor=self.scale_factor)

    @torch.no_grad()
    def decode_first_stage_uint8(self, z):
        """decode + clamp((x+1)/2,0,1)*255 -> uint8 HWC (stable_txt2img.py:713-715,764-765) in one pass."""
        return self.first_stage_model.decode(z, scale_factor=self.scale_factor, return_uint8=True)

    @torch.no_grad()
    def encode_first_stage(self, x, mask=None):
        """ddpm.py:1372-1410 (the non-patched branch): first_stage_model.encode -> posterior."""
        return self.first_stage_model.encode(x, mask)

    @torch.no_grad()
    def get_first_stage_encoding(self, encoder_posterior):
        """ddpm.py:947-954: sample the posterior (a tensor passes through) and apply scale_factor."""
        from adaface_amd.ldm.models.autoencoder import DiagonalGaussianDistribution
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            return encoder_posterior.sample(scale=self.scale_factor)
        if isinstance(encoder_posterior, torch.Tensor):
            return self.scale_factor * encoder_posterior
        raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")

    # ---- fp8 mode: calibrated activation scales (adaface_hip.h, af_fp8_*) --------------------------
    @torch.no_grad()
    def calibrate_fp8(self, conditioning, unconditional_conditioning=None, shape=None, batch_size=1, S=10,
                      guidance_scale=7.5, x_T=None, passes=2, headroom=1):
        """Static per-site activation scales for the fp8 mode from a short DDIM sample (S steps, eta 0) with the caller's
        conditioning (as get_learned_conditioning returns it).  Needs set_compute_dtype('fp8') and weights loaded.  The
        sample is run `passes` times, each on the scales the one before derived.  Returns {site name: (amax, shift, nsat
        of the last pass)}; the shifts stay with the UNet module (save_fp8_scales) until the next load_state_dict."""
        from adaface_amd.ldm.models.diffusion.ddim import DDIMSampler
        unet = self.model.diffusion_model
        if shape is None:
            shape = [unet.out_channels, unet.image_size, unet.image_size]     # (the latent: a hybrid U-Net takes more)
        if x_T is None:
            x_T = torch.randn(batch_size, *shape, generator=torch.Generator().manual_seed(0)).to(self.device)
        sampler = DDIMSampler(self)

        def run():
            sampler.sample(S=S, conditioning=conditioning, batch_size=batch_size, shape=list(shape), verbose=False,
                           guidance_scale=guidance_scale, unconditional_conditioning=unconditional_conditioning, eta=0.0,
                           x_T=x_T)
        return unet.calibrate_fp8(run, self.device, passes=passes, headroom=headroom)

    def save_fp8_scales(self, path):
        self.model.diffusion_model.save_fp8_scales(path)

    def load_fp8_scales(self, path):
        """Load scales AFTER the weights (load_state_dict clears them) and with the compute dtype at 'fp8'."""
        self.model.diffusion_model.load_fp8_scales(path, self.device)
        return self

    def set_token_merging(self, ratio, max_downsample=1):
        """UNetModel.set_token_merging: opt-in token merging in front of the U-Net's self-attention (0 = off)."""
        self.model.diffusion_model.set_token_merging(ratio, max_downsample)
        return self

    def set_freeu(self, version, b1=1.0, b2=1.0, s1=1.0, s2=1.0):
        """UNetModel.set_freeu: opt-in FreeU backbone scaling and Fourier-filtered skips in the U-Net (version 0 = off)."""
        self.model.diffusion_model.set_freeu(version, b1, b2, s1, s2)
        return self

    def set_pag(self, layers):
        """UNetModel.set_pag: the self-attention layers perturbed on the third leg of apply_model_cfg_pag -- names ("mid",
        "down.blocks.2", "up.blocks.1", ...) or site numbers; None or () = off."""
        self.model.diffusion_model.set_pag(layers)
        return self

    def set_sag(self, on=True):
        """UNetModel.set_sag: while on, every U-Net forward that runs the middle block also keeps the attention mass of its
        self-attention (self-attention guidance, guidance.py); sag_mass reads the last one.  The samplers switch it per call."""
        self.model.diffusion_model.set_sag(on)
        return self

    def sag_mass(self):
        """UNetModel.sag_mass: fp32 [B, N] of the last forward made with set_sag on."""
        return self.model.diffusion_model.sag_mass()

    def set_regions(self, weights):
        """UNetModel.set_regions: regional prompts (adaface_amd/regions.py).  weights [Bf, R, H, W] for the samples of the
        conditioning the samplers pass (regions.build_weights; legs=2 for a run with an unconditional conditioning), whose
        context is regions.concat_contexts' [.., R T, D]; None = off."""
        self.model.diffusion_model.set_regions(weights)
        return self

    @property
    def regions(self):
        return self.model.diffusion_model.regions

    @property
    def pag(self) -> tuple:
        return self.model.diffusion_model.pag

    @property
    def has_guidance_embedding(self) -> bool:
        return getattr(self.model.diffusion_model, "time_cond_proj_dim", None) is not None

    @property
    def guidance_embedding(self):
        """The guidance scale set_guidance_embedding folded into the U-Net's time embedding, or None."""
        return getattr(self.model.diffusion_model, "guidance_embedding", None)

    def set_guidance_embedding(self, w):
        """UNetModel.set_guidance_embedding: feed the guidance scale w through the guidance-scale embedding of a distilled LCM
        checkpoint (U-Net config key time_cond_proj_dim) in every following forward; None = off.  LCMSampler.sample(
        guidance_embedding=True) sets and removes it around a run."""
        unet = self.model.diffusion_model
        if not hasattr(unet, "set_guidance_embedding"):
            if w is None:
                return self
            raise ValueError("set_guidance_embedding: this model's U-Net has no guidance-scale embedding")
        unet.set_guidance_embedding(w)
        return self

    def set_lora(self, adapters):
        """LoRA adapters on the U-Net and the text tower (HipModule.set_lora on each): `adapters` is a list of (split, scale), at
        most 8, with split = {"unet": weights, "text": weights} as adaface_amd.lora.split_lora returns it (either key may be
        missing).  [] restores the base model.  Call it before the prompt is encoded: a text-tower adapter changes the context.
        Text weights without a HIP text tower in this model raise ValueError."""
        adapters = list(adapters or ())
        for i, item in enumerate(adapters):
            if not isinstance(item, (tuple, list)) or len(item) != 2 or not isinstance(item[0], dict) or set(item[0]) - {"unet", "text", "unused"}:
                raise ValueError(f"set_lora: adapter {i} is not a ({{'unet': ..., 'text': ...}}, scale) pair")
        text = [(split.get("text") or {}, scale) for split, scale in adapters]
        cond = self.cond_stage_model
        if any(w for w, _ in text) and not hasattr(cond, "set_lora"):
            raise ValueError("set_lora: the adapters hold text-tower weights but this model has no HIP text tower (cond_stage_model)")
        self.model.diffusion_model.set_lora([(split.get("unet") or {}, scale) for split, scale in adapters])
        if hasattr(cond, "set_lora"):
            cond.set_lora(text)
        return self

    def clear_lora(self):
        return self.set_lora([])

    def set_compute_dtype(self, dtype: str, fp8_scope: str = "base"):
        """'bf16' | 'f32' | 'f16' (alias 'fp16') | 'fp8' (the UNet's ResBlock convolutions in e4m3; VAE and text tower stay bf16).
        fp8_scope: 'base' (ResBlock convolutions and self-attention q / k / v) or 'base+ff' (also the transformer blocks'
        FeedForward); only looked at with dtype 'fp8'."""
        from adaface_amd.fp8_calib import parse_fp8_scope
        parse_fp8_scope(fp8_scope)                  # (refuse a bad scope before anything changes)
        if dtype != "fp8" and fp8_scope != "base":
            raise ValueError(f"fp8_scope={fp8_scope!r} needs the compute dtype 'fp8' (got {dtype!r})")
        if dtype == "fp16":
            dtype = "f16"
        rest = "bf16" if dtype == "fp8" else dtype
        if dtype == "fp8":
            self.model.diffusion_model.set_fp8_scope(fp8_scope)
        self.model.diffusion_model.set_compute_dtype(dtype)
        self.first_stage_model.set_compute_dtype(rest)
        if self.cond_stage_model is not None:
            self.cond_stage_model.set_compute_dtype(rest)
        return self
