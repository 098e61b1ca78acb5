"""Drop-in for ldm.modules.diffusionmodules.openaimodel.UNetModel (reference
openaimodel.py:417-1052): same constructor kwargs, same forward signature, same state_dict
keys; the forward pass is one af_unet_forward call into the hand-written HIP path.
"""
from __future__ import annotations

from typing import Optional

import torch

from adaface_amd import layout
from adaface_amd.ldm._hipmodule import HipModule, _Node, build_param_tree


class UNetModel(HipModule):
    _ckpt_prefix = "model.diffusion_model."

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None,
                 use_checkpoint=False, use_fp16=False, num_heads=-1, num_head_channels=-1, num_heads_upsample=-1,
                 use_scale_shift_norm=False, resblock_updown=False, use_new_attention_order=False,
                 use_spatial_transformer=False, transformer_depth=1, context_dim=None, n_embed=None, legacy=True,
                 time_cond_proj_dim=None):
        super().__init__()
        # the SD-v1 family is the hot path (v1-inference-ada.yaml:35-50); other branches of the
        # reference constructor are training / legacy-LDM variants outside SURVEY.md §8
        unsupported = {
            "dims != 2": dims != 2, "num_classes": num_classes is not None, "use_scale_shift_norm": use_scale_shift_norm,
            "resblock_updown": resblock_updown, "n_embed": n_embed is not None, "dropout": dropout != 0,
            "not conv_resample": not conv_resample, "not use_spatial_transformer": not use_spatial_transformer,
            "num_head_channels": num_head_channels != -1,
            "num_heads_upsample": num_heads_upsample not in (-1, num_heads),
        }
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"UNetModel: options outside the SD-v1 denoising path: {bad}")
        if context_dim is None or num_heads == -1:
            raise ValueError("UNetModel: context_dim and num_heads are required (spatial transformer)")
        if hasattr(context_dim, "__len__"):
            context_dim = list(context_dim)
            if len(context_dim) != 1:
                raise NotImplementedError("a single context_dim is supported")
            context_dim = context_dim[0]
        self.image_size = image_size
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = tuple(attention_resolutions)
        self.channel_mult = tuple(channel_mult)
        self.num_heads = num_heads
        self.context_dim = int(context_dim)
        self.transformer_depth = transformer_depth
        self.use_checkpoint = use_checkpoint  # accepted, meaningless at inference (util.py:115)
        self.dtype = torch.float32            # dtype of the tensors crossing the boundary
        self.debug_attn = False
        if use_fp16:
            self.compute_dtype = "bf16"
        shapes = layout.unet_param_shapes(**self._layout_kwargs())
        build_param_tree(self, shapes, zero_init=layout.unet_zero_init_names(shapes))
        object.__setattr__(self, "_ctx_key", None)
        object.__setattr__(self, "_control", None)     # ControlNet (set_control)
        # the guidance-scale embedding of a distilled LCM checkpoint (not in the reference; None = absent, nothing changes):
        # time_embed.cond_proj.weight [model_channels, dim], no bias.  The weight lives on the Python side only -- it is folded
        # into the engine's time_embed.0.bias (set_guidance_embedding), never an engine tensor.  Zero until a checkpoint is loaded.
        self.time_cond_proj_dim = None if time_cond_proj_dim is None else int(time_cond_proj_dim)
        if self.time_cond_proj_dim is not None:
            if self.time_cond_proj_dim < 4:
                raise ValueError(f"UNetModel: time_cond_proj_dim {time_cond_proj_dim!r} (None, or at least 4)")
            node = _Node()
            node.register_parameter("weight", torch.nn.Parameter(torch.zeros(model_channels, self.time_cond_proj_dim),
                                                                 requires_grad=False))
            self.time_embed.add_module("cond_proj", node)
            self._register_load_state_dict_pre_hook(self._accept_diffusers_cond_proj)
        object.__setattr__(self, "_guidance_w", None)  # set_guidance_embedding

    @staticmethod
    def _accept_diffusers_cond_proj(state_dict, prefix, *args):
        """diffusers names the weight time_embedding.cond_proj.weight; either name loads."""
        theirs, ours = prefix + "time_embedding.cond_proj.weight", prefix + "time_embed.cond_proj.weight"
        if theirs in state_dict and ours not in state_dict:
            state_dict[ours] = state_dict.pop(theirs)

    def _layout_kwargs(self):
        return dict(in_channels=self.in_channels, model_channels=self.model_channels, out_channels=self.out_channels,
                    num_res_blocks=self.num_res_blocks, attention_resolutions=self.attention_resolutions,
                    channel_mult=self.channel_mult, context_dim=self.context_dim,
                    transformer_depth=self.transformer_depth)

    def _engine_kwargs(self):
        kw = self._layout_kwargs()
        kw.update(num_heads=self.num_heads, n_context_layers=16)
        return {"unet": kw}

    def _mark_dirty(self):
        super()._mark_dirty()
        object.__setattr__(self, "_ctx_key", None)  # cached K/V depend on the weights

    def _lora_changed(self):
        object.__setattr__(self, "_ctx_key", None)  # (set_lora: attn2.to_k / to_v may have changed, as in _mark_dirty)
        if self._guidance_w is not None and self._engine is not None and not self._weights_dirty:
            self._load_time_bias()      # (the folded bias holds the merged time_embed.0 weight, which may have changed)

    # ---- guidance-scale embedding (distilled LCM checkpoints) -------------------------------------
    @property
    def guidance_embedding(self):
        """The guidance scale w folded into the time embedding, or None."""
        return self._guidance_w

    def folded_time_bias(self, w):
        """time_embed.0.bias + W0 (Wc wemb(w)), a float64 host tensor: the bias under which time_embed.0(temb) equals
        time_embed.0(temb + Wc wemb) (the engine takes it rounded once to fp32).  W0 is the
        EFFECTIVE time_embed.0 weight, base plus the adapters of set_lora (adaface_amd.lora.merge_host).  The fold is exact: w is
        constant over a run and time_embed.0 is linear."""
        from adaface_amd.ldm.modules.diffusionmodules.util import guidance_scale_embedding
        from adaface_amd.lora import merge_host
        if self.time_cond_proj_dim is None:
            raise ValueError("UNetModel: no guidance-scale embedding (built without time_cond_proj_dim: there is no "
                             "time_embed.cond_proj.weight)")
        params = dict(self.named_parameters())
        wemb = torch.from_numpy(guidance_scale_embedding(w, self.time_cond_proj_dim))
        W0 = merge_host(params["time_embed.0.weight"], self._lora_of("time_embed.0"))
        Wc = params["time_embed.cond_proj.weight"].detach().double().cpu()
        return params["time_embed.0.bias"].detach().double().cpu() + W0 @ (Wc @ wemb)

    def _load_time_bias(self):
        """The engine's time_embed.0.bias for the current setting: the folded one, or the parameter itself."""
        eng = self._engine
        bias = self.folded_time_bias(self._guidance_w) if self._guidance_w is not None else \
            dict(self.named_parameters())["time_embed.0.bias"]
        eng.load_tensor(self._ckpt_prefix + "time_embed.0.bias", bias)
        eng.unet_cache_invalidate()     # (a kept DeepCache feature was computed under the previous time embedding)

    def set_guidance_embedding(self, w):
        """Feed the guidance scale w through the model's guidance-scale embedding in every following forward; None = off, which
        restores the original bias exactly.  The embedding Wc wemb(w) is added in front of time_embed.0 by folding it into that
        layer's bias (folded_time_bias) -- the forward itself does not change.  Kept for every later engine and re-applied
        after set_lora and after every weight upload; a live engine is switched now."""
        if w is not None:
            self.folded_time_bias(w)                # (refuses a model without cond_proj, and a w that is no finite number)
            w = float(w)
        changed = w != self._guidance_w
        object.__setattr__(self, "_guidance_w", w)
        if changed and self._engine is not None and not self._weights_dirty:
            self._load_time_bias()
        return self

    def sync_weights(self):
        super().sync_weights()
        if self._engine is not None and self._guidance_w is not None:
            self._load_time_bias()

    def _compel_cfg(self, context, B, info):
        """Inference-time compel cfg (openaimodel.py:898-916 + prob_apply_compel_cfg, util.py:2063-2094): per conditioned
        layer, with probability apply_compel_cfg_prob, the context of the FIRST half of the batch becomes
        (ctx - empty) * 1.1**level + empty.  The Python `random` draws are made in the reference's order (one per layer,
        then the level and two inner draws when it applies), so a seeded run re-weights the same layers.  Returns the
        re-weighted context and whether it may be cached (prob >= 1 and a degenerate level range: the reference
        re-draws on every forward otherwise).  The arithmetic is af_lincomb: w*ctx + (1-w)*empty."""
        import random
        from adaface_amd import ops
        empty, rng, prob = info.get("empty_context", None), info.get("compel_cfg_weight_level_range", None), info["apply_compel_cfg_prob"]
        if empty is None or rng is None:
            return context, True
        is_range = isinstance(rng, (list, tuple))
        deterministic = prob >= 1 and (not is_range or rng[0] == rng[1])
        key = ("compel", id(context), getattr(context, "_version", 0), id(empty), prob, tuple(rng) if is_range else rng)
        if deterministic and getattr(self, "_compel_key", None) == key:
            return self._compel_ctx, True
        L = 16
        ctx = context.reshape(B, L, -1, context.shape[-1]).clone()
        half = B // 2
        e = empty.to(ctx.device, torch.float32).expand(half, *ctx.shape[2:]).contiguous()
        for l in range(L):
            if random.random() > prob:
                continue
            level = random.uniform(*rng) if is_range else rng
            random.random(); random.random()          # the recursive calls on (v, k) draw once each (util.py:2077)
            w = 1.1 ** level
            if half > 0:
                ctx[:half, l] = ops.lincomb([(ctx[:half, l].contiguous(), w), (e, 1.0 - w)])
        ctx = ctx.reshape(context.shape)
        if deterministic:
            object.__setattr__(self, "_compel_key", key)
            object.__setattr__(self, "_compel_ctx", ctx)
            object.__setattr__(self, "_compel_refs", (context, empty))
        return ctx, deterministic

    def set_token_merging(self, ratio, max_downsample=1):
        """Token merging in front of every self-attention whose map is the latent's divided by at most max_downsample (1 or 2):
        `ratio` in [0, 0.75] of a map's tokens are merged into their most similar neighbour of a 2 x 2 cell before attn1 and
        copied back after it (ToMe for Stable Diffusion; not in the reference, off by default, 0 = off).  Kept for every later
        engine; a live one is switched now.  bf16 and f32 compute dtypes."""
        from adaface_amd.engine import check_tome_args
        setting = check_tome_args(ratio, max_downsample)
        if setting[0] > 0.0 and self.compute_dtype in ("f16", "fp8"):
            raise ValueError(f"token merging runs with the compute dtypes 'bf16' and 'f32' (compute dtype is {self.compute_dtype!r})")
        if self._engine is not None:
            self._engine.set_tome(*setting)
        object.__setattr__(self, "_tome", setting)
        return self

    @property
    def token_merging(self) -> tuple:
        return self._tome

    def set_freeu(self, version, b1=1.0, b2=1.0, s1=1.0, s2=1.0):
        """FreeU (Si et al., CVPR 2024; not in the reference, off by default): in front of every output block whose incoming
        backbone has 4 * model_channels (b1, s1) or 2 * model_channels (b2, s2) channels, the first half of the backbone's
        channels is scaled by b (version 1) or by (b - 1) * mhat + 1 (version 2) and the skip's lowest frequencies by s.
        version 0 = off; b in [1, 2], s in [0, 1].  Kept for every later engine; a live one is switched now.  Every compute
        dtype."""
        from adaface_amd.engine import check_freeu_args
        setting = check_freeu_args(version, b1, b2, s1, s2)
        if self._engine is not None:
            self._engine.set_freeu(*setting)
        object.__setattr__(self, "_freeu", setting)
        return self

    @property
    def freeu(self) -> tuple:
        return self._freeu

    def set_pag(self, layers):
        """Perturbed-attention guidance (Ahn et al., ECCV 2024; not in the reference, off by default): the self-attention
        layers whose attention map is the identity on the third leg of forward(cfg_pag=True) -- names ("mid", "down.blocks.0..2",
        "up.blocks.1..3") and / or site numbers in forward order; None or () = off.  Every other forward ignores the set.  Kept
        for every later engine; a live one is switched now.  Every compute dtype."""
        from adaface_amd.engine import pag_sites_of
        sites = pag_sites_of(self._layout_kwargs(), layers)
        if self._engine is not None:
            self._engine.set_pag(sites)
        object.__setattr__(self, "_pag", sites)
        return self

    @property
    def pag(self) -> tuple:
        return self._pag

    def set_sag(self, on=True):
        """Self-attention guidance capture (Hong et al., ICCV 2023; not in the reference, off by default): while on, every
        forward that runs the middle block also keeps the attention mass per key of middle_block.1.transformer_blocks.0.attn1 for
        all samples of the call (sag_mass reads it); the forward's result is unchanged.  Kept for every later engine; a live one
        is switched now.  Every compute dtype except fp8; cfg_pag, tgate, a ControlNet, regional prompts and a DeepCache reuse
        step then raise NotImplementedError."""
        on = bool(on)
        if on and self.compute_dtype == "fp8":
            raise ValueError("self-attention guidance does not run with the compute dtype 'fp8'")
        if self._engine is not None:
            self._engine.set_sag(on)
        object.__setattr__(self, "_sag", on)
        return self

    @property
    def sag(self) -> bool:
        return self._sag

    def sag_mass(self):
        """The attention mass of the last forward made while set_sag was on, fp32 [B, N] (Engine.sag_mass)."""
        if self._engine is None:
            raise RuntimeError("sag_mass: no forward has run yet")
        return self._engine.sag_mass()

    def set_regions(self, weights):
        """Regional prompts (attention couple; not in the reference, off by default; adaface_amd/regions.py): weights
        [Bf, R, H, W] >= 0 at the latent resolution, for the Bf samples of the context the following forwards are given (under
        cfg_twin: both legs, unconditional ones (1, 0, ..., 0)).  That context's token axis is R segments of equal length,
        segment 0 the base prompt.  None = off.  cfg_pag, tgate, a ControlNet and conv attention then raise
        NotImplementedError."""
        if weights is not None:
            weights = torch.as_tensor(weights)
            if weights.dim() != 4:
                raise ValueError(f"set_regions: weights of shape {tuple(weights.shape)}, expected [Bf, R, H, W]")
            if not torch.isfinite(weights).all() or bool((weights < 0).any()):
                raise ValueError("set_regions: weights must be finite and >= 0")
            if weights.shape[2] % 8 or weights.shape[3] % 8:
                raise ValueError(f"set_regions: weight map {tuple(weights.shape[2:])}: sides must be multiples of 8")
            if not 1 <= weights.shape[1] <= 8:
                raise ValueError(f"set_regions: {weights.shape[1]} regions (1 .. 8, the base prompt included)")
            weights = weights.detach().float().contiguous()
        object.__setattr__(self, "_regions", weights)
        return self

    @property
    def regions(self):
        return getattr(self, "_regions", None)

    def _apply_regions(self, eng, B):
        """Bring the engine's regions in line with set_regions for the context just set (key _ctx_key)."""
        w = self.regions
        applied = getattr(self, "_regions_applied", None)
        if w is None:
            if applied is not None:
                eng.set_regions(None)
                object.__setattr__(self, "_regions_applied", None)
            return
        if w.shape[0] not in (B, 2 * B):
            raise ValueError(f"set_regions: weights for {w.shape[0]} samples, this forward's context has {B}")
        key = (id(w), B, self._ctx_key, id(eng))
        if key != applied or eng.region_state()["R"] != w.shape[1]:
            eng.set_regions(w[:B])      # (a single-leg call of a guided run: the conditional legs, which come first)
            object.__setattr__(self, "_regions_applied", key)

    def set_control(self, controlnet, hint=None, scale=1.0, scales=None, t_range=None, cond_only=False):
        """ControlNet (Zhang et al., ICCV 2023; not in the reference, off by default): every forward whose timesteps ALL lie in
        t_range = (t_lo, t_hi) (DDPM timesteps; None = always) also runs `controlnet` (a ControlNet module of this U-Net's
        layout and storage dtype) on (x, t, the context this forward uses, hint) and adds its 13 residuals, times `scale` or the
        per-residual list `scales`, to the skip connections where the decoder reads them and to the middle block's output.
        hint: [1 or B, 3, 8 H, 8 W] in [0, 1]; its features are computed once.  Under cfg_twin the control branch runs on both
        legs; cond_only=True runs it on the conditional samples only and leaves the unconditional leg bit for bit as it is
        without control.  Outside the window the forward is exactly the uncontrolled one.  deep_cache composes (a reuse step of
        depth k runs the first k control blocks only); cfg_pag and tgate are refused.  set_control(None) switches it off."""
        from adaface_amd.engine import check_control_scales, check_control_window
        if controlnet is None:
            object.__setattr__(self, "_control", None)
            if self._engine is not None:
                self._engine.set_control(None)
            return self
        from adaface_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
        if not isinstance(controlnet, ControlNet):
            raise TypeError(f"set_control: a ControlNet module is needed, got {type(controlnet).__name__}")
        if self.in_channels != self.out_channels:
            raise NotImplementedError(f"set_control: ControlNet on a hybrid U-Net ({self.in_channels} input channels, "
                                      f"{self.out_channels} latent channels) is not built")
        mine, theirs = self._layout_kwargs(), controlnet._layout_kwargs()
        for k in ("in_channels", "model_channels", "num_res_blocks", "attention_resolutions", "channel_mult", "context_dim",
                  "transformer_depth"):
            if mine[k] != theirs[k]:
                raise ValueError(f"set_control: the ControlNet's {k} = {theirs[k]!r}, this U-Net's {mine[k]!r}")
        if hint is None or hint.dim() != 4 or hint.shape[1] != controlnet.hint_channels:
            raise ValueError(f"set_control: hint [1 or B, {controlnet.hint_channels}, 8 H, 8 W] is needed")
        if hint.shape[2] % 8 or hint.shape[3] % 8:
            raise ValueError(f"set_control: hint sides {tuple(hint.shape[2:])} must be multiples of 8")
        n = len(layout.unet_blocks(self.model_channels, self.channel_mult, self.num_res_blocks, self.attention_resolutions,
                                   self.in_channels)[0]) + 1
        ctl = dict(net=controlnet, hint=hint, scales=check_control_scales(scale, scales, n), window=check_control_window(t_range),
                   cond_only=bool(cond_only))
        object.__setattr__(self, "_control", ctl)
        return self

    @property
    def control(self):
        return self._control

    def _apply_control(self, eng, x, timesteps, ctx, given, B1, layerwise, cfg_twin, deep_cache):
        """Run the control branch for this forward and attach its residuals to `eng` (or detach, outside the window)."""
        from adaface_amd.engine import control_active
        ctl = self._control
        if ctl is None:
            return
        if not control_active(timesteps, ctl["window"]):
            eng.set_control(None)
            return
        net, hint = ctl["net"], ctl["hint"]
        H, W = x.shape[2], x.shape[3]
        storage = lambda d: "bf16" if d == "fp8" else d
        if storage(net.compute_dtype) != storage(self.compute_dtype):
            raise ValueError(f"ControlNet: its compute dtype {net.compute_dtype!r} is not this U-Net's storage dtype "
                             f"{storage(self.compute_dtype)!r} (set_compute_dtype on the ControlNet)")
        if tuple(hint.shape[2:]) != (8 * H, 8 * W):
            raise ValueError(f"ControlNet: the hint is {tuple(hint.shape[2:])}, 8 times the {H} x {W} latent is {(8 * H, 8 * W)}")
        if hint.shape[0] not in (1, B1):
            raise ValueError(f"ControlNet: hint batch {hint.shape[0]} for {B1} samples (1 or {B1})")
        ceng = net.engine(x.device)
        cond_only = ctl["cond_only"] and cfg_twin
        both = cfg_twin and not cond_only
        Bc = 2 * B1 if both else B1
        if cfg_twin and not both:                       # the conditional samples' context: whole samples, their layer slices together
            per = ctx.shape[0] // (2 * B1)
            ctx = ctx[:B1 * per]
        net._set_hint(ceng, hint)
        net._set_context(ceng, ctx, (given, Bc), Bc, layerwise)
        xc = torch.cat([x, x]) if both else x
        tc = torch.cat([timesteps, timesteps]) if both else timesteps
        n_blocks, scales = None, ctl["scales"]
        if deep_cache is not None and deep_cache[0] == "reuse":
            n_blocks = int(deep_cache[1])
            scales = scales[:n_blocks]
        flat = ceng.control_forward(xc, tc.to(x.device), n_blocks)
        eng.set_control(flat, scales, cond_only=cond_only, source=ceng, shape=(Bc, H, W))

    @staticmethod
    def _conv_attn_spec(ks, placeholder2indices):
        """(ks, batch indices, token positions) for Engine.set_conv_attn from the reference's
        extra_info['placeholder2indices'] = {subject string: (indices_B, indices_N)} (util.py:711-727): the M >= ks*ks
        positions of each subject sample are consecutive in indices_N; the first ks*ks are used.  Every subject string of
        the dict contributes its own rows (attention.py:208-216 loops over them); a sample that carries several strings
        appears once per string, in the dict's order.  Kernel sizes 2, 3, 4 as the reference (util.py:747-760)."""
        if ks is None or ks <= 1 or not placeholder2indices:
            return (0, (), ())
        if ks not in (2, 3, 4):
            raise NotImplementedError(f"conv attention kernel size {ks}: the reference pads for 2, 3 and 4 only (util.py:747-760)")
        batch, tokens = [], []
        for indices in placeholder2indices.values():
            if indices is None:
                continue
            idx_b = [int(v) for v in torch.as_tensor(indices[0]).tolist()]
            idx_n = [int(v) for v in torch.as_tensor(indices[1]).tolist()]
            if not idx_b:
                continue
            uniq = sorted(set(idx_b))
            M = len(idx_n) // len(uniq)
            if M < ks * ks:
                raise ValueError(f"{M} embeddings are not enough to cover a {ks}x{ks} kernel")
            for i, bi in enumerate(uniq):
                batch.append(bi)
                tokens.append(tuple(idx_n[i * M: i * M + ks * ks]))
        return (ks, tuple(batch), tuple(tokens))

    @torch.no_grad()
    def forward(self, x, timesteps=None, context=None, y=None, context_in=None, extra_info=None, cfg_twin=False, deep_cache=None,
                cfg_pag=False, tgate=None, **kwargs):
        """x [B,C,H,W], timesteps [B], context [B*16,T,D] (layerwise) or [B,T,D]; returns eps [B,C,H,W] fp32.
        Mirrors openaimodel.py:827-1052 for inference: `extra_info` keys read at :849-859.
        cfg_twin (not in the reference; used by this package's samplers): x / timesteps are ONE half of the
        classifier-free-guidance batch, the context is that of [x; x] (cond first, ddim.py:236-247); returns eps for the
        2B samples exactly as forward(torch.cat([x] * 2), torch.cat([t] * 2), context) would.
        deep_cache (not in the reference; DeepCache, set by this package's samplers): None = the plain forward;
        ("refresh", k) = the same forward, which also keeps the input of output_blocks[-k]; ("reuse", k) = only
        input_blocks[:k] and output_blocks[-k:] run, on the feature the last refresh kept.  A context or conv-attention spec
        that differs from the previous call's drops the kept feature (a reuse then raises AfError).
        cfg_pag (not in the reference; perturbed-attention guidance, set_pag): x / timesteps are ONE leg, the context is the
        twin condition of 2B samples (cond first), exactly what cfg_twin takes; returns eps for 3B samples, legs (cond, uncond,
        perturbed).  The third leg's context is the first B samples' AFTER the compel-cfg weighting, with their layerwise
        slices, and the conv-attention rows of the samples < B are repeated for the samples + 2B.
        tgate (not in the reference; T-GATE, set by this package's samplers, tgate.py): None = off; "capture" = this forward
        (plain or cfg_twin), which also keeps every cross-attention output, averaged over the legs; "replay" = the plain
        forward with every cross-attention replaced by what the capture kept -- the context is neither set nor read.
        With a ControlNet set (set_control) and every timestep inside its window, the control branch runs first on the same x,
        timesteps and context (after the compel-cfg weighting) and its residuals are added inside this forward; cfg_pag and
        tgate then raise NotImplementedError."""
        if y is not None:
            raise NotImplementedError("class-conditional UNet (num_classes) is not on the path")
        if tgate not in (None, "capture", "replay"):
            raise ValueError(f"UNetModel.forward: tgate {tgate!r} (None, \"capture\" or \"replay\")")
        if tgate is not None and cfg_pag:
            raise NotImplementedError("UNetModel.forward: T-GATE with the PAG form (the third leg has no cached counterpart)")
        if self._control is not None and (cfg_pag or tgate is not None):
            raise NotImplementedError("UNetModel.forward: ControlNet does not combine with the PAG form or T-GATE (set_control(None))")
        if self.regions is not None and (cfg_pag or tgate is not None or self._control is not None):
            raise NotImplementedError("UNetModel.forward: regional prompts do not combine with the PAG form, T-GATE or a ControlNet "
                                      "(set_regions(None))")
        if self._sag and (cfg_pag or tgate is not None or self._control is not None or self.regions is not None or
                          (deep_cache is not None and deep_cache[0] == "reuse")):
            raise NotImplementedError("UNetModel.forward: self-attention guidance capture does not combine with the PAG form, T-GATE, "
                                      "a ControlNet, regional prompts or a DeepCache reuse step (set_sag(False))")
        if tgate == "replay":
            if cfg_twin:
                raise ValueError("UNetModel.forward: a T-GATE replay runs one leg (no cfg_twin)")
            if timesteps is None:
                raise ValueError("UNetModel.forward needs timesteps")
            eng = self.engine(x.device)
            if deep_cache is None:
                out = eng.unet_forward(x, timesteps.to(x.device), tgate="replay")
            else:
                mode, depth = deep_cache
                out = eng.unet_forward_cached(x, timesteps.to(x.device), depth=int(depth), mode=mode, twin=False, tgate="replay")
            if extra_info is not None:
                extra_info["ca_layers_activations"] = {k: {} for k in ("outfeat", "attn", "attnscore", "q")}
            return out.type(x.dtype) if x.dtype != torch.float32 else out
        if timesteps is None or context is None:
            raise ValueError("UNetModel.forward needs timesteps and context")
        info = extra_info if extra_info is not None else {}
        layerwise = bool(info.get("use_layerwise_context", False))
        ks = info.get("use_conv_attn_kernel_size", None)
        conv = self._conv_attn_spec(ks, info.get("placeholder2indices", None))
        if info.get("img_mask", None) is not None or info.get("capture_distill_attn", False):
            raise NotImplementedError("img_mask / capture_distill_attn are training-time options")
        if info.get("iter_type", "normal_recon") == "mix_hijk":
            raise NotImplementedError("iter_type 'mix_hijk' (separate k/v contexts) is a training-time option")
        if cfg_pag and cfg_twin:
            raise ValueError("UNetModel.forward: cfg_pag and cfg_twin are two forms of one call; give one")
        if cfg_pag and not self._pag:
            raise ValueError("UNetModel.forward(cfg_pag=True): no PAG layer is set (set_pag)")
        eng = self.engine(x.device)
        B1 = x.shape[0]
        B = B1 * (2 if (cfg_twin or cfg_pag) else 1)           # samples of the context as given
        cache_ok = True
        given = context
        if layerwise and info.get("apply_compel_cfg_prob", 0) > 0:
            context, cache_ok = self._compel_cfg(context.to(x.device), B, info)
        if cfg_pag:
            B = 3 * B1
            if conv[0]:
                extra = [(b + 2 * B1, tok) for b, tok in zip(conv[1], conv[2]) if b < B1]
                conv = (conv[0], conv[1] + tuple(b for b, _ in extra), conv[2] + tuple(tok for _, tok in extra))
        # Hoisted cross-attention K/V are cached per context TENSOR OBJECT: a reference to it is kept so that its
        # id / storage cannot be recycled for another prompt while the cache is live (data_ptr alone is unsafe).
        key = (id(context), getattr(context, "_version", 0), tuple(context.shape), layerwise, B, conv)
        if self.regions is not None and conv[0]:
            raise NotImplementedError("UNetModel.forward: regional prompts do not combine with conv attention (set_regions(None))")
        if self.regions is None and getattr(self, "_regions_applied", None) is not None:
            self._apply_regions(eng, B)         # (off again, before set_conv_attn below could be refused)
        if key != self._ctx_key or not cache_ok:
            if key != self._ctx_key:
                eng.unet_cache_invalidate()     # (the kept DeepCache feature was computed under the previous conditioning)
            eng.set_conv_attn(*conv)
            ctx = context.to(x.device)
            if cfg_pag:                         # [c; uc] -> [c; uc; c]: whole samples (their 16 layer slices lie together)
                per = ctx.shape[0] // (2 * B1)
                ctx = torch.cat([ctx, ctx[:B1 * per]])
            eng.set_context(ctx, B, layerwise)
            object.__setattr__(self, "_ctx_key", key if cache_ok else None)
            object.__setattr__(self, "_ctx_ref", (context, given))
        if self.regions is not None:
            self._apply_regions(eng, B)
        if self._control is not None:
            # (the context AFTER the compel-cfg weighting, and that tensor object as the key of the control branch's K / V)
            self._apply_control(eng, x, timesteps.to(x.device), context.to(x.device), context, B1, layerwise, bool(cfg_twin), deep_cache)
        tg = {} if tgate is None else {"tgate": tgate}
        if deep_cache is None:
            fwd = eng.unet_forward_pag if cfg_pag else eng.unet_forward_twin if cfg_twin else eng.unet_forward
            out = fwd(x, timesteps.to(x.device), **tg)
        else:
            mode, depth = deep_cache
            out = eng.unet_forward_cached(x, timesteps.to(x.device), depth=int(depth), mode=mode,
                                          twin="pag" if cfg_pag else bool(cfg_twin), **tg)
        if extra_info is not None:
            # the reference writes the (here empty) distillation capture into the caller's dict (:1031-1035)
            extra_info["ca_layers_activations"] = {k: {} for k in ("outfeat", "attn", "attnscore", "q")}
        return out.type(x.dtype) if x.dtype != torch.float32 else out
