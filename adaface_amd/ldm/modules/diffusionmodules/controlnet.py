"""ControlNet (Zhang, Rao, Agrawala, ICCV 2023) for the SD-v1 U-Net: cldm/cldm.py's `ControlNet` with the same constructor
arguments and the same state_dict keys (`control_model.<k>` in a checkpoint), its forward one af_control_forward call into the
HIP path.  Not in the AdaFace reference; opt-in through UNetModel.set_control.

    h = x;  emb = time_embed(timestep_embedding(t));  g = input_hint_block(hint)
    for i, block in enumerate(input_blocks):  h = block(h, emb, ctx);  if i == 0: h = h + g;  r[i] = zero_convs[i](h)
    r[n_in] = middle_block_out(middle_block(h, emb, ctx))
"""
from __future__ import annotations

import torch

from adaface_amd import layout
from adaface_amd.ldm._hipmodule import HipModule, build_param_tree

SD15_CONTROLNET = dict(image_size=32, in_channels=4, model_channels=320, hint_channels=3, num_res_blocks=2,
                       attention_resolutions=(4, 2, 1), channel_mult=(1, 2, 4, 4), num_heads=8, context_dim=768,
                       transformer_depth=1, use_spatial_transformer=True, legacy=False)


def strip_control_prefix(raw: dict, prefix: str = "control_model.") -> dict:
    """The ControlNet's own tensors of a checkpoint dict: keys behind `control_model.` when any key carries that prefix
    (everything else in such a file belongs to the other networks of a cldm checkpoint), else the dict as it is."""
    if any(k.startswith(prefix) for k in raw):
        return {k[len(prefix):]: v for k, v in raw.items() if k.startswith(prefix)}
    return dict(raw)


class ControlNet(HipModule):
    _ckpt_prefix = "control_model."

    def __init__(self, image_size, in_channels, model_channels, hint_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, use_checkpoint=False, use_fp16=False, num_heads=-1,
                 num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False, use_spatial_transformer=False, transformer_depth=1, context_dim=None,
                 n_embed=None, legacy=True, disable_self_attentions=None, num_attention_blocks=None,
                 disable_middle_self_attn=False, use_linear_in_transformer=False):
        super().__init__()
        unsupported = {
            "dims != 2": dims != 2, "use_scale_shift_norm": use_scale_shift_norm, "resblock_updown": resblock_updown,
            "n_embed": n_embed is not None, "dropout": dropout != 0, "not conv_resample": not conv_resample,
            "not use_spatial_transformer": not use_spatial_transformer, "num_head_channels": num_head_channels != -1,
            "num_heads_upsample": num_heads_upsample not in (-1, num_heads),
            "disable_self_attentions": disable_self_attentions is not None, "num_attention_blocks": num_attention_blocks is not None,
            "disable_middle_self_attn": bool(disable_middle_self_attn), "use_linear_in_transformer": bool(use_linear_in_transformer),
        }
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"ControlNet: options outside the SD-v1 denoising path: {bad}")
        if context_dim is None or num_heads == -1:
            raise ValueError("ControlNet: context_dim and num_heads are required (spatial transformer)")
        if hasattr(context_dim, "__len__"):
            context_dim = list(context_dim)
            if len(context_dim) != 1:
                raise NotImplementedError("a single context_dim is supported")
            context_dim = context_dim[0]
        self.image_size = image_size
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.hint_channels = hint_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = tuple(attention_resolutions)
        self.channel_mult = tuple(channel_mult)
        self.num_heads = num_heads
        self.context_dim = int(context_dim)
        self.transformer_depth = transformer_depth
        self.use_checkpoint = use_checkpoint
        self.dtype = torch.float32
        if use_fp16:
            self.compute_dtype = "bf16"
        shapes = layout.controlnet_param_shapes(**self._layout_kwargs())
        build_param_tree(self, shapes, zero_init=layout.controlnet_zero_init_names(shapes))
        object.__setattr__(self, "_ctx_key", None)
        object.__setattr__(self, "_hint_key", None)

    def _layout_kwargs(self):
        return dict(in_channels=self.in_channels, model_channels=self.model_channels, hint_channels=self.hint_channels,
                    num_res_blocks=self.num_res_blocks, attention_resolutions=self.attention_resolutions,
                    channel_mult=self.channel_mult, context_dim=self.context_dim, transformer_depth=self.transformer_depth)

    def _engine_kwargs(self):
        kw = self._layout_kwargs()
        kw.update(num_heads=self.num_heads, n_context_layers=16, out_channels=self.in_channels)
        return {"controlnet": kw}

    def _mark_dirty(self):
        super()._mark_dirty()
        object.__setattr__(self, "_ctx_key", None)    # cached K/V and the hint feature depend on the weights
        object.__setattr__(self, "_hint_key", None)

    def set_compute_dtype(self, dtype: str):
        if dtype == "fp8":
            raise ValueError("ControlNet: the fp8 mode is not built for the control branch (run it in 'bf16' beside an fp8 U-Net)")
        return super().set_compute_dtype(dtype)

    def set_lora(self, adapters):
        if adapters:
            raise NotImplementedError("ControlNet: LoRA adapters are not applied to the control branch")
        return super().set_lora(adapters)

    def engine(self, device):
        before = self._engine
        eng = super().engine(device)
        if eng is not before:
            object.__setattr__(self, "_ctx_key", None)
            object.__setattr__(self, "_hint_key", None)
        return eng

    @classmethod
    def from_file(cls, path, **ctor):
        """A ControlNet from `control_sd15_*.pth` / `control_v11p_sd15_*.pth|.safetensors` / `.ckpt`: keys with or without the
        `control_model.` prefix.  ctor: constructor arguments that differ from SD-1.5's (SD15_CONTROLNET)."""
        from adaface_amd.lora import load_lora_file
        net = cls(**{**SD15_CONTROLNET, **ctor})
        net.load_control_state_dict(load_lora_file(path), what=str(path))
        return net

    def load_control_state_dict(self, raw: dict, what: str = "state dict"):
        sd = strip_control_prefix(raw)
        own = self.state_dict()
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError(f"{what}: {len(missing)} ControlNet tensors missing, e.g. {missing[:3]}")
        for k, v in own.items():
            if tuple(sd[k].shape) != tuple(v.shape):
                raise ValueError(f"{what}: '{k}' has shape {tuple(sd[k].shape)}, this ControlNet expects {tuple(v.shape)}")
        self.load_state_dict({k: sd[k].float() for k in own}, strict=True)
        return self

    # ---- the pieces UNetModel.forward drives ------------------------------------------------------------------------------
    def _set_hint(self, eng, hint):
        key = (id(hint), getattr(hint, "_version", 0), tuple(hint.shape))
        if key != self._hint_key:
            eng.control_set_hint(hint.to(eng.device, torch.float32))
            object.__setattr__(self, "_hint_key", key)
            object.__setattr__(self, "_hint_ref", hint)

    def _set_context(self, eng, ctx, given, B, layerwise):
        key = (id(given), getattr(given, "_version", 0), tuple(ctx.shape), layerwise, B)
        if key != self._ctx_key:
            eng.set_context(ctx, B, layerwise)
            object.__setattr__(self, "_ctx_key", key)
            object.__setattr__(self, "_ctx_ref", given)

    @torch.no_grad()
    def forward(self, x, hint, timesteps, context, n_blocks=None, layerwise=None, **kwargs):
        """cldm's ControlNet.forward(x, hint, timesteps, context): the list of residuals, fp32 NCHW.  context [B*16, T, D]
        (layerwise: slices 0 .. 6 are read) or [B, T, D]."""
        eng = self.engine(x.device)
        B, _, H, W = x.shape
        if layerwise is None:
            layerwise = context.shape[0] == 16 * B
        if hint.shape[0] not in (1, B) or tuple(hint.shape[2:]) != (8 * H, 8 * W):
            raise ValueError(f"ControlNet: hint {tuple(hint.shape)} for a latent batch {tuple(x.shape)} (batch 1 or {B}, sides 8x)")
        self._set_hint(eng, hint)
        self._set_context(eng, context.to(x.device), context, B, bool(layerwise))
        flat = eng.control_forward(x, timesteps.to(x.device), n_blocks)
        return [r.permute(0, 3, 1, 2).float() for r in eng.control_residuals(flat, B, H, W, n_blocks)]
