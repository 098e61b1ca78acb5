"""LoRA adapter files: reading, key-name mapping and the host-side checks (no GPU is needed for anything here).

An adapter file holds, per adapted conv / linear layer, `lora_up.weight` [out, r(, 1, 1)], `lora_down.weight` [r, in(, k, k)] and
optionally `alpha` (missing: r); the layer's weight becomes W + scale * alpha / r * up @ down.  Two naming schemes are understood:

  (a) kohya:  lora_unet_<diffusers module path with "_"> / lora_te_<transformers module path with "_">, mapped onto this
      package's (the reference's ldm) parameter names from channel_mult, num_res_blocks and attention_resolutions;
  (b) native: <ldm parameter name without ".weight">, optionally behind "model.diffusion_model." or "cond_stage_model.".

split_lora returns what HipModule.set_lora takes: {parameter name without ".weight": (up, down, alpha)} per module.
DoRA, LoHa, LoKr and Tucker (lora_mid) adapters are refused by name.
"""
from __future__ import annotations

import re
from typing import Dict, List, Tuple

import torch

from . import layout
from ._lib import LORA_MAX_ADAPTERS, LORA_MAX_RANK

UNET_PREFIX = "model.diffusion_model."
TEXT_PREFIX = "cond_stage_model."
_SUFFIXES = ("lora_up.weight", "lora_down.weight", "alpha")
# keys of the adapter kinds that are not plain LoRA: (substring, kind)
_OTHER_KINDS = (("dora_scale", "DoRA"), ("hada_", "LoHa"), ("lokr_", "LoKr"), ("lora_mid", "Tucker (lora_mid)"))


# ---------------------------------------------------------------------------------------------- shapes
def check_lora_pair(what: str, base_shape: Tuple[int, ...], up_shape: Tuple[int, ...], down_shape: Tuple[int, ...]) -> int:
    """The rank of an (up, down) pair that fits a weight of `base_shape` [rows, cin(, ks, ks)]: up [rows, r] with trailing ones,
    down [r, cin(, ks, ks)] (or flattened [r, cin * ks * ks] for a conv), 1 <= r <= 256.  ValueError naming `what` otherwise."""
    rows, per_row = int(base_shape[0]), 1
    for d in base_shape[1:]:
        per_row *= int(d)
    r = int(down_shape[0]) if len(down_shape) >= 1 else 0
    n_up, n_down = 1, 1
    for d in up_shape:
        n_up *= int(d)
    for d in down_shape:
        n_down *= int(d)
    ok = (len(base_shape) >= 2 and len(up_shape) >= 2 and len(down_shape) >= 2 and int(up_shape[0]) == rows and int(up_shape[1]) == r
          and n_up == rows * r and n_down == r * per_row
          and (int(down_shape[1]) == int(base_shape[1]) or (len(down_shape) == 2 and int(down_shape[1]) == per_row)))
    if not ok:
        raise ValueError(f"LoRA {what}: lora_up {tuple(up_shape)} / lora_down {tuple(down_shape)} do not fit a weight of shape "
                         f"{tuple(base_shape)} (up [{rows}, r], down [r, {', '.join(str(int(d)) for d in base_shape[1:])}])")
    if not 1 <= r <= LORA_MAX_RANK:
        raise ValueError(f"LoRA {what}: rank {r} (1 .. {LORA_MAX_RANK})")
    return r


def lora_factor(scale: float, alpha: float, r: int) -> float:
    """s = scale * alpha / r, formed in double (the library takes it as fp32)."""
    return float(scale) * float(alpha) / float(r)


def merge_host(base: torch.Tensor, adapters) -> torch.Tensor:
    """The effective weight base + sum_a s_a * up_a @ down_a on the host in float64, base's shape.  adapters: [(up, down, s)] as
    HipModule._lora_of gives them, s taken as the fp32 value the library receives.  What the repack kernel forms in fp32 on the
    device, for host-side arithmetic that needs the merged weight (the guidance-embedding fold)."""
    out = base.detach().double().cpu().reshape(base.shape[0], -1).clone()
    for up, down, s in adapters:
        r = int(down.shape[0])
        s32 = float(torch.tensor(float(s), dtype=torch.float32))
        out += s32 * (up.detach().double().cpu().reshape(base.shape[0], r) @ down.detach().double().cpu().reshape(r, -1))
    return out.reshape(base.shape)


# ---------------------------------------------------------------------------------------------- names
def _cfg_get(unet_cfg):
    return unet_cfg.get if isinstance(unet_cfg, dict) else (lambda k, d=None: getattr(unet_cfg, k, d))


def kohya_unet_map(unet_cfg) -> Dict[str, str]:
    """{diffusers module path with "_" (what follows "lora_unet_"): ldm parameter name without ".weight"} of every conv / linear
    layer of a UNetModel, from its constructor arguments (a dict or an object with in_channels, model_channels, channel_mult,
    num_res_blocks, attention_resolutions[, transformer_depth])."""
    get = _cfg_get(unet_cfg)
    n, depth = int(get("num_res_blocks")), int(get("transformer_depth", 1) or 1)
    inputs, middle, outputs = layout.unet_blocks(int(get("model_channels")), list(get("channel_mult")), n,
                                                 list(get("attention_resolutions")), int(get("in_channels")))
    out: Dict[str, str] = {"conv_in": "input_blocks.0.0", "conv_out": "out.2", "time_embedding_linear_1": "time_embed.0",
                           "time_embedding_linear_2": "time_embed.2"}

    def res(k, p, desc):
        out[k + "_conv1"], out[k + "_conv2"], out[k + "_time_emb_proj"] = p + ".in_layers.2", p + ".out_layers.3", p + ".emb_layers.1"
        if desc[1] != desc[2]:
            out[k + "_conv_shortcut"] = p + ".skip_connection"

    def xfmr(k, p):
        out[k + "_proj_in"], out[k + "_proj_out"] = p + ".proj_in", p + ".proj_out"
        for d in range(depth):
            kt, pt = f"{k}_transformer_blocks_{d}", f"{p}.transformer_blocks.{d}"
            for attn in ("attn1", "attn2"):
                for proj in ("to_q", "to_k", "to_v"):
                    out[f"{kt}_{attn}_{proj}"] = f"{pt}.{attn}.{proj}"
                out[f"{kt}_{attn}_to_out_0"] = f"{pt}.{attn}.to_out.0"
            out[kt + "_ff_net_0_proj"], out[kt + "_ff_net_2"] = pt + ".ff.net.0.proj", pt + ".ff.net.2"

    def block(kb, p, j, layers):
        for idx, desc in enumerate(layers):
            if desc[0] == "res":
                res(f"{kb}_resnets_{j}", f"{p}.{idx}", desc)
            elif desc[0] == "xfmr":
                xfmr(f"{kb}_attentions_{j}", f"{p}.{idx}")
            elif desc[0] == "down":
                out[f"{kb}_downsamplers_0_conv"] = f"{p}.{idx}.op"
            elif desc[0] == "up":
                out[f"{kb}_upsamplers_0_conv"] = f"{p}.{idx}.conv"

    for b, layers in enumerate(inputs[1:], 1):          # input block b = 1 + (n + 1) * level + j; j = n is the downsampler
        level, j = divmod(b - 1, n + 1)
        block(f"down_blocks_{level}", f"input_blocks.{b}", j, layers)
    for idx, (desc, k) in enumerate(zip(middle, ("resnets_0", "attentions_0", "resnets_1"))):
        res("mid_block_" + k, f"middle_block.{idx}", desc) if desc[0] == "res" else xfmr("mid_block_" + k, f"middle_block.{idx}")
    for b, layers in enumerate(outputs):                # output block b = (n + 1) * i + j, i = 0 the deepest level
        i, j = divmod(b, n + 1)
        block(f"up_blocks_{i}", f"output_blocks.{b}", j, layers)
    return out


_TE_RE = re.compile(r"^text_model_encoder_layers_(\d+)_(self_attn_(?:q|k|v|out)_proj|mlp_fc[12])$")


def kohya_text_name(module: str):
    """"text_model_encoder_layers_N_self_attn_q_proj" (what follows "lora_te_") -> FrozenCLIPEmbedder's parameter name without
    ".weight", or None."""
    m = _TE_RE.match(module)
    if not m:
        return None
    sub = m.group(2).replace("self_attn_", "self_attn.").replace("mlp_", "mlp.")
    return f"transformer.text_model.encoder.layers.{int(m.group(1))}.{sub}"


# ---------------------------------------------------------------------------------------------- files
def load_lora_file(path) -> Dict[str, torch.Tensor]:
    """The raw {key: tensor} of an adapter file: .safetensors, or a .pt / .ckpt holding a plain tensor dict (optionally under
    "state_dict"), read with torch.load(weights_only=True)."""
    path = str(path)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return dict(load_file(path, device="cpu"))
    raw = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(raw, dict) and isinstance(raw.get("state_dict"), dict):
        raw = raw["state_dict"]
    if not isinstance(raw, dict) or not all(isinstance(k, str) and isinstance(v, torch.Tensor) for k, v in raw.items()):
        raise ValueError(f"{path}: not a plain dict of tensors")
    return dict(raw)


def split_lora(raw: Dict[str, torch.Tensor], unet_cfg, strict: bool = False) -> dict:
    """{"unet": weights, "text": weights, "unused": [keys]} with weights = {parameter name without ".weight": (up, down, alpha)}
    in UNetModel's / FrozenCLIPEmbedder's own names.  A missing alpha is the rank.  NotImplementedError for keys of other adapter
    kinds (DoRA, LoHa, LoKr, Tucker), ValueError for a layer with only one of its two matrices; keys that map onto no layer are
    returned under "unused", or raise KeyError with the list when strict."""
    for key in raw:
        for sub, kind in _OTHER_KINDS:
            if sub in key:
                raise NotImplementedError(f"LoRA file: key {key!r} belongs to a {kind} adapter; only plain LoRA "
                                          "(lora_up / lora_down / alpha) is supported")
    groups: Dict[str, Dict[str, torch.Tensor]] = {}
    unused: List[str] = []
    for key, t in raw.items():
        for suf in _SUFFIXES:
            if key.endswith("." + suf):
                groups.setdefault(key[:-len(suf) - 1], {})[suf] = t
                break
        else:
            unused.append(key)
    kmap = kohya_unet_map(unet_cfg)
    get = _cfg_get(unet_cfg)
    shapes = layout.unet_param_shapes(**{k: get(k) for k in ("in_channels", "model_channels", "out_channels", "num_res_blocks",
                                                             "attention_resolutions", "channel_mult", "context_dim")},
                                      transformer_depth=int(get("transformer_depth", 1) or 1))
    out = {"unet": {}, "text": {}}
    for module, parts in groups.items():
        where, name = None, None
        if module.startswith("lora_unet_"):
            where, name = "unet", kmap.get(module[len("lora_unet_"):])
        elif module.startswith("lora_te_"):
            where, name = "text", kohya_text_name(module[len("lora_te_"):])
        elif module.startswith(UNET_PREFIX):
            where, name = "unet", module[len(UNET_PREFIX):]
        elif module.startswith(TEXT_PREFIX):
            where, name = "text", module[len(TEXT_PREFIX):]
        elif module.startswith("transformer.text_model."):
            where, name = "text", module
        else:
            where, name = "unet", module
        if where == "unet" and name is not None and (len(shapes.get(name + ".weight", ())) < 2):
            name = None                                  # (no such conv / linear layer in this U-Net)
        if where == "text" and name is not None and not name.startswith("transformer.text_model.encoder.layers."):
            name = None
        if name is None:
            unused.extend(f"{module}.{suf}" for suf in parts)
            continue
        if "lora_up.weight" not in parts or "lora_down.weight" not in parts:
            raise ValueError(f"LoRA file: {module!r} has {sorted(parts)} but not both lora_up.weight and lora_down.weight")
        up, down = parts["lora_up.weight"].float(), parts["lora_down.weight"].float()
        alpha = float(parts["alpha"]) if "alpha" in parts else float(down.shape[0])
        if name in out[where]:
            raise ValueError(f"LoRA file: {module!r} and another key both map onto {name!r}")
        out[where][name] = (up, down, alpha)
    if strict and unused:
        raise KeyError(f"LoRA file: {len(unused)} keys map onto no layer: {sorted(unused)}")
    out["unused"] = sorted(unused)
    return out


def parse_lora_arg(spec: str) -> Tuple[str, float]:
    """"PATH[:SCALE]" of the command line -> (path, scale); the scale is what follows the LAST colon when that is a number, so a
    path may hold colons itself.  The scale defaults to 1."""
    head, sep, tail = spec.rpartition(":")
    if sep and head:
        try:
            return head, float(tail)
        except ValueError:
            pass
    return spec, 1.0


def check_adapter_list(adapters) -> list:
    """[(weights, scale)] as set_lora takes it, at most 8 entries; ValueError otherwise."""
    adapters = list(adapters or ())
    if len(adapters) > LORA_MAX_ADAPTERS:
        raise ValueError(f"LoRA: {len(adapters)} adapters (at most {LORA_MAX_ADAPTERS})")
    out = []
    for i, item in enumerate(adapters):
        if not isinstance(item, (tuple, list)) or len(item) != 2 or not isinstance(item[0], dict):
            raise ValueError(f"LoRA: adapter {i} is not a (weights dict, scale) pair")
        scale = item[1]
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or scale != scale or scale in (float("inf"), float("-inf")):
            raise ValueError(f"LoRA: adapter {i} has scale {scale!r} (a finite number)")
        out.append((dict(item[0]), float(scale)))
    return out
