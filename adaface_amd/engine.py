"""Engine: Python owner of one af_handle (include/adaface_hip.h).

One Engine = the HIP-side twin of one reference nn.Module (a UNetModel or an
AutoencoderKL decoder): repacked weights + activation arena living in HBM, driven on the
current torch HIP stream.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, Iterable, Optional, Sequence

import torch

from . import _lib
from ._lib import AfConfig, DTYPES, check, ptr, stream_ptr
from .lora import check_lora_pair

UNET_PREFIX = "model.diffusion_model."
VAE_PREFIX = "first_stage_model."


def check_tome_args(ratio, max_downsample=1):
    """(ratio, max_downsample) of token merging as the C library takes them; ValueError for anything it would refuse.  No GPU
    is needed."""
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 <= float(ratio) <= 0.75:
        raise ValueError(f"token merging: ratio {ratio!r} (a number in [0, 0.75]; 0 = off)")
    if isinstance(max_downsample, bool) or max_downsample not in (1, 2):
        raise ValueError(f"token merging: max_downsample {max_downsample!r} (1: the outermost level only, 2: the next one too)")
    return float(ratio), int(max_downsample)


def check_freeu_args(version, b1=1.0, b2=1.0, s1=1.0, s2=1.0):
    """(version, b1, b2, s1, s2) of FreeU as the C library takes them; ValueError for anything it would refuse.  Version 0 (off)
    takes any numbers and returns ones.  No GPU is needed."""
    if isinstance(version, bool) or version not in (0, 1, 2):
        raise ValueError(f"FreeU: version {version!r} (0 = off, 1, 2)")
    if version == 0:
        return 0, 1.0, 1.0, 1.0, 1.0
    vals = []
    for name, v, lo, hi in (("b1", b1, 1.0, 2.0), ("b2", b2, 1.0, 2.0), ("s1", s1, 0.0, 1.0), ("s2", s2, 0.0, 1.0)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= float(v) <= hi:
            raise ValueError(f"FreeU: {name} {v!r} (a number in [{lo:g}, {hi:g}])")
        vals.append(float(v))
    return (int(version), *vals)


def pag_layout(unet_cfg) -> dict:
    """The PAG sites of a UNetModel, from its constructor arguments alone (a dict or an object with channel_mult,
    num_res_blocks, attention_resolutions[, transformer_depth]): {"n_sites", "blocks" (site -> block in the forward order
    input blocks, middle block, output blocks), "ds" (site -> downsample factor of its map), "n_input_blocks", "names" (name ->
    tuple of sites)}.  A site is the
    self-attention of one transformer block in forward order; the names are diffusers': "mid", "down.blocks.L" (resolution
    level L of the encoder) and "up.blocks.K" (decoder levels, K = 0 the deepest).  No GPU is needed."""
    get = unet_cfg.get if isinstance(unet_cfg, dict) else (lambda k, d=None: getattr(unet_cfg, k, d))
    mult, nres = list(get("channel_mult")), int(get("num_res_blocks"))
    attn, depth = set(int(a) for a in get("attention_resolutions")), int(get("transformer_depth", 1) or 1)
    nlev = len(mult)
    blocks, factors, names = [], [], {}

    def add(name, block):
        names.setdefault(name, [])
        for _ in range(depth):
            names[name].append(len(blocks))
            blocks.append(block)
            factors.append(ds)
    blk, ds = 1, 1                                   # (input block 0 is conv_in)
    for lev in range(nlev):
        for _ in range(nres):
            if ds in attn:
                add(f"down.blocks.{lev}", blk)
            blk += 1
        if lev != nlev - 1:
            blk += 1                                 # (the downsample block)
            ds *= 2
    n_in = blk
    add("mid", blk)
    blk += 1
    for lev in reversed(range(nlev)):
        for i in range(nres + 1):
            if ds in attn:
                add(f"up.blocks.{nlev - 1 - lev}", blk)
            blk += 1
        if lev:
            ds //= 2
    return {"n_sites": len(blocks), "blocks": tuple(blocks), "ds": tuple(factors), "n_input_blocks": n_in, "names": {k: tuple(v) for k, v in names.items()}}


def pag_sites_of(unet_cfg, layers) -> tuple:
    """Names ("mid", "down.blocks.1", ...) and / or site numbers -> the sorted tuple of distinct sites; None or () = off.
    ValueError for an unknown name, a site out of range or anything that is neither.  No GPU is needed."""
    if layers is None:
        return ()
    if isinstance(layers, (str, int)) and not isinstance(layers, bool):
        layers = (layers,)
    lay = pag_layout(unet_cfg)
    sites = set()
    for item in layers:
        if isinstance(item, str):
            if item not in lay["names"]:
                raise ValueError(f"PAG: layer {item!r} (one of {sorted(lay['names'])}, or a site number below {lay['n_sites']})")
            sites.update(lay["names"][item])
        elif isinstance(item, int) and not isinstance(item, bool):
            if not 0 <= item < lay["n_sites"]:
                raise ValueError(f"PAG: site {item} outside 0 .. {lay['n_sites'] - 1}")
            sites.add(int(item))
        else:
            raise ValueError(f"PAG: layer {item!r} is neither a name nor a site number")
    return tuple(sorted(sites))


def pag_plan(unet_cfg, layers, depth: int = 0, share_prefix: bool = True) -> dict:
    """What af_pag_plan_query reports, from the constructor arguments alone: the first block (forward order) with a set site
    (-1: none), the input blocks a full forward runs on two legs, and those of a DeepCache reuse step of `depth`."""
    lay, sites = pag_layout(unet_cfg), pag_sites_of(unet_cfg, layers)
    first = min((lay["blocks"][s] for s in sites), default=-1)
    full = min(first, lay["n_input_blocks"]) if first >= 0 and share_prefix else 0
    return {"first_block": first, "two_leg_blocks": full, "two_leg_blocks_reuse": min(full, depth) if depth > 0 else 0}


def pag_scale_at(t, pag_scale: float, pag_adaptive_scale: float = 0.0) -> float:
    """The PAG scale of the step at timestep t, as diffusers' PAG pipelines compute it: max(s - a (1000 - t), 0)."""
    return max(float(pag_scale) - float(pag_adaptive_scale) * (1000.0 - float(t)), 0.0)


def check_control_scales(scale=1.0, scales=None, n: int = 13) -> tuple:
    """The n per-residual scales of ControlNet: `scale` on every residual, or the caller's list of exactly n finite numbers
    (cldm's guess mode is the list scale * 0.825 ** (n - 1 - i)).  ValueError for anything else.  No GPU is needed."""
    import math
    if scales is None:
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(float(scale)):
            raise ValueError(f"ControlNet: scale {scale!r} (a finite number)")
        return (float(scale),) * n
    scales = list(scales)
    if len(scales) != n:
        raise ValueError(f"ControlNet: {len(scales)} scales for {n} residuals")
    for i, v in enumerate(scales):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
            raise ValueError(f"ControlNet: scale {i} is {v!r} (a finite number)")
    return tuple(float(v) for v in scales)


def check_control_window(t_range) -> tuple:
    """(t_lo, t_hi) of the control window in DDPM timesteps; None = always (0, 999).  ValueError for anything else."""
    if t_range is None:
        return (0, 999)
    try:
        lo, hi = t_range
        lo, hi = int(lo), int(hi)
    except (TypeError, ValueError):
        raise ValueError(f"ControlNet: t_range {t_range!r} (a pair (t_lo, t_hi) of timesteps)") from None
    if lo > hi:
        raise ValueError(f"ControlNet: t_range ({lo}, {hi}) is empty")
    return (lo, hi)


def control_window_from_fractions(start: float = 0.0, end: float = 1.0) -> tuple:
    """Fractions of the schedule (0 = the first, noisiest step, 1 = the last) -> (t_lo, t_hi) = (999 (1 - end), 999 (1 - start)),
    rounded to the nearest timestep."""
    for name, v in (("start", start), ("end", end)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"ControlNet: control {name} {v!r} (a fraction in [0, 1])")
    if float(start) > float(end):
        raise ValueError(f"ControlNet: control start {start} is behind control end {end}")
    return (int(round(999 * (1.0 - float(end)))), int(round(999 * (1.0 - float(start)))))


def control_active(t, window) -> bool:
    """Is control on at this call?  Iff t_lo <= t <= t_hi for EVERY timestep of the batch."""
    ts = [int(v) for v in (t.reshape(-1).tolist() if hasattr(t, "reshape") else list(t))]
    return all(window[0] <= v <= window[1] for v in ts)


def control_plan(unet_cfg, H: int, W: int) -> list:
    """[(C, H, W, element offset for one sample)] of the 13 (SD-1.5) ControlNet residuals of an H x W latent, from the
    constructor arguments alone (af_control_plan_query).  No GPU is needed."""
    get = unet_cfg.get if isinstance(unet_cfg, dict) else (lambda k, d=None: getattr(unet_cfg, k, d))
    kw = {k: get(k) for k in ("in_channels", "model_channels", "num_res_blocks", "attention_resolutions", "channel_mult",
                              "num_heads", "context_dim")}
    return _lib.control_plan_query(kw, H, W)


def _fill(arr, values: Sequence[int]):
    if len(values) > 8:
        raise ValueError("at most 8 entries supported")
    for i, v in enumerate(values):
        arr[i] = int(v)


class Engine:
    def __init__(self, *, dtype: str = "bf16", device: int = 0, unet: Optional[dict] = None, vae: Optional[dict] = None,
                 clip: Optional[dict] = None, controlnet: Optional[dict] = None):
        """unet: UNetModel ctor kwargs (in_channels, model_channels, out_channels, num_res_blocks,
        attention_resolutions, channel_mult, num_heads, context_dim, transformer_depth);
        vae: Decoder ddconfig (ch, out_ch, ch_mult, num_res_blocks, z_channels) + embed_dim;
        controlnet: cldm ControlNet ctor kwargs (the U-Net's, plus hint_channels): a control handle, a handle of its own."""
        self._lib = _lib.load()
        self._h = C.c_void_p()
        if not torch.cuda.is_available():
            raise _lib.AfError("adaface_amd.Engine needs a HIP device (there is no CPU path)")
        cfg = AfConfig()
        cfg.dtype = DTYPES[dtype]
        self.dtype = dtype
        self.device = torch.device("cuda", device)
        if unet is not None:
            cfg.build_unet = 1
            _lib.fill_unet_config(cfg, unet)
        if vae is not None:
            cfg.build_vae = 1
            cfg.vae_ch = vae["ch"]
            cfg.vae_out_ch = vae["out_ch"]
            cfg.vae_num_res_blocks = vae["num_res_blocks"]
            cfg.vae_z_channels = vae["z_channels"]
            cfg.vae_embed_dim = vae.get("embed_dim", vae["z_channels"])
            vm = list(vae["ch_mult"])
            cfg.n_vae_ch_mult = len(vm)
            _fill(cfg.vae_ch_mult, vm)
            if vae.get("encoder", False):
                cfg.build_vae_encoder = 1
                cfg.vae_in_channels = vae.get("in_channels", 3)
        if clip is not None:   # CLIP text tower (vocab, hidden, layers, heads, intermediate, max_pos)
            cfg.build_clip = 1
            cfg.clip_vocab, cfg.clip_hidden, cfg.clip_layers = clip["vocab"], clip["hidden"], clip["layers"]
            cfg.clip_heads, cfg.clip_intermediate, cfg.clip_max_pos = clip["heads"], clip["intermediate"], clip["max_pos"]
        if controlnet is not None:
            if unet is not None or vae is not None or clip is not None:
                raise ValueError("Engine: a ControlNet is an engine of its own (controlnet= with nothing else)")
            cfg.build_controlnet = 1
            _lib.fill_unet_config(cfg, controlnet)
            cfg.hint_channels = controlnet.get("hint_channels", 3)
            unet = dict(controlnet)         # (set_context and the plan read the U-Net fields)
        self.unet_cfg, self.vae_cfg, self.clip_cfg = unet, vae, clip
        self.is_control = controlnet is not None
        self._control_ref = None            # (set_control: the residual buffer the handle points into stays alive here)
        torch.cuda.init()
        check(self._lib.af_create(device, C.byref(cfg), C.byref(self._h)), "af_create")
        self._ctx_key = None

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.af_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights --------------------------------------------------------------------------
    def tensor_table(self) -> Dict[str, tuple]:
        """name -> expected shape, as the C library derived it."""
        n = self._lib.af_num_tensors(self._h)
        out = {}
        buf = (C.c_int64 * 4)()
        for i in range(n):
            name = self._lib.af_tensor_name(self._h, i).decode()
            nd = self._lib.af_tensor_shape(self._h, i, buf)
            out[name] = tuple(int(buf[d]) for d in range(nd))
        return out

    def missing_tensors(self):
        n = self._lib.af_num_tensors(self._h)
        return [self._lib.af_tensor_name(self._h, i).decode() for i in range(n)
                if not self._lib.af_tensor_loaded(self._h, i)]

    def load_tensor(self, name: str, t: torch.Tensor):
        t = t.detach().to(torch.float32).contiguous()
        shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
        fn = self._lib.af_load_tensor_device if t.is_cuda else self._lib.af_load_tensor
        check(fn(self._h, name.encode(), C.c_void_p(t.data_ptr()), t.dim(), shape), f"af_load_tensor({name})")

    def load_tensor_lora(self, name: str, base: torch.Tensor, adapters):
        """af_load_tensor_lora: load_tensor(name, base + sum_a s_a * up_a @ down_a), merged in fp32 by the repack kernel itself and
        rounded once.  adapters: up to 8 of (up [rows, r(, 1, 1)], down [r, cin(, ks, ks)], s) -- s the whole factor
        (scale * alpha / r); the matrices are moved to the engine's device.  Conv / linear weights only.  [] is load_tensor."""
        adapters = list(adapters)
        if not adapters:
            return self.load_tensor(name, base)
        if len(adapters) > _lib.LORA_MAX_ADAPTERS:
            raise ValueError(f"load_tensor_lora({name}): {len(adapters)} adapters (at most {_lib.LORA_MAX_ADAPTERS})")
        base = base.detach().to(torch.float32).contiguous()
        rows, per_row = base.shape[0], base[0].numel() if base.dim() > 1 else 1
        ups, downs, ranks, scales = [], [], [], []
        for i, (up, down, s) in enumerate(adapters):
            check_lora_pair(f"{name} (adapter {i})", tuple(base.shape), tuple(up.shape), tuple(down.shape))
            ups.append(up.detach().to(self.device, torch.float32).contiguous())
            downs.append(down.detach().to(self.device, torch.float32).contiguous())
            ranks.append(int(down.shape[0]))
            scales.append(float(s))
        assert all(u.numel() == rows * r and d.numel() == r * per_row for u, d, r in zip(ups, downs, ranks))
        n = len(adapters)
        shape = (C.c_int64 * max(1, base.dim()))(*base.shape)
        check(self._lib.af_load_tensor_lora(self._h, name.encode(), C.c_void_p(base.data_ptr()), 1 if base.is_cuda else 0, base.dim(),
                                            shape, n, (C.c_void_p * n)(*[u.data_ptr() for u in ups]),
                                            (C.c_void_p * n)(*[d.data_ptr() for d in downs]), (C.c_int * n)(*ranks),
                                            (C.c_float * n)(*scales)), f"af_load_tensor_lora({name})")

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = "", strict: bool = True):
        """Feed every tensor the library expects from `sd` (keys = `prefix` + library name)."""
        table = self.tensor_table()
        for name in table:
            key = name if not prefix else name  # library names already carry the checkpoint prefix
            if key in sd:
                self.load_tensor(name, sd[key])
        missing = self.missing_tensors()
        if strict and missing:
            raise KeyError(f"{len(missing)} tensors missing from state_dict, e.g. {missing[:5]}")
        return missing

    # -- hot path -------------------------------------------------------------------------
    def set_context(self, ctx: torch.Tensor, Bf: int, layerwise: bool):
        """ctx: fp32 device tensor [Bf*16, T, D] (layerwise) or [Bf, T, D]."""
        if not ctx.is_cuda:
            raise ValueError("context must be a device tensor")
        ctx = ctx.contiguous().float()
        n_tokens = ctx.shape[1]
        L = self.unet_cfg.get("n_context_layers", 16) if layerwise else 1
        if ctx.shape[0] != Bf * L or ctx.shape[2] != self.unet_cfg["context_dim"]:
            raise ValueError(f"context shape {tuple(ctx.shape)} does not match batch {Bf} x layers {L}")
        check(self._lib.af_set_context(self._h, ptr(ctx), Bf, n_tokens, 1 if layerwise else 0, stream_ptr()),
              "af_set_context")

    def set_regions(self, weights: Optional[torch.Tensor]):
        """af_set_regions (regional prompts, adaface_amd/regions.py): weights [Bf, R, H, W] >= 0 at the latent resolution of the
        forwards that follow, for the context set last ([.., R T, D]: R segments of T tokens, segment 0 the base prompt); None
        switches regions off.  A later set_context of the same shape keeps them, one of another shape drops them."""
        if weights is None:
            check(self._lib.af_set_regions(self._h, None, 0, 0, 0, 0, stream_ptr()), "af_set_regions")
            return
        if weights.dim() != 4:
            raise ValueError(f"region weights of shape {tuple(weights.shape)}: expected [Bf, R, H, W]")
        if not torch.isfinite(weights).all() or bool((weights < 0).any()):
            raise ValueError("region weights must be finite and >= 0")
        w = weights.to(device=self.device, dtype=torch.float32).contiguous()
        Bf, R, H, W = w.shape
        check(self._lib.af_set_regions(self._h, ptr(w), Bf, R, H, W, stream_ptr()), "af_set_regions")

    def region_state(self) -> dict:
        """af_region_state: {"R" (0 = off), "H", "W", "fused_sites" of the last forward}."""
        out = (C.c_int * 4)()
        check(self._lib.af_region_state(self._h, out), "af_region_state")
        return {"R": out[0], "H": out[1], "W": out[2], "fused_sites": out[3]}

    def _no_regions(self, what: str):
        if self.region_state()["R"]:
            raise NotImplementedError(f"{what} is not supported while regional prompts are set (set_regions(None) switches them off)")

    def set_conv_attn(self, ks: int, batch_idx=(), token_idx=()):
        """Subject-token conv attention (attention.py:208-216), kernel size ks = 2, 3 or 4: sample `batch_idx[i]` carries a
        subject string whose first ks*ks token positions are `token_idx[i]` (a sample with several subject strings appears
        once per string).  ks <= 1 or no samples switches it off.  Invalidates the cached context."""
        n = len(batch_idx)
        bi = (C.c_int * max(n, 1))(*[int(b) for b in batch_idx])
        flat = [int(t) for row in token_idx for t in row]
        ti = (C.c_int * max(len(flat), 1))(*flat)
        if n and len(flat) != ks * ks * n:
            raise ValueError(f"set_conv_attn: {ks * ks} token positions per subject sample for a {ks}x{ks} kernel")
        if n and ks > 1:
            self._no_regions("conv attention with a subject")
        check(self._lib.af_set_conv_attn(self._h, int(ks), n, bi, ti), "af_set_conv_attn")
        self._ctx_key = None

    @contextlib.contextmanager
    def _tgate(self, tgate):
        """af_tgate_set around one forward: the mode is OFF again afterwards, also on error.  None costs nothing."""
        if tgate not in _lib.TGATE_MODES:
            raise ValueError(f"tgate {tgate!r} (None, \"capture\" or \"replay\")")
        if tgate is None:
            yield
            return
        self._no_regions("T-GATE capture / replay")
        check(self._lib.af_tgate_set(self._h, _lib.TGATE_MODES[tgate]), "af_tgate_set")
        try:
            yield
        finally:
            self._lib.af_tgate_set(self._h, 0)

    def unet_forward(self, x: torch.Tensor, t: torch.Tensor, out: Optional[torch.Tensor] = None, tgate=None) -> torch.Tensor:
        """tgate (T-GATE): "capture" = this forward, which also keeps the cross-attention outputs per site; "replay" = every
        cross-attention replaced by the kept output (no context needed); None = off."""
        x = x.contiguous().float()
        t = t.contiguous().long()
        Bf, _, H, W = x.shape
        if out is None:
            out = torch.empty(Bf, self.unet_cfg["out_channels"], H, W, device=x.device, dtype=torch.float32)
        with self._tgate(tgate):
            check(self._lib.af_unet_forward(self._h, ptr(x), ptr(t), ptr(out), Bf, H, W, stream_ptr()), "af_unet_forward")
        return out

    def unet_forward_twin(self, x: torch.Tensor, t: torch.Tensor, out: Optional[torch.Tensor] = None, tgate=None) -> torch.Tensor:
        """af_unet_forward_twin: the UNet on the CFG batch [x; x], [t; t] (context set for 2 * len(x) samples, cond first)
        without materialising the concatenation; the context-independent prefix runs once.  Returns eps [2B, C, H, W].
        tgate="capture": the kept cross-attention outputs are the means over the two legs."""
        x = x.contiguous().float()
        t = t.contiguous().long()
        B, _, H, W = x.shape
        if out is None:
            out = torch.empty(2 * B, self.unet_cfg["out_channels"], H, W, device=x.device, dtype=torch.float32)
        with self._tgate(tgate):
            check(self._lib.af_unet_forward_twin(self._h, ptr(x), ptr(t), ptr(out), 2 * B, H, W, stream_ptr()),
                  "af_unet_forward_twin")
        return out

    # -- ControlNet ---------------------------------------------------------------
    def control_plan(self, H: int, W: int) -> list:
        """[(C, H, W, element offset for one sample)] of the residuals of an H x W latent (af_control_plan_query)."""
        return control_plan(self.unet_cfg, H, W)

    def control_set_hint(self, hint: torch.Tensor):
        """af_control_set_hint (a control engine): hint fp32 [Bh, hint_channels, 8 H, 8 W], values in [0, 1], through the hint
        network once; the forwards that follow read the kept feature (Bh = 1: one hint for every sample)."""
        if not hint.is_cuda or hint.dim() != 4:
            raise ValueError("control_set_hint: the hint must be a device tensor [Bh, C, 8 H, 8 W]")
        hint = hint.contiguous().float()
        Bh, Ch, H8, W8 = hint.shape
        if Ch != self.unet_cfg.get("hint_channels", 3):
            raise ValueError(f"control_set_hint: {Ch} hint channels, the ControlNet takes {self.unet_cfg.get('hint_channels', 3)}")
        if H8 % 8 or W8 % 8:
            raise ValueError(f"control_set_hint: hint sides {H8} x {W8} must be multiples of 8")
        check(self._lib.af_control_set_hint(self._h, ptr(hint), Bh, H8, W8, stream_ptr()), "af_control_set_hint")
        self.hint_shape = (Bh, H8, W8)

    def control_forward(self, x: torch.Tensor, t: torch.Tensor, n_blocks: Optional[int] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """af_control_forward (a control engine; context set for len(x) samples, hint set): the residuals of the first n_blocks
        blocks (None: all, input blocks and middle block) as ONE flat tensor in the engine's storage dtype -- residual i of the
        batch is out[B * off_i : B * (off_i + C_i H_i W_i)] viewed [B, H_i, W_i, C_i] (control_plan; control_residuals splits)."""
        x = x.contiguous().float()
        t = t.contiguous().long()
        B, _, H, W = x.shape
        plan = self.control_plan(H, W)
        n = len(plan) if n_blocks is None else int(n_blocks)
        if not 1 <= n <= len(plan):
            raise ValueError(f"control_forward: n_blocks {n_blocks!r} outside 1 .. {len(plan)}")
        total = B * sum(c * hh * ww for c, hh, ww, _ in plan[:n])
        from .ops import STORAGE_TORCH
        dt = next(v for k, v in STORAGE_TORCH.items() if DTYPES[k] == DTYPES[self.dtype])
        if out is None:
            out = torch.empty(total, device=x.device, dtype=dt)
        elif out.dtype != dt or out.numel() < total or not out.is_contiguous():
            raise ValueError("control_forward: out must be a contiguous tensor of the storage dtype with room for the residuals")
        check(self._lib.af_control_forward(self._h, ptr(x), ptr(t), B, H, W, n, ptr(out), stream_ptr()), "af_control_forward")
        return out

    def control_residuals(self, flat: torch.Tensor, B: int, H: int, W: int, n_blocks: Optional[int] = None) -> list:
        """Views [B, H_i, W_i, C_i] (NHWC) of the residuals inside control_forward's flat result."""
        plan = self.control_plan(H, W)
        n = len(plan) if n_blocks is None else int(n_blocks)
        return [flat[B * off: B * (off + c * hh * ww)].view(B, hh, ww, c) for c, hh, ww, off in plan[:n]]

    def set_control(self, residuals: Optional[torch.Tensor], scales=None, cond_only: bool = False, source=None, shape=None):
        """af_unet_set_control (a U-Net engine): attach control_forward's flat result (its first len(scales) residuals) to the
        forwards that follow; None detaches.  shape = (B, H, W) of the x that control_forward ran on.  source: the control engine that made them -- its storage dtype and device must be
        this engine's (ValueError otherwise).  The buffer is kept alive until it is replaced or detached."""
        if residuals is None:
            check(self._lib.af_unet_set_control(self._h, None, 0, 0, 0, 0, None, 0), "af_unet_set_control")
            self._control_ref = None
            return
        self._no_regions("ControlNet")
        from .ops import STORAGE_TORCH
        if source is not None:
            if DTYPES[source.dtype] != DTYPES[self.dtype]:
                raise ValueError(f"set_control: the control engine's dtype {source.dtype!r} is not this engine's storage dtype {self.dtype!r}")
            if source.device != self.device:
                raise ValueError(f"set_control: the control engine lives on {source.device}, this engine on {self.device}")
        names = {v: k for k, v in STORAGE_TORCH.items()}
        if not residuals.is_cuda or residuals.device != self.device or not residuals.is_contiguous():
            raise ValueError(f"set_control: the residuals must be a contiguous tensor on {self.device}")
        if residuals.dtype not in names or DTYPES[names[residuals.dtype]] != DTYPES[self.dtype]:
            raise ValueError(f"set_control: residuals of {residuals.dtype}, this engine stores {self.dtype!r}")
        scales = [float(v) for v in scales]
        if shape is None:
            raise ValueError("set_control: shape=(B, H, W) of the control forward is needed")
        B, H, W = (int(v) for v in shape)
        plan = self.control_plan(H, W)
        if not 1 <= len(scales) <= len(plan):
            raise ValueError(f"set_control: {len(scales)} scales for at most {len(plan)} residuals")
        need = B * sum(c * hh * ww for c, hh, ww, _ in plan[:len(scales)])
        if residuals.numel() < need:
            raise ValueError(f"set_control: {residuals.numel()} elements, {len(scales)} residuals of {B} x {H} x {W} take {need}")
        arr = (C.c_float * len(scales))(*scales)
        check(self._lib.af_unet_set_control(self._h, ptr(residuals), B, H, W, len(scales), arr, 1 if cond_only else 0),
              "af_unet_set_control")
        self._control_ref = residuals

    def control_stats(self) -> dict:
        """af_control_stats: {"launches", "segments"} of the residual add in the last U-Net forward."""
        out = (C.c_int * 2)()
        check(self._lib.af_control_stats(self._h, out), "af_control_stats")
        return {"launches": int(out[0]), "segments": int(out[1])}

    def tgate_num_sites(self) -> int:
        """Cross-attention sites of the U-Net (forward order, the numbering of pag_sites)."""
        return int(self._lib.af_tgate_num_sites(self._h))

    def tgate_state(self) -> dict:
        """af_tgate_state: {"valid", "B", "H", "W"} of the T-GATE cache (the capture that wrote it)."""
        out = (C.c_int * 4)()
        check(self._lib.af_tgate_state(self._h, out), "af_tgate_state")
        return {"valid": bool(out[0]), "B": int(out[1]), "H": int(out[2]), "W": int(out[3])}

    def tgate_site(self, i: int) -> torch.Tensor:
        """af_tgate_read_site: the kept cross-attention output of site i as fp32 [B, N, C].  Tests and scripts."""
        st = self.tgate_state()
        if not st["valid"]:
            raise _lib.AfError("tgate_site: no valid cache (a capture forward must come first)")
        if not 0 <= int(i) < self.tgate_num_sites():
            raise ValueError(f"tgate_site: site {i} outside 0 .. {self.tgate_num_sites() - 1}")
        ds = self.pag_sites()[int(i)][2]
        mc, mult = self.unet_cfg["model_channels"], list(self.unet_cfg["channel_mult"])
        lvl = ds.bit_length() - 1
        out = torch.empty(st["B"], (st["H"] // ds) * (st["W"] // ds), mc * mult[lvl], device=self.device, dtype=torch.float32)
        check(self._lib.af_tgate_read_site(self._h, int(i), ptr(out), stream_ptr()), "af_tgate_read_site")
        return out

    def set_sag(self, on: bool = True):
        """af_sag_set (self-attention guidance): while on, every forward that runs the middle block also writes the
        attention mass per key of its attn1, for all samples of the call, into a buffer the handle owns (sag_mass reads it).
        The forward's own launches and results are unchanged.  Off: the forwards are what they are without this call."""
        if on:
            self._no_regions("self-attention guidance")
        check(self._lib.af_sag_set(self._h, 1 if on else 0), "af_sag_set")
        self.sag = bool(on)

    def sag_state(self) -> dict:
        """af_sag_state: {"on", "B", "N"}: the setting, and the batch and token count of the last capture (0, 0: none)."""
        out = (C.c_int * 3)()
        check(self._lib.af_sag_state(self._h, out), "af_sag_state")
        return {"on": bool(out[0]), "B": int(out[1]), "N": int(out[2])}

    def sag_mass(self) -> torch.Tensor:
        """af_sag_read: the attention mass of the last capture as fp32 [B, N] (B: every sample of that forward, cond first for
        the twin form; N: the middle block's tokens)."""
        st = self.sag_state()
        if not st["B"]:
            raise _lib.AfError("sag_mass: no capture (set_sag(True), then a forward that runs the middle block)")
        out = torch.empty(st["B"], st["N"], device=self.device, dtype=torch.float32)
        check(self._lib.af_sag_read(self._h, ptr(out), out.numel(), stream_ptr()), "af_sag_read")
        return out

    def set_pag(self, sites=()):
        """af_set_pag: the self-attention layers whose attention map is the identity on the third leg of unet_forward_pag --
        names ("mid", "down.blocks.2", "up.blocks.1", ...) and / or site numbers (pag_layout); None or () = off.  The plain and
        twin forwards ignore the set.  Drops a kept DeepCache feature when the set changes."""
        sites = pag_sites_of(self.unet_cfg, sites)
        arr = (C.c_int * max(len(sites), 1))(*sites)
        check(self._lib.af_set_pag(self._h, arr, len(sites)), "af_set_pag")
        self.pag = sites

    def pag_sites(self) -> list:
        """[(block in forward order, depth index, downsample factor, set)] of every PAG site, as the handle reports them."""
        out = (C.c_int * 4)()
        sites = []
        for i in range(int(self._lib.af_pag_num_sites(self._h))):
            check(self._lib.af_pag_site(self._h, i, out), "af_pag_site")
            sites.append((int(out[0]), int(out[1]), int(out[2]), bool(out[3])))
        return sites

    def pag_plan(self, depth: int = 0) -> dict:
        """af_pag_plan_query: first block with a set site, input blocks on two legs in a full forward / in a reuse step."""
        out = (C.c_int * 3)()
        check(self._lib.af_pag_plan_query(self._h, int(depth), out), "af_pag_plan_query")
        return {"first_block": int(out[0]), "two_leg_blocks": int(out[1]), "two_leg_blocks_reuse": int(out[2])}

    def unet_forward_pag(self, x: torch.Tensor, t: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """af_unet_forward_pag: the UNet on [x; x; x], [t; t; t] with legs (cond, uncond, perturbed); the context was set for
        3 * len(x) samples as [c; uc; c].  Leg 2 is leg 0 except that its self-attention at the set sites is the identity map.
        Returns eps [3B, C, H, W]."""
        self._no_regions("the PAG forward")
        x = x.contiguous().float()
        t = t.contiguous().long()
        B, _, H, W = x.shape
        if out is None:
            out = torch.empty(3 * B, self.unet_cfg["out_channels"], H, W, device=x.device, dtype=torch.float32)
        check(self._lib.af_unet_forward_pag(self._h, ptr(x), ptr(t), ptr(out), 3 * B, H, W, stream_ptr()), "af_unet_forward_pag")
        return out

    def unet_forward_cached(self, x: torch.Tensor, t: torch.Tensor, *, depth: int, mode: str, twin=False,
                            out: Optional[torch.Tensor] = None, tgate=None) -> torch.Tensor:
        """af_unet_forward_cached (DeepCache).  mode "refresh": unet_forward / unet_forward_twin bit for bit, which also keeps
        the output of output_blocks[n_out - depth - 1] in a buffer the handle owns.  mode "reuse": only input_blocks[:depth]
        and output_blocks[n_out - depth:] run, on that kept feature; AfError when no refresh with the same batch, latent size,
        twin and depth came before.  twin: x, t hold B samples and eps 2 B, as unet_forward_twin; twin="pag": eps 3 B, as
        unet_forward_pag (the form is part of the kept feature's key).  set_context / set_conv_attn
        do not drop the kept feature: call unet_cache_invalidate when the conditioning changes.  tgate: as unet_forward
        ("capture" with a refresh only; "replay" on the plain form); the mode is part of the kept feature's key."""
        if mode not in _lib.DEEPCACHE_MODES:
            raise ValueError(f"unet_forward_cached: mode {mode!r} (\"refresh\" or \"reuse\")")
        x = x.contiguous().float()
        t = t.contiguous().long()
        B, _, H, W = x.shape
        if twin not in _lib.UNET_FORMS:
            raise ValueError(f"unet_forward_cached: twin {twin!r} (False, True or \"pag\")")
        form = _lib.UNET_FORMS[twin]
        Bf = _lib.UNET_FORM_LEGS[form] * B
        if out is None:
            out = torch.empty(Bf, self.unet_cfg["out_channels"], H, W, device=x.device, dtype=torch.float32)
        with self._tgate(tgate):
            check(self._lib.af_unet_forward_cached(self._h, ptr(x), ptr(t), ptr(out), Bf, H, W, form, int(depth),
                                                   _lib.DEEPCACHE_MODES[mode], stream_ptr()), "af_unet_forward_cached")
        return out

    def set_tome(self, ratio: float, max_downsample: int = 1):
        """af_set_tome: token merging (ToMe for Stable Diffusion, tomesd's defaults without the random dst choice) in front of
        the self-attention of every transformer block whose map is the latent's divided by at most max_downsample.  ratio in
        [0, 0.75]: the share of a map's tokens that is merged away; 0 = off.  bf16 and f32 engines without the fp8 mode
        (AfError otherwise).  Drops a kept DeepCache feature when the setting changes."""
        ratio, max_downsample = check_tome_args(ratio, max_downsample)
        check(self._lib.af_set_tome(self._h, ratio, max_downsample), "af_set_tome")
        self.tome = (ratio, max_downsample)

    def tome_num_sites(self) -> int:
        """Transformer blocks that merge under the current setting (forward order)."""
        return int(self._lib.af_tome_num_sites(self._h))

    def set_freeu(self, version: int, b1: float = 1.0, b2: float = 1.0, s1: float = 1.0, s2: float = 1.0):
        """af_set_freeu: FreeU in front of every output block whose incoming backbone has 4 (b1, s1) or 2 (b2, s2) times
        model_channels channels: the first half of the backbone's channels scaled by b (version 1) or by (b - 1) * mhat + 1
        (version 2: mhat the min-max normalised channel mean), the skip's lowest frequencies scaled by s.  version 0 = off;
        b in [1, 2], s in [0, 1].  Every dtype and mode.  Drops a kept DeepCache feature when the setting changes."""
        setting = check_freeu_args(version, b1, b2, s1, s2)
        check(self._lib.af_set_freeu(self._h, *setting), "af_set_freeu")
        self.freeu = setting

    def freeu_num_sites(self) -> int:
        """Output blocks FreeU acts on (whether or not it is switched on)."""
        return int(self._lib.af_freeu_num_sites(self._h))

    def freeu_sites(self) -> list:
        """[(output block j, Ch, Cs, pair)] of the FreeU sites in forward order; pair 0: (b1, s1), 1: (b2, s2)."""
        out = (C.c_int * 4)()
        sites = []
        for i in range(self.freeu_num_sites()):
            check(self._lib.af_freeu_site(self._h, i, out), "af_freeu_site")
            sites.append(tuple(int(v) for v in out))
        return sites

    def unet_cache_invalidate(self):
        """Drop the feature kept by unet_forward_cached(mode="refresh"): the next reuse call raises until a refresh ran."""
        check(self._lib.af_unet_cache_invalidate(self._h), "af_unet_cache_invalidate")

    def unet_block_outputs(self, x: torch.Tensor, t: torch.Tensor, blocks=None) -> Dict[int, torch.Tensor]:
        """Outputs of U-Net blocks (forward order: input_blocks, middle_block, output_blocks) as fp32 NCHW tensors, one
        forward per requested block through the diagnostic tap (af_unet_set_tap).  Parity tests only."""
        x = x.contiguous().float()
        Bf, _, H, W = x.shape
        n = self._lib.af_unet_num_blocks(self._h)
        out = {}
        c, hh, ww = C.c_int(), C.c_int(), C.c_int()
        for b in (range(n) if blocks is None else blocks):
            check(self._lib.af_unet_block_shape(self._h, b, H, W, C.byref(c), C.byref(hh), C.byref(ww)), "af_unet_block_shape")
            buf = torch.empty(Bf, c.value, hh.value, ww.value, device=x.device, dtype=torch.float32)
            check(self._lib.af_unet_set_tap(self._h, b, ptr(buf)), "af_unet_set_tap")
            try:
                self.unet_forward(x, t)
            finally:
                self._lib.af_unet_set_tap(self._h, -1, None)
            out[b] = buf
        return out

    def vae_decode(self, z: torch.Tensor, scale_factor: float = 1.0, want_uint8: bool = False, want_float: bool = True):
        z = z.contiguous().float()
        B, _, H, W = z.shape
        f = 2 ** (len(self.vae_cfg["ch_mult"]) - 1)
        img = torch.empty(B, self.vae_cfg["out_ch"], H * f, W * f, device=z.device, dtype=torch.float32) if want_float else None
        u8 = torch.empty(B, H * f, W * f, 3, device=z.device, dtype=torch.uint8) if want_uint8 else None
        check(self._lib.af_vae_decode(self._h, ptr(z), float(scale_factor), ptr(img), ptr(u8), B, H, W, stream_ptr()),
              "af_vae_decode")
        if want_float and want_uint8:
            return img, u8
        return u8 if want_uint8 else img

    def vae_encode(self, x: torch.Tensor) -> torch.Tensor:
        """Encoder + quant_conv: x [B,3,H,W] -> posterior parameters [B, 2*embed_dim, H/f, W/f] (mean | logvar)."""
        x = x.contiguous().float()
        B, _, H, W = x.shape
        f = 2 ** (len(self.vae_cfg["ch_mult"]) - 1)
        ed = self.vae_cfg.get("embed_dim", self.vae_cfg["z_channels"])
        mom = torch.empty(B, 2 * ed, H // f, W // f, device=x.device, dtype=torch.float32)
        check(self._lib.af_vae_encode(self._h, ptr(x), ptr(mom), B, H, W, stream_ptr()), "af_vae_encode")
        return mom

    def posterior_sample(self, moments: torch.Tensor, noise: Optional[torch.Tensor], scale: float = 1.0) -> torch.Tensor:
        moments = moments.contiguous().float()
        B, C2, H, W = moments.shape
        z = torch.empty(B, C2 // 2, H, W, device=moments.device, dtype=torch.float32)
        nz = None if noise is None else noise.contiguous().float()
        check(self._lib.af_posterior_sample(ptr(moments), ptr(nz), float(scale), ptr(z), B, C2 // 2, H * W, stream_ptr()),
              "af_posterior_sample")
        return z

    # -- conditioning producer (CLIP text tower) --------------------------------------------
    def clip_embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        """token_embedding(input_ids): int64 [B, T] device tensor -> fp32 [B, T, hidden]."""
        ids = ids.contiguous().long()
        out = torch.empty(*ids.shape, self.clip_cfg["hidden"], device=ids.device, dtype=torch.float32)
        check(self._lib.af_clip_embed_tokens(self._h, ptr(ids), ids.numel(), ptr(out), stream_ptr()), "af_clip_embed_tokens")
        return out

    def clip_text_forward(self, inputs_embeds: torch.Tensor, w_prev: float = 0.5, w_last: float = 0.5) -> torch.Tensor:
        """inputs_embeds fp32 [Bn, T, hidden] (before the position embeddings) -> blended, final-LayerNormed states."""
        x = inputs_embeds.contiguous().float()
        Bn, T, D = x.shape
        if D != self.clip_cfg["hidden"]:
            raise ValueError(f"inputs_embeds width {D} != hidden {self.clip_cfg['hidden']}")
        out = torch.empty_like(x)
        check(self._lib.af_clip_text_forward(self._h, ptr(x), Bn, T, float(w_prev), float(w_last), ptr(out), stream_ptr()),
              "af_clip_text_forward")
        return out

    def clip_text_forward3(self, inputs_embeds: torch.Tensor, w_prev2: float, w_prev: float, w_last: float) -> torch.Tensor:
        """As clip_text_forward with three blended hidden states (weights are used as given: normalise them first)."""
        x = inputs_embeds.contiguous().float()
        Bn, T, D = x.shape
        if D != self.clip_cfg["hidden"]:
            raise ValueError(f"inputs_embeds width {D} != hidden {self.clip_cfg['hidden']}")
        out = torch.empty_like(x)
        check(self._lib.af_clip_text_forward3(self._h, ptr(x), Bn, T, float(w_prev2), float(w_prev), float(w_last), ptr(out),
                                              stream_ptr()), "af_clip_text_forward3")
        return out

    def set_fp8(self, on: bool = True, scope=("base",)):
        """af_set_fp8: the UNet's ResBlock 3x3 convolutions and self-attention q / k / v projections read e4m3 activations /
        weights (bf16 engines only).  Activation scales: 2^3 per site until calibrate_fp8 / set_fp8_shifts.
        scope: ("base",) or ("base", "ff") / "base+ff" -- the latter adds the transformer blocks' FeedForward (af_set_fp8_scope):
        32 more sites behind the base ones; shifts set before the scope changed keep their sites."""
        from .fp8_calib import parse_fp8_scope
        mask = parse_fp8_scope(scope)
        if on:
            check(self._lib.af_set_fp8_scope(self._h, mask), "af_set_fp8_scope")
        check(self._lib.af_set_fp8(self._h, 1 if on else 0), "af_set_fp8")
        self.fp8 = bool(on)

    @property
    def fp8_scope(self) -> tuple:
        from .fp8_calib import fp8_scope_names
        return fp8_scope_names(int(self._lib.af_get_fp8_scope(self._h)))

    # -- fp8 mode: calibrated per-site activation scales (adaface_hip.h, af_fp8_*) ----------------
    def fp8_site_names(self):
        n = self._lib.af_fp8_num_sites(self._h)
        return [self._lib.af_fp8_site_name(self._h, i).decode() for i in range(n)]

    def fp8_shifts(self) -> Dict[str, int]:
        names = self.fp8_site_names()
        buf = (C.c_int * max(len(names), 1))()
        check(self._lib.af_fp8_get_shifts(self._h, len(names), buf), "af_fp8_get_shifts")
        return {n: int(buf[i]) for i, n in enumerate(names)}

    def set_fp8_shifts(self, shifts: Optional[Dict[str, int]]):
        """{site name: shift} for every site (unknown or missing names are refused); None: every site back to 2^3."""
        if shifts is None:
            check(self._lib.af_fp8_set_shifts(self._h, 0, None), "af_fp8_set_shifts")
            return
        from .fp8_calib import check_shifts
        names = self.fp8_site_names()
        shifts = check_shifts(shifts, names)
        buf = (C.c_int * max(len(names), 1))(*[shifts[n] for n in names])
        check(self._lib.af_fp8_set_shifts(self._h, len(names), buf), "af_fp8_set_shifts")

    @contextlib.contextmanager
    def fp8_record(self):
        """Within the block every fp8-mode forward also records, per site, the largest |activation| its producer wrote and
        how many elements saturated (fp8_read_record).  Entering zeroes the table; what the forwards write is unchanged."""
        check(self._lib.af_fp8_record(self._h, 1, stream_ptr()), "af_fp8_record")
        try:
            yield self
        except BaseException:
            self._lib.af_fp8_record(self._h, 0, stream_ptr())      # (the exception under way is the one to report)
            raise
        check(self._lib.af_fp8_record(self._h, 0, stream_ptr()), "af_fp8_record")

    def fp8_read_record(self) -> Dict[str, tuple]:
        """{site name: (amax, nsat)} of the last recording (synchronises the current stream)."""
        names = self.fp8_site_names()
        amax = (C.c_float * max(len(names), 1))()
        nsat = (C.c_int64 * max(len(names), 1))()
        check(self._lib.af_fp8_read_record(self._h, len(names), amax, nsat, stream_ptr()), "af_fp8_read_record")
        return {n: (float(amax[i]), int(nsat[i])) for i, n in enumerate(names)}

    def calibrate_fp8(self, run, passes: int = 2, headroom: int = 1) -> Dict[str, tuple]:
        """Static activation scales from a calibration run.  `run` drives this engine (forwards, or a whole sampler run) in
        fp8 mode.  Per pass: record, run(), read, derive every site's shift from its recorded maximum, set the shifts.  The
        second pass runs on the first pass's scales, so a trajectory that clipping distorted in pass one is measured again.
        A site no forward reached keeps its shift.  Returns {site name: (amax, shift, nsat)} of the last pass -- nsat is what
        saturated DURING that pass (on the previous pass's scales); nothing runs after it."""
        from .fp8_calib import shift_for_amax
        if not getattr(self, "fp8", False):
            raise _lib.AfError("calibrate_fp8: switch the fp8 mode on first (set_fp8)")
        if passes < 1:
            raise ValueError("calibrate_fp8: at least one pass")
        out = {}
        for _ in range(passes):
            with self.fp8_record():
                run()
                rec = self.fp8_read_record()
            shifts = self.fp8_shifts()
            for name, (amax, _n) in rec.items():
                if amax > 0.0:
                    shifts[name] = shift_for_amax(amax, headroom)
            self.set_fp8_shifts(shifts)
            out = {name: (amax, shifts[name], nsat) for name, (amax, nsat) in rec.items()}
        return out

    def arena_bytes(self) -> int:
        return int(self._lib.af_arena_bytes(self._h))
