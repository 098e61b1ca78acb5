"""Base class of the HIP-backed drop-in modules.

A reference module (UNetModel, AutoencoderKL) is an nn.Module whose state_dict keys are
the weights contract.  The drop-in keeps that contract — parameters are
registered under exactly the reference's dotted names, so load_state_dict / .to / .eval /
state_dict work unchanged — while the arithmetic lives in an adaface_amd.engine.Engine
(repacked weights in HBM + HIP kernels).  The Engine is created on first use on a HIP
device and re-fed whenever the parameters may have changed.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Tuple

import torch
import torch.nn as nn


class _Node(nn.Module):
    """Bare container so that dotted reference names map onto nested attributes."""


def build_param_tree(root: nn.Module, shapes: Dict[str, Tuple[int, ...]], zero_init: Iterable[str] = ()) -> None:
    zero = set(zero_init)
    g = torch.Generator().manual_seed(0)
    for name, shape in shapes.items():
        parts = name.split(".")
        node = root
        for p in parts[:-1]:
            if p not in node._modules:
                node.add_module(p, _Node())
            node = node._modules[p]
        if name in zero:
            t = torch.zeros(shape)
        elif len(shape) == 1:
            t = torch.ones(shape) if parts[-1] == "weight" else torch.zeros(shape)
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            bound = 1.0 / math.sqrt(fan_in)
            t = (torch.rand(shape, generator=g) * 2 - 1) * bound
        node.register_parameter(parts[-1], nn.Parameter(t, requires_grad=False))


class HipModule(nn.Module):
    """nn.Module facade over an Engine.  Subclasses set `_engine_kwargs()` and `_ckpt_prefix`."""

    _ckpt_prefix = ""          # prefix the C library expects in front of this module's keys
    compute_dtype = "bf16"     # "bf16" (throughput), "f32" (parity mode), "f16" (the reference's autocast precision) or "fp8" (bf16 + e4m3 ResBlock convolutions)

    def __init__(self):
        super().__init__()
        object.__setattr__(self, "_engine", None)
        object.__setattr__(self, "_weights_dirty", True)
        # calibrated fp8 activation shifts {site name: shift} (None: the fixed 2^3).  They live here, not on the engine: the
        # engine is rebuilt when the compute dtype or the device changes, and every fp8 engine gets them again
        object.__setattr__(self, "_fp8_shifts", None)
        object.__setattr__(self, "_fp8_scope", ("base",))     # kept here like the shifts: every fp8 engine gets it again
        object.__setattr__(self, "_tome", (0.0, 1))           # token merging (UNetModel.set_token_merging), kept the same way
        object.__setattr__(self, "_freeu", (0, 1.0, 1.0, 1.0, 1.0))   # FreeU (UNetModel.set_freeu), kept the same way
        object.__setattr__(self, "_pag", ())                          # PAG sites (UNetModel.set_pag), kept the same way
        object.__setattr__(self, "_sag", False)                       # SAG capture (UNetModel.set_sag), kept the same way
        object.__setattr__(self, "_lora", [])                       # LoRA adapters [(weights, scale)] (set_lora), kept the same way
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._after_load_state_dict())

    # ---- weight synchronisation -----------------------------------------------------------
    def _mark_dirty(self):
        object.__setattr__(self, "_weights_dirty", True)

    def _after_load_state_dict(self):
        self._mark_dirty()
        self.set_fp8_shifts(None)      # a calibration belongs to the checkpoint it was made with

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._mark_dirty()
        return out

    def set_compute_dtype(self, dtype: str):
        """'bf16', 'f32', 'f16' (alias 'fp16': fp16 storage on the f16 MFMA, fp32 accumulation) or 'fp8' (bf16 storage with the
        UNet's ResBlock 3x3 convolutions on the block-scaled fp8 MFMA; modules without such layers run it as bf16); takes effect
        at the next forward (the engine is rebuilt)."""
        if dtype == "fp16":
            dtype = "f16"
        if dtype not in ("bf16", "f32", "f16", "fp8"):
            raise ValueError(dtype)
        if dtype in ("f16", "fp8") and self._tome[0] > 0.0:
            raise ValueError(f"compute dtype {dtype!r} does not combine with token merging (set_token_merging(0) first)")
        if dtype == "fp8" and self._sag:
            raise ValueError("compute dtype 'fp8' does not combine with self-attention guidance (set_sag(False) first)")
        if dtype != self.compute_dtype:
            self.compute_dtype = dtype
            if self._engine is not None:
                self._engine.close()
            object.__setattr__(self, "_engine", None)
            self._mark_dirty()
        return self

    @property
    def fp8_scope(self) -> tuple:
        return self._fp8_scope

    def set_fp8_scope(self, scope):
        """("base",) | ("base", "ff") | "base+ff": which layers the fp8 mode covers (adaface_hip.h, AF_FP8_SCOPE_*).  Kept for
        every later fp8 engine; a live one is switched now.  Calibrated shifts name the sites of the scope they were made
        under, so a scope change drops them (calibrate or load_fp8_scales again)."""
        from adaface_amd.fp8_calib import fp8_scope_names, parse_fp8_scope
        names = fp8_scope_names(parse_fp8_scope(scope))
        if names != self._fp8_scope:
            object.__setattr__(self, "_fp8_scope", names)
            object.__setattr__(self, "_fp8_shifts", None)
            if self._engine is not None and self.compute_dtype == "fp8":
                self._engine.set_fp8_shifts(None)
                self._engine.set_fp8(True, scope=names)
        return self

    def _engine_kwargs(self) -> dict:  # pragma: no cover - abstract
        raise NotImplementedError

    def engine(self, device: torch.device):
        """The Engine on `device`, with current weights uploaded.  Raises if no HIP device."""
        from adaface_amd.engine import Engine
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}: inputs must be on a HIP device (got {device}); "
                               "adaface_amd has no CPU path")
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._engine is None or self._engine.device.index != idx:
            if self._engine is not None:
                self._engine.close()
            fp8 = self.compute_dtype == "fp8"
            object.__setattr__(self, "_engine", Engine(dtype="bf16" if fp8 else self.compute_dtype, device=idx,
                                                       **self._engine_kwargs()))
            try:
                if fp8:
                    self._engine.set_fp8(True, scope=self._fp8_scope)
                    if self._fp8_shifts is not None:
                        try:
                            self._engine.set_fp8_shifts(self._fp8_shifts)
                        except KeyError as e:
                            raise KeyError(f"{type(self).__name__}: the shifts given to set_fp8_shifts / load_fp8_scales do not "
                                           f"name this model's fp8 sites ({e.args[0]})") from None
                if self._tome[0] > 0.0:
                    self._engine.set_tome(*self._tome)
                if self._freeu[0]:
                    self._engine.set_freeu(*self._freeu)
                if self._pag:
                    self._engine.set_pag(self._pag)
                if self._sag:
                    self._engine.set_sag(True)
            except Exception:
                # (an engine whose configuration failed is not kept: the next call builds and configures again)
                self._engine.close()
                object.__setattr__(self, "_engine", None)
                raise
            self._mark_dirty()
        if self._weights_dirty:
            self.sync_weights()
        return self._engine

    # ---- fp8 mode: calibrated activation scales --------------------------------------------
    def _fp8_engine(self, device):
        if self.compute_dtype != "fp8":
            raise RuntimeError(f"{type(self).__name__}: set_compute_dtype('fp8') first (compute dtype is {self.compute_dtype})")
        return self.engine(torch.device(device))

    def fp8_shifts(self):
        """The calibrated shifts {site name: shift}, or None while the fp8 mode runs on the fixed 2^3."""
        return None if self._fp8_shifts is None else dict(self._fp8_shifts)

    def set_fp8_shifts(self, shifts):
        """Keep `shifts` ({site name: shift} for every fp8 site; None = back to 2^3) and apply them to the live engine.  A
        load_state_dict clears them: a calibration belongs to a checkpoint, so load scales after weights.
        Every value must be an integer in [-16, 8] (checked here).  The site NAMES are only known to an engine: with a
        live fp8 engine they are checked here too, otherwise when the next fp8 engine is built (engine() then raises a
        KeyError that names this call)."""
        if shifts is not None:
            from adaface_amd.fp8_calib import check_shifts
            shifts = check_shifts(shifts, list(shifts))          # (values; the names against themselves)
        eng = self._engine if self.compute_dtype == "fp8" else None
        if eng is not None:
            eng.set_fp8_shifts(shifts)          # (validates the names against the engine's sites)
        object.__setattr__(self, "_fp8_shifts", shifts)
        return self

    def calibrate_fp8(self, run, device, passes: int = 2, headroom: int = 1):
        """Engine.calibrate_fp8 on this module's fp8 engine; the shifts are kept for every later engine.  `run` drives the
        module (forwards or a sampler run).  Returns {site name: (amax, shift, nsat of the last pass)}."""
        eng = self._fp8_engine(device)
        out = eng.calibrate_fp8(run, passes=passes, headroom=headroom)
        if self._engine is not eng:
            raise RuntimeError("calibrate_fp8: `run` rebuilt the engine (compute dtype or device changed during calibration)")
        object.__setattr__(self, "_fp8_shifts", eng.fp8_shifts())
        return out

    def save_fp8_scales(self, path):
        """Write the calibrated shifts as JSON keyed by site name (adaface_amd.fp8_calib.save_scales)."""
        from adaface_amd.fp8_calib import save_scales
        if self._fp8_shifts is None:
            raise RuntimeError("save_fp8_scales: nothing calibrated or loaded")
        save_scales(path, self._fp8_shifts)

    def load_fp8_scales(self, path, device):
        """Read a scale file; a file whose site names are not exactly this model's fp8 sites is refused."""
        from adaface_amd.fp8_calib import load_scales
        eng = self._fp8_engine(device)
        return self.set_fp8_shifts(load_scales(path, eng.fp8_site_names()))

    def sync_weights(self):
        """Upload (repack) every parameter into the engine; the targets of set_lora go through the fused merge."""
        eng = self._engine
        if eng is None:
            return
        table = eng.tensor_table()
        sd = self.state_dict()
        targets = set(self.lora_targets())
        for name in table:
            key = name[len(self._ckpt_prefix):] if name.startswith(self._ckpt_prefix) else name
            if key not in sd:
                raise KeyError(f"engine expects tensor '{name}' but the module has no parameter '{key}'")
            if key.endswith(".weight") and key[:-len(".weight")] in targets:
                eng.load_tensor_lora(name, sd[key], self._lora_of(key[:-len(".weight")]))
            else:
                eng.load_tensor(name, sd[key])
        object.__setattr__(self, "_weights_dirty", False)

    # ---- LoRA adapters: an overlay on the engine's weights, never on the parameters --------------
    def lora_targets(self) -> list:
        """The sorted parameter names (without ".weight") the current adapter set touches."""
        return sorted({name for weights, _ in self._lora for name in weights})

    def _lora_of(self, pname: str) -> list:
        """[(up, down, s)] of the adapters that touch `pname`, in list order, s = scale * alpha / r formed in double."""
        from adaface_amd.lora import lora_factor
        return [(w[pname][0], w[pname][1], lora_factor(scale, w[pname][2], w[pname][1].shape[0]))
                for w, scale in self._lora if pname in w]

    def _lora_changed(self):
        """Hook: state outside the engine that depends on the weights (UNetModel: the hoisted context K / V)."""

    def set_lora(self, adapters):
        """LoRA adapters on top of this module's weights: `adapters` is a list of (weights, scale), at most 8, with weights =
        {parameter name without ".weight": (up, down, alpha)} in this module's own names (adaface_amd.lora.split_lora makes
        them from a file).  The engine's copy of each touched weight becomes W + sum_a scale_a * alpha_a / r_a * up_a @ down_a,
        formed in fp32 by the repack kernel and rounded once; the module's parameters and state_dict() never change, so
        set_lora([]) / clear_lora() give the base model back exactly.  Names and shapes are checked first (KeyError /
        ValueError naming the key).  On a live engine only the weights in the union of the previous and the new target set are
        loaded again (those that dropped out, plainly); everything the engine derives from weights is refreshed before the next
        forward.  The list is kept for every later engine (device or compute-dtype change).  A change of the adapter set drops
        calibrated fp8 shifts, as a checkpoint load does: calibrate or load_fp8_scales after set_lora."""
        import math
        from adaface_amd.lora import check_adapter_list, check_lora_pair
        adapters = check_adapter_list(adapters)
        params = dict(self.named_parameters())
        for i, (weights, _scale) in enumerate(adapters):
            for pname, entry in weights.items():
                p = params.get(f"{pname}.weight") if isinstance(pname, str) else None
                if p is None or p.dim() < 2:
                    raise KeyError(f"{type(self).__name__}.set_lora: adapter {i} names {pname!r}, which is no conv / linear weight "
                                   "of this module")
                if not isinstance(entry, (tuple, list)) or len(entry) != 3:
                    raise ValueError(f"{type(self).__name__}.set_lora: adapter {i}, {pname!r}: expected (up, down, alpha)")
                up, down, alpha = entry
                check_lora_pair(f"adapter {i}, {pname!r}", tuple(p.shape), tuple(up.shape), tuple(down.shape))
                if not math.isfinite(float(alpha)):
                    raise ValueError(f"{type(self).__name__}.set_lora: adapter {i}, {pname!r}: alpha {alpha!r} is not finite")
        old = set(self.lora_targets())
        if not old and not any(w for w, _ in adapters):
            object.__setattr__(self, "_lora", adapters)
            return self
        object.__setattr__(self, "_lora", adapters)
        touched = sorted(old | set(self.lora_targets()))
        self.set_fp8_shifts(None)
        self._lora_changed()
        eng = self._engine
        if eng is not None and not self._weights_dirty:
            table = eng.tensor_table()
            for pname in touched:
                key = f"{pname}.weight"
                name = self._ckpt_prefix + key if self._ckpt_prefix + key in table else key
                eng.load_tensor_lora(name, params[key], self._lora_of(pname))
        return self

    def clear_lora(self):
        """set_lora([]): back to the base weights."""
        return self.set_lora([])
