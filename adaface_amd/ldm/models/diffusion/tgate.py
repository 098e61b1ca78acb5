"""T-GATE (Zhang et al., "Cross-Attention Makes Inference Cumbersome in Text-to-Image Diffusion Models", 2024) for this
package's samplers: up to the gate step the run is what it is without it; the last step before the gate also keeps every
cross-attention output, averaged over the guidance legs (af_tgate_set, include/adaface_hip.h); from the gate step on the
U-Net runs on one leg with those outputs in place of cross-attention, and guidance is no longer applied.  Not part of the
reference; opt-in.

This file is the schedule and the per-run bookkeeping, both host-only; the capture and replay calls themselves are made
where every step's model call is (model_calls.py).
"""
from __future__ import annotations

from typing import List, Optional


def tgate_phases(n: int, g) -> List[Optional[str]]:
    """The phase of every loop index 0 .. n-1 of a run gated at step g: None for i < g - 1, "capture" for i = g - 1,
    "replay" for i >= g.  g None or 0 = off (all None); otherwise an int with 1 <= g <= n - 1 (ValueError for anything
    else, a bool or a float included)."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"tgate_phases: {n!r} steps")
    if g is None:
        return [None] * n
    if isinstance(g, bool) or not isinstance(g, int):
        raise ValueError(f"tgate_step: {g!r} (None or 0 = off, or an integer 1 .. steps - 1)")
    if g == 0:
        return [None] * n
    if g < 1 or g > n - 1:
        raise ValueError(f"tgate_step: {g} outside 1 .. {n - 1} (a run of {n} steps; None or 0 = off)")
    return [None] * (g - 1) + ["capture"] + ["replay"] * (n - g)


def refuse_guided(tgate_step, pag_scale=0., guidance_rescale=0.):
    """A gated run ends on one leg without a guidance combine: perturbed-attention guidance and the guidance rescale have
    nothing to act on there."""
    if tgate_step in (None, 0) or isinstance(tgate_step, bool):
        return
    if pag_scale or guidance_rescale:
        raise NotImplementedError("tgate_step with pag_scale / guidance_rescale: after the gate the U-Net runs on one leg and no "
                                  "guidance combine is made, so neither has a prediction to act on")


class TGateRun:
    """One sampling run's bookkeeping.  step(i) returns the `tgate=` argument of that step's model call (None, "capture" or
    "replay") and logs it.  form(i, base) is the call form handed to DeepCacheRun.step: with the gate on it carries the phase
    as a fifth element, which forces a DeepCache refresh at the capture step and at the first replay step."""

    def __init__(self, model, total_steps: int, gate_step):
        self.phases = tgate_phases(int(total_steps), gate_step)
        self.active = any(p is not None for p in self.phases)
        if self.active and not getattr(model, "supports_tgate", False):
            raise NotImplementedError("tgate_step: the model has no T-GATE entry point (apply_model(..., tgate=))")
        self.log: List[Optional[str]] = []

    def step(self, i: int) -> Optional[str]:
        ph = self.phases[i] if self.active else None
        self.log.append(ph)
        return ph

    def form(self, base: tuple, phase) -> tuple:
        return tuple(base) + ((phase,) if self.active else ())
