"""DeepCache (Ma, Fang, Wang, "DeepCache: Accelerating Diffusion Models for Free", CVPR 2024) for this package's samplers:
the full U-Net runs on the refresh steps only; on the steps between, its outermost `depth` input / output blocks run on the
deep feature the last refresh kept (af_unet_forward_cached, include/adaface_hip.h).  Not part of the reference; opt-in.

This file is the schedule and the per-run bookkeeping, both host-only.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

Interval = Union[None, int, Sequence[int]]


def refresh_steps(total_steps: int, interval: Interval) -> List[bool]:
    """Which loop indices 0 .. total_steps-1 run the full U-Net.  interval None or 1: all of them (the feature is off);
    an integer N >= 2: every index with i % N == 0; a sequence of loop indices: exactly those -- it must contain 0 (nothing
    is kept before the first refresh), indices past the run are ignored."""
    total_steps = int(total_steps)
    if total_steps < 0:
        raise ValueError(f"refresh_steps: {total_steps} steps")
    if interval is None:
        return [True] * total_steps
    if isinstance(interval, bool):
        raise ValueError("deep_cache_interval: an integer >= 1 or a sequence of loop indices, not a bool")
    if hasattr(interval, "__iter__"):
        idx = set()
        for v in interval:
            if int(v) != v or int(v) < 0:
                raise ValueError(f"deep_cache_interval: loop index {v!r}")
            idx.add(int(v))
        if 0 not in idx:
            raise ValueError("deep_cache_interval: an explicit list of refresh steps must contain step 0")
        return [i in idx for i in range(total_steps)]
    if int(interval) != interval or int(interval) < 1:
        raise ValueError(f"deep_cache_interval: {interval!r} (an integer >= 1, or a sequence of loop indices)")
    n = int(interval)
    return [i % n == 0 for i in range(total_steps)]


def is_off(interval: Interval) -> bool:
    """None and 1 both mean "every step through the ordinary entry points"."""
    return interval is None or (not hasattr(interval, "__iter__") and not isinstance(interval, bool) and interval == 1)


class DeepCacheRun:
    """One sampling run's bookkeeping.  step(i, form) returns the `deep_cache=` argument of that step's model call -- None
    (plain full forward), ("refresh", depth) or ("reuse", depth) -- and logs "full" / "refresh" / "reuse".  `form` is the call
    form (twin or not, batch, latent height, width): a step whose form differs from the last refresh's is forced to refresh,
    since the kept feature belongs to that exact call (annealed guidance that reaches 1 drops to the single-batch call).
    Inactive -- everything "full" -- when the interval is off or the model has no engine behind it."""

    def __init__(self, model, total_steps: int, interval: Interval, depth: int = 2):
        self.log: List[str] = []
        self.depth = int(depth)
        self.active = not is_off(interval) and bool(getattr(model, "supports_deep_cache", False))
        if not is_off(interval):
            if self.depth < 1:
                raise ValueError(f"deep_cache_depth: {depth!r} (1 .. number of input blocks - 1)")
            self.refresh = refresh_steps(total_steps, interval)     # (validated even where the model ignores it)
        self._form = None

    def step(self, i: int, form) -> Optional[tuple]:
        if not self.active:
            self.log.append("full")
            return None
        if self.refresh[i] or form != self._form:
            self._form = form
            self.log.append("refresh")
            return ("refresh", self.depth)
        self.log.append("reuse")
        return ("reuse", self.depth)
