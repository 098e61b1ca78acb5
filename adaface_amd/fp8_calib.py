"""Static activation scales of the fp8 mode: the host side of a calibration (no GPU needed for anything in here).

An fp8 site (include/adaface_hip.h) writes its activation as e4m3 of value * 2^shift.  A calibration records the largest
|value| each site produces over a representative run and derives the shift from it; the result is a small table keyed by
site name (the checkpoint key of the consumer's weight), which travels with a checkpoint as a JSON file.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, Iterable

FP8_SHIFT_MIN, FP8_SHIFT_MAX, FP8_SHIFT_DEFAULT = -16, 8, 3
FP8_DEFAULT_HEADROOM = 1      # binades the recorded maximum may grow before anything clips
SCALES_FORMAT = "adaface_amd.fp8_scales/1"
# scope of the fp8 mode (AF_FP8_SCOPE_*, adaface_hip.h): "base" = ResBlock convolutions + self-attention q / k / v (always
# part of it), "ff" = the transformer blocks' FeedForward (GEGLU + ff.net.2) on top
FP8_SCOPE_BASE, FP8_SCOPE_FF = 1, 2
_SCOPE_BITS = {"base": FP8_SCOPE_BASE, "ff": FP8_SCOPE_FF}


def parse_fp8_scope(scope) -> int:
    """'base' | 'base+ff' | ('base', 'ff') | a mask -> the AF_FP8_SCOPE_* mask.  'base' must be part of it."""
    if isinstance(scope, bool):
        raise ValueError(f"fp8 scope: {scope!r}")
    if isinstance(scope, int):
        mask = scope
    else:
        parts = scope.split("+") if isinstance(scope, str) else list(scope)
        mask = 0
        for part in parts:
            if not isinstance(part, str) or part.strip() not in _SCOPE_BITS:
                raise ValueError(f"fp8 scope: unknown part {part!r} (known: {sorted(_SCOPE_BITS)})")
            mask |= _SCOPE_BITS[part.strip()]
    if not (mask & FP8_SCOPE_BASE) or (mask & ~(FP8_SCOPE_BASE | FP8_SCOPE_FF)):
        raise ValueError(f"fp8 scope {scope!r}: 'base' is always part of the scope, 'ff' may be added")
    return mask


def fp8_scope_names(mask: int) -> tuple:
    return tuple(n for n, b in _SCOPE_BITS.items() if mask & b)


def shift_for_amax(amax: float, headroom: int = FP8_DEFAULT_HEADROOM) -> int:
    """af_fp8_shift_for_amax: the largest shift in [-16, 8] with amax * 2^(shift + headroom) <= 448 (the library's answer,
    so that Python and the executor can never disagree)."""
    from . import _lib
    return int(_lib.load().af_fp8_shift_for_amax(float(amax), int(headroom)))


def check_shifts(shifts: Dict[str, int], site_names: Iterable[str]) -> Dict[str, int]:
    """`shifts` must name exactly the sites in `site_names`, each with an integer in [-16, 8]; returns it as {name: int}."""
    names = list(site_names)
    unknown = sorted(set(shifts) - set(names))
    missing = sorted(set(names) - set(shifts))
    if unknown or missing:
        raise KeyError(f"fp8 scales do not match the model's fp8 sites: {len(unknown)} unknown (e.g. {unknown[:3]}), "
                       f"{len(missing)} missing (e.g. {missing[:3]})")
    out = {}
    for n in names:
        v = shifts[n]
        if isinstance(v, bool) or not isinstance(v, int) or not FP8_SHIFT_MIN <= v <= FP8_SHIFT_MAX:
            raise ValueError(f"fp8 shift of {n}: {v!r} is not an integer in [{FP8_SHIFT_MIN}, {FP8_SHIFT_MAX}]")
        out[n] = v
    return out


def save_scales(path, shifts: Dict[str, int], amax: Dict[str, float] = None, headroom: int = None) -> None:
    """Write {site name: shift} (and, for the reader's information, the recorded maxima) as JSON."""
    doc = {"format": SCALES_FORMAT, "shifts": {k: int(v) for k, v in shifts.items()}}
    if amax is not None:
        doc["amax"] = {k: float(v) for k, v in amax.items()}
    if headroom is not None:
        doc["headroom"] = int(headroom)
    tmp = f"{os.fspath(path)}.tmp"
    with open(tmp, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    os.replace(tmp, path)


def load_scales(path, site_names: Iterable[str]) -> Dict[str, int]:
    """Read a file save_scales wrote; refuses a file whose site names are not exactly `site_names`."""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("format") != SCALES_FORMAT or not isinstance(doc.get("shifts"), dict):
        raise ValueError(f"{path}: not an fp8 scale file ({SCALES_FORMAT})")
    return check_shifts(doc["shifts"], site_names)


def shift_reference(amax: float, headroom: int = FP8_DEFAULT_HEADROOM) -> int:
    """The rule restated with math.frexp (documentation and tests; the engine asks the library)."""
    if not (amax > 0.0) or math.isinf(amax):
        return FP8_SHIFT_DEFAULT
    m, e = math.frexp(amax)                      # amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    s = 9 - e - (1 if m > 0.875 else 0) - headroom
    return max(FP8_SHIFT_MIN, min(FP8_SHIFT_MAX, s))
