"""Regional prompts (attention couple): host side of af_set_regions.

A sample's context is R segments of T tokens, segment 0 the base prompt; a weight map m [Bf, R, H, W] >= 0 at the latent
resolution says which regions a latent pixel listens to.  At a cross-attention site whose map is (H / f, W / f):

    a_r(p) = mean of m_r over the f x f box of p;   s(p) = sum_r a_r(p);
    w_r(p) = a_r(p) / s(p) where s(p) > 0, else w_0 = 1 and w_{r > 0} = 0;
    o(p)   = sum over {r : w_r(p) > 0} of w_r(p) softmax(q_p K_r^T dh^-1/2) V_r.

Base-ratio blending, overlapping and soft regions are all expressed through m here, on the host; the device normalises.
Everything below is plain torch on the CPU (float64 where it restates the device's arithmetic)."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

MAX_REGIONS = 8          # AF_REGION_MAX (csrc/af_kernels.h), the base prompt included
LEVELS = 4               # f = 1, 2, 4, 8
PLANS = ("refused", "composition", "fused")    # af_region_plan_query


def parse_box(spec: str):
    """"x0,y0,x1,y1[:weight]" in image fractions -> (x0, y0, x1, y1, weight); weight defaults to 1."""
    body, _, wt = str(spec).partition(":")
    parts = body.split(",")
    if len(parts) != 4:
        raise ValueError(f"region box {spec!r}: expected x0,y0,x1,y1[:weight]")
    try:
        x0, y0, x1, y1 = (float(p) for p in parts)
        weight = float(wt) if wt else 1.0
    except ValueError:
        raise ValueError(f"region box {spec!r}: not numbers") from None
    if not all(math.isfinite(v) for v in (x0, y0, x1, y1, weight)):
        raise ValueError(f"region box {spec!r}: non-finite value")
    if not (0.0 <= x0 < x1 <= 1.0 and 0.0 <= y0 < y1 <= 1.0):
        raise ValueError(f"region box {spec!r}: need 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1")
    if weight < 0.0:
        raise ValueError(f"region box {spec!r}: negative weight")
    return x0, y0, x1, y1, weight


def _cover(lo: float, hi: float, n: int) -> torch.Tensor:
    """fraction of each of n unit cells covered by [lo n, hi n]"""
    e = torch.arange(n + 1, dtype=torch.float64)
    a, b = lo * n, hi * n
    return (torch.minimum(e[1:], torch.tensor(b, dtype=torch.float64)) - torch.maximum(e[:-1], torch.tensor(a, dtype=torch.float64))).clamp_(min=0.0)


def masks_from_boxes(boxes: Sequence, H: int, W: int) -> torch.Tensor:
    """boxes (strings or parse_box tuples) -> float64 [n, H, W]: a cell's weight is the covered fraction of its area times the
    box's weight."""
    out = torch.zeros(len(boxes), H, W, dtype=torch.float64)
    for i, b in enumerate(boxes):
        x0, y0, x1, y1, wt = parse_box(b) if isinstance(b, str) else b
        out[i] = wt * _cover(y0, y1, H)[:, None] * _cover(x0, x1, W)[None, :]
    return out


def _area_matrix(n_out: int, n_in: int) -> torch.Tensor:
    """[n_out, n_in]: the fraction of output cell i's extent that input cell j covers (rows sum to 1)"""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i in range(n_out):
        m[i] = _cover(i / n_out, (i + 1) / n_out, n_in) * n_out / n_in
    return m


def mask_from_image(img, H: int, W: int) -> torch.Tensor:
    """A 2-D mask image (tensor / array, or a path readable by PIL; values scaled to [0, 1] if integer) area-averaged to the
    latent grid: float64 [H, W]."""
    if isinstance(img, (str, bytes)) or hasattr(img, "__fspath__"):
        import numpy as np
        from PIL import Image
        img = np.asarray(Image.open(img).convert("L"))
    t = torch.as_tensor(img)
    if t.dim() == 3:
        t = t.double().mean(dim=-1) if t.shape[-1] in (1, 3, 4) else t[0]
    if t.dim() != 2:
        raise ValueError(f"mask image of shape {tuple(t.shape)}: expected 2-D")
    scale = 255.0 if not t.is_floating_point() else 1.0
    t = t.double() / scale
    _check(t, "mask image")
    return _area_matrix(H, t.shape[0]) @ t @ _area_matrix(W, t.shape[1]).T


def _check(t: torch.Tensor, what: str):
    if not torch.isfinite(t).all():
        raise ValueError(f"{what}: non-finite weight")
    if (t < 0).any():
        raise ValueError(f"{what}: negative weight")


def build_weights(region_masks, base_weight: float = 0.2, B: int = 1, legs: int = 1) -> torch.Tensor:
    """region_masks [n, H, W] (shared by the B samples) or [B, n, H, W] -> fp32 [B legs, 1 + n, H, W]: segment 0 (the base
    prompt) weighs base_weight everywhere, region i its mask.  legs = 2: the CFG batch, conditional samples first, then B
    unconditional legs with (1, 0, ..., 0) -- segments 1.. of their context are never read."""
    m = torch.as_tensor(region_masks).double()
    if m.dim() == 3:
        m = m[None].expand(B, *m.shape)
    if m.dim() != 4 or m.shape[0] != B:
        raise ValueError(f"region masks of shape {tuple(m.shape)}: expected [n, H, W] or [{B}, n, H, W]")
    if legs not in (1, 2):
        raise ValueError(f"legs {legs} (1 or 2)")
    if not (math.isfinite(base_weight) and base_weight >= 0.0):
        raise ValueError(f"base weight {base_weight}: must be finite and >= 0")
    _check(m, "region masks")
    n, H, W = m.shape[1:]
    if 1 + n > MAX_REGIONS:
        raise ValueError(f"{n} regions + the base prompt exceed {MAX_REGIONS}")
    if H % 8 or W % 8:
        raise ValueError(f"weight map {H} x {W}: sides must be multiples of 8")
    cond = torch.cat([torch.full((B, 1, H, W), float(base_weight), dtype=torch.float64), m], dim=1)
    if legs == 1:
        return cond.float()
    unc = torch.zeros_like(cond)
    unc[:, 0] = 1.0
    return torch.cat([cond, unc]).float()


def concat_contexts(contexts: Sequence[torch.Tensor], uncond: Optional[torch.Tensor] = None) -> torch.Tensor:
    """R contexts [rows, T, D] (segment 0 first) -> [rows, R T, D]; with uncond [rows, T, D]: the CFG batch [2 rows, R T, D],
    the negative prompt repeated R times along the token axis for the unconditional legs."""
    contexts = list(contexts)
    if not contexts or len(contexts) > MAX_REGIONS:
        raise ValueError(f"{len(contexts)} contexts (1 .. {MAX_REGIONS})")
    shp = tuple(contexts[0].shape)
    if len(shp) != 3 or any(tuple(c.shape) != shp for c in contexts):
        raise ValueError("contexts must share one shape [rows, T, D]")
    cond = torch.cat(contexts, dim=1)
    if uncond is None:
        return cond
    if tuple(uncond.shape) != shp:
        raise ValueError(f"unconditional context of shape {tuple(uncond.shape)}, expected {shp}")
    return torch.cat([cond, uncond.repeat(1, len(contexts), 1)])


def pyramid(weights: torch.Tensor) -> list:
    """The float64 restatement of region_weights_kernel: weights [Bf, R, H, W] -> [w_0 .. w_3], w_l float64 [Bf, R, H >> l, W >> l]."""
    m = torch.as_tensor(weights).double()
    if m.dim() != 4:
        raise ValueError(f"weights of shape {tuple(m.shape)}: expected [Bf, R, H, W]")
    _check(m, "region weights")
    Bf, R, H, W = m.shape
    if not 1 <= R <= MAX_REGIONS:
        raise ValueError(f"{R} regions (1 .. {MAX_REGIONS})")
    if H % 8 or W % 8:
        raise ValueError(f"weight map {H} x {W}: sides must be multiples of 8")
    out = []
    for l in range(LEVELS):
        f = 1 << l
        a = m.reshape(Bf, R, H // f, f, W // f, f).sum(dim=(3, 5)) / (f * f)
        s = a.sum(dim=1, keepdim=True)
        w = torch.where(s > 0, a / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(a))
        w[:, 0] = torch.where(s[:, 0] > 0, w[:, 0], torch.ones_like(w[:, 0]))
        out.append(w)
    return out


def active_pairs(w: torch.Tensor) -> torch.Tensor:
    """One pyramid level [Bf, R, h, w] (or [Bf, R, N]) -> int64 [Bf, ceil(N / 32)]: bit r of word j is set iff some w_r > 0 among
    queries 32 j .. 32 j + 31 (row-major pixels)."""
    w = torch.as_tensor(w)
    Bf, R = w.shape[:2]
    flat = w.reshape(Bf, R, -1) > 0
    N = flat.shape[2]
    nblk = (N + 31) // 32
    pad = torch.zeros(Bf, R, nblk * 32, dtype=torch.bool)
    pad[:, :, :N] = flat
    any_ = pad.reshape(Bf, R, nblk, 32).any(dim=3).long()
    return (any_ << torch.arange(R).reshape(1, R, 1)).sum(dim=1)


def level_offsets(Bf: int, R: int, H: int, W: int):
    """(float offsets of the four levels in af_op_region_weights' pyramid, word offsets in its bits, totals) -- AfRegionLayout"""
    wo, bo, w_off, b_off = 0, 0, [], []
    for l in range(LEVELS):
        N = (H >> l) * (W >> l)
        w_off.append(wo)
        b_off.append(bo)
        wo += Bf * R * N
        bo += Bf * ((N + 31) // 32)
    return w_off, b_off, wo, bo


def plan_query(dtype, dh: int, T: int, R: int) -> str:
    """af_region_plan_query: "refused", "composition" or "fused".  Honours the knob region_fused.  Host only."""
    import ctypes as C

    from . import _lib
    dt = _lib.DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    out = C.c_int64()
    _lib.check(_lib.load().af_region_plan_query(dt, int(dh), int(T), int(R), C.byref(out)), "af_region_plan_query")
    return PLANS[out.value]
