"""Reference restatement of perturbed-attention guidance (Ahn et al., ECCV 2024; the SD-1.5 PAG pipelines of diffusers) and of
guidance rescale (Lin et al., WACV 2024, section 3.4; diffusers' rescale_noise_cfg) for the tests: the combine in fp64, the
adaptive scale, the site numbering, and a context manager that perturbs the oracle's self-attention."""
import contextlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from oracle import ldm_oracle as O  # noqa: E402


def guidance(e_c, e_u, e_p, w, s, phi):
    """e = e_u + w (e_c - e_u) + s (e_c - e_p) in fp64 (e_u None: no w term, e_p None: no s term), then, for phi > 0,
    e (phi f + 1 - phi) with f = std(e_c) / std(e) per sample over all its elements, unbiased.  Returns (e, f or None)."""
    c = e_c.double()
    e = c.clone()
    if e_u is not None:
        u = e_u.double()
        e = u + float(w) * (c - u)
    if e_p is not None:
        e = e + float(s) * (c - e_p.double())
    if not phi > 0:
        return e, None
    dims = tuple(range(1, e.dim()))
    f = c.std(dim=dims, keepdim=True) / e.std(dim=dims, keepdim=True)
    return e * (float(phi) * f + (1.0 - float(phi))), f.reshape(-1)


def pag_scale_at(t, s, a):
    """The scale of the step at timestep t: max(s - a (1000 - t), 0), as diffusers' _get_pag_scale."""
    return max(float(s) - float(a) * (1000.0 - float(t)), 0.0)


def site_blocks(cfg):
    """site -> (block in forward order: input blocks, middle block, output blocks; name) from the oracle's own layout"""
    inputs, middle, outputs = O._unet_layout(cfg)
    n_lev = len(cfg.channel_mult)
    out, ds = [], 1
    for bi, blk in enumerate(list(inputs) + [middle] + list(outputs)):
        for d in blk:
            if d[0] == "xfmr":
                lev = {1: 0, 2: 1, 4: 2, 8: 3, 16: 4}[ds]
                name = "mid" if bi == len(inputs) else (f"down.blocks.{lev}" if bi < len(inputs) else f"up.blocks.{n_lev - 1 - lev}")
                out += [(bi, name)] * cfg.transformer_depth
            elif d[0] == "down":
                ds *= 2
            elif d[0] == "up":
                ds //= 2
    return out


def sites_of(cfg, names):
    """names and / or site numbers -> the sorted tuple of sites"""
    if names is None:
        return ()
    if isinstance(names, (str, int)):
        names = (names,)
    blocks = site_blocks(cfg)
    known = {n for _, n in blocks}
    sites = set()
    for item in names:
        if isinstance(item, str):
            if item not in known:
                raise ValueError(f"unknown PAG layer {item!r}")
            sites.update(i for i, (_, n) in enumerate(blocks) if n == item)
        else:
            if not 0 <= int(item) < len(blocks):
                raise ValueError(f"PAG site {item} out of range")
            sites.add(int(item))
    return tuple(sorted(sites))


def identity_attention(sd, p, n):
    """attn1 with the identity as its attention map: to_out(to_v(n))"""
    return O._lin(sd, p + ".to_out.0", O._lin(sd, p + ".to_v", n))


@contextlib.contextmanager
def patched(sites, legs):
    """While active, O.unet_forward perturbs the self-attention of the given sites (forward order, one per transformer block)
    for the samples `legs` (a slice or an index tensor over the batch): attn1(n) = to_out(to_v(n)), n = norm1(h).  Every other
    sample and everything else in the block is the oracle's own arithmetic."""
    sites = set(int(s) for s in sites)
    site = [0]

    def spatial_transformer(sd, p, x, ctx, heads, depth, conv_attn=None):
        mine = [site[0] + d for d in range(depth)]
        site[0] += depth
        if not sites.intersection(mine):
            return original(sd, p, x, ctx, heads, depth, conv_attn=conv_attn)
        B, C, H, W = x.shape
        h = O._conv(sd, p + ".proj_in", O._gn(sd, p + ".norm", x, 1e-6), pad=0)
        h = h.permute(0, 2, 3, 1).reshape(B, H * W, C)
        for d in range(depth):
            t = f"{p}.transformer_blocks.{d}"
            n = O._ln(sd, t + ".norm1", h)
            a = O.cross_attention(sd, t + ".attn1", n, None, None, heads)
            if mine[d] in sites:
                a = a.clone()
                a[legs] = identity_attention(sd, t + ".attn1", n[legs])
            h = a + h
            ca = None if conv_attn is None else (conv_attn[0], (H, W), conv_attn[1])
            h = h + O.cross_attention(sd, t + ".attn2", O._ln(sd, t + ".norm2", h), ctx, ctx, heads, conv_attn=ca)
            h = O.feed_forward(sd, t + ".ff", O._ln(sd, t + ".norm3", h)) + h
        h = h.reshape(B, H, W, C).permute(0, 3, 1, 2)
        return O._conv(sd, p + ".proj_out", h, pad=0) + x

    original = O.spatial_transformer
    O.spatial_transformer = spatial_transformer
    try:
        yield
    finally:
        O.spatial_transformer = original
