"""Reference restatement of token merging in front of the U-Net's self-attention (Bolya & Hoffman, "Token Merging for Fast
Stable Diffusion", CVPR-W 2023; tomesd with sx = sy = 2, use_rand = False, merge_attn only), in torch float64, written from the
algorithm's text and never from the product code.

Per sample, on an H x W map (both even), N = H W tokens in raster order i = y W + x, t = the block's input:

 1. dst tokens: y and x even, ordinal d = (y / 2)(W / 2) + x / 2, Nd = N / 4.  src tokens: the others, ordinals in raster
    order, Ns = N - Nd.
 2. score[s, d] = t_s . t_d rn_s rn_d, rn_i = (sum t_i^2)^-1/2 (0 for a zero row); normalize = False: rn = 1.
 3. node_max[s] = max_d score[s, d], node_idx[s] = the lowest d attaining it.
 4. r = min(Ns, int(N ratio)); the r src tokens of largest node_max are merged, ties to the lower s.
 5. N' = N - r rows: the dst tokens in ordinal order, then the unmerged src tokens in raster order.  map[i] = the row of token
    i: its ordinal (dst), its own row (unmerged src), node_idx (merged src).
 6. merged row j = mean over {i : map[i] = j} of LayerNorm(t_i).
 7. q / k / v, attention and to_out on the N' rows.
 8. t1_i = t_i + o[map[i]].

For the model, `patched` swaps a merging version of O.spatial_transformer, built from the oracle's own helpers, into
oracle.ldm_oracle while O.unet_forward runs."""
import contextlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from oracle import ldm_oracle as O  # noqa: E402


def plan(H, W, ratio):
    """(Nd, Ns, r, N')"""
    assert H > 0 and W > 0 and H % 2 == 0 and W % 2 == 0, (H, W)
    N = H * W
    Nd = N // 4
    Ns = N - Nd
    r = min(Ns, int(N * ratio))
    return Nd, Ns, r, N - r


def partition(H, W):
    """(token indices of the dst tokens in ordinal order, of the src tokens in ordinal order)"""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    is_dst = ((y % 2 == 0) & (x % 2 == 0)).reshape(-1)
    i = torch.arange(H * W)
    return i[is_dst], i[~is_dst]


def scores(t, H, W, normalize=True):
    """[B, Ns, Nd] float64 from t [B, N, C]"""
    t = t.detach().cpu().double()
    dst, src = partition(H, W)
    if normalize:
        n2 = (t * t).sum(-1, keepdim=True)
        rn = torch.where(n2 > 0, n2.clamp_min(1e-300).rsqrt(), torch.zeros_like(n2))
        return torch.einsum("bsc,bdc->bsd", t[:, src], t[:, dst]) * rn[:, src] * rn[:, dst].transpose(1, 2)
    return torch.einsum("bsc,bdc->bsd", t[:, src], t[:, dst])


def match_from_scores(sc, H, W, ratio):
    """(node_idx int64 [B, Ns], node_max float64 [B, Ns], map int64 [B, N], merged bool [B, Ns]) from the score matrix"""
    B, Ns, Nd = sc.shape
    _, _, r, _ = plan(H, W, ratio)
    node_max = sc.max(-1).values
    d = torch.arange(Nd).expand(B, Ns, Nd)
    node_idx = torch.where(sc == node_max[..., None], d, torch.full_like(d, Nd)).min(-1).values     # the lowest d of the maximum
    order = torch.sort(node_max, dim=-1, descending=True, stable=True).indices                       # ties: the lower s first
    merged = torch.zeros(B, Ns, dtype=torch.bool)
    merged.scatter_(1, order[:, :r], True)
    dst, src = partition(H, W)
    tmap = torch.empty(B, H * W, dtype=torch.int64)
    tmap[:, dst] = torch.arange(Nd).expand(B, Nd)
    own_row = Nd + torch.cumsum((~merged).long(), dim=1) - 1
    tmap[:, src] = torch.where(merged, node_idx, own_row)
    return node_idx, node_max, tmap, merged


def match(t, H, W, ratio, normalize=True):
    return match_from_scores(scores(t, H, W, normalize), H, W, ratio)


def merge(v, tmap, n_rows):
    """[B, n_rows, C]: row j = the mean of v[b, i] over the tokens with tmap[b, i] = j (a row without tokens: zero)"""
    B, N, C = v.shape
    tmap = tmap.to(v.device).long()
    out = torch.zeros(B, n_rows, C, dtype=v.dtype, device=v.device)
    out.scatter_add_(1, tmap[..., None].expand(B, N, C), v)
    cnt = torch.zeros(B, n_rows, dtype=v.dtype, device=v.device)
    cnt.scatter_add_(1, tmap, torch.ones(B, N, dtype=v.dtype, device=v.device))
    return out / cnt.clamp_min(1)[..., None]


def unmerge(o, tmap):
    """[B, N, C]: token i gets row tmap[b, i] of o"""
    tmap = tmap.to(o.device).long()
    return torch.gather(o, 1, tmap[..., None].expand(*tmap.shape, o.shape[-1]))


def site_sizes(cfg, H, W, max_downsample):
    """Tokens of every merging site (one per transformer block, forward order) for an H x W latent"""
    inputs, middle, outputs = O._unet_layout(cfg)
    sizes, h, w = [], H, W
    for blk in list(inputs) + [middle] + list(outputs):
        for d in blk:
            if d[0] == "xfmr" and H // h <= max_downsample:
                sizes += [h * w] * cfg.transformer_depth
            elif d[0] == "down":
                h, w = h // 2, w // 2
            elif d[0] == "up":
                h, w = h * 2, w * 2
    return sizes


@contextlib.contextmanager
def patched(ratio, max_downsample, latent_hw, maps=None, log=None):
    """While active, O.unet_forward runs with token merging: every transformer whose map is the latent's divided by at most
    max_downsample merges in front of attn1.  maps: the map of every site in forward order (int [B, N]) to impose instead of
    the reference's own choice.  log: a list that receives, per site, dict(scores, map, own_map, hw)."""
    site = [0]

    def spatial_transformer(sd, p, x, ctx, heads, depth, conv_attn=None):
        B, C, H, W = x.shape
        if latent_hw[0] // H > max_downsample or ratio <= 0:
            return original(sd, p, x, ctx, heads, depth, conv_attn=conv_attn)
        n_rows = plan(H, W, ratio)[3]
        h = O._conv(sd, p + ".proj_in", O._gn(sd, p + ".norm", x, 1e-6), pad=0)
        h = h.permute(0, 2, 3, 1).reshape(B, H * W, C)
        for d in range(depth):
            t = f"{p}.transformer_blocks.{d}"
            sc = scores(h, H, W, True)
            own = match_from_scores(sc, H, W, ratio)[2]
            tmap = own if maps is None else maps[site[0]].detach().cpu().long()
            if log is not None:
                log.append(dict(scores=sc, map=tmap, own_map=own, hw=(H, W)))
            site[0] += 1
            o = O.cross_attention(sd, t + ".attn1", merge(O._ln(sd, t + ".norm1", h), tmap, n_rows), None, None, heads)
            h = unmerge(o, tmap) + h
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


def check_map_structure(tmap, H, W, ratio):
    """What every valid map satisfies, whatever the scores: exactly r src tokens per sample are merged and point at dst rows;
    dst tokens and unmerged src tokens are their own rows, the latter Nd, Nd + 1, ... in raster order."""
    tmap = tmap.detach().cpu().long()
    Nd, Ns, r, n_rows = plan(H, W, ratio)
    dst, src = partition(H, W)
    assert tmap.min() >= 0 and tmap.max() < n_rows
    assert torch.equal(tmap[:, dst], torch.arange(Nd).expand(tmap.shape[0], Nd))
    m = tmap[:, src]
    merged = m < Nd
    assert torch.equal(merged.sum(1), torch.full((tmap.shape[0],), r)), merged.sum(1)
    own_row = Nd + torch.cumsum((~merged).long(), dim=1) - 1
    assert torch.equal(m[~merged], own_row[~merged])
    return merged


def check_map_against_scores(tmap, sc, H, W, ratio, delta):
    """A map is acceptable for the reference's scores within delta: every merged token's target scores >= its best - delta,
    every merged token's node_max >= cut - delta and every unmerged one's <= cut + delta, cut = the r-th largest node_max."""
    merged = check_map_structure(tmap, H, W, ratio)
    Nd, Ns, r, _ = plan(H, W, ratio)
    if r == 0:
        return
    _, src = partition(H, W)
    node_max = sc.max(-1).values
    target = tmap.detach().cpu().long()[:, src].clamp(max=Nd - 1)
    chosen = torch.gather(sc, 2, target[..., None])[..., 0]
    assert bool((chosen[merged] >= node_max[merged] - delta).all()), float((node_max - chosen)[merged].max())
    cut = torch.sort(node_max, dim=-1, descending=True).values[:, r - 1:r]
    assert bool((node_max >= cut - delta)[merged].all())
    if r < Ns:
        assert bool((node_max <= cut + delta)[~merged].all())
