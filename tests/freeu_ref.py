"""Reference restatement of FreeU (Si, Huang, Jiang, Liu, "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024) for the tests, written
from the authors' LDM patch (ChenyangSi/FreeU: Free_UNetModel.forward and Fourier_filter) and never from the product code.

For every output block, with h the incoming backbone (Ch channels) and hs_ the popped skip, before h = cat([h, hs_], 1):

    Ch == 4 * model_channels: (b, s) = (b1, s1);  Ch == 2 * model_channels: (b, s) = (b2, s2);  any other Ch: untouched
    (the patch says 1280 / 640, which is this for SD-1.5; the generalisation gives the narrow test model its sites)

    version 1:  h[:, :Ch/2] *= b
    version 2:  m = h.mean(1); mhat = (m - min m) / (max m - min m) per sample; h[:, :Ch/2] *= (b - 1) * mhat + 1
    hs_ = Fourier_filter(hs_, threshold=1, scale=s)

The filter is written literally with torch.fft; `fourier_filter_closed` is the closed form the kernels use, kept here so that
the CPU test can hold the two against each other.  Everything is float64; the walk casts back to the oracle's dtype.
"""
import math
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from oracle import ldm_oracle as O  # noqa: E402

V1_SD15 = (1.2, 1.4, 0.9, 0.2)      # b1, b2, s1, s2 of the FreeU repository for SD-1.5
V2_SD15 = (1.3, 1.4, 0.9, 0.2)


def fourier_filter(x, threshold, scale):
    """Fourier_filter of the FreeU repository, in float64.  x [B, C, H, W]."""
    x = x.double()
    x_freq = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    B, C, H, W = x_freq.shape
    mask = torch.ones((B, C, H, W), dtype=torch.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = x_freq * mask
    return torch.fft.ifftn(torch.fft.ifftshift(x_freq, dim=(-2, -1)), dim=(-2, -1)).real


def fourier_filter_closed(x, scale):
    """The same for threshold = 1 without an FFT: x + (scale - 1) * low, low the projection onto (ky, kx) in {-1, 0}^2."""
    x = x.double()
    H, W = x.shape[-2:]
    assert H >= 2 and W >= 2
    ty = (2 * math.pi * torch.arange(H, dtype=torch.float64) / H)[:, None]
    tx = (2 * math.pi * torch.arange(W, dtype=torch.float64) / W)[None, :]
    basis = [torch.ones(H, W, dtype=torch.float64), torch.cos(ty).expand(H, W), torch.sin(ty).expand(H, W),
             torch.cos(tx).expand(H, W), torch.sin(tx).expand(H, W), torch.cos(ty + tx), torch.sin(ty + tx)]
    low = sum((x * f).sum((-2, -1), keepdim=True) * f for f in basis) / (H * W)
    return x + (scale - 1.0) * low


def backbone(h, version, b):
    """The backbone half of FreeU.  h [B, Ch, H, W] -> float64."""
    h = h.double().clone()
    half = h.shape[1] // 2
    if version == 1:
        h[:, :half] = h[:, :half] * b
    else:
        m = h.mean(1, keepdim=True)
        B = m.shape[0]
        mx = m.view(B, -1).max(-1).values.view(B, 1, 1, 1)
        mn = m.view(B, -1).min(-1).values.view(B, 1, 1, 1)
        m = (m - mn) / (mx - mn)
        h[:, :half] = h[:, :half] * ((b - 1.0) * m + 1.0)
    return h


def apply_site(h, skip, version, b, s):
    """(h', hs_') of one site, float64."""
    return backbone(h, version, b), fourier_filter(skip, 1, s)


def sites(cfg):
    """[(output block j, Ch, Cs, pair)] in forward order; pair 0: (b1, s1), 1: (b2, s2)."""
    inputs, _, outputs = O._unet_layout(cfg)

    def out_ch(blk, ch):
        for d in blk:
            if d[0] in ("conv_in", "res"):
                ch = d[2]
        return ch

    chans, ch = [], None
    for blk in inputs:
        ch = out_ch(blk, ch)
        chans.append(ch)
    mc, found = cfg.model_channels, []
    for j, blk in enumerate(outputs):
        cs = chans.pop()
        assert blk[0][1] == ch + cs
        if ch in (4 * mc, 2 * mc):
            found.append((j, ch, cs, 0 if ch == 4 * mc else 1))
        ch = out_ch(blk, ch)
    return found


def unet_forward(sd, cfg, x, timesteps, context, freeu=None, use_layerwise_context=True, prefix=O.UNET_PREFIX, taps=None):
    """O.unet_forward restated from its building blocks with the FreeU patch in front of the concatenation.
    freeu: None (off) or (version, b1, b2, s1, s2).  taps: block outputs, and "freeu.<j>" = (h', hs_') of every site."""
    B = x.shape[0]
    emb = O._lin(sd, prefix + "time_embed.2",
                 F.silu(O._lin(sd, prefix + "time_embed.0", O.timestep_embedding(timesteps, cfg.model_channels))))
    ctx_layers = None
    if use_layerwise_context:
        ctx_layers = context.reshape(B, cfg.n_context_layers, -1, context.shape[-1]).permute(1, 0, 2, 3)
    ca_idx = 0

    def run(block_prefix, descs, h):
        nonlocal ca_idx
        for j, d in enumerate(descs):
            p = f"{block_prefix}.{j}"
            if d[0] == "conv_in":
                h = O._conv(sd, p, h)
            elif d[0] == "res":
                h = O.resblock(sd, p, h, emb)
            elif d[0] == "xfmr":
                ctx = ctx_layers[ca_idx] if use_layerwise_context else context
                ca_idx += 1
                h = O.spatial_transformer(sd, p, h, ctx, cfg.num_heads, cfg.transformer_depth, conv_attn=None)
            elif d[0] == "down":
                h = O._conv(sd, p + ".op", h, stride=2)
            elif d[0] == "up":
                h = O._conv(sd, p + ".conv", F.interpolate(h, scale_factor=2, mode="nearest"))
        return h

    inputs, middle, outputs = O._unet_layout(cfg)
    mc = cfg.model_channels
    hs, h = [], x.float()
    for i, blk in enumerate(inputs):
        h = run(f"{prefix}input_blocks.{i}", blk, h)
        hs.append(h)
        if taps is not None:
            taps[f"input_blocks.{i}"] = h
    h = run(f"{prefix}middle_block", middle, h)
    if taps is not None:
        taps["middle_block"] = h
    for j, blk in enumerate(outputs):
        hs_ = hs.pop()
        if freeu is not None and freeu[0] and h.shape[1] in (4 * mc, 2 * mc):
            version, b1, b2, s1, s2 = freeu
            b, s = (b1, s1) if h.shape[1] == 4 * mc else (b2, s2)
            h64, hs64 = apply_site(h, hs_, version, b, s)
            h, hs_ = h64.to(h.dtype), hs64.to(hs_.dtype)
            if taps is not None:
                taps[f"freeu.{j}"] = (h, hs_)
        h = run(f"{prefix}output_blocks.{j}", blk, torch.cat([h, hs_], dim=1))
        if taps is not None:
            taps[f"output_blocks.{j}"] = h
    return O._conv(sd, prefix + "out.2", F.silu(O._gn(sd, prefix + "out.0", h, 1e-5)))
