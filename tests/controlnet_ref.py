"""Reference restatement of ControlNet (Zhang, Rao, Agrawala, ICCV 2023; cldm/cldm.py of lllyasviel/ControlNet) for the tests, built
from the CPU oracle's own functions and never from the product code.

    emb  = time_embed(timestep_embedding(t))                              control_model.time_embed.{0,2}
    g    = input_hint_block(hint): 3x3 convs 3->16, 16->16, 16->32 /2, 32->32, 32->96 /2, 96->96, 96->256 /2, 256->mc, SiLU
           between them (keys .0 .2 ... .14, all pad 1)
    h    = x
    for i, block in enumerate(input_blocks):  h = block(h, emb, ctx);  if i == 0: h = h + g;  r[i] = zero_convs.i.0(h)
    r[n_in] = middle_block_out.0(middle_block(h, emb, ctx))

The controlled U-Net is O.unet_forward with h = middle(h) + s[n_in] r[n_in] and every cat([h, hs.pop()]) reading
hs.pop() + s[i] r[i]; the input blocks see the unmodified skips.  The control branch's 7 cross-attention layers read the layer
slices 0 .. 6 of a layerwise context.  FreeU filters the controlled skip; a DeepCache reuse step of depth k adds r[0 .. k - 1].
"""
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from oracle import ldm_oracle as O  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent))
import freeu_ref  # noqa: E402

CONTROL_PREFIX = "control_model."
HINT_CHANNELS = (16, 16, 32, 32, 96, 96, 256)
HINT_STRIDES = (1, 1, 2, 1, 2, 1, 2, 1)


def n_residuals(cfg):
    return len(O._unet_layout(cfg)[0]) + 1


def skip_channels(cfg):
    """Channels of every input block's output, then of the middle block's."""
    inputs, _, _ = O._unet_layout(cfg)
    out, ch = [], None
    for blk in inputs:
        for d in blk:
            if d[0] in ("conv_in", "res"):
                ch = d[2]
        out.append(ch)
    return out + [ch]


def param_shapes(cfg, hint_channels=3, prefix=CONTROL_PREFIX):
    """The inventory this restatement reads: the oracle's U-Net encoder under `prefix`, the hint network, the zero convs."""
    unet = O.unet_param_shapes(cfg, prefix=prefix)
    out = {k: v for k, v in unet.items() if k[len(prefix):].startswith(("time_embed.", "input_blocks.", "middle_block."))}
    chans = (hint_channels,) + HINT_CHANNELS + (cfg.model_channels,)
    for k in range(8):
        out[f"{prefix}input_hint_block.{2 * k}.weight"] = (chans[k + 1], chans[k], 3, 3)
        out[f"{prefix}input_hint_block.{2 * k}.bias"] = (chans[k + 1],)
    sk = skip_channels(cfg)
    for i, c in enumerate(sk[:-1]):
        out[f"{prefix}zero_convs.{i}.0.weight"] = (c, c, 1, 1)
        out[f"{prefix}zero_convs.{i}.0.bias"] = (c,)
    out[f"{prefix}middle_block_out.0.weight"] = (sk[-1], sk[-1], 1, 1)
    out[f"{prefix}middle_block_out.0.bias"] = (sk[-1],)
    return out


def plan(cfg, H, W):
    """[(C, H, W, element offset for one sample)] of the residuals, from the layout alone."""
    inputs, _, _ = O._unet_layout(cfg)
    out, off, hh, ww = [], 0, H, W
    for blk, c in zip(inputs, skip_channels(cfg)):
        if blk[0][0] == "down":
            hh, ww = hh // 2, ww // 2
        out.append((c, hh, ww, off))
        off += c * hh * ww
    out.append((skip_channels(cfg)[-1], hh, ww, off))
    return out


def hint_features(sd, hint, prefix=CONTROL_PREFIX):
    h = hint.float()
    for k in range(8):
        h = O._conv(sd, f"{prefix}input_hint_block.{2 * k}", h, stride=HINT_STRIDES[k])
        if k < 7:
            h = F.silu(h)
    return h


def _emb(sd, cfg, t, prefix):
    return O._lin(sd, prefix + "time_embed.2", F.silu(O._lin(sd, prefix + "time_embed.0", O.timestep_embedding(t, cfg.model_channels))))


def _ctx_layers(cfg, context, B, layerwise):
    if not layerwise:
        return None
    return context.reshape(B, cfg.n_context_layers, -1, context.shape[-1]).permute(1, 0, 2, 3)


def _runner(sd, cfg, emb, ctx_layers, context):
    """run(block_prefix, descs, h, ca_idx) -> (h, ca_idx): one block from the oracle's layer functions."""
    def run(block_prefix, descs, h, ca_idx):
        for j, d in enumerate(descs):
            p = f"{block_prefix}.{j}"
            if d[0] == "conv_in":
                h = O._conv(sd, p, h)
            elif d[0] == "res":
                h = O.resblock(sd, p, h, emb)
            elif d[0] == "xfmr":
                ctx = ctx_layers[ca_idx] if ctx_layers is not None else context
                ca_idx += 1
                h = O.spatial_transformer(sd, p, h, ctx, cfg.num_heads, cfg.transformer_depth, conv_attn=None)
            elif d[0] == "down":
                h = O._conv(sd, p + ".op", h, stride=2)
            elif d[0] == "up":
                h = O._conv(sd, p + ".conv", F.interpolate(h, scale_factor=2, mode="nearest"))
        return h, ca_idx
    return run


def control_forward(sd, cfg, x, t, ctx, hint, n_blocks=None, use_layerwise_context=True, prefix=CONTROL_PREFIX):
    """The list of residuals (NCHW), the first n_blocks of them (None: all n_in + 1).  hint [B or 1, 3, 8H, 8W]."""
    inputs, middle, _ = O._unet_layout(cfg)
    n_in = len(inputs)
    n = n_in + 1 if n_blocks is None else n_blocks
    assert 1 <= n <= n_in + 1
    B = x.shape[0]
    emb = _emb(sd, cfg, t, prefix)
    run = _runner(sd, cfg, emb, _ctx_layers(cfg, ctx, B, use_layerwise_context), ctx)
    g = hint_features(sd, hint, prefix)
    assert g.shape[0] in (1, B) and tuple(g.shape[2:]) == tuple(x.shape[2:])
    res, h, ca = [], x.float(), 0
    for i in range(min(n, n_in)):
        h, ca = run(f"{prefix}input_blocks.{i}", inputs[i], h, ca)
        if i == 0:
            h = h + g
        res.append(O._conv(sd, f"{prefix}zero_convs.{i}.0", h, pad=0))
    if n > n_in:
        h, ca = run(f"{prefix}middle_block", middle, h, ca)
        res.append(O._conv(sd, f"{prefix}middle_block_out.0", h, pad=0))
    return res


def _add(h, r, s, cond_only):
    """h + s r; cond_only: onto the first len(r) samples of h only (the rest is returned as it is)."""
    if not cond_only:
        return h + s * r
    out = h.clone()
    out[: r.shape[0]] = h[: r.shape[0]] + s * r
    return out


def controlled_unet_forward(sd, cfg, x, t, ctx, residuals, scales, cond_only=False, use_layerwise_context=True,
                            prefix=O.UNET_PREFIX, freeu=None, keep=None, reuse=None):
    """O.unet_forward restated with the ControlNet residuals.  residuals: control_forward's list (for the first half of the batch
    when cond_only); scales: one per residual.
    freeu: None or (version, b1, b2, s1, s2): the FreeU patch of freeu_ref on the CONTROLLED skip.
    keep = k: a DeepCache refresh, returns (eps, D) with D the output of output_blocks[n_out - k - 1].
    reuse = (D, k): a DeepCache reuse step: input blocks 0 .. k - 1, residuals 0 .. k - 1, output blocks n_out - k .. from D."""
    inputs, middle, outputs = O._unet_layout(cfg)
    n_in, n_out = len(inputs), len(outputs)
    B = x.shape[0]
    emb = _emb(sd, cfg, t, prefix)
    run = _runner(sd, cfg, emb, _ctx_layers(cfg, ctx, B, use_layerwise_context), ctx)
    n_xf = lambda blocks: sum(1 for blk in blocks for d in blk if d[0] == "xfmr")
    mc = cfg.model_channels
    k_reuse = reuse[1] if reuse is not None else None
    n_run = k_reuse if reuse is not None else n_in
    assert len(residuals) >= (n_run if reuse is not None else n_in + 1) and len(scales) >= len(residuals)
    hs, h, ca = [], x.float(), 0
    for i in range(n_run):
        h, ca = run(f"{prefix}input_blocks.{i}", inputs[i], h, ca)
        hs.append(h)                                               # (the encoder reads the unmodified skips)
    if reuse is None:
        h, ca = run(f"{prefix}middle_block", middle, h, ca)
        h = _add(h, residuals[n_in], scales[n_in], cond_only)
        j0 = 0
    else:
        h = reuse[0]
        j0 = n_out - k_reuse
        ca = n_xf(inputs) + n_xf([middle]) + n_xf(outputs[:j0])
    D = None
    for j in range(j0, n_out):
        i = n_in - 1 - j
        hs_ = _add(hs.pop(), residuals[i], scales[i], cond_only)
        if freeu is not None and freeu[0] and h.shape[1] in (4 * mc, 2 * mc):
            version, b1, b2, s1, s2 = freeu
            b, s = (b1, s1) if h.shape[1] == 4 * mc else (b2, s2)
            h64, hs64 = freeu_ref.apply_site(h, hs_, version, b, s)      # (D is kept unscaled: every step scales what it reads)
            h, hs_ = h64.to(h.dtype), hs64.to(hs_.dtype)
        h, ca = run(f"{prefix}output_blocks.{j}", outputs[j], torch.cat([h, hs_], dim=1), ca)
        if keep is not None and j == n_out - keep - 1:
            D = h
    assert not hs
    eps = O._conv(sd, prefix + "out.2", F.silu(O._gn(sd, prefix + "out.0", h, 1e-5)))
    return (eps, D) if keep is not None else eps


class ControlledApplyModel:
    """apply_model(x, t, ctx) for O.ddim_sample / dpmpp_ref.sample_ref: the controlled forward, with the control branch run on
    the same (x, t, ctx), while every t of the call lies in the window (t_lo, t_hi); the plain O.unet_forward outside it."""

    def __init__(self, sd, csd, cfg, hint, scales, window=(0, 999)):
        self.sd, self.csd, self.cfg, self.hint, self.scales, self.window = sd, csd, cfg, hint, list(scales), window
        self.log = []

    def __call__(self, x, t, ctx):
        on = all(self.window[0] <= int(v) <= self.window[1] for v in t.reshape(-1).tolist())
        self.log.append(on)
        if not on:
            return O.unet_forward(self.sd, self.cfg, x, t, ctx)
        hint = self.hint
        if hint.shape[0] not in (1, x.shape[0]):                   # (the sampler's CFG batch [x; x]: one hint per leg)
            hint = hint.repeat(x.shape[0] // hint.shape[0], 1, 1, 1)
        res = control_forward(self.csd, self.cfg, x, t, ctx, hint)
        return controlled_unet_forward(self.sd, self.cfg, x, t, ctx, res, self.scales)


# ---- the inputs the CPU and the GPU tests share ----------------------------------------------------------------------------
SEED_UNET, SEED_CONTROL = 11, 31


def weights(cfg):
    """(U-Net state dict, ControlNet state dict): the oracle's seeded draws, so the zero convolutions are NOT zero."""
    return (O.synth_state_dict(O.unet_param_shapes(cfg), seed=SEED_UNET),
            O.synth_state_dict(param_shapes(cfg), seed=SEED_CONTROL))


def case(cfg, B, H, W, seed=5, shared_hint=False):
    """x [B, 4, H, W], t [B], layerwise context [B * 16, 77, D], hint [B or 1, 3, 8 H, 8 W] in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cfg.in_channels, H, W, generator=g)
    t = torch.tensor([901, 401, 1, 650][:B] if B <= 4 else list(range(1, 1000, 1000 // B))[:B])
    ctx = torch.randn(B * cfg.n_context_layers, 77, cfg.context_dim, generator=g)
    hint = torch.rand(1 if shared_hint else B, 3, 8 * H, 8 * W, generator=g)
    return x, t, ctx, hint


def case_scales(cfg):
    """Distinct per-residual scales 0.5 + 0.1 i: a permuted or dropped segment shows."""
    return [0.5 + 0.1 * i for i in range(n_residuals(cfg))]
