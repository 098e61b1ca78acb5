"""Reference restatement of DeepCache (Ma, Fang, Wang, CVPR 2024) for the tests, built from the CPU oracle's own functions and
never from the product code.

With n_in input and n_out output blocks and a depth 1 <= k <= n_in - 1:

    refresh step   the oracle's full unet_forward; D = output of output_blocks[n_out - k - 1] is kept
    reuse step     emb = time embedding; h = x; for i < k: h = input_blocks[i](h), pushed as a skip;
                   h = D; for j >= n_out - k: h = output_blocks[j](cat[h, skip.pop()]); out(h)

Every transformer that runs keeps the cross-attention layer index it has in the full forward (the layerwise context slice
and the "layers 6-10 use kernel size 1" conv-attention rule follow it).  With the (x, t) of the refresh the shallow forward
repeats exactly the operations of the full one on exactly the same values, so it equals it bit for bit.
"""
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from oracle import ldm_oracle as O  # noqa: E402


def n_blocks(cfg):
    inputs, _, outputs = O._unet_layout(cfg)
    return len(inputs), len(outputs)


def kept_name(cfg, k):
    """The oracle tap that holds D."""
    _, n_out = n_blocks(cfg)
    return f"output_blocks.{n_out - k - 1}"


def full_forward(sd, cfg, x, t, context, k, **kw):
    """(eps, D) of a refresh step: O.unet_forward and its own tap."""
    taps = {}
    eps = O.unet_forward(sd, cfg, x, t, context, taps=taps, **kw)
    return eps, taps[kept_name(cfg, k)]


def shallow_forward(sd, cfg, x, t, context, D, k, use_layerwise_context=True, prefix=O.UNET_PREFIX, taps=None,
                    placeholder_indices=None, conv_attn_kernel_size=-1):
    """The reuse step.  taps: as O.unet_forward's, for the blocks that run."""
    inputs, middle, outputs = O._unet_layout(cfg)
    n_in, n_out = len(inputs), len(outputs)
    assert n_in == n_out and 1 <= k <= n_in - 1, k
    B = x.shape[0]
    emb = O._lin(sd, prefix + "time_embed.2",
                 F.silu(O._lin(sd, prefix + "time_embed.0", O.timestep_embedding(t, cfg.model_channels))))
    ctx_layers = None
    if use_layerwise_context:
        ctx_layers = context.reshape(B, cfg.n_context_layers, -1, context.shape[-1]).permute(1, 0, 2, 3)
    n_xf = lambda blocks: sum(1 for blk in blocks for d in blk if d[0] == "xfmr")

    def run(block_prefix, descs, h, ca_idx):
        for j, d in enumerate(descs):
            p = f"{block_prefix}.{j}"
            if d[0] == "conv_in":
                h = O._conv(sd, p, h)
            elif d[0] == "res":
                h = O.resblock(sd, p, h, emb)
            elif d[0] == "xfmr":
                ctx = ctx_layers[ca_idx] if use_layerwise_context else context
                ca = None
                if placeholder_indices is not None and conv_attn_kernel_size > 0:
                    ca = (placeholder_indices, 1 if 6 <= ca_idx <= 10 else conv_attn_kernel_size)
                ca_idx += 1
                h = O.spatial_transformer(sd, p, h, ctx, cfg.num_heads, cfg.transformer_depth, conv_attn=ca)
            elif d[0] == "down":
                h = O._conv(sd, p + ".op", h, stride=2)
            elif d[0] == "up":
                h = O._conv(sd, p + ".conv", F.interpolate(h, scale_factor=2, mode="nearest"))
        return h, ca_idx

    hs, h, ca = [], x.float(), 0
    for i in range(k):
        h, ca = run(f"{prefix}input_blocks.{i}", inputs[i], h, ca)
        hs.append(h)
        if taps is not None:
            taps[f"input_blocks.{i}"] = h
    h = D
    ca = n_xf(inputs) + n_xf([middle]) + n_xf(outputs[:n_out - k])     # the layer index the first output block that runs has
    for j in range(n_out - k, n_out):
        h, ca = run(f"{prefix}output_blocks.{j}", outputs[j], torch.cat([h, hs.pop()], dim=1), ca)
        if taps is not None:
            taps[f"output_blocks.{j}"] = h
    assert not hs
    return O._conv(sd, prefix + "out.2", F.silu(O._gn(sd, prefix + "out.0", h, 1e-5)))


class CachedApplyModel:
    """apply_model(x, t, ctx) for O.ddim_sample / dpmpp_ref.sample_ref: call i is a refresh when refresh[i] (it keeps its own
    D), a reuse step from that D otherwise.  `log` records what each call was."""

    def __init__(self, sd, cfg, refresh, k):
        self.sd, self.cfg, self.refresh, self.k = sd, cfg, list(refresh), k
        self.D, self.log = None, []

    def __call__(self, x, t, ctx):
        i = len(self.log)
        if self.refresh[i]:
            eps, self.D = full_forward(self.sd, self.cfg, x, t, ctx, self.k)
            self.log.append("refresh")
            return eps
        assert self.D is not None and self.D.shape[0] == x.shape[0]
        self.log.append("reuse")
        return shallow_forward(self.sd, self.cfg, x, t, ctx, self.D, self.k)
