"""Reference restatement of T-GATE (Zhang et al., "Cross-Attention Makes Inference Cumbersome in Text-to-Image Diffusion
Models", 2024) as this project pins it, built from the CPU oracle's own functions and never from the product code.

A run has n loop steps and a gate g, 1 <= g <= n - 1.  A site is the attn2 of one transformer block in forward order.

    i < g        the ordinary step: twin forward, classifier-free guidance
    i = g - 1    that same step, which also keeps, per site, A = mean over the L legs of attn2's output (to_out with its bias,
                 before the residual), [B, N, C]; L = 2 for the twin call (sample b with b + B), 1 for a single-leg call
    i >= g       the U-Net on the B samples of x alone; every site computes h + A[site] in place of h + attn2(norm2(h), ctx);
                 eps goes to the update as it is, without a guidance combine

`patched` restates the per-site change on O.spatial_transformer (as pag_ref.patched does for PAG); GatedApplyModel is the
stateful apply_model the reference sampler loops take (O.ddim_sample, dpmpp_ref.sample_ref, philox_ref.sde_sample_ref): they call
it on cat[x, x] and combine e_u + g (e_c - e_u); a single-leg step returns cat[e, e], for which that combine is e exactly.
"""
import contextlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import deep_cache_ref as DR  # noqa: E402
import tome_ref as TM  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402


def phases(n, g):
    """None / "capture" / "replay" per loop index, from the statement above (g None or 0: off)."""
    if not g:
        return [None] * n
    assert 1 <= g <= n - 1, (n, g)
    return [None if i < g - 1 else "capture" if i == g - 1 else "replay" for i in range(n)]


def site_of_prefix(cfg, prefix=O.UNET_PREFIX):
    """transformer parameter prefix -> its first site, from the oracle's own layout"""
    inputs, middle, outputs = O._unet_layout(cfg)
    out, site = {}, 0
    named = [(f"{prefix}input_blocks.{i}", b) for i, b in enumerate(inputs)] + [(f"{prefix}middle_block", middle)] + \
            [(f"{prefix}output_blocks.{i}", b) for i, b in enumerate(outputs)]
    for name, blk in named:
        for j, d in enumerate(blk):
            if d[0] == "xfmr":
                out[f"{name}.{j}"] = site
                site += cfg.transformer_depth
    return out, site


def n_sites(cfg):
    return site_of_prefix(cfg)[1]


@contextlib.contextmanager
def patched(cfg, mode, record, legs=1, tome=None):
    """While active, the oracle's transformers run a T-GATE step.  mode "capture": record[site] = the mean over `legs` legs of
    O.cross_attention(..attn2..) (fp32; the batch is legs * B, leg-major), everything else the oracle's own arithmetic; mode
    "replay": h + record[site] in place of the cross-attention, the context is not read.  The site follows from the
    transformer's parameter prefix, so a DeepCache reuse step (deep_cache_ref.shallow_forward) finds the right records.
    tome = (ratio, max_downsample, latent (H, W), maps): token merging in front of attn1 as tome_ref.patched restates it, with
    the given map of every merging site in forward order imposed (a full forward only)."""
    assert mode in ("capture", "replay")
    sites, _ = site_of_prefix(cfg)
    tome_site = [0]

    def spatial_transformer(sd, p, x, ctx, heads, depth, conv_attn=None):
        B, C, H, W = x.shape
        h = O._conv(sd, p + ".proj_in", O._gn(sd, p + ".norm", x, 1e-6), pad=0)
        h = h.permute(0, 2, 3, 1).reshape(B, H * W, C)
        for d in range(depth):
            t = f"{p}.transformer_blocks.{d}"
            site = sites[p] + d
            if tome is not None and tome[0] > 0 and tome[2][0] // H <= tome[1]:
                tmap = tome[3][tome_site[0]].detach().cpu().long()
                tome_site[0] += 1
                n_rows = TM.plan(H, W, tome[0])[3]
                o1 = O.cross_attention(sd, t + ".attn1", TM.merge(O._ln(sd, t + ".norm1", h), tmap, n_rows), None, None, heads)
                h = TM.unmerge(o1, tmap) + h
            else:
                h = O.cross_attention(sd, t + ".attn1", O._ln(sd, t + ".norm1", h), None, None, heads) + h
            if mode == "capture":
                ca = None if conv_attn is None else (conv_attn[0], (H, W), conv_attn[1])
                o = O.cross_attention(sd, t + ".attn2", O._ln(sd, t + ".norm2", h), ctx, ctx, heads, conv_attn=ca)
                assert B % legs == 0
                record[site] = o.float().reshape(legs, B // legs, H * W, C).sum(0) * (1.0 / legs)
                h = h + o
            else:
                assert tuple(record[site].shape) == (B, H * W, C), (site, tuple(record[site].shape), (B, H * W, C))
                h = h + record[site]
            h = O.feed_forward(sd, t + ".ff", O._ln(sd, t + ".norm3", h)) + h
        h = h.reshape(B, H, W, C).permute(0, 3, 1, 2)
        return O._conv(sd, p + ".proj_out", h, pad=0) + x

    original = O.spatial_transformer
    O.spatial_transformer = spatial_transformer
    try:
        yield record
    finally:
        O.spatial_transformer = original


def capture_forward(sd, cfg, x, t, ctx, legs, forward=O.unet_forward, tome=None, **kw):
    """(eps, record) of a capture forward on the batch x (legs * B samples, leg-major)."""
    with patched(cfg, "capture", {}, legs, tome=tome) as rec:
        eps = forward(sd, cfg, x, t, ctx, **kw)
    return eps, rec


def replay_forward(sd, cfg, x, t, record, forward=O.unet_forward, tome=None, **kw):
    """eps of a replay forward on the B samples of x: no context (a dummy one stands where the oracle wants a tensor)."""
    dummy = torch.zeros(x.shape[0] * cfg.n_context_layers, 1, cfg.context_dim)
    with patched(cfg, "replay", record, tome=tome):
        return forward(sd, cfg, x, t, dummy, **kw)


class GatedApplyModel:
    """apply_model(x [2B], t [2B], ctx [2B ...]) for the reference sampler loops: call i runs phase phases[i].  single[i]: that
    step is a single-leg call (no unconditional conditioning, or guidance 1) -- the first half of the batch alone, returned
    twice.  refresh / k: with DeepCache composed, call i is a refresh (keeps its own D) or a reuse step from that D; the form
    (legs, phase) of a step that differs from the last refresh's forces a refresh, as DeepCacheRun.step does.
    `log` records the phases, `dc_log` what each call was for DeepCache."""

    def __init__(self, sd, cfg, phases, single=None, refresh=None, k=None):
        self.sd, self.cfg, self.phases = sd, cfg, list(phases)
        self.single = list(single) if single is not None else [False] * len(self.phases)
        self.refresh, self.k = (list(refresh) if refresh is not None else None), k
        self.record, self.D, self._form = {}, None, None
        self.log, self.dc_log = [], []

    def _run(self, x, t, ctx, form):
        """one U-Net evaluation with DeepCache's choice for this call"""
        if self.refresh is None:
            self.dc_log.append("full")
            return O.unet_forward(self.sd, self.cfg, x, t, ctx)
        i = len(self.dc_log)
        if self.refresh[i] or form != self._form:
            self._form = form
            self.dc_log.append("refresh")
            eps, self.D = DR.full_forward(self.sd, self.cfg, x, t, ctx, self.k)
            return eps
        self.dc_log.append("reuse")
        return DR.shallow_forward(self.sd, self.cfg, x, t, ctx, self.D, self.k)

    def __call__(self, x, t, ctx):
        i = len(self.log)
        ph = self.phases[i]
        self.log.append(ph)
        b = x.shape[0] // 2
        one = self.single[i] or ph == "replay"
        if one:
            x, t, ctx = x[:b], t[:b], ctx[:ctx.shape[0] // 2]
        form = (not one, ph)
        if ph == "replay":
            ctx = torch.zeros(b * self.cfg.n_context_layers, 1, self.cfg.context_dim)
            with patched(self.cfg, "replay", self.record):
                e = self._run(x, t, ctx, form)
        elif ph == "capture":
            self.record = {}
            with patched(self.cfg, "capture", self.record, 1 if one else 2):
                e = self._run(x, t, ctx, form)
        else:
            e = self._run(x, t, ctx, form)
        return torch.cat([e, e]) if one else e
