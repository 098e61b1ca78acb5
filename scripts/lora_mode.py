#!/usr/bin/env python
"""What switching LoRA adapters costs (af_load_tensor_lora): SD-1.5 with synthetic weights (as bench.py builds
them), bf16, a synthetic rank-32 adapter on every attention and FeedForward linear plus proj_in / proj_out of the U-Net.

    (a) UNetModel.set_lora on a live engine (the fused merge of the touched weights only) and clear_lora (the way back);
    (b) the route available without the fused load, for the same tensors: merge in torch on the device (W + s up @ down in fp32),
        then Engine.load_tensor of each touched tensor;
    (c) a full sync_weights (what a load_state_dict of a pre-merged checkpoint costs the engine, without reading the file);
    (d) the kernel through ops.lora_repack at the three widths, beside the same kernel with zero adapters (the plain repack's
        work) -- at these sizes an upper bound: the wrapper's call rate, not the kernel, sets the figure;
    (e) one twin forward with the adapter set and without: the same launches (af_gemm_plan_counts) and therefore the same time.
Host clock to a device synchronise for (a) - (c) and (e), HIP events for (d); best, median and worst of --reps.

    python scripts/lora_mode.py [--out profiles/lora_<commit>.txt]
"""
import argparse
import re
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--rank", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--burst", type=int, default=10)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib, ops  # noqa: E402
from adaface_amd.lora import lora_factor  # noqa: E402
from bench import build_model  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def stats(v):
    v = sorted(v)
    return f"{1e3 * v[0]:9.3f} {1e3 * v[len(v) // 2]:9.3f} {1e3 * v[-1]:9.3f}"


def clock(fn, prepare=lambda: None):
    out = []
    for _ in range(args.reps):
        prepare()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


B, R = args.batch, args.rank
model = build_model(dev, "bf16")
unet = model.model.diffusion_model
eng = unet.engine(dev)
g = torch.Generator().manual_seed(42)
x = torch.randn(B, 4, 64, 64, generator=g).to(dev)
t = torch.full((B,), 500, dtype=torch.long, device=dev)
ctx = torch.randn(2 * B * 16, 77, 768, generator=g).to(dev)
out = torch.empty(2 * B, 4, 64, 64, device=dev)
params = dict(unet.named_parameters())
pat = re.compile(r"\.(attn[12]\.to_[qkv]|attn[12]\.to_out\.0|ff\.net\.0\.proj|ff\.net\.2|proj_in|proj_out)\.weight$")
names = sorted(k[:-len(".weight")] for k in params if pat.search(k))


def adapter(seed):
    gg = torch.Generator(device=dev).manual_seed(seed)
    w = {}
    for n in names:
        p = params[n + ".weight"]
        up = torch.randn((p.shape[0], R) + (1,) * (p.dim() - 2), generator=gg, device=dev) * 0.02
        down = torch.randn((R,) + tuple(p.shape[1:]), generator=gg, device=dev) * 0.02
        w[n] = (up, down, float(R))
    return w


A, A2 = adapter(1), adapter(2)
n_el = sum(params[n + ".weight"].numel() for n in names)
say(f"LoRA switch at SD-1.5 widths: bf16, rank {R} on {len(names)} of the U-Net's {len(eng.tensor_table())} tensors "
    f"({n_el / 1e6:.1f} M of {sum(p.numel() for p in params.values()) / 1e6:.1f} M weights)")
say(f"device: {torch.cuda.get_device_name(0)}")
say()
say(f"    [ms]                                         best    median     worst   ({args.reps} runs, host clock to a device synchronise)")
unet.set_lora([(A, 1.0)])
flip = [A2, A]
say(f"(a) set_lora, another adapter on the same weights {stats(clock(lambda: unet.set_lora([(flip[0], 1.0)]), lambda: flip.reverse()))}")
say(f"    clear_lora (touched weights loaded plainly)   {stats(clock(unet.clear_lora, lambda: unet.set_lora([(A, 1.0)])))}")
unet.clear_lora()


def host_route(w):
    for n in names:
        p = params[n + ".weight"]
        up, down, alpha = w[n]
        merged = p.float().reshape(p.shape[0], -1) + lora_factor(1.0, alpha, R) * (up.reshape(p.shape[0], R) @ down.reshape(R, -1))
        eng.load_tensor(unet._ckpt_prefix + n + ".weight", merged.reshape(p.shape))


say(f"(b) torch merge on the device + load_tensor each   {stats(clock(lambda: host_route(A)))}")
say(f"(c) full sync_weights                              {stats(clock(unet.sync_weights))}")
say()

say(f"(d) the kernel alone, bf16, rank {R} (HIP events around {args.burst} launches, best of {args.reps}) beside itself with zero adapters")
for C_ in (320, 640, 1280):
    base = torch.randn(C_, C_, device=dev)
    ad = [(torch.randn(C_, R, device=dev), torch.randn(R, C_, device=dev), 0.01)]
    buf = torch.empty(C_, C_, device=dev, dtype=torch.bfloat16)
    res = {}
    for label, ads in (("merge", ad), ("plain", [])):
        best = float("inf")
        ops.lora_repack(base, ads, out=buf)
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.burst):
                ops.lora_repack(base, ads, out=buf)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, 1e3 * e0.elapsed_time(e1) / args.burst)
        res[label] = best
    say(f"    {C_:4d} x {C_:4d}: {res['merge']:7.1f} us with the adapter, {res['plain']:7.1f} us without "
        f"({2.0 * C_ * C_ * R / res['merge'] / 1e6:.2f} TFLOP/s fp32 FMA)")
say()


def fwd():
    eng.unet_forward_twin(x, t, out)


def burst():
    for _ in range(args.burst):
        fwd()


say(f"(e) one twin forward, Bf = {2 * B}, 64x64 ([ms] per forward over bursts of {args.burst}; alternating)")
res, counts, outs = {"base": [], "lora": []}, {}, {}
for rep in range(args.reps + 1):
    for label in ("base", "lora"):
        unet.set_lora([(A, 1.0)] if label == "lora" else [])
        eng.set_context(ctx, 2 * B, layerwise=True)
        fwd()
        _lib.plan_counts(reset=True)
        fwd()
        counts[label] = _lib.plan_counts(reset=True)
        outs[label] = out.clone()
        if rep:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            burst()
            torch.cuda.synchronize()
            res[label].append((time.perf_counter() - t0) / args.burst)
for label in ("base", "lora"):
    say(f"    {label:5s} {stats(res[label])}")
say(f"    launch counters equal: {'yes' if counts['base'] == counts['lora'] else 'NO'}; eps differs: {'yes' if not torch.equal(outs['base'], outs['lora']) else 'NO'}")
say(f"    af_gemm_plan_counts base: {counts['base']}")
say(f"    af_gemm_plan_counts lora: {counts['lora']}")
unet.clear_lora()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
