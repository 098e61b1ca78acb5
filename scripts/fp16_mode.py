#!/usr/bin/env python
"""What the fp16 compute mode costs and what it buys, at BASELINE config 1's shape: SD-1.5 with synthetic weights (as
bench.py builds them), batch 8 -> CFG batch Bf = 16, 64x64 latents, annealed guidance [10, 4].

Timed (HIP events around af_unet_forward_twin, best and median of --reps after --warmup):
    (a) fp16 mode                     the four-wave kernels on v_mfma_f32_32x32x16_f16
    (b) f32 mode                      the same kernels on v_mfma_f32_32x32x2_f32
    (c) bf16 mode as shipped          eight-wave kernels, fusions, packed cross-attention operands
    (d) bf16 mode, every bf16-only kernel switched off through its knob: the four-wave kernels (a) runs, on the BF16 MFMA.
        The F16 MFMA takes the BF16 MFMA's cycles, so (a) and (d) should agree within run-to-run noise.
Deviation from the f32 mode of the same batch, as max-abs / max|.| and rms / rms:
    per forward (the eps of the timed forward) and the final latent after --steps DDIM steps, for fp16 and for bf16.
The launch counters of each timed forward and its kernel time by class (HIP-event brackets around every launch of one more
forward) are printed beside it: which kernels ran, and where two modes that should cost the same differ.

    python scripts/fp16_mode.py [--steps 50] [--out profiles/fp16_mode_<commit>.txt]
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402

# every kernel or fusion that exists for bf16 storage only, by the knob that switches it off
BF16_ONLY_OFF = {"gemm_pp": 0, "conv_halo8": 0, "geglu_rowpanel": 0, "gemm_m128": 0, "attn_ring": 0, "attn_short": 0,
                 "xattn_fused": 0, "conv_attn_short": 0, "ln_fuse": 0, "gn_producer": 0, "gn_consumer": 0, "conv_up_phase4": 0}
BF16_ONLY_COUNTERS = ("tile4", "tile5", "halo8", "rowpanel", "up_phase4", "gn_producer", "gn_consumer", "attn_short", "xattn_fused",
                      "conv_attn_short", "ln_consumer", "ln_producer", "fp8")

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B, S = args.batch, args.steps
model = build_model(dev, "f32")
unet = model.model.diffusion_model
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
c_emb = synth_context(B, seed=100, device=dev)
uc_emb = synth_context(B, seed=101, device=dev, shared=True)
t0 = torch.full((B,), 901, dtype=torch.long, device=dev)
ctx2 = torch.cat([c_emb, uc_emb])


def rebuild(mode):
    """A fresh engine in `mode` (the knobs are read when a launch is planned and when weights are folded at load)."""
    unet.set_compute_dtype("f32" if mode != "f32" else "bf16")
    model.set_compute_dtype(mode)


def chain():
    c, uc = model.get_learned_conditioning(c_emb), model.get_learned_conditioning(uc_emb)
    lat, _ = DDIMSampler(model).sample(S=S, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False, guidance_scale=[10.0, 4.0],
                                       unconditional_conditioning=uc, eta=0.0, x_T=x_T)
    torch.cuda.synchronize()
    return lat.clone()


def timed_forward():
    """-> (eps [2B, 4, 64, 64], best ms, median ms, launch counters of ONE forward, per-class kernel ms of one forward)"""
    eng = unet.engine(dev)
    eng.set_context(ctx2, 2 * B, layerwise=True)
    object.__setattr__(unet, "_ctx_key", None)            # (the module's context cache no longer describes the engine)
    for _ in range(args.warmup):
        eps = eng.unet_forward_twin(x_T, t0)
    torch.cuda.synchronize()
    _lib.plan_counts(reset=True)
    eps = eng.unet_forward_twin(x_T, t0)
    torch.cuda.synchronize()
    pc = _lib.plan_counts(reset=True)
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eps = eng.unet_forward_twin(x_T, t0)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    # per-class kernel time of one more forward (HIP-event brackets around every launch: slows the forward, classes comparable)
    lib = _lib.load()
    lib.af_prof_reset()
    lib.af_prof_set_stride(1)
    lib.af_prof_enable(0x3ff)
    eng.unet_forward_twin(x_T, t0)
    torch.cuda.synchronize()
    lib.af_prof_enable(0)
    n = 10
    cms, cla, cfl, cby = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)()
    _lib.check(lib.af_prof_collect(n, cms, cla, cfl, cby), "af_prof_collect")
    lib.af_prof_reset()
    names = ["four-wave gemm/conv", "attention", "groupnorm", "layernorm", "other", "pp160_gather", "pp160_plain", "pp128", "fp8", "halo8"]
    cls = ", ".join(f"{names[i]} {cms[i]:.2f} ({cla[i]})" for i in range(n) if cla[i])
    return eps.clone(), ms[0], ms[len(ms) // 2], pc, cls


def dev_of(a, ref):
    d = (a - ref).double()
    return d.abs().max().item() / ref.abs().max().item(), (d.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


say(f"fp16 mode at config 1's shape: SD-1.5 synthetic weights, Bf = {2 * B}, 64x64 latents, {S} DDIM steps, guidance [10, 4]")
say(f"device: {torch.cuda.get_device_name(0)}; forward = af_unet_forward_twin, HIP events, {args.warmup} warm-up + {args.reps} timed")
say()
res = {}
for tag, mode, knobs in (("b", "f32", None), ("a", "fp16", None), ("c", "bf16", None), ("d", "bf16", BF16_ONLY_OFF)):
    _lib.reset_knobs()
    for k, v in (knobs or {}).items():
        _lib.set_knob(k, v)
    rebuild(mode)
    lat = chain() if knobs is None else None
    eps, best, med, pc, cls = timed_forward()
    assert torch.isfinite(eps).all() and (lat is None or torch.isfinite(lat).all()), mode
    res[tag] = (eps, lat, best, med, pc)
    only = {k: pc[k] for k in BF16_ONLY_COUNTERS if pc[k]}
    four = {k: pc[k] for k in ("tile0", "tile1", "tile2", "tile3", "halo", "splitk")}
    name = {"a": "fp16 mode", "b": "f32 mode", "c": "bf16 mode as shipped", "d": "bf16 mode, bf16-only kernels off"}[tag]
    say(f"({tag}) {name:34s} twin forward best {best:8.3f} ms  median {med:8.3f} ms   ({2 * B / 2 / (best * 1e-3) / S:6.2f} img/s of UNet time at {S} steps)")
    say(f"      four-wave launches {four}")
    say(f"      bf16-only launches {only if only else 'none'}")
    say(f"      kernel ms by class (launches), every launch bracketed: {cls}")
_lib.reset_knobs()
say()
ta, tb, tc, td = (res[k][2] for k in "abcd")
say(f"(b) / (a) = {tb / ta:.2f}x   f32 forward time over fp16 forward time (the mode's reason to exist: must be > 1)")
say(f"(a) / (d) = {ta / td:.3f}    fp16 over bf16 on the same four-wave kernels (expected 1 within noise)")
say(f"(d) / (c) = {td / tc:.2f}x   what the bf16-only kernels and fusions are worth; (d) - (c) = {td - tc:.3f} ms per forward")
say(f"(a) / (c) = {ta / tc:.2f}x   fp16 over bf16 as shipped")
say()
e32, l32 = res["b"][0], res["b"][1]
say("deviation from the f32 mode of the same batch        max-abs / max|.|    rms / rms")
for tag, name in (("a", "fp16"), ("c", "bf16"), ("d", "bf16, bf16-only kernels off")):
    m, r = dev_of(res[tag][0], e32)
    say(f"  per forward (eps, t = 901)  {name:28s} {m:10.3e}      {r:10.3e}")
for tag, name in (("a", "fp16"), ("c", "bf16")):
    m, r = dev_of(res[tag][1], l32)
    say(f"  final latent, {S:3d} steps      {name:28s} {m:10.3e}      {r:10.3e}")
ma, ra = dev_of(res["a"][1], l32)
mc, rc = dev_of(res["c"][1], l32)
fa, fra = dev_of(res["a"][0], e32)
fc, frc = dev_of(res["c"][0], e32)
say(f"  bf16 / fp16: per forward max-abs {fc / fa:.1f}x  rms {frc / fra:.1f}x;  {S}-step final latent max-abs {mc / ma:.1f}x  rms {rc / ra:.1f}x")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
