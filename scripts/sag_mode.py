#!/usr/bin/env python
"""What self-attention guidance (af_sag_set / af_sag_degrade) costs at BASELINE config 1's shape: SD-1.5 with
synthetic weights (as bench.py builds them), batch 8, 64x64 latents, bf16, annealed guidance [10, 4].

    (a) one U-Net forward: the twin forward (Bf = 16) without and with the attention-mass capture: host clock around --burst
        forwards that end in a device synchronise, best, median and worst of --reps rounds, the two variants ALTERNATING within a
        round in one process on one device; the calls of the mass kernels (a pair of launches each) per forward.
    (b) the two kernels alone, between HIP events around --burst calls, beside the torch composition each replaces: the mass of
        the middle block's q | k ([16, 64, 3 x 1280] bf16: an einsum, a softmax, a mean and a sum) and the degraded input on the
        real latent ([8, 4, 64, 64] fp32: a pad, a grouped convolution, a nearest upsample, a blend and two axpys); calls of each
        (the mass is two launches per call, the degrade one); the largest difference between kernel and composition.
    (c) one sample() call, DDIM S = 50 and DPM-Solver++(2M) S = 20, each without and with sag_scale 0.75; and the final latent's
        rms deviation from the run without.
The deviation is measured on SYNTHETIC random weights: it is a mode deviation, not a quality figure.

    python scripts/sag_mode.py [--out profiles/sag_<commit>.txt]
"""
import argparse
import math
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--burst", type=int, default=10)
ap.add_argument("--skip-samplers", dest="skip_samplers", action="store_true")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import ops  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402
from ldm.models.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B = args.batch
say(f"Self-attention guidance at config 1's shape: SD-1.5 synthetic weights, bf16, batch {B}, 64x64 latents, guidance [10, 4]")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

model = build_model(dev, "bf16")
unet = model.model.diffusion_model
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
c = model.get_learned_conditioning(synth_context(B, seed=100, device=dev))
uc = model.get_learned_conditioning(synth_context(B, seed=101, device=dev, shared=True))
SAMPLE = dict(conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False, guidance_scale=[10.0, 4.0],
              unconditional_conditioning=uc, eta=0.0, x_T=x_T)
DDIMSampler(model).sample(S=1, **SAMPLE)          # (builds the engine and uploads the weights)
eng = unet.engine(dev)
t = torch.full((B,), 500, dtype=torch.long, device=dev)
out2 = torch.empty(2 * B, 4, 64, 64, device=dev)
ctx2 = torch.randn(2 * B * 16, 77, 768, generator=g).to(dev)
object.__setattr__(unet, "_ctx_key", None)        # (the engine's context is set by hand below; the sampler of (c) sets its own)


def burst(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.burst):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.burst


def rotate(legs):
    """legs: [(name, prepare, fn)]; every round runs each leg's burst once, in order.  -> {name: sorted times}"""
    got = {name: [] for name, _, _ in legs}
    for name, prepare, fn in legs:
        prepare()
        fn()
    for _ in range(args.reps):
        for name, prepare, fn in legs:
            prepare()
            got[name].append(burst(fn))
    return {k: sorted(v) for k, v in got.items()}


def between_events(fn):
    """us per call: HIP events around --burst back-to-back calls, best of --reps"""
    fn()
    best = float("inf")
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.burst):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, 1e3 * e0.elapsed_time(e1) / args.burst)
    return best


# ---------------------------------------------------------------- (a) one forward ------------------------------------
eng.set_context(ctx2, 2 * B, layerwise=True)
fwd2 = lambda: eng.unet_forward_twin(x_T, t, out2)
legs = [("twin", lambda: eng.set_sag(False), fwd2), ("twin + capture", lambda: eng.set_sag(True), fwd2)]
say(f"(a) one U-Net forward (host clock around {args.burst} forwards to a device synchronise, {args.reps} alternating rounds)")
say("    variant            best [ms]   median    worst   x twin (best)   mass-kernel calls per forward")
times = rotate(legs)
for name, prepare, fn in legs:
    prepare()
    n0 = ops.sag_launches()["mass"]
    fn()
    v = times[name]
    say(f"    {name:16s} {1e3 * v[0]:9.3f} {1e3 * v[len(v) // 2]:9.3f} {1e3 * v[-1]:8.3f}   {v[0] / times['twin'][0]:8.3f}   "
        f"{ops.sag_launches()['mass'] - n0:14d}")
eng.set_sag(False)
tw, tc = times["twin"], times["twin + capture"]
cost = tc[len(tc) // 2] - tw[len(tw) // 2]
spread = max(tw[-1] - tw[0], tc[-1] - tc[0])
say(f"    the capture costs {1e3 * cost:.3f} ms (medians) against a run-to-run spread of {1e3 * spread:.3f} ms: "
    f"{'beyond the spread' if cost > spread else 'NOT beyond the spread'}")
say()

# ---------------------------------------------------------------- (b) the kernels ------------------------------------
HEADS, DH = 8, 160
Cq = HEADS * DH
qkv = torch.randn(2 * B, 64, 3 * Cq, generator=g).to(dev).to(torch.bfloat16)


def torch_mass():
    q = qkv[:, :, :Cq].reshape(2 * B, 64, HEADS, DH).permute(0, 2, 1, 3).float()
    k = qkv[:, :, Cq:2 * Cq].reshape(2 * B, 64, HEADS, DH).permute(0, 2, 1, 3).float()
    return (torch.einsum("bhid,bhjd->bhij", q, k) * DH ** -0.5).softmax(-1).mean(1).sum(1)


acp_t = 0.31
alpha, sigma = math.sqrt(acp_t), math.sqrt(1.0 - acp_t)
e_g = torch.randn(B, 4, 64, 64, generator=g).to(dev)
mass = ops.sag_mass(qkv[B:, :, :Cq], qkv[B:, :, Cq:2 * Cq], HEADS)
w = torch.tensor(ops.sag_taps(1.0), device=dev, dtype=torch.float32)
k2 = (w[:, None] * w[None, :]).expand(4, 1, 9, 9).contiguous()
x_deg = torch.empty_like(x_T)


def torch_degrade():
    x0 = (x_T - sigma * e_g) / alpha
    blur = F.conv2d(F.pad(x0, (4, 4, 4, 4), mode="reflect"), k2, groups=4)
    on = F.interpolate((mass > 1.0).view(B, 1, 8, 8).float(), scale_factor=8, mode="nearest").bool()
    return alpha * torch.where(on, blur, x0) + sigma * e_g


say(f"(b) the kernels alone (us per call: HIP events around {args.burst} back-to-back calls, best of {args.reps}) beside the torch")
say("    composition each replaces; calls counted by the library (mass: two launches per call, degrade: one)")
say("    operator                                    kernel [us]   torch [us]      calls   max |kernel - torch|")
n0 = ops.sag_launches()
km = ops.sag_mass(qkv[:, :, :Cq], qkv[:, :, Cq:2 * Cq], HEADS)
kd = ops.sag_degrade(x_T, e_g, mass, alpha, sigma, 1.0, out=x_deg)
n1 = ops.sag_launches()
t_km = between_events(lambda: ops.sag_mass(qkv[:, :, :Cq], qkv[:, :, Cq:2 * Cq], HEADS))
t_tm = between_events(torch_mass)
t_kd = between_events(lambda: ops.sag_degrade(x_T, e_g, mass, alpha, sigma, 1.0, out=x_deg))
t_td = between_events(torch_degrade)
say(f"    mass    [{2 * B}, 64, 8 x 160] bf16 q | k         {t_km:10.1f}   {t_tm:10.1f}   {n1['mass'] - n0['mass']:8d}   "
    f"{float((km - torch_mass()).abs().max()):.3e}")
say(f"    degrade [{B}, 4, 64, 64] fp32, {float((mass > 1).float().mean()):.2f} of cells on   {t_kd:10.1f}   {t_td:10.1f}   "
    f"{n1['degrade'] - n0['degrade']:8d}   {float((kd - torch_degrade()).abs().max()):.3e}")
say()


# ---------------------------------------------------------------- (c) the samplers -----------------------------------
def run(cls, steps, **kw):
    s = cls(model)
    t0 = time.perf_counter()
    lat, _ = s.sample(S=steps, **SAMPLE, **kw)
    torch.cuda.synchronize()
    return lat.clone(), time.perf_counter() - t0


def rms_dev(a, ref):
    return ((a - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


if not args.skip_samplers:
    say(f"(c) one sample() call, batch {B} (host clock to a device synchronise, best of {args.reps} after a warm-up call; no VAE decode).")
    say("    rms: the final latent against the run without, SYNTHETIC weights -- a mode deviation, no quality claim")
    for sname, cls, steps in (("DDIM", DDIMSampler, 50), ("DPM-Solver++(2M)", DPMSolverSampler, 20)):
        ref, base = None, None
        for vname, kw in (("off", {}), ("SAG 0.75", dict(sag_scale=0.75))):
            lat, _ = run(cls, steps, **kw)
            wall = min(run(cls, steps, **kw)[1] for _ in range(args.reps))
            assert torch.isfinite(lat).all(), (sname, vname)
            if ref is None:
                ref, base = lat, wall
            say(f"    {sname:17s} S = {steps:3d}  {vname:9s}: {1e3 * wall:8.1f} ms   {B / wall:6.2f} latents/s   {wall / base:5.3f} x off"
                f"   rms {rms_dev(lat, ref):.3e}")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
