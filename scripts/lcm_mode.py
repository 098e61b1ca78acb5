#!/usr/bin/env python
"""What the LCM / TCD sampler costs, at BASELINE config 1's shape: SD-1.5 with synthetic weights (as bench.py builds them),
batch 8, 64x64 latents.

    (a) af_lcm_step (ONE launch: CFG combine, x0, the denoised sample D, re-noising with z generated in registers) beside the
        torch composition it replaces (randn and the element-wise lines of the update, one launch each, counted as they run) at
        n = 8*4*64*64: HIP events, best of --reps, one event pair around one call (less what an empty pair measures) and one
        pair around --burst back-to-back calls divided by their number.  With a given z the two are compared element by
        element (the kernel contracts its product-sums into fmaf, the composition rounds every product: not the same bits,
        the largest difference is reported beside max |result|); the kernel with z in registers against the kernel with
        af_philox_randn's tensor handed in must be the same bits.
    (b) bf16: wall time of LCMSampler.sample at S = 4 and 8 -- with classifier-free guidance (two legs per step, the LCM-LoRA
        use) and at guidance 1 (one leg, the use of a distilled checkpoint with its guidance-scale embedding), LCM and TCD --
        beside DDIMSampler.sample at S = --steps and DPMSolverSampler.sample at S = --dpm-steps (host clock around a call that
        ends in a device synchronise, best of --reps after one warm-up call; no VAE decode).

Synthetic weights: a consistency sampler needs consistency-distilled weights (an LCM checkpoint or an LCM-LoRA) to produce an
image at all.  None are available offline, so IMAGE QUALITY IS NOT MEASURED here; the numbers are cost only.

    python scripts/lcm_mode.py [--out profiles/lcm_<commit>.txt]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50, help="DDIM steps of the benchmark, for (b)")
ap.add_argument("--dpm-steps", dest="dpm_steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--burst", type=int, default=200)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib, ops  # noqa: E402
from adaface_amd.ldm.models.diffusion import lcm as L  # noqa: E402
from adaface_amd.noise import PhiloxNoise  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402
from ldm.models.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402
from ldm.models.diffusion.lcm import LCMSampler  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B, S, SD = args.batch, args.steps, args.dpm_steps
say(f"LCM / TCD sampling at config 1's shape: SD-1.5 synthetic weights, batch {B}, 64x64 latents")
say(f"device: {torch.cuda.get_device_name(0)}")
say("image quality needs real LCM / LCM-LoRA weights and is NOT measured: cost only")
say()

# ---------------------------------------------------------------- (a) the step kernel -------------------------------
lib = _lib.load()
shape = (B, 4, 64, 64)
n = B * 4 * 64 * 64
g = torch.Generator().manual_seed(1)
x, e_c, e_u = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
out_x, out_d = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
f32 =lambda v: float(np.float32(v))
GUIDE = 1.5
launched = [0]


def _op(fn, *a):
    launched[0] += 1
    return fn(*a)


def make(row):
    co = [f32(v) for v in row[L.COL_ALPHA:L.COL_S]]          # alpha, sigma, k_out, k_skip, c_x, c_0, c_n

    def fused(z=None, step=3):
        return ops.lcm_step(x, e_c, e_u, GUIDE, *co, noise=z, seed=42, step=step, x_next=out_x, d_out=out_d)

    def composition(z=None):
        """the update as torch lines, one launch per operator"""
        alpha, sigma, k_out, k_skip, c_x, c_0, c_n = co
        if z is None:
            z = _op(lambda: torch.randn(shape, device=dev))
        e = _op(torch.add, e_u, _op(torch.mul, _op(torch.sub, e_c, e_u), GUIDE))
        x0 = _op(torch.div, _op(torch.sub, x, _op(torch.mul, e, sigma)), alpha)
        d = _op(torch.add, _op(torch.mul, x0, k_out), _op(torch.mul, x, k_skip))
        xn = _op(torch.add, _op(torch.add, _op(torch.mul, x, c_x), _op(torch.mul, x0, c_0)), _op(torch.mul, z, c_n))
        return xn, d
    return fused, composition


def bracket(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / count


from adaface_amd.ldm.modules.diffusionmodules.util import make_beta_schedule  # noqa: E402
acp = np.cumprod(1.0 - np.asarray(make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012), dtype=np.float64))
table = L.lcm_schedule(acp, L.lcm_timesteps(4))
fused, composition = make(table[1])
for fn in (fused, composition):
    for _ in range(20):
        fn()
torch.cuda.synchronize()
launched[0] = 0
composition()
n_comp = launched[0]
before = ops.lcm_step_launches()
fused()
n_fused = ops.lcm_step_launches() - before
empty = lib.af_prof_event_overhead_us(_lib.stream_ptr(), 64)
single = {fn.__name__: min(bracket(fn, 1) for _ in range(args.reps * 8)) for fn in (fused, composition)}
burst = {"fused": [], "composition": []}
for _ in range(args.reps):                       # alternating, so a clock or neighbour drift hits both
    for fn in (fused, composition):
        burst[fn.__name__].append(bracket(fn, args.burst))
say(f"(a) one LCM step at n = {n} fp32 elements, guidance {GUIDE}, z generated (HIP events; an empty event pair measures {empty:.2f} us)")
for name, key, k in (("af_lcm_step, in-kernel noise", "fused", n_fused), ("torch composition (randn + update)", "composition", n_comp)):
    say(f"    {name:36s} {k:2d} launch(es); one call per event pair, best of {args.reps * 8}: {single[key]:7.2f} us "
        f"({single[key] - empty:7.2f} us less the empty pair);  {args.burst} calls per pair, best of {args.reps}: {min(burst[key]):7.2f} us per call")
say("    caveats: the fused figure is a bound on a kernel of a few microseconds, not its execution time: one call per pair adds the")
say("    dispatch and the events' own cost, many calls per pair run at the rate the host can enqueue them through ctypes.")
z = torch.randn(shape, generator=g).to(dev)
xn_f, d_f = (t.clone() for t in fused(z))
xn_c, d_c = composition(z)
for what, a, b in (("x_next", xn_f, xn_c), ("D", d_f, d_c)):
    diff = (a - b).abs().max().item()
    say(f"    given z, kernel vs composition, {what}: {100.0 * (a == b).float().mean().item():.1f} % of the elements the same bits, "
        f"largest |difference| {diff:.3e} = {diff / b.abs().max().item():.2e} of max |{what}| (fmaf against separately rounded products)")
xn_reg = fused(None, step=5)[0].clone()
zt = ops.philox_randn(B, 4 * 64 * 64, 42, 1, 5, device=dev).view(shape)
say(f"    z in registers vs af_philox_randn's tensor handed in: {'the same bits' if torch.equal(fused(zt)[0], xn_reg) else 'DIFFERENT BITS'}")
say()

# ---------------------------------------------------------------- (b) the samplers ----------------------------------
model = build_model(dev, "bf16")
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
c = model.get_learned_conditioning(synth_context(B, seed=100, device=dev))
uc = model.get_learned_conditioning(synth_context(B, seed=101, device=dev, shared=True))
RUNS = (("DDIM", DDIMSampler, S, dict(guidance_scale=[10.0, 4.0], eta=0.0)),
        ("DPM-Solver++(2M) logSNR", DPMSolverSampler, SD, dict(guidance_scale=[10.0, 4.0], skip_type="logSNR")),
        ("LCM, guidance 1.5 (two legs)", LCMSampler, 8, dict(guidance_scale=1.5)),
        ("LCM, guidance 1.5 (two legs)", LCMSampler, 4, dict(guidance_scale=1.5)),
        ("TCD gamma 0.3, guidance 1.5", LCMSampler, 4, dict(guidance_scale=1.5, tcd_gamma=0.3)),
        ("LCM, guidance 1 (one leg)", LCMSampler, 8, dict(guidance_scale=1.0)),
        ("LCM, guidance 1 (one leg)", LCMSampler, 4, dict(guidance_scale=1.0)),
        ("LCM, guidance 1 (one leg)", LCMSampler, 2, dict(guidance_scale=1.0)))


def run(cls, steps, kw):
    extra = dict(noise_source=PhiloxNoise(42)) if cls is LCMSampler else {}
    t0 = time.perf_counter()
    lat, _ = cls(model).sample(S=steps, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False,
                               unconditional_conditioning=uc, x_T=x_T, **kw, **extra)
    torch.cuda.synchronize()
    assert torch.isfinite(lat).all()
    return time.perf_counter() - t0


wall = []
for name, cls, steps, kw in RUNS:
    run(cls, steps, kw)                                  # warm-up
    wall.append(min(run(cls, steps, kw) for _ in range(args.reps)))
say(f"(b) bf16, batch {B}: wall time of one sample() call (host clock to device synchronise, best of {args.reps}; no VAE decode)")
base = wall[0]
for (name, cls, steps, kw), t in zip(RUNS, wall):
    say(f"    {name:30s} S = {steps:3d}: {1e3 * t:8.1f} ms   {B / t:7.2f} latents/s   {base / t:6.2f} x the rate of DDIM S = {S}")
say("    (synthetic weights: what these runs produce is not an image; the rates are the cost of the sampler at that step count)")
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
