#!/usr/bin/env python
"""What perturbed-attention guidance and guidance rescale (af_set_pag / af_unet_forward_pag / af_guidance) cost at
BASELINE config 1's shape: SD-1.5 with synthetic weights (as bench.py builds them), batch 8, 64x64 latents, bf16, annealed
guidance [10, 4].

    (a) one U-Net forward: the twin forward (Bf = 16) and the PAG forward (Bf = 24) with knob pag_share_prefix 0 and 1, for
        the layers `mid` and `mid + up.blocks.1`: host clock around --burst forwards that end in a device synchronise, best,
        median and worst of --reps rounds, the variants ALTERNATING within a round in one process on one device.
    (b) a DeepCache reuse step at depth 3, twin and PAG (mid).
    (c) the guidance kernels on the real latent ([8, 4, 64, 64] fp32): by profiling class and between HIP events, with and
        without rescale.
    (d) one sample() call, DDIM S = 50 and DPM-Solver++(2M) S = 20, each without and with PAG 3.0 on `mid` + rescale 0.7; and
        the final latent's rms deviation from the run without.
The deviation is measured on SYNTHETIC random weights: it is a mode deviation, not a quality figure.

    python scripts/pag_mode.py [--out profiles/pag_<commit>.txt]
"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import torch

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

from adaface_amd import _lib, ops  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402
from ldm.models.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B = args.batch
say(f"PAG and guidance rescale at config 1's shape: SD-1.5 synthetic weights, bf16, batch {B}, 64x64 latents, guidance [10, 4]")
say(f"device: {torch.cuda.get_device_name(0)}")
say()

model = build_model(dev, "bf16")
unet = model.model.diffusion_model
g = torch.Generator().manual_seed(42)
x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
c = model.get_learned_conditioning(synth_context(B, seed=100, device=dev))
uc = model.get_learned_conditioning(synth_context(B, seed=101, device=dev, shared=True))
lib = _lib.load()
SAMPLE = dict(conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False, guidance_scale=[10.0, 4.0],
              unconditional_conditioning=uc, eta=0.0, x_T=x_T)
DDIMSampler(model).sample(S=1, **SAMPLE)          # (builds the engine and uploads the weights)
eng = unet.engine(dev)
t = torch.full((B,), 500, dtype=torch.long, device=dev)
out2 = torch.empty(2 * B, 4, 64, 64, device=dev)
out3 = torch.empty(3 * B, 4, 64, 64, device=dev)
N_CLS = 22                                        # AF_K_COUNT (af_common.h)
ctx_c = torch.randn(B * 16, 77, 768, generator=g).to(dev)
ctx_u = torch.randn(B * 16, 77, 768, generator=g).to(dev)
ctx2, ctx3 = torch.cat([ctx_c, ctx_u]), torch.cat([ctx_c, ctx_u, ctx_c])
object.__setattr__(unet, "_ctx_key", None)        # (the engine's context is set by hand below; the sampler of (d) sets its own)


def by_class(fn):
    """(us, launches) per profiling class of one call of fn: every launch between its own pair of HIP events, the empty
    pair's time taken off"""
    lib.af_prof_reset()
    lib.af_prof_set_stride(1)
    lib.af_prof_enable((1 << N_CLS) - 1)
    fn()
    torch.cuda.synchronize()
    lib.af_prof_enable(0)
    ms, la, fl, by = (C.c_double * N_CLS)(), (C.c_int64 * N_CLS)(), (C.c_double * N_CLS)(), (C.c_double * N_CLS)()
    lib.af_prof_collect(N_CLS, ms, la, fl, by)
    return [1e3 * ms[k] - ovh * la[k] for k in range(N_CLS)], [int(v) for v in la]


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


def as_twin():
    eng.set_pag(())
    eng.set_context(ctx2, 2 * B, layerwise=True)


def as_pag(layers, share):
    def prepare():
        eng.set_pag(layers)
        _lib.set_knob("pag_share_prefix", share)
        eng.set_context(ctx3, 3 * B, layerwise=True)
    return prepare


ovh = float(lib.af_prof_event_overhead_us(_lib.stream_ptr(), 200))
LAYERS = (("mid", ("mid",)), ("mid+up1", ("mid", "up.blocks.1")))

# ---------------------------------------------------------------- (a) one forward ------------------------------------
fwd2 = lambda: eng.unet_forward_twin(x_T, t, out2)
fwd3 = lambda: eng.unet_forward_pag(x_T, t, out3)
legs = [("twin", as_twin, fwd2)]
for lname, layers in LAYERS:
    for share in (0, 1):
        legs.append((f"pag {lname} share {share}", as_pag(layers, share), fwd3))
say(f"(a) one U-Net forward (host clock around {args.burst} forwards to a device synchronise, {args.reps} alternating rounds)")
say("    variant                  best [ms]   median    worst   x twin (best)   two-leg input blocks   all kernel launches")
times = rotate(legs)
for name, prepare, fn in legs:
    prepare()
    v = times[name]
    two = eng.pag_plan()["two_leg_blocks"] if name != "twin" else 0
    say(f"    {name:22s} {1e3 * v[0]:9.3f} {1e3 * v[len(v) // 2]:9.3f} {1e3 * v[-1]:8.3f}   {v[0] / times['twin'][0]:8.3f}   {two:14d}   "
        f"{sum(by_class(fn)[1]):14d}")
_lib.reset_knobs()
tw = times["twin"]
say(f"    run-to-run spread of the twin forward: {1e3 * (tw[-1] - tw[0]):.3f} ms")
for lname, _ in LAYERS:
    s0, s1 = times[f"pag {lname} share 0"], times[f"pag {lname} share 1"]
    gain = s0[len(s0) // 2] - s1[len(s1) // 2]
    spread = max(s0[-1] - s0[0], s1[-1] - s1[0])
    say(f"    {lname}: sharing saves {1e3 * gain:.3f} ms (medians) against a spread of {1e3 * spread:.3f} ms: "
        f"{'beyond the spread' if gain > spread else 'NOT beyond the spread'}; without sharing {s0[0] / tw[0]:.3f} x twin "
        f"(the limit the issue expects: 1.5 x)")
say()

# ---------------------------------------------------------------- (b) DeepCache reuse steps --------------------------
say("(b) DeepCache reuse step, depth 3: best [ms] of the alternating rounds")


def refresh_twin():
    as_twin()
    eng.unet_forward_cached(x_T, t, depth=3, mode="refresh", twin=True, out=out2)


def refresh_pag():
    as_pag(("mid",), 1)()
    eng.unet_forward_cached(x_T, t, depth=3, mode="refresh", twin="pag", out=out3)


legs = [("twin", refresh_twin, lambda: eng.unet_forward_cached(x_T, t, depth=3, mode="reuse", twin=True, out=out2)),
        ("pag mid", refresh_pag, lambda: eng.unet_forward_cached(x_T, t, depth=3, mode="reuse", twin="pag", out=out3))]
times = rotate(legs)
for name, _, _ in legs:
    say(f"    {name:10s} {1e3 * times[name][0]:9.3f}   ({times[name][0] / times['twin'][0]:.3f} x twin)")
_lib.reset_knobs()
eng.set_pag(())
say()

# ---------------------------------------------------------------- (c) the guidance kernels ---------------------------
say(f"(c) af_guidance on [{B}, 4, 64, 64] fp32 (cond, uncond, perturbed -> out), us: by profiling class ({ovh:.2f} us per empty event")
say(f"    pair taken off, best of {args.reps}; in brackets the launches) and the whole call between two HIP events")
e3 = torch.randn(3 * B, 4, 64, 64, generator=g).to(dev)
gout = torch.empty(B, 4, 64, 64, device=dev)
say("    rescale     statistics     apply / combine    whole call")
for phi in (0.0, 0.7):
    call = lambda: ops.guidance(e3[:B], e3[B:2 * B], e3[2 * B:], 7.5, 3.0, phi, out=gout)
    call()
    best, la = None, None
    for _ in range(args.reps):
        us, la = by_class(call)
        best = us if best is None else [min(a, b) for a, b in zip(best, us)]
    whole = float("inf")
    for _ in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        whole = min(whole, 1e3 * e0.elapsed_time(e1))
    cells = [f"{best[k]:7.1f} ({la[k]:d})" if la[k] else "      - (0)" for k in (20, 21)]
    say(f"    {phi:4.1f}      {cells[0]}      {cells[1]}      {whole:9.1f}")
say()


# ---------------------------------------------------------------- (d) the samplers -----------------------------------
def run(cls, steps, **kw):
    s = cls(model)
    t0 = time.perf_counter()
    lat, _ = s.sample(S=steps, **SAMPLE, **kw)
    torch.cuda.synchronize()
    return lat.clone(), time.perf_counter() - t0


def rms_dev(a, ref):
    return ((a - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


if not args.skip_samplers:
    say(f"(d) one sample() call, batch {B} (host clock to a device synchronise, best of {args.reps} after a warm-up call; no VAE decode).")
    say("    rms: the final latent against the run without, SYNTHETIC weights -- a mode deviation, no quality claim")
    for sname, cls, steps in (("DDIM", DDIMSampler, 50), ("DPM-Solver++(2M)", DPMSolverSampler, 20)):
        ref, base = None, None
        for vname, kw in (("off", {}), ("rescale 0.7", dict(guidance_rescale=0.7)), ("PAG 3.0 mid + rescale 0.7", dict(pag_scale=3.0, guidance_rescale=0.7))):
            model.set_pag(("mid",) if "pag_scale" in kw else ())
            lat, _ = run(cls, steps, **kw)
            wall = min(run(cls, steps, **kw)[1] for _ in range(args.reps))
            assert torch.isfinite(lat).all(), (sname, vname)
            if ref is None:
                ref, base = lat, wall
            say(f"    {sname:17s} S = {steps:3d}  {vname:26s}: {1e3 * wall:8.1f} ms   {B / wall:6.2f} latents/s   {wall / base:5.3f} x off"
                f"   rms {rms_dev(lat, ref):.3e}")
    model.set_pag(())
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
