#!/usr/bin/env python
"""What FreeU (af_set_freeu) costs at BASELINE config 1's shape: SD-1.5 with synthetic weights (as bench.py builds
them), batch 8 -> CFG twin batch Bf = 16, 64x64 latents, bf16, annealed guidance [10, 4].

    (a) one twin forward off / version 1 / version 2 (the published SD-1.5 values): host clock around --burst forwards that end
        in a device synchronise, best and spread of --reps rounds, the settings ALTERNATING within a round; all kernel launches
        of one forward.  With --parent-lib (the library of the parent commit, built from its checkout) a second handle on that
        library joins the rotation: off must be no slower than its spread and return its bits.
    (b) kernel time of one forward by profiling class: each of the four new kernels (its own class).  Beside the chunked-form
        kernels (the 32x32 and 64x64 sites) a strided device copy of the bytes they move: per site, [Bf H W][Cs] read for the
        sums and [Bf H W][Ch / 2 + Cs] read and written for the apply pass, out of and into rows of pitch Ch + Cs.
    (c) a DeepCache reuse step at depth 3 (the kept concatenation is site 9: its skip alone is filtered).
    (d) one sample() call, DDIM S = --steps, per setting; and the final latent's rms deviation from the FreeU-off run.
The deviation is measured on SYNTHETIC random weights: it is a mode deviation, not a quality figure.

    python scripts/freeu_mode.py [--parent-lib /path/to/libadaface_hip.so] [--out profiles/freeu_<commit>.txt]
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
ap.add_argument("--steps", type=int, default=50, help="DDIM steps of the benchmark")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--burst", type=int, default=10)
ap.add_argument("--parent-lib", dest="parent_lib", type=str, default=None)
ap.add_argument("--skip-samplers", dest="skip_samplers", action="store_true")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

from adaface_amd import _lib  # noqa: E402
from adaface_amd.engine import Engine  # noqa: E402
from adaface_amd.synth import synth_context  # noqa: E402
from bench import build_model  # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B = args.batch
say(f"FreeU at config 1's shape: SD-1.5 synthetic weights, bf16, twin Bf = {2 * B}, 64x64 latents, guidance [10, 4]")
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
# one sampler step sets the engine's context for the twin batch exactly as a run does
DDIMSampler(model).sample(S=1, **SAMPLE)
eng = unet.engine(dev)
t = torch.full((B,), 500, dtype=torch.long, device=dev)
out = torch.empty(2 * B, 4, 64, 64, device=dev)
N_CLS = 20                                   # AF_K_COUNT (af_common.h)
FREEU_CLS = (("mean", 16), ("sums", 17), ("apply", 18), ("small", 19))
SETTINGS = [("off", (0, 1.0, 1.0, 1.0, 1.0)), ("v1", (1, 1.2, 1.4, 0.9, 0.2)), ("v2", (2, 1.3, 1.4, 0.9, 0.2))]


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


# ---------------------------------------------------------------- (a) one forward ------------------------------------
fwd = lambda: eng.unet_forward_twin(x_T, t, out)
# (a)-(c) drive the engine directly, on a context of their own that the parent's handle gets too; the sampler of (d) sets its own
ctx = torch.randn(2 * B * 16, 77, 768, generator=g).to(dev)
eng.set_context(ctx, 2 * B, layerwise=True)
object.__setattr__(unet, "_ctx_key", None)
legs = [(name, (lambda st=st: eng.set_freeu(*st)), fwd) for name, st in SETTINGS]
if args.parent_lib:
    plib = C.CDLL(args.parent_lib)
    for name, res, argt in _lib._SIGS:
        if hasattr(plib, name):
            getattr(plib, name).restype, getattr(plib, name).argtypes = res, argt
    mine, _lib._lib = _lib._lib, plib
    try:
        peng = Engine(dtype="bf16", device=0, **unet._engine_kwargs())
    finally:
        _lib._lib = mine
    sd = unet.state_dict()
    for name in peng.tensor_table():
        peng.load_tensor(name, sd[name[len(unet._ckpt_prefix):] if name.startswith(unet._ckpt_prefix) else name])
    peng.set_context(ctx, 2 * B, layerwise=True)
    pout = torch.empty_like(out)
    legs.insert(1, ("parent", lambda: None, lambda: peng.unet_forward_twin(x_T, t, pout)))
ovh = float(lib.af_prof_event_overhead_us(_lib.stream_ptr(), 200))
say(f"(a) one twin U-Net forward (host clock around {args.burst} forwards to a device synchronise, {args.reps} alternating rounds)")
say("    setting      best [ms]   median   worst    all kernel launches")
times = rotate(legs)
for name, prepare, fn in legs:
    prepare()
    v = times[name]
    if name == "parent":
        say(f"    {name:10s} {1e3 * v[0]:9.3f} {1e3 * v[len(v) // 2]:9.3f} {1e3 * v[-1]:9.3f}   (the parent commit's library)")
        continue
    say(f"    {name:10s} {1e3 * v[0]:9.3f} {1e3 * v[len(v) // 2]:9.3f} {1e3 * v[-1]:9.3f}   {sum(by_class(fn)[1]):10d}")
if args.parent_lib:
    a, p = times["off"], times["parent"]
    say(f"    off no slower than the parent's spread [{1e3 * p[0]:.3f}, {1e3 * p[-1]:.3f}] ms: "
        f"{'yes' if a[len(a) // 2] <= p[-1] else 'NO'} (median {1e3 * a[len(a) // 2]:.3f} ms)")
    eng.set_freeu(0)
    fwd()
    peng.unet_forward_twin(x_T, t, pout)
    say(f"    off == the parent library's forward, bit for bit: {'yes' if torch.equal(out, pout) else 'NO'}")
eng.set_freeu(0)
say()

# ---------------------------------------------------------------- (b) the kernels ------------------------------------
say(f"(b) kernel time of one twin forward by class, us (every launch between its own HIP events, {ovh:.2f} us per empty pair taken off;")
say(f"    best of {args.reps} forwards; in brackets the launches)")
say("    setting       mean          sums          apply         small")
best_of = {}
for name, st in SETTINGS:
    eng.set_freeu(*st)
    fwd()
    best, la = None, None
    for _ in range(args.reps):
        us, la = by_class(fwd)
        best = us if best is None else [min(a, b) for a, b in zip(best, us)]
    best_of[name] = best
    cells = [f"{best[k]:7.1f} ({la[k]:2d})" if la[k] else "      - ( 0)" for _, k in FREEU_CLS]
    say(f"    {name:8s} " + "  ".join(cells))
eng.set_freeu(0)
# the chunked sites' bytes as strided device copies (torch), one site after the other, best of --reps
sites = eng.freeu_sites()
shapes = {}   # output block j -> map side: 8, 8, 8, 16, 16, 16, 32, 32, 32, 64 for SD-1.5 at 64x64
side, up_after = 8, (2, 5, 8)
for j in range(12):
    shapes[j] = side
    if j in up_after:
        side *= 2
chunked = [(j, Ch, Cs, shapes[j]) for j, Ch, Cs, _ in sites if shapes[j] * shapes[j] > 256]
bufs = [(torch.empty(2 * B * s * s, Ch + Cs, device=dev, dtype=torch.bfloat16).normal_(), Ch, Cs) for _, Ch, Cs, s in chunked]


def copy_time(fn):
    best = float("inf")
    for _ in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, 1e3 * e0.elapsed_time(e1))
    return best


sums_scratch = [torch.empty(buf.shape[0], Cs, device=dev, dtype=torch.bfloat16) for buf, Ch, Cs in bufs]
t_sums = copy_time(lambda: [dst.copy_(buf[:, Ch:]) for (buf, Ch, Cs), dst in zip(bufs, sums_scratch)])
twins = [torch.empty_like(buf) for buf, _, _ in bufs]


def apply_copy():
    for (buf, Ch, Cs), dst in zip(bufs, twins):
        dst[:, :Ch // 2].copy_(buf[:, :Ch // 2])
        dst[:, Ch:].copy_(buf[:, Ch:])


t_apply = copy_time(apply_copy)
gb_sums = sum(buf.shape[0] * Cs * 2 for buf, Ch, Cs in bufs) / 1e9
gb_apply = sum(2 * buf.shape[0] * (Ch // 2 + Cs) * 2 for buf, Ch, Cs in bufs) / 1e9
say(f"    chunked sites {[j for j, *_ in chunked]}: sums read {gb_sums:.3f} GB, apply reads and writes {gb_apply:.3f} GB")
say(f"    strided torch copies of the same bytes (events, best of {args.reps + 1}): the skips out of their rows {t_sums:.1f} us "
    f"(writes them too); the touched columns row to row {t_apply:.1f} us")
say(f"    v1: sums {best_of['v1'][17]:.1f} us = {best_of['v1'][17] / t_sums:.2f} x that copy; apply {best_of['v1'][18]:.1f} us = "
    f"{best_of['v1'][18] / t_apply:.2f} x that copy")
del bufs, twins, sums_scratch
say()

# ---------------------------------------------------------------- (c) DeepCache reuse steps --------------------------
say("(c) DeepCache reuse step, depth 3 (the kept concatenation is FreeU site 9): best [ms] of the alternating rounds")
legs = []
for name, st in SETTINGS:
    def prepare(st=st):
        eng.set_freeu(*st)
        eng.unet_forward_cached(x_T, t, depth=3, mode="refresh", twin=True, out=out)
    legs.append((name, prepare, lambda: eng.unet_forward_cached(x_T, t, depth=3, mode="reuse", twin=True, out=out)))
times = rotate(legs)
for name, _, _ in legs:
    say(f"    {name:10s} {1e3 * times[name][0]:9.3f}   ({times[name][0] / times['off'][0]:.3f} x off)")
eng.set_freeu(0)
say()


# ---------------------------------------------------------------- (d) the sampler ------------------------------------
def run(steps):
    s = DDIMSampler(model)
    t0 = time.perf_counter()
    lat, _ = s.sample(S=steps, **SAMPLE)
    torch.cuda.synchronize()
    return lat.clone(), time.perf_counter() - t0


def rms_dev(a, ref):
    return ((a - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


if not args.skip_samplers:
    say(f"(d) one sample() call, batch {B} (host clock to a device synchronise, best of {args.reps} after a warm-up call; no VAE decode).")
    say("    rms: the final latent against the FreeU-off run, SYNTHETIC weights -- a mode deviation, no quality claim")
    ref, base = None, None
    for sname, st in SETTINGS:
        model.set_freeu(*st)
        lat, _ = run(args.steps)
        wall = min(run(args.steps)[1] for _ in range(args.reps))
        assert torch.isfinite(lat).all(), sname
        if ref is None:
            ref, base = lat, wall
        say(f"    DDIM S = {args.steps:3d}  freeu {sname:4s}: {1e3 * wall:8.1f} ms   {B / wall:6.2f} latents/s   {wall / base:5.3f} x off"
            f"   rms {rms_dev(lat, ref):.3e}")
    model.set_freeu(0)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
