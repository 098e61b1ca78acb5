#!/usr/bin/env python
"""What token merging (af_set_tome) costs and saves at BASELINE config 1's shape: SD-1.5 with synthetic weights
(as bench.py builds them), batch 8 -> CFG twin batch Bf = 16, 64x64 latents, bf16, annealed guidance [10, 4].

    (a) one twin forward at ratio 0 / 0.25 / 0.5 / 0.75 (max_downsample 1) and at 0.5 with max_downsample 2: host clock around
        --burst forwards that end in a device synchronise, best and spread of --reps rounds, the settings ALTERNATING within a
        round; conv / GEMM launches and all kernel launches of one forward.  With --parent-lib (the library of the parent
        commit, built from its checkout) a second handle on that library joins the rotation: ratio 0 must sit inside its spread.
    (b) kernel time of one forward per setting by profiling class: each of the six new kernels (its own class), the attention
        launches, the conv / GEMM launches (q/k/v and to_out at N' rows among them) and the LayerNorm launches.
    (c) DeepCache reuse steps (depth 2) with and without merging.
    (d) one sample() call, DDIM S = --steps and DPM-Solver++(2M) S = --dpm-steps, per setting; and the final latent's rms
        deviation from the un-merged run of the same sampler.
The deviation is measured on SYNTHETIC random weights: it is a mode deviation, not a quality figure.

    python scripts/tome_mode.py [--parent-lib /path/to/libadaface_hip.so] [--out profiles/tome_<commit>.txt]
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
ap.add_argument("--dpm-steps", dest="dpm_steps", type=int, default=20)
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
from ldm.models.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


B = args.batch
say(f"Token merging at config 1's shape: SD-1.5 synthetic weights, bf16, twin Bf = {2 * B}, 64x64 latents, guidance [10, 4]")
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


def conv_gemm(pc):
    return sum(pc[f"tile{i}"] for i in range(6)) + pc["halo"] + pc["fp8"] + pc["up_phase4"]


def all_launches(fn):
    lib.af_prof_reset()
    lib.af_prof_set_stride(1)
    lib.af_prof_enable(0xffff)              # (every class: the token-merging kernels have one each)
    fn()
    torch.cuda.synchronize()
    lib.af_prof_enable(0)
    n = 16
    ms, la, fl, by = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)()
    lib.af_prof_collect(n, ms, la, fl, by)
    return int(sum(la))


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
SETTINGS = [("off", 0.0, 1), ("0.25", 0.25, 1), ("0.5", 0.5, 1), ("0.75", 0.75, 1), ("0.5 md2", 0.5, 2)]
fwd = lambda: eng.unet_forward_twin(x_T, t, out)
# (a)-(c) drive the engine directly, on a context of their own that the parent's handle gets too; the samplers of (d) set theirs
ctx = torch.randn(2 * B * 16, 77, 768, generator=g).to(dev)
eng.set_context(ctx, 2 * B, layerwise=True)
object.__setattr__(unet, "_ctx_key", None)
legs = [(name, (lambda r=r, md=md: eng.set_tome(r, md)), fwd) for name, r, md in SETTINGS]
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
say(f"(a) one twin U-Net forward (host clock around {args.burst} forwards to a device synchronise, {args.reps} alternating rounds)")
say("    setting      best [ms]   median   worst    conv/GEMM launches   all kernel launches")
times = rotate(legs)
for name, prepare, fn in legs:
    prepare()
    v = times[name]
    if name == "parent":
        say(f"    {name:10s} {1e3 * v[0]:9.3f} {1e3 * v[len(v) // 2]:9.3f} {1e3 * v[-1]:9.3f}   (the parent commit's library, ratio unknown to it)")
        continue
    _lib.plan_counts(reset=True)
    fn()
    torch.cuda.synchronize()
    n_gemm = conv_gemm(_lib.plan_counts(reset=True))
    say(f"    {name:10s} {1e3 * v[0]:9.3f} {1e3 * v[len(v) // 2]:9.3f} {1e3 * v[-1]:9.3f}   {n_gemm:10d}   {all_launches(fn):14d}")
if args.parent_lib:
    a, p = times["off"], times["parent"]
    say(f"    ratio 0 inside the parent's spread [{1e3 * p[0]:.3f}, {1e3 * p[-1]:.3f}] ms: "
        f"{'yes' if p[0] <= a[len(a) // 2] <= p[-1] else 'NO'} (median {1e3 * a[len(a) // 2]:.3f} ms)")
    eng.set_tome(0.0)
    fwd()
    peng.unet_forward_twin(x_T, t, pout)
    say(f"    ratio 0 == the parent library's forward, bit for bit: {'yes' if torch.equal(out, pout) else 'NO'}")
eng.set_tome(0.0)
say()


# ---------------------------------------------------------------- (b) the kernels ------------------------------------
N_CLS = 16                                   # the classes of af_common.h in front of the FreeU ones (off here)
GEMM_CLS, ATTN_CLS, LN_CLS = (0, 5, 6, 7, 8, 9), 1, 3
TOME_CLS = (("rnorm", 10), ("match", 11), ("rank", 12), ("map", 13), ("merge", 14), ("unmerge", 15))


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


ovh = float(lib.af_prof_event_overhead_us(_lib.stream_ptr(), 200))
say(f"(b) kernel time of one twin forward by class, us (every launch between its own HIP events, {ovh:.2f} us per empty pair taken off;")
say(f"    best of {args.reps} forwards; in brackets the launches).  md 1: five merging blocks at 64x64, the first on the 8 shared samples")
say("    setting      rnorm        match         rank         map         merge       unmerge    | attention     conv/GEMM    layernorm")
for name, r, md in SETTINGS:
    eng.set_tome(r, md)
    fwd()
    best, la = None, None
    for _ in range(args.reps):
        us, la = by_class(fwd)
        best = us if best is None else [min(a, b) for a, b in zip(best, us)]
    cells = [f"{best[k]:7.1f} ({la[k]:2d})" if la[k] else "      - ( 0)" for _, k in TOME_CLS]
    say(f"    {name:8s} " + " ".join(cells) + f" | {best[ATTN_CLS]:7.1f} ({la[ATTN_CLS]:2d}) "
        f"{sum(best[k] for k in GEMM_CLS):8.1f} ({sum(la[k] for k in GEMM_CLS):3d}) {best[LN_CLS]:7.1f} ({la[LN_CLS]:2d})")
eng.set_tome(0.0)
say()

# ---------------------------------------------------------------- (c) DeepCache reuse steps --------------------------
say("(c) DeepCache reuse step, depth 2 (the 64x64 level only): best [ms] of the alternating rounds")
legs = []
for name, r, md in SETTINGS[:4]:
    def prepare(r=r, md=md):
        eng.set_tome(r, md)
        eng.unet_forward_cached(x_T, t, depth=2, mode="refresh", twin=True, out=out)
    legs.append((name, prepare, lambda: eng.unet_forward_cached(x_T, t, depth=2, mode="reuse", twin=True, out=out)))
times = rotate(legs)
for name, _, _ in legs:
    say(f"    {name:10s} {1e3 * times[name][0]:9.3f}   ({times['off'][0] / times[name][0]:.3f} x off)")
eng.set_tome(0.0)
say()


# ---------------------------------------------------------------- (d) the samplers -----------------------------------
def run(cls, steps):
    s = cls(model)
    t0 = time.perf_counter()
    lat, _ = s.sample(S=steps, **SAMPLE)
    torch.cuda.synchronize()
    return lat.clone(), time.perf_counter() - t0


def rms_dev(a, ref):
    return ((a - ref).double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


if not args.skip_samplers:
    say(f"(d) one sample() call, batch {B} (host clock to a device synchronise, best of {args.reps} after a warm-up call; no VAE decode).")
    say("    rms: the final latent against the un-merged run of the same sampler, SYNTHETIC weights -- a mode deviation, no quality claim")
    for name, cls, steps in (("DDIM", DDIMSampler, args.steps), ("DPM-Solver++(2M)", DPMSolverSampler, args.dpm_steps)):
        ref, base = None, None
        for sname, r, md in SETTINGS:
            model.set_token_merging(r, md)
            lat, _ = run(cls, steps)
            wall = min(run(cls, steps)[1] for _ in range(args.reps))
            assert torch.isfinite(lat).all(), (name, sname)
            if ref is None:
                ref, base = lat, wall
            say(f"    {name:17s} S = {steps:3d}  tome {sname:8s}: {1e3 * wall:8.1f} ms   {B / wall:6.2f} latents/s   {base / wall:5.3f} x off"
                f"   rms {rms_dev(lat, ref):.3e}")
    model.set_token_merging(0.0)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
