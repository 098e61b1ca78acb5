#!/usr/bin/env python
"""Headline benchmark: 512x512 images/sec @ 50 DDIM steps, batch 8 per GPU (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload config1|config2|config3] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch: DDIMSampler.sample (50 steps x CFG-doubled UNet forward
at Bf=16 on 4x64x64 latents with a [256,77,768] layerwise context) + decode_first_stage to 8 uint8 512x512
frames, through the drop-in classes (ldm.models.diffusion.ddim.DDIMSampler, LatentDiffusion.apply_model,
AutoencoderKL.decode) and the C ABI underneath.  Inputs are resident in HBM before the timed region.

A plain run does what the headline needs and nothing more: it sets up, warms up, times the steps (with the sampled
HIP-event brackets behind `kernels` / `roofline` unless --no-kernel-timing), writes --dump-outputs and prints the line.
--full adds the legs that cost time of their own: the device clock probe before the warm-up, the untimed f32 parity
leg with its bar (exit code 3 if exceeded) and the CPU baseline.  In a plain run their fields are null, and so is
`roofline.frac_of_device_mfma_loop`, which divides by the clock probe.  The serving leg needs its own --serving-leg.

Multi-GPU: independent samples, one process per GPU, ONE RCCL all-gather of the decoded uint8 frames
per step.  `--gpus N` without a launcher (no WORLD_SIZE / RANK in the environment) starts the N ranks itself, as
fresh child processes under torch.distributed.run, before this process has touched the GPU; the JSON line's
`n_gpus` is the number of ranks the process group actually connected, and the run fails if that is not N.

Workloads (BASELINE.json `configs`, 0-based):
  config1 (default)  SD v1.5 512x512, 50 steps, batch 8 per GPU, plain-prompt context (16 identical layer copies)
  config2            the same with the AdaPrompt subject vectors injected: rows 6..21 of every layer copy differ
  config3            global batch 64 in micro-batches of 8 per forward, sharded over the ranks (strong scaling)
Synthetic data and seeded random-init weights of the SD-1.5 architecture (no checkpoint exists offline).

--plumbing-test replaces the HIP path by a stub and the backend by gloo: it exists so that the launcher, rendezvous,
sharding, gather and JSON assembly of THIS file can be driven by a world-size-2 CPU test; it measures nothing and
says so in its output.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

F_UNET = 803.273e9      # algorithmic FLOP per sample-forward
F_VAE = 2514.519e9      # algorithmic FLOP per decoded image
PEAK_BF16 = 2.5e15      # dense bf16 MFMA peak, MI355X_MICROARCH.md
PEAK_F32 = 157.3e12
PEAK_MXFP8 = 5.0e15     # dense block-scaled fp8 MFMA peak (the fp8 convolutions' own roofline)
# af_prof classes (include/adaface_hip.h)
K_NAMES = ["conv_gemm_other", "attention (+ the fused cross-attention layers)", "groupnorm", "layernorm", "other", "conv_gemm_pp<160,gather> + conv3x3_s8",
           "conv_gemm_pp<160,plain>", "conv_gemm_pp<128>", "conv_gemm_pp<fp8>", "conv3x3_halo8"]
GEMM_CLASSES = (0, 5, 6, 7, 8, 9)
DOMINANT = 9            # conv3x3_halo8_kernel: the 3x3 / stride-1 convolutions, the largest single kernel of a bf16 step
DOMINANT_KERNEL = "conv3x3_halo8_kernel"
DOMINANT_FP8 = 8        # fp8 mode: the same convolutions with e4m3 operands (both tile widths in one class)
DOMINANT_FP8_KERNEL = "conv_gemm_pp_kernel<160|128, true, 0, true, 2>"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="config1", choices=["config1", "config2", "config3", "config4"],
                    help="BASELINE.json configs[1..4]; config4 = identity context + fp8 convolutions, global batch 64")
    ap.add_argument("--batch", type=int, default=8, help="images per UNet micro-batch (CFG forward batch = 2x)")
    ap.add_argument("--global-batch", type=int, default=None, help="images per step over all ranks (config3: 64)")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--dtype", default=None, choices=["bf16", "f32", "fp8"],
                    help="compute mode (default bf16; config4: fp8 = bf16 with e4m3 ResBlock convolutions)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: the device clock probe, the untimed f32 parity leg "
                         "(exit code 3 past its bar) and the CPU baseline (the serving leg still needs --serving-leg)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-kernel-timing", action="store_true", help="skip the HIP-event roofline leg")
    ap.add_argument("--no-parity-leg", action="store_true",
                    help="with --full: skip the untimed f32-mode batch (f32-mode images/s and the bf16 final-latent deviation)")
    ap.add_argument("--serving-leg", action="store_true",
                    help="after the timed region, also run the serving leg (two independent batch-8 requests in flight on two HIP "
                         "streams: a second 859 M-parameter model, ~10 s; never part of `value`).  Default off: BASELINE's metric is "
                         "one batch of 8 at a time (DESIGN.md section 5 keeps the round-3 finding, +9.7 %)")
    ap.add_argument("--no-inflight-leg", action="store_true", help=argparse.SUPPRESS)   # (round-3 spelling; the leg is off by default now)
    ap.add_argument("--parity-bar-bf16", type=float, default=3e-2,
                    help="bar on the bf16 final-latent deviation from the f32 mode of the same batch, of max|latent| (exit code 3 if exceeded)")
    ap.add_argument("--parity-bar-fp8", type=float, default=1e-1, help="the same for the fp8 mode")
    ap.add_argument("--event-stride", type=int, default=29,
                    help="HIP-event bracket every n-th GEMM / attention launch inside the timed region (1 = all).  An event pair "
                         "costs ~9 us of stream time: every 7th launch measured 833 ms per batch against 822 ms untimed, every 29th "
                         "824 ms (still ~160 samples of the dominant kernel in three batches; 29 is coprime to its 31 launches per "
                         "forward, so every shape is sampled)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy in float32: "
                         "frames (the gathered uint8 frames) and latents (this rank's final latents); at most 64 MB in all")
    ap.add_argument("--plumbing-test", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def build_model(device, dtype):
    import torch
    from adaface_amd.configs import sd15_config
    from ldm.util import instantiate_from_config
    model = instantiate_from_config(sd15_config()["model"]).eval()
    model.set_compute_dtype(dtype)
    model = model.to(device)
    # seeded synthetic weights, drawn in HBM (identical on every rank)
    g = torch.Generator(device=device).manual_seed(1234)
    with torch.no_grad():
        for name, p in sorted(model.named_parameters()):
            if p.dim() == 1:
                t = torch.randn(p.shape, generator=g, device=device)
                p.copy_(1.0 + 0.1 * t if name.endswith(".weight") else 0.05 * t)
            else:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g, device=device) * fan_in ** -0.5)
    model.model.diffusion_model._mark_dirty()
    model.first_stage_model._mark_dirty()
    return model


def cpu_baseline(ddim_steps):
    """Oracle (CPU restatement of the reference, oracle/ldm_oracle.py) on the host cores: one UNet forward at
    CFG batch 2 (= 1/ddim_steps of one image's denoising) + one VAE decode, extrapolated to images/sec."""
    import torch
    from oracle import ldm_oracle as O
    # one GPU's share of the host is 16 cores; more threads than that oversubscribes the box
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(7)
    sd = O.synth_state_dict(O.unet_param_shapes(O.SD15_UNET), seed=21)
    x = torch.randn(2, 4, 64, 64, generator=g)
    t = torch.tensor([981, 981])
    ctx = torch.randn(2 * 16, 77, 768, generator=g)
    with torch.no_grad():
        O.unet_forward(sd, O.SD15_UNET, x, t, ctx)            # warm-up (page-in, thread pool)
        t0 = time.perf_counter()
        for _ in range(2):
            O.unet_forward(sd, O.SD15_UNET, x, t, ctx)
        t_unet = (time.perf_counter() - t0) / 2
        del sd
        vsd = O.synth_state_dict(O.vae_param_shapes(O.SD15_VAE), seed=22)
        z = torch.randn(1, 4, 64, 64, generator=g) * 0.18215
        t0 = time.perf_counter()
        O.vae_decode(vsd, O.SD15_VAE, z)
        t_vae = time.perf_counter() - t0
    return {"value": 1.0 / (ddim_steps * t_unet + t_vae), "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": f"UNet forward at CFG batch 2 (warm-up + mean of 2: {t_unet:.2f} s) + 1 VAE decode ({t_vae:.2f} s), fp32 torch CPU, "
                      f"extrapolated as 1/({ddim_steps}*t_unet + t_vae)"}


def traffic_record():
    """HBM bytes per launch of the dominant kernel from the committed PMC passes (scripts/pmc_bench.sh: separate
    FETCH_SIZE / WRITE_SIZE runs, gfx950 corrections) — NOT measured in this run, and labelled so."""
    tf = ROOT / "profiles" / "traffic_latest.json"
    if not tf.exists():
        return None, None
    try:
        d = json.loads(tf.read_text())
    except Exception:
        return None, None
    k = (d.get("kernels") or {}).get(DOMINANT_KERNEL)
    src = {"file": "profiles/traffic_latest.json", "commit": d.get("commit"), "measured_in_run": False,
           "method": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in two separate passes of `bench.py --steps 1`, FETCH_SIZE x 2 (gfx950)"}
    return (k or {}).get("hbm_bytes_per_launch"), src


DUMP_BYTES = 64_000_000     # --dump-outputs: all files together, .npy headers included


def dump_outputs(dirname, arrays):
    """Write each tensor of `arrays` (name -> tensor) as DIR/<name>.npy in float32.  Arrays that do not fit their share of
    DUMP_BYTES are cut to a sample of their leading-dimension rows (images) drawn with a fixed seed and kept in ascending
    order, so that every run with the same arguments writes the same rows.  Returns the shapes and sampled rows."""
    import numpy as np
    import torch
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    left, info = DUMP_BYTES - 1024 * len(arrays), {}
    items = sorted(arrays.items(), key=lambda kv: kv[1].numel())
    for i, (name, t) in enumerate(items):
        n, row_bytes = t.shape[0], t[0].numel() * 4
        share = left // (len(items) - i)
        rows = None
        if n * row_bytes > share:
            k = share // row_bytes
            assert k >= 1, (name, tuple(t.shape))
            rows = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:k].sort().values
            t = t[rows.to(t.device)]
        a = t.detach().float().cpu().numpy()
        np.save(d / f"{name}.npy", a)
        left -= a.nbytes
        info[name] = {"shape": list(arrays[name].shape), "rows": None if rows is None else rows.tolist()}
    total = sum((d / f"{name}.npy").stat().st_size for name in arrays)
    assert total <= DUMP_BYTES, total
    return {"dir": os.fspath(d), "dtype": "float32", "bytes": total, "arrays": info}


def main():
    args = parse()
    if args.dtype is None:
        args.dtype = "fp8" if args.workload == "config4" else "bf16"
    # ---- N > 1 without a launcher: start the ranks ourselves, BEFORE anything here touches the GPU ----
    from adaface_amd.parallel import init_distributed, launch_ranks, launched_by_torchrun
    if args.gpus > 1 and not launched_by_torchrun():
        raise SystemExit(launch_ranks(args.gpus, os.fspath(Path(__file__).resolve()), sys.argv[1:]))

    import torch
    import torch.distributed as dist
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    stub = args.plumbing_test
    if stub:
        device = torch.device("cpu")
        rank, world = init_distributed(args.gpus, backend="gloo")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: adaface_amd has no CPU path")
        if torch.cuda.device_count() < args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but only {torch.cuda.device_count()} device(s) visible")
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
        rank, world = init_distributed(args.gpus, backend="nccl", device=device)
    from adaface_amd.parallel import STATS, gather_frames, shard_batch
    from adaface_amd.synth import synth_context, synth_context_adaprompt, synth_context_identity

    B, S = args.batch, args.ddim_steps
    strong = args.workload in ("config3", "config4") or args.global_batch is not None
    G = args.global_batch if args.global_batch is not None else (64 if args.workload in ("config3", "config4") else B * world)
    if G % world or (G // world) % B:
        raise SystemExit(f"global batch {G} must split into micro-batches of {B} on each of {world} rank(s)")
    n_micro = G // world // B
    # global inputs generated from one seed on the host, sliced per rank (results independent of world size)
    g = torch.Generator().manual_seed(42)
    x_T_all = shard_batch(torch.randn(G, 4, 64, 64, generator=g), rank, world).to(device)
    make_ctx = {"config2": synth_context_adaprompt, "config4": synth_context_identity}.get(args.workload, synth_context)
    c_all = shard_batch(make_ctx(G, seed=100, device="cpu"), rank, world, per_sample=16).to(device)
    uc_emb = synth_context(B, seed=101, device=device, shared=True)

    if stub:
        lib = None

        def run_micro(x_T, c_emb):   # deterministic stand-in of the right output shape; NOTHING is measured
            v = (x_T.sum(dim=(1, 2, 3)) + c_emb.reshape(x_T.shape[0], -1).sum(dim=1)).mul(7).to(torch.uint8)
            return v[:, None, None, None].expand(-1, 8, 8, 3).contiguous(), x_T
    else:
        from adaface_amd import _lib
        from ldm.models.diffusion.ddim import DDIMSampler
        lib = _lib.load()
        def make_runner(mdl):
            smp = DDIMSampler(mdl)
            uc_ = mdl.get_learned_conditioning(uc_emb)
            conds_ = [mdl.get_learned_conditioning(c_all[i * B * 16:(i + 1) * B * 16]) for i in range(n_micro)]

            def denoise(x_T, cond):
                samples, _ = smp.sample(S=S, conditioning=cond, batch_size=B, shape=[4, 64, 64], verbose=False,
                                        guidance_scale=[10.0, 4.0], unconditional_conditioning=uc_, eta=0.0, x_T=x_T)
                return samples

            def run(x_T, cond):
                samples = denoise(x_T, cond)
                return mdl.decode_first_stage_uint8(samples), samples
            run.denoise, run.decode = denoise, mdl.decode_first_stage_uint8
            return run, conds_

        model = build_model(device, args.dtype)
        run_micro, conds = make_runner(model)

    step_latents = []       # the final latents of every micro-batch of the latest step

    # (round 3 measured `AutoencoderKL.decode` of batch i on a second stream under the denoising of batch i + 1 at +0.4 %:
    # DESIGN.md section 5; the variant left the bench in round 4 -- `git show d4cf8f4:bench.py` has it)
    gather_ms = []          # per step: HIP-event duration of the frame all-gather on this rank (N > 1 or a launcher-made group)

    def step():
        frames = []
        step_latents.clear()
        for i in range(n_micro):
            f, lat = run_micro(x_T_all[i * B:(i + 1) * B], c_all[i * B * 16:(i + 1) * B * 16] if stub else conds[i])
            frames.append(f)
            step_latents.append(lat)
        frames = frames[0] if n_micro == 1 else torch.cat(frames)
        if stub or not dist.is_initialized():
            return gather_frames(frames, global_batch=G)  # one all-gather per step (no process group: returns its input)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out_ = gather_frames(frames, global_batch=G)      # one RCCL all-gather per step, on the sampling stream
        e1.record()
        gather_ms.append((e0, e1))
        return out_

    def fence():
        if world > 1:
            dist.barrier()
        if not stub:
            torch.cuda.synchronize()

    # held-clock proxy of THIS device, taken before the warm-up: devices of one pool differ by +-5 % on MFMA-dense kernels
    clock = None
    if lib is not None and args.full:
        mhz, tfl = C.c_double(0.0), C.c_double(0.0)
        _lib.check(lib.af_clock_probe(C.c_void_p(torch.cuda.current_stream().cuda_stream), 0, C.byref(mhz), C.byref(tfl)),
                   "af_clock_probe")
        clock = {"mfma_loop_mhz": mhz.value, "mfma_loop_tflops": tfl.value,
                 "what": "register-only v_mfma_f32_32x32x16_bf16 loop, two waves per SIMD on every CU, ~5 ms, before the warm-up: "
                         "median in-kernel clock (s_memtime / s_memrealtime) and its rate"}
    for _ in range(args.warmup):
        step()
    fence()
    if lib is not None:
        lib.af_flops_issued(1)
    timing = not args.no_kernel_timing and not stub
    if timing:
        lib.af_prof_reset()
        lib.af_prof_set_stride(args.event_stride)  # sample: an event pair per launch would cost ~10 % of the step
        lib.af_prof_enable(sum(1 << c for c in GEMM_CLASSES) | 0b10)  # conv/linear kernels + attention
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    fence()
    dt = time.perf_counter() - t0
    flops_executed = None
    if lib is not None:
        lib.af_prof_enable(0)
        flops_executed = float(lib.af_flops_issued(1))   # this rank's GEMM / conv / attention FLOPs inside the timed region
    assert out.shape[0] == G and out.shape[-1] == 3 and out.dtype == torch.uint8
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, {"frames": out, "latents": torch.cat(step_latents)})
    # per-rank view (outside the timed region): this rank's own wall time and its all-gather durations, so that a SCALE line can
    # tell compute skew between the ranks from the cost of the collective.  `value` uses the MAX over ranks, as the contract says.
    dt_rank = dt
    ag_rank = [a_.elapsed_time(b_) for a_, b_ in gather_ms[-args.steps:]] if gather_ms else []
    per_rank = {"dt_s_min": dt_rank, "dt_s_max": dt_rank, "all_gather_ms_per_step_mean": (sum(ag_rank) / len(ag_rank)) if ag_rank else None,
                "all_gather_ms_per_step_max_over_ranks": max(ag_rank) if ag_rank else None}
    if dist.is_initialized():
        dev_r = torch.device("cpu") if stub else device
        tmax = torch.tensor([dt_rank, max(ag_rank) if ag_rank else 0.0], device=dev_r, dtype=torch.float64)
        tmin = torch.tensor([dt_rank], device=dev_r, dtype=torch.float64)
        tsum = torch.tensor([sum(ag_rank) / len(ag_rank) if ag_rank else 0.0], device=dev_r, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(tmin, op=dist.ReduceOp.MIN)
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        dt = float(tmax[0].item())
        per_rank = {"dt_s_min": float(tmin[0].item()), "dt_s_max": dt,
                    "all_gather_ms_per_step_mean": float(tsum[0].item()) / world if ag_rank else None,
                    "all_gather_ms_per_step_max_over_ranks": float(tmax[1].item()) if ag_rank else None}

    roof = None
    kernels = {}
    if timing:
        n = len(K_NAMES)
        ms = (C.c_double * n)()
        launches = (C.c_int64 * n)()
        flops = (C.c_double * n)()
        byts = (C.c_double * n)()
        _lib.check(lib.af_prof_collect(n, ms, launches, flops, byts), "af_prof_collect")
        # an event pair measures its own cost too (several us per bracket): measured with empty pairs on the same stream
        # and subtracted, so that avg_launch_us can be held against the kernel durations of a rocprofv3 trace
        ev_us = float(lib.af_prof_event_overhead_us(C.c_void_p(torch.cuda.current_stream().cuda_stream), 64))
        ev_us = max(ev_us, 0.0)
        for i in range(n):
            ms[i] = max(ms[i] - launches[i] * ev_us * 1e-3, 1e-9) if launches[i] else ms[i]
        peak = PEAK_F32 if args.dtype == "f32" else PEAK_BF16
        for i, k in enumerate(K_NAMES):
            if launches[i]:
                kernels[k] = {"launches_timed": int(launches[i]), "ms_total": ms[i], "avg_us": 1e3 * ms[i] / launches[i],
                              "algorithmic_tflops": flops[i] / (ms[i] * 1e-3) / 1e12 if flops[i] else None,
                              "algorithmic_bytes_per_launch": byts[i] / launches[i]}
        cls_ms = sum(ms[c] for c in GEMM_CLASSES)
        cls_fl = sum(flops[c] for c in GEMM_CLASSES)
        cls_n = sum(launches[c] for c in GEMM_CLASSES)
        # the f32 parity mode has no ping-pong kernel: its dominant kernel is the four-wave / halo class
        d = DOMINANT_FP8 if (args.dtype == "fp8" and launches[DOMINANT_FP8]) else (DOMINANT if launches[DOMINANT] else 0)
        if d == DOMINANT_FP8:
            peak = PEAK_MXFP8
        if launches[d]:
            traffic, tsrc = traffic_record() if d == DOMINANT else (None, None)
            ach = flops[d] / (ms[d] * 1e-3)
            kname = {DOMINANT: DOMINANT_KERNEL + " (3x3 / stride-1 convolutions of the UNet at 64x64 / 32x32: eight-wave "
                               "256x160x64 implicit GEMM, input halo resident in LDS, weight tiles by LDS-DMA, merged "
                               "staging/compute schedule)",
                     DOMINANT_FP8: DOMINANT_FP8_KERNEL + " (ResBlock 3x3 convolutions with OCP e4m3 operands on "
                                   "v_mfma_scale_f32_16x16x128_f8f6f4; peak = dense block-scaled fp8)"}.get(
                d, "conv_gemm_kernel / conv3x3_halo_kernel (f32 parity mode)")
            roof = {"kernel": kname,
                    "bound": "mfma", "achieved": ach / 1e12, "peak": peak / 1e12, "unit": "TFLOP/s", "frac": ach / peak,
                    "flops_per_launch": flops[d] / launches[d], "avg_launch_us": 1e3 * ms[d] / launches[d],
                    "launches_timed": int(launches[d]), "sampled_every": args.event_stride,
                    "event_pair_overhead_us_subtracted": ev_us,
                    "algorithmic_bytes_per_launch": byts[d] / launches[d],
                    "traffic": traffic, "traffic_source": tsrc,
                    # the same against what THIS device sustains on a register-only MFMA loop (device_clock_probe): under a
                    # dense MFMA stream the chip holds ~1.7 GHz, not the 2.4 GHz behind the 2.5 PFLOP/s figure
                    "frac_of_device_mfma_loop": (ach / 1e12 / clock["mfma_loop_tflops"]) if (clock and d != DOMINANT_FP8) else None,
                    "conv_linear_class": {"kernels": [K_NAMES[c] for c in GEMM_CLASSES], "achieved": cls_fl / (cls_ms * 1e-3) / 1e12,
                                          "frac": cls_fl / (cls_ms * 1e-3) / peak, "launches_timed": int(cls_n)}}

    # ---- serving leg (rank 0, N = 1; NOT `value`): two independent batch-B requests in flight on two HIP streams ----
    # Between two dependent launches of ONE request the device idles for a couple of microseconds (drain, dispatch, ramp: ~460
    # launches per UNet forward); a second request's launches fill those gaps.  Two engines (each its own weights, arena and
    # stream), two host threads.  Reported beside the headline, never in it: the headline is one batch of 8 at a time.
    inflight = None
    if rank == 0 and world == 1 and not stub and args.serving_leg and n_micro == 1:
        try:
            import threading
            model_b = build_model(device, args.dtype)
            run_b, conds_b = make_runner(model_b)
            lanes = [(run_micro, conds[0], torch.cuda.Stream()), (run_b, conds_b[0], torch.cuda.Stream())]
            n_each = max(1, min(args.steps, 2))
            errs = []

            got = {}

            def lane(run, cond, stream, n):
                try:
                    torch.cuda.set_device(device)
                    with torch.cuda.stream(stream):
                        for _ in range(n):
                            got[id(stream)] = run(x_T_all[:B], cond)[0]
                except Exception as e:  # noqa: BLE001  (reported in the JSON line; the headline is already measured)
                    errs.append(repr(e))

            def both(n):
                th = [threading.Thread(target=lane, args=(r, c, st, n)) for r, c, st in lanes]
                for t_ in th:
                    t_.start()
                for t_ in th:
                    t_.join()
                torch.cuda.synchronize()

            torch.cuda.synchronize()
            both(1)                                   # warm-up: second engine's first call, both streams' first launches
            ta = time.perf_counter()
            both(n_each)
            tb = time.perf_counter() - ta
            # both engines hold the same weights and ran the timed region's own inputs: with nothing shared between the two
            # streams their frames are the single-stream frames, byte for byte
            same = all(torch.equal(f, out[:B]) for f in got.values()) and len(got) == 2
            inflight = {"value": 2 * n_each * B / tb, "unit": "images/sec", "requests_in_flight": 2, "batch_per_request": B,
                        "frames_equal_single_stream": bool(same),
                        "batches_timed": 2 * n_each, "ms_per_pair_of_batches": 1e3 * tb / n_each, "errors": errs or None,
                        "note": "two independent batch-%d requests (two engines, two HIP streams, two host threads); NOT the headline "
                                "`value`, which runs one batch at a time" % B}
            del model_b, run_b, conds_b, lanes
            torch.cuda.empty_cache()
        except Exception as e:  # noqa: BLE001
            inflight = {"value": None, "errors": [repr(e)]}

    # ---- untimed parity leg (rank 0, N = 1): the SAME batch in f32 parity mode ----
    parity = None
    if rank == 0 and world == 1 and not stub and args.full and not args.no_parity_leg and args.dtype in ("bf16", "fp8"):
        lat16 = step_latents[-1].clone()
        model.set_compute_dtype("f32")
        run_micro(x_T_all[(n_micro - 1) * B:], conds[-1])          # engine build + weight upload + first call
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        _, lat32 = run_micro(x_T_all[(n_micro - 1) * B:], conds[-1])
        torch.cuda.synchronize()
        t32 = time.perf_counter() - t1
        sc = lat32.abs().max().item()
        rel = (lat16 - lat32).abs().max().item() / sc
        bar = args.parity_bar_bf16 if args.dtype == "bf16" else args.parity_bar_fp8
        parity = {"f32_mode_images_per_sec": B / t32,
                  f"{args.dtype}_final_latent_rel_err": rel, "bar": bar, "within_bar": bool(rel <= bar),
                  f"{args.dtype}_final_latent_max_abs_err": (lat16 - lat32).abs().max().item(), "final_latent_max_abs": sc,
                  # the rms of the same deviation over the rms of the f32 latent: unlike the max-abs figure it does not move
                  # with the draw of the rounding noise (DESIGN.md section 2 p')
                  f"{args.dtype}_final_latent_rms_over_rms": ((lat16 - lat32).double().pow(2).mean().sqrt() /
                                                              lat32.double().pow(2).mean().sqrt()).item(),
                  "note": "same x_T / context / weights; the f32 (parity) mode is the one pinned to <= 1e-3 max-abs "
                          "against the CPU oracle (tests/test_model_gpu.py::test_config0_*, profiles/*parity_50step*); "
                          f"{args.dtype} is the timed throughput mode and this is its measured deviation after all DDIM steps"}
        model.set_compute_dtype(args.dtype)

    if rank == 0:
        images = G * args.steps
        value = images / dt
        flop_img = S * 2 * F_UNET + F_VAE
        res = {
            "metric": "512x512 images/sec @ 50 DDIM steps, batch 8",
            "value": value, "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{args.workload}: SD v1.5 512x512, {S} DDIM steps, batch {B} per forward "
                                   f"(CFG Bf={2 * B}), {n_micro} micro-batch(es) per GPU per step, layerwise 16x77x768 context"
                                   + (" with per-layer AdaPrompt subject rows 6..21" if args.workload == "config2" else "")
                                   + (" with a synthetic unit-norm 512-d identity embedding (zero-padded to 768) in rows 4..19 of "
                                      "every layer copy; ResBlock 3x3 convolutions with e4m3 operands" if args.workload == "config4" else "")
                                   + ", random-init weights"
                                   + "; decode on the sampling stream",
                       "global_batch": G, "latent": [4, 64, 64], "guidance_scale": [10.0, 4.0], "parallelism": f"dp{world}"},
            "whole_path_algorithmic_tflops": value * flop_img / 1e12 / world,
            "whole_path_frac_of_mfma_peak": value * flop_img / world / (PEAK_F32 if args.dtype == "f32" else PEAK_BF16),
            # the same with the FLOPs the kernels were actually handed (rank 0's launches in the timed region): the four-phase
            # upsamplers run 4/9 of the reference's MACs and the CFG twin forward shares the context-independent prefix, so
            # this is the number to read as MFMA utilisation; the line above is the metric SURVEY.md 8(d) defines
            "whole_path_executed_flops_frac": (flops_executed / dt / (PEAK_F32 if args.dtype == "f32" else PEAK_BF16)
                                               if flops_executed else None),
            "executed_over_reference_flops": (flops_executed / (images / world * flop_img) if flops_executed else None),
            "device_clock_probe": clock,
            "distributed": dict(STATS, per_rank=per_rank),
            "roofline": roof, "kernels": kernels, "parity": parity, "two_requests_in_flight": inflight,
            "dumped_outputs": dumped, "full": args.full,
        }
        if stub:
            res.update(metric="PLUMBING TEST - stub in place of the HIP path, nothing measured", value=None, dtype="none",
                       checksum=int(out.to(torch.int64).sum().item()),
                       frames_sha256=__import__("hashlib").sha256(out.contiguous().numpy().tobytes()).hexdigest())
        if world == 1 and args.full and not args.no_cpu_baseline and not stub:
            res["cpu_baseline"] = cpu_baseline(S)
        else:
            res["cpu_baseline"] = None
        print(json.dumps(res))
    if world > 1 or dist.is_initialized():
        dist.destroy_process_group()
    if parity is not None and not parity["within_bar"]:
        sys.stderr.write(f"bench.py: {args.dtype} final latent deviates {parity[f'{args.dtype}_final_latent_rel_err']:.3e} of max|latent| "
                         f"from the f32 mode (bar {parity['bar']:.1e})\n")
        raise SystemExit(3)


if __name__ == "__main__":
    main()
