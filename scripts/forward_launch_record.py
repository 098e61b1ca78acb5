#!/usr/bin/env python
"""What the library launches and computes on every path of its model executor, for comparing two builds of it:

    python scripts/forward_launch_record.py --out DIR          # in each tree (the tree the script lies in is the one it runs)
    python scripts/forward_launch_record.py --out DIR --only bf16_vae bf16_vae_encode    # these records alone
    python scripts/forward_launch_record.py --compare A B [C]  # every later record against the first

SD-1.5 with synthetic weights and inputs as bench.py builds them.  One record per line of this table; each holds the
`[af plan]` lines of the call (knob plan_log: the conv / GEMM launches), `_lib.plan_counts()` after it, the launches per kernel
class (af_prof_enable / af_prof_collect: GroupNorm, LayerNorm, attention and copy launches show up only here; counted in a
forward of their own, because the event records would otherwise join the forward whose tensors are kept), the engine's
`arena_bytes()` and the output tensors.  Every record runs on an engine of its own, so that its arena is sized by its own
forward.

    bf16, f32, fp16, fp8_ff   twin forward at the benchmark configuration: batch 8 -> CFG batch 16, 64x64 latents
    bf16_vae                  VAE decode of two latents
  batch 2 -> CFG batch 4, 64x64 latents unless noted, bf16 unless named otherwise:
    bf16_plain                unet_forward on the batch of 4 (no twin prefix)
    bf16_convattn             conv attention, ks 3: sample 0 carries one subject string, sample 1 two, samples 2 and 3 none
                              (three runs of the run loop); default knobs = the one-pass kernel
    bf16_convattn_merge       ... with knob conv_attn_short = 0: flash attention + merge
    f32_convattn              ... on an f32 handle: the merge path's dtype dispatch
    bf16_deepcache            unet_forward_cached, twin, depth 2: refresh, then reuse (both outputs)
    bf16_vae_encode           vae_encode of a 2x3x64x64 image
    bf16_clip, bf16_clip3     clip_text_forward / clip_text_forward3 on 2 x 77 token embeddings
    bf16_twin32               twin forward at 32x32 latents (other LayerNorm-folding and fusion decisions, half-batch probes)

--compare prints, per record, whether the launch lines, the counters and the per-class launch counts are identical (with the
sha256 of the lines), the arena sizes, and the max abs difference of every tensor (0 = bit for bit).  Exit code 1 if anything
differs.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
MODES = (("bf16", "bf16", "base"), ("f32", "f32", "base"), ("fp16", "fp16", "base"), ("fp8_ff", "fp8", "base+ff"))
N_CLASSES = 10    # the classes of af_common.h in front of the token-merging ones (off here)


def record(out: Path, only=None):
    sys.path.insert(0, str(ROOT))
    import torch
    from adaface_amd import _lib
    from adaface_amd.synth import synth_context
    from bench import build_model
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    out.mkdir(parents=True, exist_ok=True)
    lib = _lib.load()
    meta = {}

    def capture(tag, eng, run):
        """run() -> {name: tensor}: once to size the arena and fold weights, once logged (its tensors are kept), once counted"""
        if only and tag not in only:
            return
        run()
        torch.cuda.synchronize()
        _lib.plan_counts(reset=True)
        _lib.set_knob("plan_log", 1)
        sys.stderr.flush()
        saved, log = os.dup(2), out / f"{tag}_plan.log"
        fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        os.dup2(fd, 2)
        try:
            tensors = run()
            torch.cuda.synchronize()
        finally:
            os.dup2(saved, 2)
            os.close(fd)
            os.close(saved)
            _lib.set_knob("plan_log", 0)
        lines = [ln for ln in log.read_text().splitlines() if ln.startswith("[af plan]")]
        log.write_text("\n".join(lines) + "\n")
        counts = _lib.plan_counts(reset=True)
        lib.af_prof_reset()
        lib.af_prof_set_stride(1)
        lib.af_prof_enable((1 << N_CLASSES) - 1)
        try:
            run()
            torch.cuda.synchronize()
        finally:
            lib.af_prof_enable(0)
        ms, la = (C.c_double * N_CLASSES)(), (C.c_int64 * N_CLASSES)()
        fl, by = (C.c_double * N_CLASSES)(), (C.c_double * N_CLASSES)()
        lib.af_prof_collect(N_CLASSES, ms, la, fl, by)
        lib.af_prof_reset()
        _lib.plan_counts(reset=True)
        meta[tag] = {"counts": counts, "class_launches": list(la), "arena_bytes": eng.arena_bytes(), "plan_lines": len(lines)}
        torch.save({k: v.cpu() for k, v in tensors.items()}, out / f"{tag}.pt")
        print(f"recorded {tag}: {len(lines)} plan lines, launches per class {list(la)}", flush=True)

    model = build_model(dev, "bf16")
    unet = model.model.diffusion_model
    g = torch.Generator().manual_seed(42)
    B, Bs = 8, 2
    x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
    x32 = torch.randn(Bs, 4, 32, 32, generator=g).to(dev)
    image = torch.randn(Bs, 3, 64, 64, generator=g).clamp(-1, 1).to(dev)
    tok_emb = (torch.randn(Bs, 77, 768, generator=g) * 0.02).to(dev)
    t0 = torch.full((B,), 901, dtype=torch.long, device=dev)
    ctx2 = torch.cat([synth_context(B, seed=100, device=dev), synth_context(B, seed=101, device=dev, shared=True)])
    ctx2s = torch.cat([synth_context(Bs, seed=100, device=dev), synth_context(Bs, seed=101, device=dev, shared=True)])
    xs, ts = x_T[:Bs], t0[:Bs]
    # subject strings as tests/conv_attn_cases.py places them: distinct key positions drawn by a seeded permutation
    pos = torch.randperm(77, generator=torch.Generator().manual_seed(1000 * 3 + 77)).tolist()
    subj_batch, subj_tokens = [0, 1, 1], [pos[0:9], pos[9:18], pos[18:27]]

    def fresh(mod):
        """a new engine for `mod` in its current mode, weights uploaded again: arena_bytes() then tells what THIS record needs"""
        cur = mod.compute_dtype
        mod.set_compute_dtype("bf16" if cur == "f32" else "f32")
        mod.set_compute_dtype(cur)
        return mod.engine(dev)

    def unet_record(tag, ctx, run, conv_attn=False, conv_attn_short=1):
        if only and tag not in only:
            return
        eng = fresh(unet)
        object.__setattr__(unet, "_ctx_key", None)            # (the module's context cache no longer describes the engine)
        if conv_attn:
            eng.set_conv_attn(3, subj_batch, subj_tokens)
        eng.set_context(ctx, ctx.shape[0] // 16, layerwise=True)
        _lib.set_knob("conv_attn_short", conv_attn_short)
        try:
            capture(tag, eng, lambda: run(eng))
        finally:
            _lib.set_knob("conv_attn_short", 1)

    def twin_small(eng):
        return {"eps": eng.unet_forward_twin(xs, ts)}

    for tag, dtype, scope in MODES:
        model.set_compute_dtype(dtype, fp8_scope=scope) if dtype == "fp8" else model.set_compute_dtype(dtype)
        unet_record(tag, ctx2, lambda eng: {"eps": eng.unet_forward_twin(x_T, t0)})
        if tag == "f32":
            unet_record("f32_convattn", ctx2s, twin_small, conv_attn=True)
        if tag != "bf16":
            continue
        vae = model.first_stage_model
        capture("bf16_vae", fresh(vae), lambda: {"image": model.decode_first_stage(x_T[:2])})
        veng = fresh(vae)
        capture("bf16_vae_encode", veng, lambda: {"moments": veng.vae_encode(image)})
        unet_record("bf16_convattn", ctx2s, twin_small, conv_attn=True)
        unet_record("bf16_convattn_merge", ctx2s, twin_small, conv_attn=True, conv_attn_short=0)
        unet_record("bf16_plain", ctx2s, lambda eng: {"eps": eng.unet_forward(torch.cat([xs, xs]), torch.cat([ts, ts]))})
        unet_record("bf16_twin32", ctx2s, lambda eng: {"eps": eng.unet_forward_twin(x32, ts)})
        unet_record("bf16_deepcache", ctx2s,
                    lambda eng: {"refresh": eng.unet_forward_cached(xs, ts, depth=2, mode="refresh", twin=True),
                                 "reuse": eng.unet_forward_cached(xs, ts, depth=2, mode="reuse", twin=True)})
        clip = getattr(model, "cond_stage_model", None)
        if clip is not None and hasattr(clip, "clip_config") and clip.clip_config["hidden"] == tok_emb.shape[2]:
            ceng = fresh(clip)
            capture("bf16_clip", ceng, lambda: {"states": ceng.clip_text_forward(tok_emb)})
            ceng = fresh(clip)
            capture("bf16_clip3", ceng, lambda: {"states": ceng.clip_text_forward3(tok_emb, 0.25, 0.25, 0.5)})
        else:
            for tag in ("bf16_clip", "bf16_clip3"):
                if not only or tag in only:
                    meta[tag] = {"absent": "the bench model builds no CLIP text tower"}
    (out / "meta.json").write_text(json.dumps(meta, indent=1, sort_keys=True))


def compare(dirs):
    import torch
    ref, bad = dirs[0], 0
    m0 = json.loads((ref / "meta.json").read_text())
    for d in dirs[1:]:
        m = json.loads((d / "meta.json").read_text())
        print(f"== {d} against {ref}")
        for tag in sorted(set(m0) | set(m)):
            if tag not in m0 or tag not in m or "absent" in m0[tag] or "absent" in m[tag]:
                same = tag in m0 and tag in m and m0[tag] == m[tag]
                bad += not same
                print(f"{tag:20s} {'absent in both: ' + m[tag]['absent'] if same else 'RECORDED IN ONE ONLY'}")
                continue
            a, b = (ref / f"{tag}_plan.log").read_bytes(), (d / f"{tag}_plan.log").read_bytes()
            r0, r1 = m0[tag], m[tag]
            same_l, same_c, same_k = a == b, r0["counts"] == r1["counts"], r0["class_launches"] == r1["class_launches"]
            same_a = r0["arena_bytes"] == r1["arena_bytes"]
            t0, t1 = torch.load(ref / f"{tag}.pt"), torch.load(d / f"{tag}.pt")
            diffs = {k: (t0[k] - t1[k]).abs().max().item() if k in t1 and t0[k].shape == t1[k].shape else float("inf") for k in t0}
            bad += (not same_l) + (not same_c) + (not same_k) + (not same_a) + any(v != 0 for v in diffs.values())
            print(f"{tag:20s} [af plan] lines {'identical' if same_l else 'DIFFERENT'} ({r1['plan_lines']} lines, sha256 "
                  f"{hashlib.sha256(a).hexdigest()[:16]} / {hashlib.sha256(b).hexdigest()[:16]}); plan_counts "
                  f"{'identical' if same_c else 'DIFFERENT'}; launches per class {'identical' if same_k else 'DIFFERENT'} "
                  f"{r1['class_launches']}; arena_bytes {r0['arena_bytes']} -> {r1['arena_bytes']}; "
                  + "; ".join(f"{k} max abs diff {v:.3e} (max |{k}| {t0[k].abs().max().item():.3e})" for k, v in diffs.items()))
            if not same_c:
                print("   ", r0["counts"], "\n   ", r1["counts"])
            if not same_k:
                print("   ", r0["class_launches"], "\n   ", r1["class_launches"])
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path)
    ap.add_argument("--compare", type=Path, nargs="+")
    ap.add_argument("--only", nargs="+", metavar="RECORD", help="with --out: record only these")
    a = ap.parse_args()
    if a.out:
        record(a.out, set(a.only) if a.only else None)
    if a.compare:
        sys.exit(1 if compare(a.compare) else 0)
