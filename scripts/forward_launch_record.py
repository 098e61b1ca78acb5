#!/usr/bin/env python
"""What one twin forward and one VAE decode launch and compute, at the benchmark configuration (SD-1.5, synthetic weights and
inputs as bench.py builds them, batch 8 -> CFG batch 16, 64x64 latents), for comparing two builds of the library:

    python scripts/forward_launch_record.py --out DIR          # in each tree (the tree the script lies in is the one it runs)
    python scripts/forward_launch_record.py --compare A B [C]  # every later record against the first

Per mode (bf16, f32, fp16, fp8 base+ff): the `[af plan]` lines of the forward (knob plan_log), `_lib.plan_counts()` after it,
`engine.arena_bytes()`, the eps tensor; in bf16 also the decoded image of one VAE decode.  --compare prints, per mode, whether
the launch lines and counters are identical (with their sha256), the arena sizes, and the max abs difference of the tensors
(0 = bit for bit).  Exit code 1 if launches or counters differ.
"""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
MODES = (("bf16", "bf16", "base"), ("f32", "f32", "base"), ("fp16", "fp16", "base"), ("fp8_ff", "fp8", "base+ff"))


def record(out: Path):
    sys.path.insert(0, str(ROOT))
    import torch
    from adaface_amd import _lib
    from adaface_amd.synth import synth_context
    from bench import build_model
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    out.mkdir(parents=True, exist_ok=True)
    B = 8
    model = build_model(dev, "bf16")
    unet = model.model.diffusion_model
    g = torch.Generator().manual_seed(42)
    x_T = torch.randn(B, 4, 64, 64, generator=g).to(dev)
    ctx2 = torch.cat([synth_context(B, seed=100, device=dev), synth_context(B, seed=101, device=dev, shared=True)])
    t0 = torch.full((B,), 901, dtype=torch.long, device=dev)
    meta = {}
    for tag, dtype, scope in MODES:
        model.set_compute_dtype(dtype, fp8_scope=scope) if dtype == "fp8" else model.set_compute_dtype(dtype)
        eng = unet.engine(dev)
        eng.set_context(ctx2, 2 * B, layerwise=True)
        object.__setattr__(unet, "_ctx_key", None)            # (the module's context cache no longer describes the engine)
        eng.unet_forward_twin(x_T, t0)                         # (sizes the arena, folds weights)
        torch.cuda.synchronize()
        _lib.plan_counts(reset=True)
        _lib.set_knob("plan_log", 1)
        sys.stderr.flush()
        saved, log = os.dup(2), out / f"{tag}_plan.log"
        fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
        os.dup2(fd, 2)
        try:
            eps = eng.unet_forward_twin(x_T, t0)
            torch.cuda.synchronize()
        finally:
            os.dup2(saved, 2)
            os.close(fd)
            os.close(saved)
            _lib.set_knob("plan_log", 0)
        lines = [ln for ln in log.read_text().splitlines() if ln.startswith("[af plan]")]
        log.write_text("\n".join(lines) + "\n")
        meta[tag] = {"counts": _lib.plan_counts(reset=True), "arena_bytes": eng.arena_bytes(), "plan_lines": len(lines)}
        torch.save(eps.cpu(), out / f"{tag}_eps.pt")
        if tag == "bf16":
            torch.save(model.decode_first_stage(x_T[:2]).cpu(), out / "bf16_vae.pt")
    (out / "meta.json").write_text(json.dumps(meta, indent=1, sort_keys=True))


def compare(dirs):
    import torch
    ref, bad = dirs[0], 0
    m0 = json.loads((ref / "meta.json").read_text())
    for d in dirs[1:]:
        m = json.loads((d / "meta.json").read_text())
        print(f"== {d} against {ref}")
        for tag, _, _ in MODES:
            a, b = (ref / f"{tag}_plan.log").read_bytes(), (d / f"{tag}_plan.log").read_bytes()
            same_l, same_c = a == b, m0[tag]["counts"] == m[tag]["counts"]
            bad += (not same_l) + (not same_c)
            e0, e1 = torch.load(ref / f"{tag}_eps.pt"), torch.load(d / f"{tag}_eps.pt")
            print(f"{tag:7s} [af plan] lines {'identical' if same_l else 'DIFFERENT'} ({m[tag]['plan_lines']} lines, sha256 "
                  f"{hashlib.sha256(a).hexdigest()[:16]} / {hashlib.sha256(b).hexdigest()[:16]}); plan_counts "
                  f"{'identical' if same_c else 'DIFFERENT'}; arena_bytes {m0[tag]['arena_bytes']} -> {m[tag]['arena_bytes']}; "
                  f"eps max abs diff {(e0 - e1).abs().max().item():.3e} (max |eps| {e0.abs().max().item():.3e})")
            if not same_c:
                print("   ", m0[tag]["counts"], "\n   ", m[tag]["counts"])
        v0, v1 = torch.load(ref / "bf16_vae.pt"), torch.load(d / "bf16_vae.pt")
        print(f"bf16    VAE decode max abs diff {(v0 - v1).abs().max().item():.3e} (max |image| {v0.abs().max().item():.3e})")
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path)
    ap.add_argument("--compare", type=Path, nargs="+")
    a = ap.parse_args()
    if a.out:
        record(a.out)
    if a.compare:
        sys.exit(1 if compare(a.compare) else 0)
