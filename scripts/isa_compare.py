#!/usr/bin/env python
"""Are the gfx950 kernels of one translation unit the same code in two builds?

    python scripts/isa_compare.py OLD.o NEW.o [--out report.txt]

For every kernel symbol of OLD: the instruction text (addresses and encodings dropped, scripts/check_isa_hazards.py
`disassemble`) and the VGPR / SGPR / scratch / LDS figures of the code object's metadata must be identical in NEW.  Kernels
that exist in NEW only are listed.  Runs without a GPU.  Exit code 1 if anything pre-existing differs or is missing.

Used when a shared body is factored out of a kernel (af_conv_gemm_pp_body.h: profiles/ff8_isa_unchanged_*.txt).
"""
import argparse
import hashlib
import importlib.util
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
          ".vgpr_spill_count", ".sgpr_spill_count", ".kernarg_segment_size", ".max_flat_workgroup_size")


def _scanner():
    spec = importlib.util.spec_from_file_location("check_isa_hazards", ROOT / "scripts" / "check_isa_hazards.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _metadata(mod, obj: Path, tmp: Path) -> dict:
    """kernel symbol -> {field: value} from the NT_AMDGPU_METADATA note of the object's gfx950 code object"""
    co = tmp / (obj.name + ".co")            # left there by disassemble()
    text = subprocess.run([mod.LLVM / "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for ln in text.split("\n"):
        m = re.match(r"^\s+(?:- )?(\.[a-z_]+):\s+(.*)$", ln)
        if not m:
            continue
        if ln.lstrip().startswith("- ") and m[1] == ".agpr_count":   # first key of a kernel entry (keys are sorted)
            cur = {}
        if m[1] in FIELDS:
            cur[m[1]] = m[2].strip()
        if m[1] == ".symbol":
            out[m[2].strip().strip("'").removesuffix(".kd")] = cur     # (the same dict: .vgpr_count follows .symbol)
    return out


def load(obj: Path):
    mod = _scanner()
    with tempfile.TemporaryDirectory() as td:
        funcs = mod.disassemble(obj, Path(td))
        if not funcs:
            raise RuntimeError(f"{obj}: no gfx950 device code")
        meta = _metadata(mod, obj, Path(td))
    return {name: ins for name, ins in funcs}, meta


def compare(old: Path, new: Path):
    fo, mo = load(old)
    fn, mn = load(new)
    lines, bad = [], 0
    for name in sorted(fo):
        if name not in mo:
            continue                               # (not a kernel: no descriptor)
        h = hashlib.sha256("\n".join(fo[name]).encode()).hexdigest()[:16]
        if name not in fn:
            lines.append(f"MISSING   {name}")
            bad += 1
            continue
        same_text = fo[name] == fn[name]
        same_meta = mo[name] == mn.get(name)
        fig = " ".join(f"{k[1:]}={mo[name].get(k, '?')}" for k in FIELDS[:5])
        lines.append(f"{'same' if same_text and same_meta else 'DIFFERENT'}  {len(fo[name]):6d} instructions  sha256 {h}  {fig}  {name}")
        if not same_text:
            k = next((i for i, (a, b) in enumerate(zip(fo[name], fn[name])) if a != b), min(len(fo[name]), len(fn[name])))
            lines.append(f"    first difference at instruction {k}: {fo[name][k:k + 1]} -> {fn[name][k:k + 1]}")
        if not same_meta:
            lines.append(f"    metadata: {mo[name]} -> {mn.get(name)}")
        bad += 0 if same_text and same_meta else 1
    added = [n for n in sorted(fn) if n not in fo and n in mn]
    for name in added:
        fig = " ".join(f"{k[1:]}={mn[name].get(k, '?')}" for k in FIELDS[:5])
        lines.append(f"new       {len(fn[name]):6d} instructions  {fig}  {name}")
    nk = sum(1 for n in fo if n in mo)
    lines.append(f"{nk} pre-existing kernels compared, {bad} different or missing, {len(added)} new")
    return lines, bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("old", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("--out", type=Path)
    a = ap.parse_args()
    lines, bad = compare(a.old, a.new)
    text = "\n".join(lines) + "\n"
    if a.out:
        a.out.write_text(text)
    sys.stdout.write(text)
    sys.exit(1 if bad else 0)
