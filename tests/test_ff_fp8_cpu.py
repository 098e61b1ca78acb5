"""FeedForward scope of the fp8 mode, the host side (no GPU): the new symbols in the header, the binding and the library; the
scope parsing of the Python layers; scale files belong to the scope they were made under; and the exact probe of
tests/test_ff_fp8_gpu.py meets its preconditions on the reference alone."""
import ctypes
import os
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("af_set_fp8_scope", "af_get_fp8_scope", "af_ff8_launches", "af_op_ff_fp8")


def test_new_symbols_in_header_binding_and_library():
    from adaface_amd import _lib, build
    header = (ROOT / "include" / "adaface_hip.h").read_text()
    declared = set(re.findall(r"\b(af_[a-z0-9_]+)\s*\(", header))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in _lib.EXPORTED_SYMBOLS, s
    assert re.search(r"#define\s+AF_FP8_SCOPE_BASE\s+1\b", header) and re.search(r"#define\s+AF_FP8_SCOPE_FF\s+2\b", header)
    if not _lib.lib_path().exists():
        build.build(verbose=False)
    cdll = ctypes.CDLL(os.fspath(_lib.lib_path()))
    for s in NEW_SYMBOLS:
        assert hasattr(cdll, s), s
    # host-only entry points answer without a device: no handle -> scope 0, the launch counter starts at 0
    lib = _lib.load()
    assert lib.af_get_fp8_scope(None) == 0
    assert lib.af_set_fp8_scope(None, 3) != 0
    assert lib.af_ff8_launches() == 0


def test_scope_parsing():
    from adaface_amd.fp8_calib import FP8_SCOPE_BASE, FP8_SCOPE_FF, fp8_scope_names, parse_fp8_scope
    assert (FP8_SCOPE_BASE, FP8_SCOPE_FF) == (1, 2)
    assert parse_fp8_scope("base") == parse_fp8_scope(("base",)) == parse_fp8_scope(1) == 1
    assert parse_fp8_scope("base+ff") == parse_fp8_scope(("base", "ff")) == parse_fp8_scope(["ff", "base"]) == parse_fp8_scope(3) == 3
    assert fp8_scope_names(1) == ("base",) and fp8_scope_names(3) == ("base", "ff")
    for bad in ("ff", ("ff",), "", "base+conv", "base,ff", 0, 2, 4, 7, True, ("base", 2)):
        with pytest.raises(ValueError):
            parse_fp8_scope(bad)


def test_dropin_modules_keep_the_scope_without_an_engine():
    """The UNet drop-in holds the scope as it holds the shifts (the engine is rebuilt on dtype / device changes); a scope change
    drops calibrated shifts (they name the sites of the scope they were made under); LatentDiffusion.set_compute_dtype
    takes fp8_scope with the default 'base' and refuses it for other dtypes."""
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    unet = instantiate_from_config(tiny_config()["model"]["params"]["unet_config"]).eval()
    assert unet.fp8_scope == ("base",)
    unet.set_fp8_shifts({"a": 1})
    assert unet.set_fp8_scope("base") is unet and unet.fp8_shifts() == {"a": 1}        # no change: shifts stay
    unet.set_fp8_scope("base+ff")
    assert unet.fp8_scope == ("base", "ff") and unet.fp8_shifts() is None
    unet.set_compute_dtype("fp8").set_compute_dtype("bf16")
    assert unet.fp8_scope == ("base", "ff")                                          # kept across dtype switches
    unet.set_fp8_scope(("base",))
    assert unet.fp8_scope == ("base",)
    for bad in ("ff", "wide", 2):
        with pytest.raises(ValueError):
            unet.set_fp8_scope(bad)
    assert unet.fp8_scope == ("base",)
    model = instantiate_from_config(tiny_config()["model"]).eval()
    du = model.model.diffusion_model
    assert model.set_compute_dtype("fp8") is model and du.compute_dtype == "fp8" and du.fp8_scope == ("base",)
    model.set_compute_dtype("fp8", fp8_scope="base+ff")
    assert du.fp8_scope == ("base", "ff") and model.first_stage_model.compute_dtype == "bf16"
    model.set_compute_dtype("fp8")
    assert du.fp8_scope == ("base",)
    with pytest.raises(ValueError):
        model.set_compute_dtype("bf16", fp8_scope="base+ff")
    with pytest.raises(ValueError):
        model.set_compute_dtype("fp8", fp8_scope="ff")
    assert du.compute_dtype == "fp8" and du.fp8_scope == ("base",)                   # a refused call changes nothing


def test_scale_files_belong_to_their_scope(tmp_path):
    """No format change: the exact-names rule of load_scales refuses a base-scope file under the wide scope and a wide-scope
    file under the base scope."""
    from adaface_amd.fp8_calib import load_scales, save_scales
    base = [f"model.diffusion_model.input_blocks.{i}.0.in_layers.2.weight" for i in (1, 2, 4)]
    base.append("model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight")
    ff = ["model.diffusion_model.input_blocks.1.1.transformer_blocks.0.ff.net.0.proj.weight",
          "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.ff.net.2.weight"]
    p_base, p_wide = tmp_path / "base.json", tmp_path / "wide.json"
    save_scales(p_base, {n: 3 for n in base})
    save_scales(p_wide, {n: 2 for n in base + ff})
    assert load_scales(p_base, base) == {n: 3 for n in base}
    assert load_scales(p_wide, base + ff) == {n: 2 for n in base + ff}
    with pytest.raises(KeyError):
        load_scales(p_base, base + ff)
    with pytest.raises(KeyError):
        load_scales(p_wide, base)


@pytest.mark.parametrize("M,C", [(2048, 320), (1100, 640)])
def test_exact_probe_preconditions_hold_on_the_reference(M, C):
    """value * 8 * 2^s is exact in torch.float8_e4m3fn for the three shifts, >= 85 % of the outputs are non-zero, >= 24
    distinct values; the chain's operands pass check_exact_case (asserted inside chain_operands)."""
    from tests.test_ff_fp8_gpu import chain_operands, check_probe_reference, probe_operands
    p = probe_operands(M, C, seed=M + C)
    for shift in (-2, 0, 1):
        want, nonzero, distinct = check_probe_reference(p, shift)
        assert want.dtype == torch.uint8 and tuple(want.shape) == (M, 4 * C)
        # +1 / -1 / 0 of the input and 8 * 2^s of a unit value have the codes the kernel will see
        assert nonzero >= 0.85 and distinct >= 24
    ch = chain_operands(p["value"] * 8.0, C, seed=M + C + 5)
    assert ch["stats"]["absbound"] < 2 ** 24 and ch["stats"]["nonzero"] >= 0.9
    x8 = p["x"].to(torch.float8_e4m3fn).view(torch.uint8)
    assert set(x8.unique().tolist()) == {0x00, 0x38, 0xB8}
