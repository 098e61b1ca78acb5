"""The fp16 compute mode (AF_DTYPE_F16: fp16 storage, v_mfma_f32_32x32x16_f16, fp32 accumulation), what can be checked
without a GPU: the enum and its Python names, the drop-in modules' set_compute_dtype, the command line, and -- read from the
built gfx950 code objects -- that the four-wave GEMM / convolution kernel and the flash attention kernel exist for _Float16
and multiply on the F16 MFMA, never on the BF16 one.  The arithmetic is tested on the GPU (tests/test_fp16_gpu.py)."""
import functools
import importlib.util
import re
import sys
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


# ----------------------------------------------------------------------------------------------------------------------
# interface
# ----------------------------------------------------------------------------------------------------------------------
def test_header_and_python_names_agree():
    from adaface_amd import _lib
    header = (ROOT / "include" / "adaface_hip.h").read_text()
    m = re.search(r"enum\s*\{([^}]*AF_DTYPE_BF16[^}]*)\}", header)
    assert m, "dtype enum not found"
    enum = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m[1].split(",")))
    assert enum == {"AF_DTYPE_BF16": 0, "AF_DTYPE_F32": 1, "AF_DTYPE_F16": 2}, enum
    assert _lib.AF_DTYPE_F16 == 2
    assert _lib.DTYPES["f16"] == _lib.DTYPES["fp16"] == _lib.DTYPES["float16"] == 2
    # the other names keep their values
    assert _lib.DTYPES["bf16"] == 0 and _lib.DTYPES["f32"] == 1 and _lib.DTYPES["fp32"] == 1


def _tiny_model():
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    return instantiate_from_config(tiny_config()["model"]).eval()


@pytest.fixture(scope="module")
def tiny_model():
    return _tiny_model()


def _fake_engine(module):
    """A stand-in for a live engine: set_compute_dtype must close and drop it when the mode changes."""
    class _E:
        closed = False

        def close(self):
            self.closed = True
    e = _E()
    object.__setattr__(module, "_engine", e)
    object.__setattr__(module, "_weights_dirty", False)
    return e


@pytest.mark.parametrize("name", ["fp16", "f16"])
def test_hipmodule_set_compute_dtype_fp16(tiny_model, name):
    unet = tiny_model.model.diffusion_model
    unet.set_compute_dtype("bf16")
    e = _fake_engine(unet)
    assert unet.set_compute_dtype(name) is unet
    assert unet.compute_dtype == "f16"
    assert e.closed and unet._engine is None and unet._weights_dirty          # as for every other change of mode
    # the same mode again keeps a live engine
    e2 = _fake_engine(unet)
    unet.set_compute_dtype("fp16")
    assert unet._engine is e2 and not e2.closed and unet.compute_dtype == "f16"
    object.__setattr__(unet, "_engine", None)
    # ... and leaving it drops the engine again
    e3 = _fake_engine(unet)
    unet.set_compute_dtype("bf16")
    assert e3.closed and unet._engine is None and unet.compute_dtype == "bf16"


def test_latent_diffusion_set_compute_dtype_fp16(tiny_model):
    m = tiny_model
    assert m.set_compute_dtype("fp16") is m
    assert m.model.diffusion_model.compute_dtype == "f16"
    assert m.first_stage_model.compute_dtype == "f16"
    assert m.cond_stage_model is not None and m.cond_stage_model.compute_dtype == "f16"
    m.set_compute_dtype("bf16")
    assert m.model.diffusion_model.compute_dtype == m.first_stage_model.compute_dtype == "bf16"


@pytest.mark.parametrize("name", ["fp16", "f16", "bf16"])
def test_fp8_scope_is_refused_with_fp16_as_with_bf16(tiny_model, name):
    tiny_model.set_compute_dtype("bf16")
    with pytest.raises(ValueError):
        tiny_model.set_compute_dtype(name, fp8_scope="base+ff")
    assert tiny_model.model.diffusion_model.compute_dtype == "bf16"           # nothing changed


def test_unknown_dtype_still_raises(tiny_model):
    for bad in ("fp17", "half", "float16", ""):
        with pytest.raises(ValueError):
            tiny_model.model.diffusion_model.set_compute_dtype(bad)
        with pytest.raises(ValueError):
            tiny_model.set_compute_dtype(bad)


def test_txt2img_parser_accepts_fp16(monkeypatch):
    spec = importlib.util.spec_from_file_location("stable_txt2img_cli", ROOT / "scripts" / "stable_txt2img.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["stable_txt2img.py", "--dtype", "fp16"])
    assert mod.parse_args().dtype == "fp16"
    monkeypatch.setattr(sys, "argv", ["stable_txt2img.py", "--dtype", "fp17"])
    with pytest.raises(SystemExit):
        mod.parse_args()


# ----------------------------------------------------------------------------------------------------------------------
# the built code objects
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _functions(obj_name):
    from adaface_amd import _lib, build
    obj = ROOT / "adaface_amd" / "_build" / obj_name
    if not _lib.lib_path().exists() or not obj.exists():
        build.build(verbose=False)        # (a fresh tree only, as tests/test_isa_budget.py does)
    spec = importlib.util.spec_from_file_location("check_isa_hazards", ROOT / "scripts" / "check_isa_hazards.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as td:
        funcs = mod.disassemble(obj, Path(td))
    assert funcs, obj
    return funcs


def _assert_f16_mfma_only(name, ins):
    mfma = {t.split()[0] for t in ins if t.startswith("v_mfma")}
    assert mfma == {"v_mfma_f32_32x32x16_f16"}, (name, sorted(mfma))


def test_conv_gemm_kernel_exists_for_fp16_on_the_f16_mfma():
    # conv_gemm_kernel<_Float16, BM, BN, DMA>: _Z16conv_gemm_kernelIDF16_Li<BM>ELi<BN>ELb<DMA>EEv14ConvGemmParams
    pat = re.compile(r"^_Z16conv_gemm_kernelIDF16_Li(\d+)ELi(\d+)ELb([01])EEv")
    found = {}
    for name, ins in _functions("af_conv_gemm.hip.o"):
        m = pat.match(name)
        if m:
            found[(int(m[1]), int(m[2]), m[3] == "1")] = (name, ins)
    want = {(bm, bn, dma) for bm in (128, 64) for bn in (128, 64) for dma in (False, True)}
    assert set(found) == want, sorted(set(found) ^ want)
    for name, ins in found.values():
        _assert_f16_mfma_only(name, ins)


def test_halo_and_splitk_kernels_exist_for_fp16():
    names = [n for n, _ in _functions("af_conv_gemm.hip.o")]
    for tw in (32, 16):
        for bn in (128, 64):
            assert f"_Z19conv3x3_halo_kernelIDF16_Li{tw}ELi{bn}EEv14ConvGemmParams" in names, (tw, bn)
    assert "_Z20splitk_reduce_kernelIDF16_Ev14ConvGemmParams" in names
    for n, ins in _functions("af_conv_gemm.hip.o"):
        if n.startswith("_Z19conv3x3_halo_kernelIDF16_"):
            _assert_f16_mfma_only(n, ins)


def test_attn_kernel_exists_for_fp16_on_the_f16_mfma():
    pat = re.compile(r"^_Z11attn_kernelIDF16_Li(\d+)EEv10AttnParams$")
    found = {}
    for name, ins in _functions("af_attention.hip.o"):
        m = pat.match(name)
        if m:
            found[int(m[1])] = (name, ins)
    assert {40, 64, 80, 160} <= set(found), sorted(found)
    for name, ins in found.values():
        _assert_f16_mfma_only(name, ins)
        # P^T goes back in as an fp16 MFMA operand: the accumulator is converted, never bit-truncated as bf16 would allow
        assert any(t.startswith("v_cvt_pk_f16_f32") or t.startswith("v_cvt_f16_f32") for t in ins), name


def test_eight_wave_kernels_are_not_instantiated_for_fp16():
    """The ring, short-key, fused cross-attention and eight-wave GEMM kernels stay bf16-only: nothing else in the code objects
    carries the _Float16 type."""
    allowed = ("conv_gemm_kernel", "conv3x3_halo_kernel", "splitk_reduce_kernel", "attn_kernel")
    for obj in ("af_conv_gemm.hip.o", "af_attention.hip.o"):
        for name, _ in _functions(obj):
            if "DF16_" in name:
                assert any(k in name for k in allowed) and "attn_kernel_w4" not in name, name
    for obj in ("af_conv_s8.hip.o", "af_xattn_fused.hip.o"):
        assert not [n for n, _ in _functions(obj) if "DF16_" in n]
