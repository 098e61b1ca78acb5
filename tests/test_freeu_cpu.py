"""CPU tests of FreeU: the closed form the kernels use against the torch.fft filter of the reference (tests/freeu_ref.py), the
restated U-Net walk with FreeU off against the oracle, the sites, the new C symbols in header, binding and library, the host-only
plan query, argument validation and the CLI flags."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import freeu_ref as FR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

SYMS = ("af_set_freeu", "af_freeu_num_sites", "af_freeu_site", "af_freeu_plan_query", "af_op_freeu")


# ------------------------------------------------------------------ the reference itself ----------------------------
@pytest.mark.parametrize("hw", [(2, 2), (2, 8), (3, 5), (4, 6), (8, 8), (16, 16), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_closed_form_is_the_fft_filter(hw):
    g = torch.Generator().manual_seed(7 + hw[0] * 100 + hw[1])
    x = torch.randn(2, 3, *hw, generator=g, dtype=torch.float64) + 3.0 * torch.randn(2, 3, 1, 1, generator=g, dtype=torch.float64)
    for s in (0.0, 0.2, 0.9, 1.0):
        ref = FR.fourier_filter(x, 1, s)
        got = FR.fourier_filter_closed(x, s)
        err = float((got - ref).abs().max())
        assert err <= 1e-12, (hw, s, err)
    assert torch.equal(FR.fourier_filter_closed(x, 1.0), x)


def test_backbone_versions():
    g = torch.Generator().manual_seed(3)
    h = torch.randn(2, 32, 4, 6, generator=g, dtype=torch.float64)
    v1 = FR.backbone(h, 1, 1.4)
    assert torch.equal(v1[:, 16:], h[:, 16:]) and torch.allclose(v1[:, :16], h[:, :16] * 1.4, rtol=0, atol=1e-15)
    v2 = FR.backbone(h, 2, 1.4)
    assert torch.equal(v2[:, 16:], h[:, 16:])
    ratio = (v2[:, :16] / h[:, :16])
    assert float(ratio.min()) >= 1.0 - 1e-12 and float(ratio.max()) <= 1.4 + 1e-12
    # the factor is 1 at the pixel of the smallest channel mean and b at the largest, per sample
    m = h.mean(1).view(2, -1)
    for b in range(2):
        r = ratio[b, 0].reshape(-1)
        assert abs(float(r[m[b].argmin()]) - 1.0) < 1e-12 and abs(float(r[m[b].argmax()]) - 1.4) < 1e-12


def test_walk_with_freeu_off_is_the_oracle():
    cfg = O.TINY_UNET
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=11)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 16, 16, generator=g)
    t = torch.tensor([981, 1])
    ctx = torch.randn(2 * 16, 77, cfg.context_dim, generator=g)
    with torch.no_grad():
        ref = O.unet_forward(sd, cfg, x, t, ctx)
        assert torch.equal(FR.unet_forward(sd, cfg, x, t, ctx), ref)
        assert torch.equal(FR.unet_forward(sd, cfg, x, t, ctx, freeu=(0, 1.3, 1.4, 0.9, 0.2)), ref)
        taps = {}
        on = FR.unet_forward(sd, cfg, x, t, ctx, freeu=(2,) + FR.V2_SD15, taps=taps)
    assert torch.isfinite(on).all() and not torch.equal(on, ref)
    assert sorted(int(k.split(".")[1]) for k in taps if k.startswith("freeu.")) == list(range(10))


@pytest.mark.parametrize("cfg", [O.SD15_UNET, O.TINY_UNET], ids=["sd15", "tiny"])
def test_sites(cfg):
    s = FR.sites(cfg)
    mc = cfg.model_channels
    assert [e[0] for e in s] == list(range(10))
    assert [e[3] for e in s] == [0] * 7 + [1] * 3
    assert [e[1] for e in s] == [4 * mc] * 7 + [2 * mc] * 3
    assert [e[2] for e in s] == [4 * mc] * 5 + [2 * mc] * 3 + [mc] * 2


# ------------------------------------------------------------------ the library, host only --------------------------
def test_header_binding_and_library_have_the_symbols():
    from adaface_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "adaface_hip.h").read_text(), flags=re.S)
    if not _lib.lib_path().exists():
        build.build(verbose=False)
    exported = subprocess.run(["nm", "-D", "--defined-only", os.fspath(_lib.lib_path())], check=True, capture_output=True,
                              text=True).stdout
    for s in SYMS:
        assert re.search(rf"\bint\s+{s}\s*\(", text), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert re.search(rf"\sT\s+{s}$", exported, flags=re.M), s
    assert "af_freeu.hip" in build.SOURCES
    # null handles are refused on the host, with a message and without a device
    lib = _lib.load()
    assert lib.af_set_freeu(None, 1, 1.2, 1.4, 0.9, 0.2) == -1 and b"af_set_freeu" in lib.af_last_error()
    assert lib.af_freeu_site(None, 0, None) == -1 and b"af_freeu_site" in lib.af_last_error()
    assert lib.af_freeu_num_sites(None) == 0
    assert lib.af_freeu_plan_query(0, 8, 8, 64, 64, 1, None) == -1


@pytest.mark.parametrize("dtype", ["bf16", "f32", "f16"])
def test_plan_query(dtype):
    from adaface_amd import _lib
    q = _lib.freeu_plan_query
    # up to 256 pixels: sums and apply in one launch, no partial sums; version 2 takes one launch more
    for hw in ((2, 2), (8, 8), (4, 2), (16, 16), (2, 128)):
        assert q(dtype, *hw, 1280, 640, 1) == {"kernel": "single", "launches": 1, "chunks": 1, "partial_bytes": 0}, hw
        assert q(dtype, *hw, 1280, 640, 2) == {"kernel": "single", "launches": 2, "chunks": 1, "partial_bytes": 0}, hw
    # above: one partial [7][Cs] fp32 per 256-pixel chunk
    assert q(dtype, 16, 17, 64, 32, 1) == {"kernel": "chunked", "launches": 2, "chunks": 2, "partial_bytes": 2 * 7 * 32 * 4}
    assert q(dtype, 32, 32, 1280, 640, 1) == {"kernel": "chunked", "launches": 2, "chunks": 4, "partial_bytes": 4 * 7 * 640 * 4}
    assert q(dtype, 64, 64, 640, 320, 2) == {"kernel": "chunked", "launches": 3, "chunks": 16, "partial_bytes": 16 * 7 * 320 * 4}
    assert q(dtype, 16, 8, 16, 8, 1)["kernel"] == "single"                      # the narrowest widths the kernels take
    for bad in ((1, 8, 64, 64, 1), (8, 1, 64, 64, 1), (1, 1, 64, 64, 2), (0, 8, 64, 64, 1), (8, 8, 72, 64, 1), (8, 8, 8, 64, 1),
                (8, 8, 64, 60, 1), (8, 8, 64, 4, 1), (8, 8, 0, 64, 1), (8, 8, 64, 0, 1), (8, 8, 64, 64, 0), (8, 8, 64, 64, 3)):
        with pytest.raises(_lib.AfError, match="FreeU"):
            q(dtype, *bad)


def test_plan_query_refuses_an_unknown_dtype():
    from adaface_amd import _lib
    with pytest.raises(_lib.AfError):
        _lib.freeu_plan_query(7, 8, 8, 64, 64, 1)


def test_set_freeu_argument_validation():
    from adaface_amd.engine import check_freeu_args
    assert check_freeu_args(1, 1.2, 1.4, 0.9, 0.2) == (1, 1.2, 1.4, 0.9, 0.2)
    assert check_freeu_args(2, 1, 2, 0, 1) == (2, 1.0, 2.0, 0.0, 1.0)
    assert check_freeu_args(0) == (0, 1.0, 1.0, 1.0, 1.0) and check_freeu_args(0, 9, 9, 9, 9) == (0, 1.0, 1.0, 1.0, 1.0)   # off is always accepted
    for bad in ((3, 1.2, 1.4, 0.9, 0.2), (-1, 1.2, 1.4, 0.9, 0.2), (True, 1.2, 1.4, 0.9, 0.2), (1.5, 1.2, 1.4, 0.9, 0.2),
                (None, 1.2, 1.4, 0.9, 0.2), (1, 0.9, 1.4, 0.9, 0.2), (1, 1.2, 2.1, 0.9, 0.2), (1, 1.2, 1.4, -0.1, 0.2),
                (1, 1.2, 1.4, 0.9, 1.1), (2, float("nan"), 1.4, 0.9, 0.2), (2, 1.2, 1.4, "0.9", 0.2), (2, 1.2, None, 0.9, 0.2),
                (1, True, 1.4, 0.9, 0.2)):
        with pytest.raises(ValueError, match="FreeU"):
            check_freeu_args(*bad)
    # the model-level setter validates before it needs an engine, and keeps the setting for the engine it will build
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    unet = instantiate_from_config(tiny_config()["model"]["params"]["unet_config"])
    assert unet.freeu == (0, 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        unet.set_freeu(3, 1.2, 1.4, 0.9, 0.2)
    with pytest.raises(ValueError):
        unet.set_freeu(1, 2.5, 1.4, 0.9, 0.2)
    assert unet.freeu == (0, 1.0, 1.0, 1.0, 1.0)
    assert unet.set_freeu(2, *FR.V2_SD15) is unet and unet.freeu == (2,) + FR.V2_SD15
    for dt in ("f16", "fp8", "f32", "bf16"):                            # every compute dtype keeps it
        assert unet.set_compute_dtype(dt).freeu == (2,) + FR.V2_SD15
    assert unet.set_token_merging(0.5).freeu == (2,) + FR.V2_SD15       # and token merging composes
    assert unet.set_freeu(0).freeu == (0, 1.0, 1.0, 1.0, 1.0)


def test_cli_flags_parse(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("stable_txt2img_cli_freeu", ROOT / "scripts" / "stable_txt2img.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    opt = cli.parse_args(["--synthetic"])
    assert opt.freeu is None and opt.freeu_version == 1
    opt = cli.parse_args(["--synthetic", "--freeu", "1.2", "1.4", "0.9", "0.2"])
    assert opt.freeu == [1.2, 1.4, 0.9, 0.2] and opt.freeu_version == 1
    opt = cli.parse_args(["--synthetic", "--freeu", "1.3", "1.4", "0.9", "0.2", "--freeu_version", "2", "--deep_cache", "3",
                          "--dpm_solver", "--ddim_steps", "20", "--gpus", "2", "--tome", "0.5"])
    assert opt.freeu == [1.3, 1.4, 0.9, 0.2] and opt.freeu_version == 2 and opt.deep_cache == 3 and opt.gpus == 2 and opt.tome == 0.5
    for dt in ("bf16", "f32", "fp16", "fp8"):
        assert cli.parse_args(["--synthetic", "--dtype", dt, "--freeu", "1", "2", "0", "1"]).freeu == [1.0, 2.0, 0.0, 1.0]
    assert cli.parse_args(["--synthetic", "--plms", "--freeu", "1.2", "1.4", "0.9", "0.2"]).plms
    for bad in (["--synthetic", "--freeu", "1.2", "1.4", "0.9"], ["--synthetic", "--freeu", "0.9", "1.4", "0.9", "0.2"],
                ["--synthetic", "--freeu", "1.2", "2.1", "0.9", "0.2"], ["--synthetic", "--freeu", "1.2", "1.4", "-0.1", "0.2"],
                ["--synthetic", "--freeu", "1.2", "1.4", "0.9", "1.5"], ["--synthetic", "--freeu", "1.2", "1.4", "0.9", "0.2", "--freeu_version", "3"],
                ["--synthetic", "--freeu", "1.2", "1.4", "0.9", "x"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code == 2, bad
    assert "--freeu" in capsys.readouterr().err
