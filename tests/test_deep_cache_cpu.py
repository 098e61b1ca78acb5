"""CPU tests of DeepCache: the reference restatement (tests/deep_cache_ref.py) against the oracle's full forward at the same
input, the refresh schedule, the per-run bookkeeping of the samplers, and the two new C symbols."""
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
import deep_cache_ref as DR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

SYMS = ("af_unet_forward_cached", "af_unet_cache_invalidate")


@pytest.fixture(scope="module")
def full_run():
    """One full oracle forward on TINY_UNET, B = 3 at 32 x 16, with every tap: shared by the identity cases."""
    cfg = O.TINY_UNET
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=11)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 4, 32, 16, generator=g)
    t = torch.tensor([981, 500, 1])
    ctx = torch.randn(3 * 16, 77, cfg.context_dim, generator=g)
    taps = {}
    with torch.no_grad():
        eps = O.unet_forward(sd, cfg, x, t, ctx, taps=taps)
    return sd, cfg, x, t, ctx, eps, taps


@pytest.mark.parametrize("k", [1, 2, 3, 4, 11])
def test_shallow_reference_equals_full_forward_at_the_same_input(full_run, k):
    sd, cfg, x, t, ctx, eps, taps = full_run
    assert DR.n_blocks(cfg) == (12, 12)
    got_taps = {}
    with torch.no_grad():
        got = DR.shallow_forward(sd, cfg, x, t, ctx, taps[DR.kept_name(cfg, k)], k, taps=got_taps)
    assert torch.equal(got, eps)
    assert sorted(got_taps) == sorted([f"input_blocks.{i}" for i in range(k)] + [f"output_blocks.{12 - 1 - i}" for i in range(k)])
    for name, v in got_taps.items():
        assert torch.equal(v, taps[name]), name


def test_shallow_reference_keeps_the_cross_attention_layer_index(full_run):
    """With a layerwise context whose 16 slices differ, a renumbered layer (0, 1, 2 instead of 0, 14, 15 at k = 2) would not
    reproduce the full forward; feeding the slices of layers 1, 2 to the output blocks must change the result."""
    sd, cfg, x, t, ctx, eps, taps = full_run
    B = x.shape[0]
    wrong = ctx.reshape(B, 16, 77, -1).clone()
    wrong[:, 14], wrong[:, 15] = wrong[:, 1].clone(), wrong[:, 2].clone()
    with torch.no_grad():
        got = DR.shallow_forward(sd, cfg, x, t, wrong.reshape(ctx.shape), taps[DR.kept_name(cfg, 2)], 2)
    assert not torch.equal(got, eps)


def test_cached_apply_model_follows_its_schedule(full_run):
    sd, cfg, x, t, ctx, eps, _ = full_run
    m = DR.CachedApplyModel(sd, cfg, [True, False, False], 3)
    with torch.no_grad():
        a, b, c = m(x, t, ctx), m(x, t, ctx), m(x + 0.05, t, ctx)
    assert m.log == ["refresh", "reuse", "reuse"]
    assert torch.equal(a, eps) and torch.equal(b, eps) and not torch.equal(c, eps)


# ------------------------------------------------------------------ schedule ----------------------------------------
def test_refresh_steps():
    from adaface_amd.ldm.models.diffusion.deep_cache import is_off, refresh_steps
    assert refresh_steps(7, None) == [True] * 7 and refresh_steps(7, 1) == [True] * 7
    assert refresh_steps(7, 3) == [True, False, False, True, False, False, True]
    assert refresh_steps(5, 2) == [True, False, True, False, True]
    assert refresh_steps(6, [0, 1, 4]) == [True, True, False, False, True, False]
    assert refresh_steps(3, (0, 9)) == [True, False, False]
    assert refresh_steps(0, 4) == []
    for bad in ([1, 3], [], 0, -2, 2.5, True, [0, -1]):
        with pytest.raises(ValueError):
            refresh_steps(7, bad)
    assert is_off(None) and is_off(1) and not is_off(2) and not is_off([0])


def test_run_bookkeeping_forces_a_refresh_when_the_call_form_changes():
    from adaface_amd.ldm.models.diffusion.deep_cache import DeepCacheRun

    class Engineless:
        pass

    class WithEngine:
        supports_deep_cache = True
    twin, single = (True, 1, 16, 16), (False, 1, 16, 16)
    run = DeepCacheRun(WithEngine(), 5, 100, 2)
    got = [run.step(i, f) for i, f in enumerate([twin, twin, single, single, twin])]
    assert got == [("refresh", 2), ("reuse", 2), ("refresh", 2), ("reuse", 2), ("refresh", 2)]
    assert run.log == ["refresh", "reuse", "refresh", "reuse", "refresh"]
    for model, interval in ((WithEngine(), None), (WithEngine(), 1), (Engineless(), 3)):
        run = DeepCacheRun(model, 3, interval, 2)
        assert [run.step(i, twin) for i in range(3)] == [None] * 3 and run.log == ["full"] * 3
    with pytest.raises(ValueError):
        DeepCacheRun(WithEngine(), 3, [1, 2], 2)
    with pytest.raises(ValueError):
        DeepCacheRun(WithEngine(), 3, 2, 0)


# ------------------------------------------------------------------ interface ---------------------------------------
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
    assert re.search(r"AF_DEEPCACHE_REFRESH\s*=\s*1\b", text) and re.search(r"AF_DEEPCACHE_REUSE\s*=\s*2\b", text)
    assert _lib.DEEPCACHE_MODES == {"refresh": 1, "reuse": 2}
    # both refuse a null handle on the host, with a message and without a device
    lib = _lib.load()
    assert lib.af_unet_cache_invalidate(None) == -1
    assert lib.af_unet_forward_cached(None, None, None, None, 2, 16, 16, 0, 2, 1, None) == -1


# ------------------------------------------------------------------ CLI ---------------------------------------------
def test_cli_flags_parse(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("stable_txt2img_cli", ROOT / "scripts" / "stable_txt2img.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    opt = cli.parse_args(["--synthetic"])
    assert opt.deep_cache is None and opt.deep_cache_depth == 2
    opt = cli.parse_args(["--synthetic", "--deep_cache", "3"])
    assert opt.deep_cache == 3 and opt.deep_cache_depth == 2
    opt = cli.parse_args(["--synthetic", "--dpm_solver", "--ddim_steps", "20", "--deep_cache", "2", "--deep_cache_depth", "3"])
    assert opt.dpm_solver and opt.deep_cache == 2 and opt.deep_cache_depth == 3
    assert cli.parse_args(["--synthetic", "--plms", "--deep_cache", "1"]).plms          # 1 is off
    for bad in (["--synthetic", "--plms", "--deep_cache", "3"], ["--synthetic", "--deep_cache", "0"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code == 2, bad
    assert "--deep_cache" in capsys.readouterr().err


def test_plms_sampler_refuses_before_it_touches_the_model():
    from adaface_amd.ldm.models.diffusion.plms import PLMSSampler

    class NoDeviceModel:
        num_timesteps = 1000
    with pytest.raises(NotImplementedError):
        PLMSSampler(NoDeviceModel()).sample(S=6, batch_size=1, shape=[4, 16, 16], deep_cache_interval=3)
