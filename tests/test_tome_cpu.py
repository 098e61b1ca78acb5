"""CPU tests of token merging: the plan query against the reference restatement (tests/tome_ref.py), the new C symbols in
header, binding and library, argument validation, the CLI flags, and two identities of the reference itself."""
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
import tome_ref as TR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

SYMS = ("af_set_tome", "af_tome_plan_query", "af_tome_num_sites", "af_tome_set_tap", "af_op_tome_match", "af_op_tome_merge",
        "af_op_tome_unmerge_add")


@pytest.mark.parametrize("hw", [(8, 8), (6, 10), (64, 64)])
@pytest.mark.parametrize("ratio", [0.0, 0.25, 0.5, 0.7, 0.75])
def test_plan_query_matches_the_reference(hw, ratio):
    from adaface_amd import _lib
    got = _lib.tome_plan_query(*hw, ratio)
    assert got == TR.plan(*hw, ratio), (got, TR.plan(*hw, ratio))
    Nd, Ns, r, n_rows = got
    assert Nd + Ns == hw[0] * hw[1] and n_rows == Nd + Ns - r and 0 <= r <= Ns
    if ratio == 0.75:
        assert r == Ns


def test_plan_values():
    """Spelled out, independent of both implementations: 64 x 64 at 0.5 merges 2048 of 3072 src tokens; 0.7 truncates."""
    from adaface_amd import _lib
    assert _lib.tome_plan_query(64, 64, 0.5) == (1024, 3072, 2048, 2048)
    assert _lib.tome_plan_query(6, 10, 0.7) == (15, 45, 42, 18)
    assert _lib.tome_plan_query(8, 8, 0.7) == (16, 48, 44, 20)         # int(64 * 0.7) = int(44.8)


@pytest.mark.parametrize("bad", [(7, 8, 0.5), (8, 9, 0.5), (0, 8, 0.5), (8, 8, 0.76), (8, 8, -0.1), (8, 8, float("nan"))])
def test_plan_query_refusals(bad):
    from adaface_amd import _lib
    with pytest.raises(_lib.AfError):
        _lib.tome_plan_query(*bad)


def test_header_binding_and_library_have_the_symbols():
    from adaface_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "adaface_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(af_\w+)\s*\(", text))
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    if not _lib.lib_path().exists():
        build.build(verbose=False)
    exported = subprocess.run(["nm", "-D", "--defined-only", os.fspath(_lib.lib_path())], check=True, capture_output=True,
                              text=True).stdout
    for s in SYMS:
        assert re.search(rf"\bint\s+{s}\s*\(", text), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert re.search(rf"\sT\s+{s}$", exported, flags=re.M), s
    assert "af_tome.hip" in build.SOURCES
    # null handles are refused on the host, with a message and without a device
    lib = _lib.load()
    assert lib.af_set_tome(None, 0.5, 1) == -1 and b"af_set_tome" in lib.af_last_error()
    assert lib.af_tome_set_tap(None, 0, None) == -1
    assert lib.af_tome_num_sites(None) == 0
    assert lib.af_tome_plan_query(8, 8, 0.5, None) == -1


def test_set_tome_argument_validation():
    from adaface_amd.engine import check_tome_args
    assert check_tome_args(0.5) == (0.5, 1) and check_tome_args(0, 2) == (0.0, 2) and check_tome_args(0.75, 1) == (0.75, 1)
    for bad in ((0.76, 1), (-0.01, 1), (float("nan"), 1), ("0.5", 1), (None, 1), (True, 1), (0.5, 0), (0.5, 3), (0.5, 4), (0.5, 1.5),
                (0.5, True)):
        with pytest.raises(ValueError):
            check_tome_args(*bad)
    # the model-level setter validates before it needs an engine, and keeps the setting for the engine it will build
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    unet = instantiate_from_config(tiny_config()["model"]["params"]["unet_config"])
    assert unet.token_merging == (0.0, 1)
    with pytest.raises(ValueError):
        unet.set_token_merging(0.8)
    with pytest.raises(ValueError):
        unet.set_token_merging(0.5, max_downsample=4)
    assert unet.set_token_merging(0.5, 2) is unet and unet.token_merging == (0.5, 2)
    assert unet.set_token_merging(0).token_merging == (0.0, 1)
    # the pairs the library would refuse are refused here, before an engine is built, whichever side comes second
    unet.set_token_merging(0.5)
    for dt in ("fp16", "f16", "fp8"):
        with pytest.raises(ValueError, match="token merging"):
            unet.set_compute_dtype(dt)
    assert unet.compute_dtype == "bf16" and unet.set_compute_dtype("f32").compute_dtype == "f32"
    unet.set_token_merging(0)
    unet.set_compute_dtype("fp8")
    with pytest.raises(ValueError, match="token merging"):
        unet.set_token_merging(0.5)
    assert unet.set_token_merging(0).token_merging == (0.0, 1)           # (off composes with everything)


def test_cli_flags_parse(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("stable_txt2img_cli_tome", ROOT / "scripts" / "stable_txt2img.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    opt = cli.parse_args(["--synthetic"])
    assert opt.tome == 0.0 and opt.tome_max_downsample == 1
    opt = cli.parse_args(["--synthetic", "--tome", "0.5"])
    assert opt.tome == 0.5 and opt.tome_max_downsample == 1
    opt = cli.parse_args(["--synthetic", "--tome", "0.25", "--tome_max_downsample", "2", "--deep_cache", "3", "--dpm_solver",
                          "--ddim_steps", "20", "--gpus", "2"])
    assert opt.tome == 0.25 and opt.tome_max_downsample == 2 and opt.deep_cache == 3 and opt.dpm_solver and opt.gpus == 2
    assert cli.parse_args(["--synthetic", "--plms", "--tome", "0.5"]).plms
    assert cli.parse_args(["--synthetic", "--dtype", "f32", "--tome", "0.5"]).tome == 0.5
    for bad in (["--synthetic", "--tome", "0.8"], ["--synthetic", "--tome", "-0.1"], ["--synthetic", "--tome", "0.5", "--tome_max_downsample", "3"],
                ["--synthetic", "--tome", "0.5", "--dtype", "fp8"], ["--synthetic", "--tome", "0.5", "--dtype", "fp16"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code == 2, bad
    assert "--tome" in capsys.readouterr().err
    assert cli.parse_args(["--synthetic", "--dtype", "fp8"]).tome == 0.0          # (off composes with everything)


# ------------------------------------------------------------------ the reference itself ----------------------------
@pytest.mark.parametrize("hw", [(8, 8), (6, 10)])
def test_reference_partition_and_maps(hw):
    H, W = hw
    g = torch.Generator().manual_seed(5)
    t = torch.randn(3, H * W, 32, generator=g)
    dst, src = TR.partition(H, W)
    assert dst.tolist() == [y * W + x for y in range(0, H, 2) for x in range(0, W, 2)]
    assert src.tolist() == [i for i in range(H * W) if (i // W) % 2 or (i % W) % 2]
    for ratio in (0.0, 0.25, 0.5, 0.7, 0.75):
        node_idx, node_max, tmap, merged = TR.match(t, H, W, ratio)
        TR.check_map_structure(tmap, H, W, ratio)
        TR.check_map_against_scores(tmap, TR.scores(t, H, W), H, W, ratio, 0.0)
        assert float(node_max.max()) <= 1.0 + 1e-12


def test_reference_identity_at_r_zero_and_constant_rows():
    H, W = 6, 10
    g = torch.Generator().manual_seed(6)
    t = torch.randn(2, H * W, 16, generator=g).double()
    _, _, tmap, _ = TR.match(t, H, W, 0.0)
    n_rows = TR.plan(H, W, 0.0)[3]
    assert n_rows == H * W
    assert torch.equal(TR.unmerge(TR.merge(t, tmap, n_rows), tmap), t)           # a permutation and its inverse
    const = torch.full((2, H * W, 16), 0.375, dtype=torch.float64)
    for ratio in (0.25, 0.5, 0.75):
        _, _, tmap, _ = TR.match(t, H, W, ratio)
        m = TR.merge(const, tmap, TR.plan(H, W, ratio)[3])
        assert torch.equal(m, torch.full_like(m, 0.375))                         # (every row is a mean of equal rows)
        assert torch.equal(TR.unmerge(m, tmap), const)


def test_reference_tie_rules():
    """Integer scores: the lowest dst ordinal wins a tied maximum, the lower src ordinal wins a tied cut."""
    H, W = 4, 4                                   # Nd = 4, Ns = 12
    sc = torch.zeros(1, 12, 4, dtype=torch.float64)
    sc[0, :, 2] = 5.0
    sc[0, :, 3] = 5.0                             # every src token: maximum 5 at d = 2 and d = 3
    node_idx, node_max, tmap, merged = TR.match_from_scores(sc, H, W, 0.25)      # r = 4
    assert (node_idx == 2).all() and (node_max == 5).all()
    assert merged[0].tolist() == [True] * 4 + [False] * 8
    _, src = TR.partition(H, W)
    assert tmap[0, src].tolist() == [2] * 4 + list(range(4, 12))


def test_reference_model_patch_is_the_oracle_when_nothing_qualifies():
    """ratio 0 inside `patched` is the oracle's own forward bit for bit; a real ratio changes it; imposing the reference's own
    maps reproduces its own run."""
    cfg = O.TINY_UNET
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=11)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 16, 16, generator=g)
    t = torch.tensor([500])
    ctx = torch.randn(16, 77, cfg.context_dim, generator=g)
    with torch.no_grad():
        plain = O.unet_forward(sd, cfg, x, t, ctx)
        with TR.patched(0.0, 1, (16, 16)):
            assert torch.equal(O.unet_forward(sd, cfg, x, t, ctx), plain)
        log = []
        with TR.patched(0.5, 1, (16, 16), log=log):
            on = O.unet_forward(sd, cfg, x, t, ctx)
        assert len(log) == 5 == len(TR.site_sizes(cfg, 16, 16, 1)) and all(e["hw"] == (16, 16) for e in log)
        assert TR.site_sizes(cfg, 16, 16, 2) == [256] * 2 + [64] * 2 + [64] * 3 + [256] * 3
        assert not torch.equal(on, plain) and torch.isfinite(on).all()
        with TR.patched(0.5, 1, (16, 16), maps=[e["map"] for e in log]):
            assert torch.equal(O.unet_forward(sd, cfg, x, t, ctx), on)
    assert O.spatial_transformer.__module__ == "oracle.ldm_oracle"
