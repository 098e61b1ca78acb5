"""CPU tests of img2img by strength and inpainting (no GPU): the mask preparation, the strength -> n -> ts[:n] arithmetic on
the three samplers' grids, the host-side refusals of af_noise_blend and of the Python layers, the CLI's flags and refusals, the
sharding of images by global sample index, and the ABI."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import dpmpp_ref as R  # noqa: E402
import inpaint_ref as IR  # noqa: E402


# ------------------------------------------------------------------ mask preparation -------------------------------
def test_repaint_to_keep_hand_written():
    """A 16 x 24 mask at f = 8 is 2 x 3 latent cells.  One white pixel in a cell repaints the cell; 0.5 is not white; a grey
    0.51 is; the keep mask is the complement."""
    from adaface_amd.img2img import repaint_to_keep
    m = torch.zeros(2, 1, 16, 24)
    m[0, 0, 7, 7] = 1.0           # cell (0, 0): its last pixel
    m[0, 0, 8, 16] = 0.51         # cell (1, 2): its first pixel, just white
    m[0, 0, 3, 12] = 0.5          # cell (0, 1): not above the threshold
    m[1, 0, 8:, :] = 1.0          # sample 1: the lower row of cells
    keep = repaint_to_keep(m, f=8)
    want = torch.tensor([[[[0., 1., 1.], [1., 1., 0.]]], [[[1., 1., 1.], [0., 0., 0.]]]])
    assert keep.shape == (2, 1, 2, 3) and torch.equal(keep, want)
    assert torch.equal(repaint_to_keep(torch.zeros(1, 1, 8, 8)), torch.ones(1, 1, 1, 1))
    assert torch.equal(repaint_to_keep(m, f=4)[0, 0, 1, 1], torch.tensor(0.))       # (7, 7) lies in cell (1, 1) at f = 4
    for bad in (torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 1, 12, 8)):
        with pytest.raises(ValueError):
            repaint_to_keep(bad)


# ------------------------------------------------------------------ strength ---------------------------------------
@pytest.fixture(scope="module")
def acp():
    return R.sd_acp()


@pytest.mark.parametrize("S", [6, 10, 20])
def test_strength_arithmetic_on_the_three_grids(acp, S):
    """n = min(len, max(1, int(len * strength))) and the executed timesteps ts[:n], largest first, on DDIM's grid (which is
    PLMS's: both call make_ddim_timesteps) and on DPM-Solver++'s two grids; the table of a DPM-Solver++ run by strength is
    dpmpp_schedule on ts[:n]."""
    from adaface_amd.ldm.models.diffusion import dpm_solver as D
    from adaface_amd.ldm.models.diffusion.blend import strength_steps, strength_timesteps
    from adaface_amd.ldm.modules.diffusionmodules.util import make_ddim_timesteps
    ddim = np.asarray(make_ddim_timesteps("uniform", S, 1000, verbose=False))
    grids = {"ddim / plms": ddim, "dpm time_uniform": D.dpmpp_timesteps(acp, S, "time_uniform"),
             "dpm logSNR": D.dpmpp_timesteps(acp, S, "logSNR")}
    assert np.array_equal(grids["ddim / plms"], grids["dpm time_uniform"]) and len(ddim) == {6: 7, 10: 10, 20: 20}[S]
    for name, ts in grids.items():
        L = len(ts)
        assert np.all(np.diff(ts) > 0), name
        for strength, n in ((0.01, 1), (0.5, L // 2), (0.99, int(L * 0.99)), (1, L), (1.0, L)):
            assert strength_steps(L, strength) == n == IR.strength_n(L, strength), (name, strength)
            sub = strength_timesteps(ts, strength)
            assert [int(t) for t in sub[::-1]] == IR.executed(ts, strength) == [int(t) for t in ts[:n][::-1]], (name, strength)
            tab = D.dpmpp_schedule(acp, sub, guidance=[10.0, 4.0])
            assert [int(t) for t in tab[:, D.COL_T]] == IR.executed(ts, strength)
            assert tab[0, D.COL_WPREV] == 0.0                                       # the first executed step is first order
            if 1 < n < 15:
                assert tab[-1, D.COL_WPREV] == 0.0                                  # the n < 15 rule applies to n
            if n >= 15:
                assert tab[-1, D.COL_WPREV] != 0.0
            assert tab[0, D.COL_G] == 10.0 and (n == 1 or tab[-1, D.COL_G] == pytest.approx(4.0))   # annealed over the n steps
    assert IR.executed(ddim, 0.5)[0] == int(ddim[len(ddim) // 2 - 1])
    assert strength_steps(7, 0.5) == 3 and strength_steps(7, 0.99) == 6 and strength_steps(20, 0.99) == 19


def test_strength_refusals():
    from adaface_amd.ldm.models.diffusion.blend import check_strength, strength_steps
    for bad in (0, 0.0, -0.1, 1.01, True, "0.5", float("nan")):
        with pytest.raises(ValueError, match="strength"):
            strength_steps(10, bad)
    with pytest.raises(ValueError, match="x0"):
        check_strength(0.5, None)
    with pytest.raises(NotImplementedError, match="timesteps"):
        check_strength(0.5, torch.zeros(1), timesteps=np.arange(3))
    check_strength(None, None, timesteps=np.arange(3))
    check_strength(0.5, torch.zeros(1), timesteps=None, ddim_use_original_steps=False)


class _NoDeviceModel:
    """Stands where the LatentDiffusion would: any use beyond the constructor's read of num_timesteps is a failure."""
    num_timesteps = 1000

    def __getattr__(self, name):
        raise AssertionError(f"the sampler touched model.{name} before refusing the option")


def test_samplers_refuse_strength_without_x0_before_any_device_use():
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    for cls in (DDIMSampler, DPMSolverSampler, PLMSSampler):
        s = cls(_NoDeviceModel())
        with pytest.raises(ValueError, match="x0"):
            s.sample(S=10, batch_size=1, shape=[4, 8, 8], verbose=False, strength=0.5)
        with pytest.raises(ValueError, match="strength"):
            s.sample(S=10, batch_size=1, shape=[4, 8, 8], verbose=False, strength=1.5, x0=torch.zeros(1, 4, 8, 8))
    with pytest.raises(NotImplementedError, match="timesteps"):
        DDIMSampler(_NoDeviceModel()).ddim_sampling(None, (1, 4, 8, 8), strength=0.5, x0=torch.zeros(1, 4, 8, 8), timesteps=5)
    with pytest.raises(NotImplementedError, match="ddim_use_original_steps"):
        DDIMSampler(_NoDeviceModel()).ddim_sampling(None, (1, 4, 8, 8), strength=0.5, x0=torch.zeros(1, 4, 8, 8),
                                                    ddim_use_original_steps=True)


def test_tgate_step_beyond_the_executed_steps_is_refused():
    """tgate_step counts the executed steps: the samplers build TGateRun on n, which refuses g > n - 1."""
    from adaface_amd.ldm.models.diffusion.blend import strength_steps
    from adaface_amd.ldm.models.diffusion.tgate import tgate_phases
    n = strength_steps(10, 0.5)
    assert n == 5 and tgate_phases(n, 4) == [None, None, None, "capture", "replay"]
    with pytest.raises(ValueError, match="tgate_step"):
        tgate_phases(n, 5)


# ------------------------------------------------------------------ ABI and host-side refusals ---------------------
def test_abi_symbol_is_exported_and_declared():
    from adaface_amd import _lib, ops
    lib = _lib.load()
    assert "af_noise_blend" in _lib.EXPORTED_SYMBOLS and "af_noise_blend_launches" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "af_noise_blend") and lib.af_noise_blend_launches() >= 0
    header = (ROOT / "include" / "adaface_hip.h").read_text()
    assert "int af_noise_blend(const float* x_dev, const float* x0_dev, const float* keep_dev, int keep_channels" in header
    assert "af_inpaint.hip" in (ROOT / "adaface_amd" / "build.py").read_text()
    from adaface_amd.noise import STREAM_QSAMPLE
    assert ops.STREAM_QSAMPLE == STREAM_QSAMPLE == 2


def test_noise_blend_host_side_refusals():
    """Every refusal is made on the host before any launch: the pointers here are never dereferenced (there is no device)."""
    from adaface_amd import _lib
    lib = _lib.load()
    n_samples, Cc, HW = 2, 4, 16
    launches = lib.af_noise_blend_launches()
    nb = n_samples * Cc * HW * 4
    X, X0, KEEP, NOISE, OUT, IDS = (0x10000 + k * 0x10000 for k in range(6))
    base = dict(x=X, x0=X0, keep=KEEP, kc=1, noise=NOISE, n=n_samples, C=Cc, HW=HW, sa=0.8, s1=0.6, ids=0, first=0, seed=42,
                stream=2, step=0, out=OUT)

    def call(**kw):
        a = dict(base, **kw)
        return lib.af_noise_blend(a["x"], a["x0"], a["keep"], a["kc"], a["noise"], a["n"], a["C"], a["HW"], a["sa"], a["s1"],
                                  a["ids"], a["first"], a["seed"], a["stream"], a["step"], a["out"], None)

    cases = {
        "keep_channels": dict(kc=2), "keep_channels 0": dict(kc=0), "a keep mask without x": dict(x=0),
        "step": dict(step=1 << 24), "stream": dict(stream=256), "first_id": dict(first=-1),
        "bad argument": dict(x0=0), "bad argument (out)": dict(out=0), "bad argument (n)": dict(n=0),
        "bad argument (C)": dict(C=0, kc=0), "bad argument (HW)": dict(HW=0),
        "overlaps x0": dict(out=X0), "overlaps x0 partly": dict(out=X0 + nb - 4), "overlaps keep": dict(out=KEEP),
        "overlaps keep's last float": dict(out=KEEP + n_samples * HW * 4 - 4, x=KEEP + n_samples * HW * 4 - 4),
        "overlaps noise": dict(out=NOISE - 4), "overlaps x partly": dict(out=X + 4), "overlaps ids": dict(ids=OUT + 8),
        "not finite": dict(sa=float("inf")), "not finite (s1)": dict(s1=float("nan")),
        "sample length": dict(C=1 << 20, kc=1, HW=1 << 20),
    }
    for name, kw in cases.items():
        assert call(**kw) == -1, name            # AF_ERR_INVALID
        msg = lib.af_last_error().decode()
        assert msg.startswith("af_noise_blend:"), (name, msg)
    assert call(kc=2) == -1 and "keep_channels 2 is neither 1 nor C = 4" in lib.af_last_error().decode()
    assert call(out=X0) == -1 and "overlaps" in lib.af_last_error().decode()
    assert call(step=1 << 24) == -1 and "step" in lib.af_last_error().decode()
    assert lib.af_noise_blend_launches() == launches


def test_ops_noise_blend_refuses_on_the_host():
    from adaface_amd import ops
    x = torch.zeros(2, 4, 8)
    with pytest.raises(ValueError, match="GPU"):
        ops.noise_blend(x, x, None, 1.0, 0.0)


# ------------------------------------------------------------------ hybrid conditioning -----------------------------
def _tiny_ldm(**unet):
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    cfg = tiny_config()
    cfg["model"]["params"]["unet_config"]["params"].update(unet)
    from adaface_amd.img2img import select_hybrid
    return select_hybrid(cfg), instantiate_from_config(cfg["model"]).eval()


def test_hybrid_model_builds_and_refuses_what_is_not_built():
    """A 9-in / 4-out U-Net selects conditioning_key 'hybrid'; its conv_in has 9 input channels; set_concat_cond checks its
    argument, a plain model refuses it, and a hybrid model without its condition says so."""
    hybrid, model = _tiny_ldm(in_channels=9)
    assert hybrid and model.model.conditioning_key == "hybrid"
    sd = model.state_dict()
    assert tuple(sd["model.diffusion_model.input_blocks.0.0.weight"].shape) == (64, 9, 3, 3)
    assert tuple(sd["model.diffusion_model.out.2.weight"].shape) == (4, 64, 3, 3)
    with pytest.raises(ValueError, match="5"):
        model.set_concat_cond(torch.zeros(1, 4, 16, 16))
    assert model.set_concat_cond(torch.zeros(1, 5, 16, 16)) is model and model.set_concat_cond(None) is model
    with pytest.raises(ValueError, match="set_concat_cond"):
        model.apply_model(torch.zeros(1, 4, 16, 16), torch.zeros(1, dtype=torch.long), torch.zeros(16, 77, 64))
    plain_is_hybrid, plain = _tiny_ldm()
    assert not plain_is_hybrid and plain.model.conditioning_key == "crossattn"
    with pytest.raises(ValueError, match="hybrid"):
        plain.set_concat_cond(torch.zeros(1, 5, 16, 16))


def test_controlnet_on_a_hybrid_unet_is_refused():
    from adaface_amd.ldm.modules.diffusionmodules.controlnet import SD15_CONTROLNET, ControlNet
    _, model = _tiny_ldm(in_channels=9)
    unet = model.model.diffusion_model
    ctor = {**SD15_CONTROLNET, **{k: v for k, v in unet._layout_kwargs().items() if k != "out_channels"}, "num_heads": unet.num_heads,
            "in_channels": 4}
    with pytest.raises(NotImplementedError, match="hybrid"):
        unet.set_control(ControlNet(**ctor), torch.zeros(1, 3, 128, 128))


# ------------------------------------------------------------------ CLI --------------------------------------------
def _load_cli():
    spec = importlib.util.spec_from_file_location("stable_txt2img_cli_inpaint", ROOT / "scripts" / "stable_txt2img.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_and_refusals(capsys):
    cli = _load_cli()
    opt = cli.parse_args(["--synthetic"])
    assert opt.img2img is None and opt.strength is None and opt.inpaint_mask is None
    opt = cli.parse_args(["--synthetic", "--img2img", "a.png"])
    assert opt.img2img == ["a.png"] and opt.strength == 0.75
    opt = cli.parse_args(["--synthetic", "--n_samples", "2", "--img2img", "a.png", "b.png", "--inpaint_mask", "m.png", "--strength",
                          "0.4", "--dpm_solver", "--noise", "philox", "--deep_cache", "2", "--controlnet", "synthetic"])
    assert opt.img2img == ["a.png", "b.png"] and opt.inpaint_mask == ["m.png"] and opt.strength == 0.4
    bad = (["--synthetic", "--strength", "0.5"],                                           # no --img2img
           ["--synthetic", "--inpaint_mask", "m.png"],                                     # no --img2img
           ["--synthetic", "--img2img", "a.png", "--init_img_paths", "b.png"],
           ["--synthetic", "--img2img", "a.png", "--strength", "0"],
           ["--synthetic", "--img2img", "a.png", "--strength", "1.5"],
           ["--synthetic", "--n_samples", "4", "--img2img", "a.png", "b.png"],             # neither 1 nor 4 images
           ["--synthetic", "--n_samples", "4", "--img2img", "a.png", "--inpaint_mask", "m.png", "n.png", "o.png"],
           ["--synthetic", "--img2img", "a.png", "--H", "500"])
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv
    assert "--img2img" in capsys.readouterr().err
    # what depends on the model (known once the config / checkpoint is read)
    plain = cli.parse_args(["--synthetic", "--controlnet", "synthetic"])
    assert cli.hybrid_problem(plain, hybrid=False) is None
    assert "--inpaint_mask" in cli.hybrid_problem(plain, hybrid=True)
    assert "--inpaint_mask" in cli.hybrid_problem(cli.parse_args(["--synthetic", "--img2img", "a.png"]), hybrid=True)
    both = ["--synthetic", "--img2img", "a.png", "--inpaint_mask", "m.png"]
    assert cli.hybrid_problem(cli.parse_args(both), hybrid=True) is None
    assert "--controlnet" in cli.hybrid_problem(cli.parse_args(both + ["--controlnet", "synthetic"]), hybrid=True)


def test_select_hybrid_reads_config_and_checkpoint(tmp_path):
    from adaface_amd.configs import sd15_config
    from adaface_amd.img2img import ckpt_in_channels, select_hybrid
    cfg = sd15_config()
    assert not select_hybrid(cfg) and cfg["model"]["params"]["conditioning_key"] == "crossattn"
    cfg["model"]["params"]["unet_config"]["params"]["in_channels"] = 9
    assert select_hybrid(cfg) and cfg["model"]["params"]["conditioning_key"] == "hybrid"
    key = "model.diffusion_model.input_blocks.0.0.weight"
    p9, p4, pn = (str(tmp_path / n) for n in ("nine.ckpt", "four.ckpt", "none.ckpt"))
    torch.save({"state_dict": {key: torch.zeros(8, 9, 3, 3)}}, p9)
    torch.save({key: torch.zeros(8, 4, 3, 3)}, p4)
    torch.save({"other": torch.zeros(1)}, pn)
    assert (ckpt_in_channels(p9), ckpt_in_channels(p4), ckpt_in_channels(pn)) == (9, 4, None)
    cfg = sd15_config()
    assert select_hybrid(cfg, p9) and cfg["model"]["params"]["unet_config"]["params"]["in_channels"] == 9
    cfg = sd15_config()
    assert not select_hybrid(cfg, p4) and not select_hybrid(cfg, pn)
    from safetensors.torch import save_file
    ps = str(tmp_path / "nine.safetensors")
    save_file({key: torch.zeros(8, 9, 3, 3)}, ps)
    assert ckpt_in_channels(ps) == 9


# ------------------------------------------------------------------ sharding ----------------------------------------
def test_images_and_masks_are_sharded_by_global_index(tmp_path):
    """One file serves every sample of every rank; a list of n_samples files is cut by global index, so the ranks' shards
    concatenate to the list whatever the world size; each file is read once per rank."""
    from adaface_amd.img2img import load_batch, load_image, load_mask, pick_shard
    from adaface_amd.parallel import shard_range
    files = [f"img{i}.png" for i in range(10)]
    for world in (1, 2, 3, 8):
        seen = []
        for rank in range(world):
            lo, hi = shard_range(10, rank, world)
            mine = pick_shard(files, 10, lo, hi)
            assert mine == files[lo:hi]
            assert pick_shard(["one.png"], 10, lo, hi) == ["one.png"] * (hi - lo)
            seen += mine
        assert seen == files
    with pytest.raises(ValueError, match="--inpaint_mask"):
        pick_shard(files[:3], 10, 0, 5, "--inpaint_mask")
    # through the loaders: constant images of value i / 10 at global index i
    from PIL import Image
    paths = []
    for i in range(4):
        p = tmp_path / f"{i}.png"
        Image.fromarray(np.full((8, 8, 3), 60 * i, dtype=np.uint8)).save(p)
        paths.append(str(p))
    reads = []

    def loader(p, h, w):
        reads.append(p)
        return load_image(p, h, w)
    got = load_batch(paths, 4, 1, 3, 16, 8, loader, "--img2img")
    assert got.shape == (2, 3, 16, 8) and reads == paths[1:3]
    assert torch.allclose(got[:, 0, 0, 0], torch.tensor([2 * 60 / 255 - 1, 2 * 120 / 255 - 1]), atol=1e-6)
    reads.clear()
    got = load_batch(paths[3:], 4, 0, 4, 8, 8, loader, "--img2img")
    assert got.shape == (4, 3, 8, 8) and reads == paths[3:] and float(got.min()) == float(got.max())
    m = load_batch(paths[:1], 4, 0, 2, 8, 16, load_mask, "--inpaint_mask")
    assert m.shape == (2, 1, 8, 16) and float(m.max()) == 0.0
