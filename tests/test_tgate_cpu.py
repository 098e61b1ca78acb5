"""CPU tests of T-GATE: the schedule and its validation, the new C symbols in header, binding and library, the samplers' and the
CLI's refusals, the DeepCache refreshes the call form forces (a stub model records the calls), and the restatement of
tests/tgate_ref.py against the oracle's own forward."""
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
import tgate_ref as TR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

SYMS = ("af_tgate_set", "af_tgate_num_sites", "af_tgate_state", "af_tgate_read_site", "af_op_tgate_add")
CFG = O.TINY_UNET


# ------------------------------------------------------------------ the schedule ------------------------------------
def test_phases():
    from adaface_amd.ldm.models.diffusion.tgate import tgate_phases
    assert tgate_phases(5, None) == [None] * 5 and tgate_phases(5, 0) == [None] * 5
    assert tgate_phases(5, 1) == ["capture", "replay", "replay", "replay", "replay"]
    assert tgate_phases(5, 3) == [None, None, "capture", "replay", "replay"]
    assert tgate_phases(5, 4) == [None, None, None, "capture", "replay"]
    assert tgate_phases(2, 1) == ["capture", "replay"]
    for n in (2, 6, 7):
        for g in range(1, n):
            assert tgate_phases(n, g) == TR.phases(n, g)
    for n, g in ((5, -1), (5, -3), (5, 5), (5, 6), (1, 1), (5, True), (5, False), (5, 2.0), (5, 2.5), (5, "2")):
        with pytest.raises(ValueError):
            tgate_phases(n, g)


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
    assert "af_tgate.hip" in build.SOURCES
    assert re.search(r"AF_TGATE_OFF\s*=\s*0,\s*AF_TGATE_CAPTURE\s*=\s*1,\s*AF_TGATE_REPLAY\s*=\s*2", text)
    assert _lib.TGATE_MODES == {None: 0, "capture": 1, "replay": 2}
    _lib.load()       # (every declared symbol resolves)


# ------------------------------------------------------------------ refusals that need no device -------------------
class _Stub:
    """A model on the CPU: the schedule buffers the samplers read, and model calls that record (form, deep_cache, tgate)."""
    num_timesteps = 1000
    parameterization = "eps"
    supports_deep_cache = True
    supports_tgate = True

    def __init__(self):
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
        self.betas = betas.float()
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0).float()
        self.alphas_cumprod_prev = torch.cat([torch.ones(1), self.alphas_cumprod[:-1]])
        self.sqrt_one_minus_alphas_cumprod = torch.sqrt(1.0 - self.alphas_cumprod)
        self.device = torch.device("cpu")
        self.pag = (6,)
        self.calls = []

    def apply_model(self, x, t, c, deep_cache=None, tgate=None):
        self.calls.append(("single", deep_cache, tgate))
        return torch.zeros_like(x)

    def apply_model_cfg_twin(self, x, t, twin, deep_cache=None, tgate=None):
        self.calls.append(("twin", deep_cache, tgate))
        return torch.zeros(2 * x.shape[0], *x.shape[1:])

    def apply_model_cfg_pag(self, *a, **k):
        raise AssertionError("the PAG entry was called")


def _samplers():
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    return {"ddim": (DDIMSampler, "guidance_scale"), "plms": (PLMSSampler, "unconditional_guidance_scale"),
            "dpm": (DPMSolverSampler, "guidance_scale")}


@pytest.fixture
def host_steps(monkeypatch):
    """The samplers' step kernels replaced by host no-ops (x' = x): the model calls are what these tests look at."""
    from adaface_amd import ops
    monkeypatch.setattr(ops, "ddim_step", lambda x, *a, **k: (x, x))
    monkeypatch.setattr(ops, "dpmpp_step", lambda x, *a, **k: (x, x))


def _kw(gkey, g=5.0):
    return dict(S=4, batch_size=1, shape=[4, 16, 16], conditioning=torch.zeros(16, 77, 64), verbose=False,
                x_T=torch.zeros(1, 4, 16, 16), unconditional_conditioning=torch.zeros(16, 77, 64), **{gkey: g})


def test_plms_refuses():
    cls, gkey = _samplers()["plms"]
    m = _Stub()
    with pytest.raises(NotImplementedError, match="PLMS"):
        cls(m).sample(tgate_step=2, **_kw(gkey))
    assert m.calls == []


@pytest.mark.parametrize("name", ["ddim", "dpm"])
def test_samplers_refuse_guided_runs_and_bad_gates(name):
    cls, gkey = _samplers()[name]
    for guided in (dict(pag_scale=3.0), dict(guidance_rescale=0.7)):
        m = _Stub()
        with pytest.raises(NotImplementedError, match="guidance combine"):
            cls(m).sample(tgate_step=2, **guided, **_kw(gkey))
        assert m.calls == []
    for bad in (-1, 4, 9, True, 2.0):            # S = 4 on the uniform grid: n = 4 steps, so 1 <= g <= 3
        m = _Stub()
        with pytest.raises(ValueError, match="tgate_step"):
            cls(m).sample(tgate_step=bad, **_kw(gkey))
        assert m.calls == []

    class NoEntry(_Stub):
        supports_tgate = False
    with pytest.raises(NotImplementedError, match="T-GATE entry point"):
        cls(NoEntry()).sample(tgate_step=2, **_kw(gkey))


@pytest.mark.parametrize("name", ["ddim", "dpm"])
def test_off_makes_the_calls_it_made(host_steps, name):
    """tgate_step None and 0: no tgate= keyword reaches the model (the stub would record it), the log is all None."""
    cls, gkey = _samplers()[name]
    for off in (None, 0):
        m = _Stub()
        s = cls(m)
        s.sample(tgate_step=off, **_kw(gkey))
        assert m.calls == [("twin", None, None)] * 4 and s.tgate_log == [None] * 4


@pytest.mark.parametrize("name", ["ddim", "dpm"])
def test_phases_reach_the_model_and_force_the_deepcache_refreshes(host_steps, name):
    """S = 6 on the uniform grid is n = 7 steps.  g = 3: steps 0-1 ordinary twin calls, step 2 the capture (twin), steps 3-6 the
    replay (single leg).  With deep_cache_interval = 100 only step 0 refreshes by schedule: the form tuple's fifth element forces
    a refresh at the capture step and at the first replay step, the later replay steps reuse."""
    cls, gkey = _samplers()[name]
    kw = _kw(gkey)
    kw["S"] = 6
    m = _Stub()
    s = cls(m)
    s.sample(tgate_step=3, **kw)
    want = [None, None, "capture", "replay", "replay", "replay", "replay"]
    assert s.tgate_log == want
    assert m.calls == [("twin", None, None)] * 2 + [("twin", None, "capture")] + [("single", None, "replay")] * 4
    m = _Stub()
    s = cls(m)
    s.sample(tgate_step=3, deep_cache_interval=100, deep_cache_depth=2, **kw)
    assert s.tgate_log == want
    assert s.deep_cache_log == ["refresh", "reuse", "refresh", "refresh", "reuse", "reuse", "reuse"]
    rf, ru = ("refresh", 2), ("reuse", 2)
    assert m.calls == [("twin", rf, None), ("twin", ru, None), ("twin", rf, "capture"), ("single", rf, "replay")] + \
        [("single", ru, "replay")] * 3
    # no unconditional conditioning: every call is single-leg, the capture too
    m = _Stub()
    s = cls(m)
    kw1 = dict(kw, unconditional_conditioning=None)
    s.sample(tgate_step=1, **kw1)
    assert m.calls == [("single", None, "capture")] + [("single", None, "replay")] * 6


def test_cli_flag(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("stable_txt2img_cli_tgate", ROOT / "scripts" / "stable_txt2img.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.parse_args(["--synthetic"]).tgate is None
    assert cli.parse_args(["--synthetic", "--tgate", "0"]).tgate == 0
    opt = cli.parse_args(["--synthetic", "--tgate", "10", "--dpm_solver", "--deep_cache", "3", "--tome", "0.5", "--freeu", "1.2",
                          "1.4", "0.9", "0.2", "--dtype", "f32"])
    assert opt.tgate == 10
    assert cli.parse_args(["--synthetic", "--tgate", "10", "--dtype", "fp16"]).tgate == 10
    for bad in (["--plms"], ["--pag_scale", "3"], ["--guidance_rescale", "0.5"], ["--dtype", "fp8"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["--synthetic", "--tgate", "10"] + bad)
        assert e.value.code == 2, bad
    for bad in (["--tgate", "-1"], ["--tgate", "x"], ["--tgate", "2.5"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["--synthetic"] + bad)
        assert e.value.code == 2, bad
    assert "--tgate" in capsys.readouterr().err


def test_unet_module_refuses_without_a_device():
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    unet = instantiate_from_config(tiny_config()["model"]["params"]["unet_config"])
    x, t, ctx = torch.zeros(1, 4, 16, 16), torch.tensor([1]), torch.zeros(32, 77, 64)
    with pytest.raises(ValueError, match="tgate"):
        unet.forward(x, t, ctx, tgate="keep")
    with pytest.raises(ValueError, match="one leg"):
        unet.forward(x, t, ctx, tgate="replay", cfg_twin=True)
    with pytest.raises(NotImplementedError, match="PAG"):
        unet.set_pag(("mid",)).forward(x, t, ctx, tgate="capture", cfg_pag=True)


# ------------------------------------------------------------------ the reference itself ----------------------------
@pytest.fixture(scope="module")
def tiny_sd():
    return O.synth_state_dict(O.unet_param_shapes(CFG), seed=11)


def test_reference_sites():
    sites, n = TR.site_of_prefix(CFG)
    assert n == 16 and sorted(sites.values()) == list(range(16))
    assert sites[O.UNET_PREFIX + "input_blocks.1.1"] == 0 and sites[O.UNET_PREFIX + "middle_block.1"] == 6


def test_reference_replay_of_its_own_capture_is_the_plain_forward(tiny_sd):
    """L = 1, the same (x, t): h + A with A the very tensor the plain forward adds -- the same bits.  The capture forward itself
    is the plain forward; with two legs the record is their mean; at another input the replay differs."""
    g = torch.Generator().manual_seed(7)
    x, t = torch.randn(2, 4, 16, 16, generator=g), torch.tensor([801, 33])
    ctx = torch.randn(2 * 16, 77, CFG.context_dim, generator=g)
    with torch.no_grad():
        plain = O.unet_forward(tiny_sd, CFG, x, t, ctx)
        eps, rec = TR.capture_forward(tiny_sd, CFG, x, t, ctx, legs=1)
        assert torch.equal(eps, plain) and sorted(rec) == list(range(16))
        assert tuple(rec[0].shape) == (2, 256, 64) and tuple(rec[6].shape) == (2, 4, 256)
        assert torch.equal(TR.replay_forward(tiny_sd, CFG, x, t, rec), plain)
        assert not torch.equal(TR.replay_forward(tiny_sd, CFG, x + 0.05, t, rec), plain)
        eps2, rec2 = TR.capture_forward(tiny_sd, CFG, x, t, ctx, legs=2)      # the two samples as the two legs of B = 1
        assert torch.equal(eps2, plain)
        for s in (0, 6, 15):
            assert tuple(rec2[s].shape) == (1,) + tuple(rec[s].shape[1:])
            assert torch.allclose(rec2[s][0], (rec[s][0] + rec[s][1]) * 0.5, rtol=0, atol=0)
    assert O.spatial_transformer.__module__ == O.__name__        # (the patch is gone)


def test_gated_reference_loop_differs_only_after_the_gate(tiny_sd):
    """DDIM, S = 6 (n = 7), g = n - 1: the capture changes nothing in the reference's arithmetic, so the trajectories agree
    bit for bit up to and including step n - 2 and differ in the last step alone."""
    g = torch.Generator().manual_seed(9)
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    c, uc = torch.randn(16, 77, CFG.context_dim, generator=g), torch.randn(16, 77, CFG.context_dim, generator=g)
    n = 7
    with torch.no_grad():
        plain = TR.GatedApplyModel(tiny_sd, CFG, TR.phases(n, None))
        _, traj0 = O.ddim_sample(plain, O.register_schedule(), 6, x_T, c, uc, (3.0, 2.0), return_trajectory=True)
        gated = TR.GatedApplyModel(tiny_sd, CFG, TR.phases(n, n - 1))
        _, traj1 = O.ddim_sample(gated, O.register_schedule(), 6, x_T, c, uc, (3.0, 2.0), return_trajectory=True)
    assert gated.log == [None] * (n - 2) + ["capture", "replay"] and sorted(gated.record) == list(range(16))
    for i in range(n - 1):
        assert torch.equal(traj0[i], traj1[i]), i
    assert not torch.equal(traj0[n - 1], traj1[n - 1])
