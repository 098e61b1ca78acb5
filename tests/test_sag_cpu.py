"""CPU tests of self-attention guidance: the host-only taps against the restatement of tests/sag_ref.py, the restatement's own
invariants (mass mean 1, reflect blur against torch's conv), the argument checkers, the new C symbols in header, binding and
library with their host-side refusals, the samplers' refusals and untouched call paths on stub models, and the CLI flags."""
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import sag_ref as SR  # noqa: E402

SYMS = ("af_sag_taps", "af_op_sag_mass", "af_sag_degrade", "af_sag_set", "af_sag_state", "af_sag_read")
COUNTERS = ("af_sag_mass_launches", "af_sag_degrade_launches")


# ------------------------------------------------------------------ taps --------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.0, 3.7])
def test_taps_against_the_restatement(sigma):
    from adaface_amd import ops
    w = np.array(ops.sag_taps(sigma))
    ref = SR.taps(sigma)
    assert w.shape == (9,) and np.abs(w - ref).max() <= 4 * np.finfo(np.float64).eps
    assert abs(w.sum() - 1.0) <= 4 * np.finfo(np.float64).eps
    assert np.array_equal(w, w[::-1]) and (np.diff(w[:5]) > 0).all()
    # the kernel's fp32 taps are these rounded once: the restatement rounds to the same floats
    assert np.array_equal(w.astype(np.float32), ref.astype(np.float32))


def test_taps_default_and_refusals():
    from adaface_amd import _lib, ops
    assert ops.sag_taps() == ops.sag_taps(1.0)
    assert abs(ops.sag_taps(1.0)[4] - 1.0 / sum(math.exp(-0.5 * d * d) for d in range(-4, 5))) < 1e-15
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.AfError, match="af_sag_taps"):
            ops.sag_taps(bad)


# ------------------------------------------------------------------ the restatement itself --------------------------
def test_reference_mass_has_mean_one_and_blur_matches_torch():
    g = torch.Generator().manual_seed(5)
    q, k = (torch.randn(3, 24, 64, generator=g).numpy() for _ in range(2))
    m = SR.mass(q, k, 2)
    assert m.shape == (3, 24) and np.abs(m.mean(axis=1) - 1.0).max() < 1e-12
    # against softmax written with torch in float64
    qh = torch.tensor(q).double().reshape(3, 24, 2, 32).permute(0, 2, 1, 3)
    kh = torch.tensor(k).double().reshape(3, 24, 2, 32).permute(0, 2, 1, 3)
    p = (qh @ kh.transpose(-1, -2) * 32 ** -0.5).softmax(-1)
    assert np.abs(p.mean(1).sum(1).numpy() - m).max() < 1e-12
    # the blur: F.pad(reflect) + a grouped convolution with the outer product of the taps
    x = torch.randn(2, 4, 8, 24, generator=g, dtype=torch.float64)
    w = torch.tensor(SR.taps(1.0))
    k2 = (w[:, None] * w[None, :]).expand(4, 1, 9, 9)
    ref = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (4, 4, 4, 4), mode="reflect"), k2, groups=4)
    assert np.abs(SR.blur(x.numpy(), SR.taps(1.0)) - ref.numpy()).max() < 1e-13
    # the mask: a cell is an 8 x 8 block, every channel
    on = SR.mask_of(np.array([[1.5, 0.5, 0.5, 1.0 + 1e-9, 1.0, 2.0]]), 16, 24)
    assert on.shape == (1, 1, 16, 24) and on[0, 0, :8, :8].all() and not on[0, 0, :8, 8:].any()
    assert on[0, 0, 8:, :8].all() and not on[0, 0, 8:, 8:16].any() and on[0, 0, 8:, 16:].all()      # (1.0 itself is off)
    # all off: the degraded input is the input
    xx, ee = np.random.default_rng(0).normal(size=(2, 1, 4, 8, 8))
    out, bound = SR.degrade(xx, ee, np.full((1, 1), 0.5), 0.8, 0.6, SR.taps(1.0))
    assert np.abs(out - xx).max() < 1e-14 and (bound > 0).all()
    assert SR.combine(3.0, 1.0, 0.5, 4.0, 0.75) == 1.0 + 4.0 * 2.0 + 0.75 * 0.5 and SR.combine(3.0, None, 0.5, 4.0, 0.75) == 3.0 + 0.75 * 2.5


# ------------------------------------------------------------------ the library, host only --------------------------
def test_header_binding_and_library_have_the_symbols():
    from adaface_amd import _lib, build, ops
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "adaface_hip.h").read_text(), flags=re.S)
    if not _lib.lib_path().exists():
        build.build(verbose=False)
    exported = subprocess.run(["nm", "-D", "--defined-only", os.fspath(_lib.lib_path())], check=True, capture_output=True,
                              text=True).stdout
    for s, ret in [(s, "int") for s in SYMS] + [(s, "int64_t") for s in COUNTERS]:
        assert re.search(rf"\b{ret}\s+{s}\s*\(", text), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert re.search(rf"\sT\s+{s}$", exported, flags=re.M), s
    assert "af_sag.hip" in build.SOURCES
    for name in ("sag_taps", "sag_mass", "sag_degrade", "sag_launches"):
        assert callable(getattr(ops, name)), name
    from adaface_amd.engine import Engine
    assert all(callable(getattr(Engine, n)) for n in ("set_sag", "sag_mass", "sag_state"))
    from adaface_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    assert callable(LatentDiffusion.set_sag) and callable(LatentDiffusion.sag_mass)
    lib = _lib.load()
    # null handles and null outputs are refused on the host, with a message and without a device
    assert lib.af_sag_set(None, 1) == -1 and b"af_sag_set" in lib.af_last_error()
    assert lib.af_sag_state(None, None) == -1 and b"af_sag_state" in lib.af_last_error()
    assert lib.af_sag_read(None, None, 0, None) == -1 and b"af_sag_read" in lib.af_last_error()
    assert lib.af_sag_taps(1.0, None) == -1 and b"af_sag_taps" in lib.af_last_error()
    assert lib.af_op_sag_mass(1, None, None, None, None, 1, 4, 2, 128, 256, 256, None) == -1 and b"null" in lib.af_last_error()
    assert lib.af_op_sag_mass(7, None, None, None, None, 1, 4, 2, 128, 256, 256, None) == -1 and b"storage" in lib.af_last_error()
    assert lib.af_sag_degrade(None, None, None, None, 1, 4, 8, 8, 0.9, 0.4, 1.0, None) == -1
    before = ops.sag_launches()
    assert set(before) == {"mass", "degrade"} and all(isinstance(v, int) for v in before.values())
    assert ops.SAG_MAX_TOKENS >= 256


def test_host_side_refusals_of_the_two_entries():
    """Shapes, alpha, blur sigma, aliasing and the token cap are refused before the device is touched: fake non-null pointers do."""
    import ctypes as C
    from adaface_amd import _lib
    lib = _lib.load()
    P = lambda v: C.c_void_p(v)
    x, e, m, o = P(0x10000), P(0x20000), P(0x30000), P(0x40000)
    deg = lambda *a: lib.af_sag_degrade(*a)
    err = lambda: lib.af_last_error().decode()
    assert deg(x, e, m, x, 1, 4, 8, 8, 0.9, 0.4, 1.0, None) == -1 and "alias" in err()
    assert deg(x, e, m, e, 1, 4, 8, 8, 0.9, 0.4, 1.0, None) == -1 and "alias" in err()
    assert deg(x, e, m, P(0x10000 + 4 * 100), 1, 4, 8, 8, 0.9, 0.4, 1.0, None) == -1 and "alias" in err()     # a partial overlap
    assert deg(x, e, m, o, 1, 4, 8, 8, 0.0, 0.4, 1.0, None) == -1 and "alpha" in err()
    assert deg(x, e, m, o, 1, 4, 8, 8, -0.5, 0.4, 1.0, None) == -1 and "alpha" in err()
    assert deg(x, e, m, o, 1, 4, 8, 8, 0.9, 0.4, 0.0, None) == -1 and "sigma" in err()
    assert deg(x, e, m, o, 1, 4, 8, 8, 0.9, 0.4, -1.0, None) == -1 and "sigma" in err()
    for H, W in ((8, 12), (12, 8), (0, 8), (8, 264)):
        assert deg(x, e, m, o, 1, 4, H, W, 0.9, 0.4, 1.0, None) == -1, (H, W)
    assert deg(x, e, m, o, 0, 4, 8, 8, 0.9, 0.4, 1.0, None) == -1
    mass = lambda *a: lib.af_op_sag_mass(*a)
    assert mass(1, x, e, o, m, 1, 257, 8, 160, 3840, 3840, None) == -1 and "256" in err()
    assert mass(1, x, e, o, m, 1, 64, 8, 160, 1279, 3840, None) == -1 and "stride" in err()
    assert mass(1, x, e, o, m, 1, 0, 8, 160, 3840, 3840, None) == -1
    assert mass(1, x, e, o, m, 0, 64, 8, 160, 3840, 3840, None) == -1
    assert mass(1, x, e, o, None, 1, 64, 8, 160, 3840, 3840, None) == -1 and "null" in err()


# ------------------------------------------------------------------ the checkers -------------------------------------
def test_argument_checkers():
    from adaface_amd.ldm.models.diffusion import guidance as G
    assert G.check_sag_args() == (0.0, 1.0) and G.check_sag_args(1, 2) == (1.0, 2.0) and G.check_sag_args(0.75, 0.5) == (0.75, 0.5)
    for bad in ((-0.1, 1.0), ("1", 1.0), (True, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (1.0, 0.0), (1.0, -1.0), (1.0, "2"),
                (1.0, float("inf")), (1.0, None)):
        with pytest.raises(ValueError, match="sag_"):
            G.check_sag_args(*bad)
    # check_args keeps its signature and return value; is_on takes the new setting with a default
    assert G.check_args() == (0.0, 0.0, 0.0) and G.check_args(3, 0.01, 1) == (3.0, 0.01, 1.0)
    assert not G.is_on(0.0, 0.0) and not G.is_on(0.0, 0.0, 0.0) and G.is_on(0.0, 0.0, 0.75) and G.is_on(3.0, 0.0) and G.is_on(0.0, 0.7)
    G.refuse_sag(object(), 0.0, 3.0, 0.7, 5, 3)                  # off: nothing is looked at


class _Stub:
    """A model that must never be called: the samplers refuse before their first step."""
    num_timesteps = 1000
    parameterization = "eps"
    supports_tgate = True
    supports_deep_cache = True
    regions = None

    def __init__(self, with_sag=True, pag=()):
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
        self.betas = betas.float()
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0).float()
        self.alphas_cumprod_prev = torch.cat([torch.ones(1), self.alphas_cumprod[:-1]])
        self.sqrt_one_minus_alphas_cumprod = torch.sqrt(1.0 - self.alphas_cumprod)
        self.device = torch.device("cpu")
        self.pag = pag
        if with_sag:
            self.set_sag = self.sag_mass = self._never

    def _never(self, *a, **k):
        raise AssertionError("the model was called")

    apply_model = apply_model_cfg_twin = apply_model_cfg_pag = _never


def _samplers():
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    return {"ddim": (DDIMSampler, "guidance_scale"), "plms": (PLMSSampler, "unconditional_guidance_scale"),
            "dpm": (DPMSolverSampler, "guidance_scale")}


def _kw(gkey):
    c = torch.zeros(16, 77, 64)
    return dict(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, unconditional_conditioning=torch.zeros(16, 77, 64),
                verbose=False, x_T=torch.zeros(1, 4, 16, 16), **{gkey: 5.0})


@pytest.mark.parametrize("name", ["ddim", "plms", "dpm"])
def test_samplers_refuse_as_specified(name):
    cls, gkey = _samplers()[name]
    kw = _kw(gkey)
    for bad in (dict(sag_scale=-1.0), dict(sag_scale="1"), dict(sag_scale=0.75, sag_blur_sigma=0.0), dict(sag_blur_sigma=-2.0)):
        with pytest.raises(ValueError, match="sag_"):
            cls(_Stub()).sample(**bad, **kw)
    with pytest.raises(NotImplementedError, match="pag_scale"):
        cls(_Stub(pag=(6,))).sample(sag_scale=0.75, pag_scale=3.0, **kw)
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        cls(_Stub()).sample(sag_scale=0.75, guidance_rescale=0.7, **kw)
    with pytest.raises(NotImplementedError, match="tgate_step"):
        cls(_Stub()).sample(sag_scale=0.75, tgate_step=2, **kw)
    with pytest.raises(NotImplementedError, match="deep_cache_interval"):
        cls(_Stub()).sample(sag_scale=0.75, deep_cache_interval=2, **kw)
    with pytest.raises(ValueError, match="set_sag"):                             # a model without the capture
        cls(_Stub(with_sag=False)).sample(sag_scale=0.75, **kw)

    class Regional(_Stub):
        regions = torch.ones(2, 2, 16, 16)
    with pytest.raises(NotImplementedError, match="regional"):
        cls(Regional()).sample(sag_scale=0.75, **kw)

    class Controlled(_Stub):
        class model:                                                            # (model.model.diffusion_model.control)
            class diffusion_model:
                control = {"net": None}
                compute_dtype = "bf16"
    with pytest.raises(NotImplementedError, match="ControlNet"):
        cls(Controlled()).sample(sag_scale=0.75, **kw)

    class Fp8(_Stub):
        class model:
            class diffusion_model:
                control = None
                compute_dtype = "fp8"
    with pytest.raises(NotImplementedError, match="fp8"):
        cls(Fp8()).sample(sag_scale=0.75, **kw)


def test_lcm_sampler_refuses():
    from ldm.models.diffusion.lcm import LCMSampler
    with pytest.raises(NotImplementedError, match="sag_scale"):
        LCMSampler(_Stub()).sample(sag_scale=0.75, **_kw("guidance_scale"))


def test_module_refusals():
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    unet = instantiate_from_config(tiny_config()["model"]["params"]["unet_config"])
    assert unet.sag is False and unet.set_sag(True) is unet and unet.sag is True
    x, t, ctx = torch.zeros(1, 4, 16, 16), torch.tensor([1]), torch.zeros(32, 77, 64)
    for kw in (dict(tgate="capture"), dict(deep_cache=("reuse", 2)), dict(cfg_pag=True)):
        with pytest.raises(NotImplementedError, match="self-attention guidance"):
            unet.set_pag(("mid",)).forward(x, t, ctx, **kw)
    unet.set_pag(())
    with pytest.raises(ValueError, match="fp8"):
        unet.set_compute_dtype("fp8")
    unet.set_sag(False)
    assert unet.sag is False
    unet.set_compute_dtype("fp8")
    with pytest.raises(ValueError, match="fp8"):
        unet.set_sag(True)
    with pytest.raises(RuntimeError, match="sag_mass"):
        unet.sag_mass()


# ------------------------------------------------------------------ off is off ---------------------------------------
def test_helper_is_not_entered_when_off(monkeypatch):
    """sag_scale = 0: the samplers make the calls they make without the feature, and guided_eps with its other settings never
    reaches the new code."""
    from adaface_amd.ldm.models.diffusion import guidance as G

    def boom(*a, **k):
        raise AssertionError("the SAG path was entered")
    monkeypatch.setattr(G, "sag_eps", boom)
    monkeypatch.setattr(G, "refuse_sag", boom)
    monkeypatch.setattr(G, "check_sag_args", boom)
    calls = []

    class Model(_Stub):
        def apply_model(self, x, t, c, **k):
            calls.append(("single", tuple(x.shape), sorted(k)))
            raise RuntimeError("stop here")

        def apply_model_cfg_twin(self, x, t, c, **k):
            calls.append(("twin", tuple(x.shape), sorted(k)))
            raise RuntimeError("stop here")

    for name, (cls, gkey) in _samplers().items():
        kw = _kw(gkey)
        for extra in ({}, dict(sag_scale=0.0), dict(sag_scale=0, sag_blur_sigma=1.0)):
            with pytest.raises(RuntimeError, match="stop here"):
                cls(Model()).sample(**extra, **kw)
        with pytest.raises(RuntimeError, match="stop here"):
            cls(Model()).sample(**{**kw, "unconditional_conditioning": None})
    assert calls == ([("twin", (1, 4, 16, 16), [])] * 3 + [("single", (1, 4, 16, 16), [])]) * 3

    # guided_eps with rescale alone: the twin call and ops.guidance, as before
    calls.clear()

    class S:
        model = Model()
    with pytest.raises(RuntimeError, match="stop here"):
        G.guided_eps(S(), torch.zeros(1, 4, 16, 16), torch.tensor([5]), torch.zeros(16, 77, 64), torch.zeros(16, 77, 64), 5.0, 5,
                     guidance_rescale=0.5)
    assert calls == [("twin", (1, 4, 16, 16), [])]


def test_guided_eps_makes_the_sag_calls_on_a_stub(monkeypatch):
    """Steps 1-5 on a stub: capture on around the usual call only, the mass read between the two forwards, the degraded forward
    on the guide leg's conditioning with the capture off, and the combine's weights; with and without CFG."""
    from adaface_amd.ldm.models.diffusion import guidance as G
    log = []
    c, uc = torch.zeros(16, 77, 64), torch.ones(16, 77, 64)
    x = torch.arange(4 * 64, dtype=torch.float32).reshape(1, 4, 8, 8)

    class Model(_Stub):
        on = False

        def set_sag(self, on=True):
            log.append(("set_sag", bool(on)))
            self.on = bool(on)

        def sag_mass(self):
            log.append(("sag_mass", self.on))
            return torch.tensor([[1.5], [0.5]]) if self.last == "twin" else torch.tensor([[2.0]])

        def apply_model_cfg_twin(self, xx, t, twin):
            log.append(("twin", self.on, tuple(twin.shape)))
            self.last = "twin"
            return torch.cat([xx + 1.0, xx + 2.0])

        def apply_model(self, xx, t, cond):
            log.append(("single", self.on, float(cond.flatten()[0]), xx is x))
            self.last = "single"
            return xx + 3.0

    def fake_degrade(xx, e, m, alpha, sigma, blur_sigma):
        log.append(("degrade", tuple(m.shape), float(m.flatten()[0]), round(alpha ** 2 + sigma ** 2, 12), blur_sigma))
        return xx * 0.5

    def fake_lincomb(terms):
        log.append(("lincomb", [round(w, 6) for _, w in terms]))
        return sum(w * t for t, w in terms)
    monkeypatch.setattr(G.ops, "sag_degrade", fake_degrade)
    monkeypatch.setattr(G.ops, "lincomb", fake_lincomb)

    class S:
        model = Model(with_sag=False)
    s = S()
    out = G.guided_eps(s, x, torch.tensor([500]), c, uc, 4.0, 500, sag_scale=0.75, sag_blur_sigma=2.0)
    assert log == [("set_sag", True), ("twin", True, (32, 77, 64)), ("sag_mass", True), ("set_sag", False),
                   ("degrade", (1, 1), 0.5, 1.0, 2.0), ("single", False, 1.0, False), ("lincomb", [4.0, -2.25, -0.75])]
    e_c, e_u, e_d = x + 1.0, x + 2.0, 0.5 * x + 3.0
    assert torch.allclose(out, e_u + 4.0 * (e_c - e_u) + 0.75 * (e_u - e_d))
    assert s.guidance_log == [(2, 0.0), (1, 0.75)]
    log.clear()
    out = G.guided_eps(s, x, torch.tensor([500]), c, uc, 1.0, 500, sag_scale=0.75)            # guidance 1: the single-leg form
    assert log == [("set_sag", True), ("single", True, 0.0, True), ("sag_mass", True), ("set_sag", False),
                   ("degrade", (1, 1), 2.0, 1.0, 1.0), ("single", False, 0.0, False), ("lincomb", [1.75, -0.75])]
    assert torch.allclose(out, (x + 3.0) + 0.75 * ((x + 3.0) - (0.5 * x + 3.0)))
    assert s.guidance_log[2:] == [(1, 0.0), (1, 0.75)]
    # the capture is switched off again when the model call raises
    log.clear()

    def boom(*a, **k):
        raise RuntimeError("stop here")
    s.model.apply_model_cfg_twin = boom
    with pytest.raises(RuntimeError, match="stop here"):
        G.guided_eps(s, x, torch.tensor([500]), c, uc, 4.0, 500, sag_scale=0.75)
    assert log == [("set_sag", True), ("set_sag", False)]


# ------------------------------------------------------------------ the CLI ------------------------------------------
def test_cli_flags_parse(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("stable_txt2img_cli_sag", ROOT / "scripts" / "stable_txt2img.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    opt = cli.parse_args(["--synthetic"])
    assert opt.sag_scale == 0.0 and opt.sag_blur_sigma == 1.0
    opt = cli.parse_args(["--synthetic", "--sag_scale", "0.75", "--sag_blur_sigma", "2"])
    assert opt.sag_scale == 0.75 and opt.sag_blur_sigma == 2.0
    for dt in ("bf16", "f32", "fp16"):
        assert cli.parse_args(["--synthetic", "--dtype", dt, "--sag_scale", "1"]).sag_scale == 1.0
    for ok in (["--plms"], ["--dpm_solver"], ["--dpm_solver", "--dpm_sde"], ["--freeu", "1.2", "1.4", "0.9", "0.2"], ["--gpus", "2"],
               ["--tome", "0.5"], ["--tome", "0.5", "--tome_max_downsample", "2"], ["--noise", "philox"], ["--scale", "1"],
               ["--deep_cache", "1"], ["--tgate", "0"]):
        assert cli.parse_args(["--synthetic", "--sag_scale", "0.75"] + ok).sag_scale == 0.75, ok
    for bad in (["--sag_scale", "-1"], ["--sag_scale", "x"], ["--sag_scale", "nan"], ["--sag_blur_sigma", "2"],
                ["--sag_scale", "1", "--sag_blur_sigma", "0"], ["--sag_scale", "1", "--sag_blur_sigma", "-1"],
                ["--sag_scale", "1", "--pag_scale", "3"], ["--sag_scale", "1", "--guidance_rescale", "0.5"],
                ["--sag_scale", "1", "--tgate", "3"], ["--sag_scale", "1", "--deep_cache", "3"],
                ["--sag_scale", "1", "--controlnet", "synthetic"], ["--sag_scale", "1", "--regions", "synthetic:2"],
                ["--sag_scale", "1", "--lcm"], ["--sag_scale", "1", "--tcd_gamma", "0.3"], ["--sag_scale", "1", "--dtype", "fp8"],
                ["--sag_scale", "1", "--H", "520"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["--synthetic"] + bad)
        assert e.value.code == 2, bad
    assert "--sag_scale" in capsys.readouterr().err
