"""CPU tests of the hires fix: af_resample_taps against torch.nn.functional.interpolate in float64, against Pillow's mode-"F"
resize and against the restatement of tests/hires_ref.py; table sanity; the plan's host-side refusals; hires.target_size,
PhiloxNoise.derive, hires.two_pass on a stub sampler; the CLI's flags and refusals; the new C symbols."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import hires_ref as HRf  # noqa: E402

SHAPES = HRf.SHAPES
TORCH_MODES = {"nearest-exact": "nearest-exact", "bilinear": "bilinear", "bicubic": "bicubic"}
SYMS = ("af_resample_taps", "af_resample_plan_create", "af_resample_plan_destroy", "af_resample_plan_tables", "af_resample2d")
COUNTERS = ("af_resample2d_launches",)


def _x(h, w, seed=0):
    return torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(seed + 31 * h + w), dtype=torch.float64)


def _lib_taps(mode, n_in, n_out):
    from adaface_amd import ops
    idx, w = ops.resample_taps(mode, n_in, n_out)
    return idx.numpy(), w.numpy()


# ------------------------------------------------------------------ taps --------------------------------------------
@pytest.mark.parametrize("src,dst", SHAPES)
@pytest.mark.parametrize("mode", ["bilinear", "bicubic", "nearest-exact"])
def test_taps_against_torch(mode, src, dst):
    """The library's tables applied in float64 against F.interpolate on float64 CPU tensors: 1e-12 of max|ref|; exact at equal
    sizes (and for nearest-exact, a gather, always)."""
    x = _x(*src)
    iy, wy = _lib_taps(mode, src[0], dst[0])
    ix, wx = _lib_taps(mode, src[1], dst[1])
    got, _ = HRf.resample_f64(x.numpy(), iy, wy, ix, wx)
    kw = {} if mode == "nearest-exact" else dict(align_corners=False)
    ref = F.interpolate(x, size=dst, mode=TORCH_MODES[mode], **kw).numpy()
    err = np.abs(got - ref).max()
    print(f"{mode} {src}->{dst}: max |err| {err:.3e} of max|ref| {np.abs(ref).max():.3f}")
    if src == dst or mode == "nearest-exact":
        assert np.array_equal(got, ref)
    assert err <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("src,dst", SHAPES)
def test_lanczos_taps_against_pillow(src, dst):
    """lanczos3 against Pillow's mode-"F" resize.  The bar is counted: 16 2^-24 S with S = sum |wy| |wx| |x| -- 7 + 7 roundings
    plus the two normalisations of Pillow's fp32 passes."""
    Image = pytest.importorskip("PIL.Image")
    x = _x(*src)[0, 0].numpy().astype(np.float32)
    iy, wy = _lib_taps("lanczos3", src[0], dst[0])
    ix, wx = _lib_taps("lanczos3", src[1], dst[1])
    got, S = HRf.resample_f64(x, iy, wy, ix, wx)
    ref = np.asarray(Image.fromarray(x).resize((dst[1], dst[0]), resample=Image.LANCZOS), dtype=np.float64)
    err = np.abs(got - ref)
    bound = 16 * 2.0 ** -24 * S
    print(f"lanczos3 {src}->{dst}: worst |err| / bound {float((err / bound).max()):.3f}, max |err| {err.max():.3e}")
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("mode", HRf.MODES)
def test_taps_against_the_restatement_and_table_sanity(mode):
    """Indices identical, weights within 4 fp64 ulp of tests/hires_ref.py; every row sums to 1 within 1e-15 x taps, every index
    lies in [0, n_in), unused taps carry weight 0."""
    for src, dst in SHAPES:
        for n_in, n_out in zip(src, dst):
            idx, w = _lib_taps(mode, n_in, n_out)
            ridx, rw = HRf.taps(mode, n_in, n_out)
            T = HRf.TAPS[mode]
            assert idx.shape == w.shape == (n_out, T)
            assert np.array_equal(idx, ridx), (mode, n_in, n_out)
            assert (np.abs(w - rw) <= 4 * np.spacing(np.abs(rw))).all(), (mode, n_in, n_out, float(np.abs(w - rw).max()))
            assert (np.abs(w.sum(axis=1) - 1.0) <= 1e-15 * T).all(), (mode, n_in, n_out)
            assert idx.min() >= 0 and idx.max() < n_in
            assert np.isfinite(w).all()
            if n_in == n_out and mode != "lanczos3":          # the identity table: one weight of exactly 1 per row
                assert np.array_equal(np.sort(w, axis=1)[:, -1], np.ones(n_out)) and np.count_nonzero(w) == n_out
                assert np.array_equal(idx[np.arange(n_out), w.argmax(axis=1)], np.arange(n_out))


# ------------------------------------------------------------------ refusals ----------------------------------------
def test_plan_creation_and_taps_refuse_on_the_host():
    """Every refusal returns AF_ERR_INVALID with a message before the device is touched (this test has no device)."""
    import ctypes as C
    from adaface_amd import _lib, ops
    lib = _lib.load()
    err = lambda: lib.af_last_error().decode()
    plan = C.c_void_p()
    create = lambda mode, H, W, Ho, Wo: lib.af_resample_plan_create(mode, H, W, Ho, Wo, C.byref(plan))
    for args, word in (((1, 8, 8, 7, 8), "upscaling only"), ((1, 8, 8, 8, 7), "upscaling only"), ((1, 0, 8, 8, 8), "n_in"),
                       ((1, 8, 0, 8, 8), "n_in"), ((1, -1, 8, 8, 8), "n_in"), ((2, 2048, 8, 8193, 8), "8192"),
                       ((2, 8, 2048, 8, 8193), "8192"), ((3, 8, 8, 65, 8), "8 x n_in"), ((3, 8, 8, 8, 65), "8 x n_in"),
                       ((4, 8, 8, 8, 8), "mode"), ((-1, 8, 8, 8, 8), "mode")):
        assert create(*args) == -1 and word in err() and "af_resample_plan_create" in err(), (args, err())
        assert not plan.value
    assert lib.af_resample_plan_create(1, 8, 8, 16, 16, None) == -1 and "null" in err()
    idx, w, taps = (C.c_int32 * 64)(), (C.c_double * 64)(), C.c_int()
    assert lib.af_resample_taps(1, 4, 8, None, w, C.byref(taps)) == -1 and "null" in err()
    assert lib.af_resample_taps(1, 4, 8, idx, None, C.byref(taps)) == -1 and "null" in err()
    assert lib.af_resample_taps(1, 4, 8, idx, w, None) == -1 and "null" in err()
    assert lib.af_resample_taps(1, 8, 4, idx, w, C.byref(taps)) == -1 and "upscaling only" in err()
    assert lib.af_resample2d(None, None, None, 1, None) == -1 and "null" in err()
    assert lib.af_resample_plan_tables(None, None, None, None, None, None) == -1 and "null" in err()
    assert lib.af_resample_plan_destroy(None) == 0
    for bad in (("bilinear", 8, 4), ("bicubic", 0, 4), ("lanczos3", 4, 33), ("nearest-exact", 2000, 8193)):
        with pytest.raises(_lib.AfError, match="af_resample_taps"):
            ops.resample_taps(*bad)
    with pytest.raises(ValueError, match="mode"):
        ops.resample_taps("area", 4, 8)
    assert isinstance(ops.resample2d_launches(), int)


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
    assert "af_resample.hip" in build.SOURCES
    for name in ("resample2d", "resample_taps", "resample2d_launches", "resample_plan"):
        assert callable(getattr(ops, name)), name
    assert ops.RESAMPLE_MAX_TAPS == 7 == max(HRf.TAPS.values()) and set(ops.RESAMPLE_MODES) == set(HRf.MODES)
    assert re.search(r"#define\s+AF_RESAMPLE_MAX_TAPS\s+7\b", text)


# ------------------------------------------------------------------ host logic --------------------------------------
def test_target_size_rounding_and_errors():
    from adaface_amd import hires
    assert hires.UPSCALERS == ("latent", "latent-bicubic", "latent-nearest", "pixel-bicubic", "pixel-lanczos")
    assert hires.target_size(64, 64, scale=1.5) == (96, 96)
    assert hires.target_size(64, 64, scale=2) == (128, 128)
    assert hires.target_size(64, 96, scale=1.25) == (80, 120)
    assert hires.target_size(64, 64, scale=1.3) == (80, 80)           # 83.2 -> 80
    assert hires.target_size(64, 64, scale=1.45) == (96, 96)          # 92.8 -> 96
    assert hires.target_size(40, 40, scale=1.1) == (48, 48)           # 44 is half way: up
    assert hires.target_size(8, 16, scale=4.0) == (32, 64)
    assert hires.target_size(64, 64, size=(96, 128)) == (96, 128)
    assert hires.target_size(64, 64, size=(100, 67)) == (104, 64)
    assert hires.target_size(64, 64, size=(64, 64)) == (64, 64)
    for kw in (dict(), dict(scale=1.5, size=(96, 96)), dict(scale=1.0), dict(scale=0.5), dict(scale=4.01), dict(scale="2"),
               dict(scale=True), dict(scale=float("nan")), dict(size=(56, 96)), dict(size=(96, 56)), dict(size=(96,)),
               dict(size=(96.0, 96)), dict(size=(0, 96))):
        with pytest.raises(ValueError, match="hires"):
            hires.target_size(64, 64, **kw)
    assert hires.target_size(62, 62, scale=1.01) == (64, 64)
    with pytest.raises(ValueError, match="hires"):
        hires.target_size(0, 8, scale=2.0)
    with pytest.raises(ValueError, match="upscaler"):
        hires.upscale_latent(None, torch.zeros(1, 4, 8, 8), (16, 16), "esrgan")


def test_derive_is_deterministic_and_distinct():
    from adaface_amd.noise import DERIVE_TAGS, PhiloxNoise, splitmix64
    assert splitmix64(0) == 0xE220A8397B1DCDAF and splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4      # the published vectors
    a = PhiloxNoise(42, first_id=3)
    d1, d2 = a.derive("hires"), a.derive("hires")
    assert d1.seed == d2.seed == splitmix64(42 + DERIVE_TAGS["hires"]) and 0 <= d1.seed < 2 ** 64
    assert d1.seed != a.seed and d1.seed != PhiloxNoise(43).derive("hires").seed and d1.seed != PhiloxNoise(43).seed
    assert d1.first_id == 3 and d1.sample_ids is None and a.seed == 42
    b = PhiloxNoise(2 ** 64 - 1, sample_ids=[5, 9]).derive("hires")
    assert b.sample_ids == [5, 9] and b.ids(2) == [5, 9] and 0 <= b.seed < 2 ** 64
    assert len({PhiloxNoise(s).derive("hires").seed for s in range(256)}) == 256
    with pytest.raises(ValueError, match="tag"):
        a.derive("other")


class _StubSampler:
    """Records its sample() calls; the result of a call is a tensor of the asked shape filled with the call's number."""

    def __init__(self):
        self.calls = []
        self.model = object()

    def sample(self, **kw):
        self.calls.append(kw)
        return torch.full([kw["batch_size"]] + list(kw["shape"]), float(len(self.calls))), {"x_inter": []}


def test_two_pass_on_a_stub(monkeypatch):
    from adaface_amd import hires
    from adaface_amd.noise import PhiloxNoise
    seen = []

    def fake_upscale(model, latent, size, upscaler):
        seen.append((model, tuple(latent.shape), tuple(size), upscaler))
        return torch.full((latent.shape[0], latent.shape[1], *size), 7.0)
    monkeypatch.setattr(hires, "upscale_latent", fake_upscale)
    s = _StubSampler()
    src = PhiloxNoise(42, first_id=2)
    first = dict(S=10, batch_size=2, shape=[4, 8, 8], conditioning="c", guidance_scale=3.0, noise_source=src, x_T="z1", verbose=False)
    second = hires.second_kwargs(first, steps=6)
    assert second == dict(S=6, batch_size=2, conditioning="c", guidance_scale=3.0, noise_source=second["noise_source"], verbose=False)
    assert second["noise_source"].seed == src.derive("hires").seed and second["noise_source"].first_id == 2
    assert hires.second_kwargs(first)["S"] == 10 and hires.second_kwargs(first, steps=0)["S"] == 10
    assert hires.second_kwargs(dict(S=3))== dict(S=3)
    noise = torch.zeros(2, 4, 16, 24)
    lat2, lat1 = hires.two_pass(s, first, second, (16, 24), "latent-bicubic", strength=0.6, noise=noise)
    assert len(s.calls) == 2 and s.calls[0] == first
    assert seen == [(s.model, (2, 4, 8, 8), (16, 24), "latent-bicubic")]
    c2 = s.calls[1]
    assert c2["shape"] == [4, 16, 24] and c2["strength"] == 0.6 and c2["x_T"] is noise and c2["S"] == 6
    assert tuple(c2["x0"].shape) == (2, 4, 16, 24) and float(c2["x0"][0, 0, 0, 0]) == 7.0
    assert c2["noise_source"] is second["noise_source"] and c2["batch_size"] == 2 and "mask" not in c2
    assert float(lat1.flatten()[0]) == 1.0 and float(lat2.flatten()[0]) == 2.0 and tuple(lat2.shape) == (2, 4, 16, 24)
    # the default noise is the sampler's own
    s2 = _StubSampler()
    hires.two_pass(s2, first, second, (16, 16))
    assert s2.calls[1]["x_T"] is None and s2.calls[1]["strength"] == 0.7 and seen[-1][3] == "latent"
    # refusals: before any call is made
    s3 = _StubSampler()
    for f, sec in ((dict(first, mask=torch.ones(1)), second), (dict(first, x0=torch.ones(1)), second),
                   (first, dict(second, mask=torch.ones(1))), (first, dict(second, x0=torch.ones(1)))):
        with pytest.raises(NotImplementedError, match="hires"):
            hires.two_pass(s3, f, sec, (16, 16))
    for extra in (dict(shape=[4, 16, 16]), dict(strength=0.5), dict(x_T=None)):
        with pytest.raises(ValueError, match="hires"):
            hires.two_pass(s3, first, dict(second, **extra), (16, 16))
    assert s3.calls == []


# ------------------------------------------------------------------ the CLI ------------------------------------------
def test_cli_flags_and_refusals(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("stable_txt2img_cli_hires", ROOT / "scripts" / "stable_txt2img.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    opt = cli.parse_args(["--synthetic"])
    assert opt.hires is None and opt.hires_upscaler == "latent" and opt.hires_strength == 0.7 and opt.hires_steps == 0
    opt = cli.parse_args(["--synthetic", "--hires_scale", "1.5"])
    assert opt.hires == (96, 96)
    opt = cli.parse_args(["--synthetic", "--hires_size", "768", "1024", "--hires_upscaler", "pixel-lanczos", "--hires_strength", "0.5",
                          "--hires_steps", "20"])
    assert opt.hires == (96, 128) and opt.hires_upscaler == "pixel-lanczos" and opt.hires_strength == 0.5 and opt.hires_steps == 20
    hs = ["--synthetic", "--hires_scale", "1.5"]
    for dt in ("bf16", "f32", "fp16"):
        assert cli.parse_args(hs + ["--dtype", dt]).hires == (96, 96)
    for ok in (["--plms"], ["--dpm_solver"], ["--dpm_solver", "--dpm_sde"], ["--lcm", "--ddim_steps", "4"], ["--tcd_gamma", "0.3",
               "--ddim_steps", "4"], ["--deep_cache", "3"], ["--tome", "0.5"], ["--freeu", "1.2", "1.4", "0.9", "0.2"],
               ["--pag_scale", "3"], ["--guidance_rescale", "0.7"], ["--sag_scale", "0.75"], ["--tgate", "10"], ["--noise", "philox"],
               ["--gpus", "2"], ["--lora", "a.safetensors:0.8"]):
        assert cli.parse_args(hs + ok).hires == (96, 96), ok
    for up in ("latent", "latent-bicubic", "latent-nearest", "pixel-bicubic", "pixel-lanczos"):
        assert cli.parse_args(hs + ["--hires_upscaler", up]).hires_upscaler == up
    for bad in (["--hires_scale", "1.5", "--hires_size", "768", "768"], ["--hires_scale", "1"], ["--hires_scale", "4.5"],
                ["--hires_scale", "x"], ["--hires_size", "768"], ["--hires_size", "700", "768"], ["--hires_size", "448", "768"],
                ["--hires_size", "0", "768"], ["--hires_upscaler", "latent-bicubic"], ["--hires_strength", "0.5"], ["--hires_steps", "10"],
                hs[1:] + ["--hires_upscaler", "esrgan"], hs[1:] + ["--hires_strength", "0"], hs[1:] + ["--hires_strength", "1.5"],
                hs[1:] + ["--hires_steps", "-1"], hs[1:] + ["--img2img", "a.png"], hs[1:] + ["--img2img", "a.png", "--inpaint_mask", "m.png"],
                hs[1:] + ["--controlnet", "synthetic"], hs[1:] + ["--regions", "synthetic:2"],
                hs[1:] + ["--region_emb", "r.pt", "--region_box", "0,0,1,1"], hs[1:] + ["--init_img_paths", "a.png"],
                hs[1:] + ["--dtype", "fp8"], hs[1:] + ["--H", "516"], hs[1:] + ["--lcm", "--ddim_steps", "4", "--hires_steps", "60"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["--synthetic"] + bad)
        assert e.value.code == 2, bad
    assert "hires" in capsys.readouterr().err
    # a hybrid (inpainting) model is refused by name before anything is built
    opt = cli.parse_args(hs)
    assert "hires" in cli.hybrid_problem(opt, True) and cli.hybrid_problem(opt, False) is None
