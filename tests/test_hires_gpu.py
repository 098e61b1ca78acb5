"""GPU tests of the hires fix: af_resample2d element by element against float64 on the plan's own fp32 tables with the rounding
count of the kernel's header (Tx + Ty), over every mode, the CPU tests' shapes, the tile edges, plane counts and alignments,
with guard floats around every output; the exact cases; batch-split invariance; one launch per call; and hires.two_pass on the
tiny model in f32 mode with DDIM, DPM-Solver++ and LCM against the three calls written out by hand."""
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
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ROOT / "tests" / "golden"
SENTINEL = -12345.5
PAD = 8                                    # guard floats on either side of every output (32 bytes: keeps 16-byte alignment)
U = 2.0 ** -24
SEED = 42
SAMPLER_TOL = 1e-3                         # tests/test_lcm_gpu.py: the drop-in sampler bar, of max |ref|, f32 mode
TH, TW = 16, 64                            # the kernel's output tile (ops.RESAMPLE_TILE, asserted below)
# the CPU tests' shapes, an output width one past the tile width, an output height one past the tile height
SHAPES = HRf.SHAPES + [((8, 40), (8, TW + 1)), ((10, 8), (TH + 1, 8))]
OFFSETS = [(0, 0), (1, 0), (0, 2), (3, 3)]         # (input, output) floats off 16-byte alignment: all four path pairs


def _guarded(shape, gpu, offset=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD + offset,), SENTINEL, device=gpu, dtype=torch.float32)
    return buf, buf[PAD + offset: PAD + offset + n].view(*shape)


def _offset_copy(host, gpu, offset):
    buf = torch.empty(host.numel() + offset, device=gpu, dtype=torch.float32)
    view = buf[offset:].view(*host.shape)
    view.copy_(host)
    assert view.data_ptr() % 16 == (buf.data_ptr() + 4 * offset) % 16 and view.is_contiguous()
    return view


def _run_case(gpu, mode, src, dst, planes, in_off=0, out_off=0, seed=0):
    """One launch against hires_ref.resample_f64 on the plan's own tables; returns worst |err| / bound over every element."""
    from adaface_amd import ops
    B, Cn = (1, planes) if planes % 4 else (planes // 4, 4)
    host = torch.randn(B, Cn, *src, generator=torch.Generator().manual_seed(seed + 7 * src[0] + src[1] + 1000 * planes))
    x = _offset_copy(host, gpu, in_off)
    plan = ops.resample_plan(mode, *src, *dst, device=gpu)
    iy, wy, ix, wx = (t.numpy() for t in plan.tables())
    T = HRf.TAPS[mode]
    assert wy.shape == (dst[0], T) and wx.shape == (dst[1], T) and wy.dtype == np.float32 and iy.dtype == np.int32
    ref, S = HRf.resample_f64(host.numpy(), iy, wy, ix, wx)
    bound = (T + T) * U * S                                    # csrc/af_resample.hip: Tx + Ty roundings on the longest path
    buf, out = _guarded((B, Cn, *dst), gpu, out_off)
    got = ops.resample2d(x, dst, mode, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    flat = buf.cpu().numpy().astype(np.float64)
    lo, n = PAD + out_off, ref.size
    tag = (mode, src, dst, planes, in_off, out_off)
    assert (flat[:lo] == SENTINEL).all() and (flat[lo + n:] == SENTINEL).all(), ("wrote outside the output", tag)
    err = np.abs(flat[lo:lo + n].reshape(ref.shape) - ref)
    ok = err <= bound
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    assert ok.all(), (tag, float(ratio.max()), np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    return float(ratio.max())


@pytest.mark.parametrize("mode", HRf.MODES)
def test_kernel_against_float64(gpu, report, mode):
    """Every output of every shape within (Tx + Ty) 2^-24 S of the float64 application of the plan's own fp32 tables, S = sum
    |wy| |wx| |x|; inputs and outputs 0 - 3 floats off 16-byte alignment (the four pairs of 16-byte / element paths); planes in
    {1, 3, 32}; nothing outside the output written."""
    from adaface_amd import ops
    assert ops.RESAMPLE_TILE == (TH, TW)
    worst = 0.0
    for k, (src, dst) in enumerate(SHAPES):
        for in_off, out_off in OFFSETS:
            worst = max(worst, _run_case(gpu, mode, src, dst, 3, in_off, out_off, seed=k))
    for planes in (1, 3, 32):
        for src, dst in (((8, 8), (12, 12)), ((5, 7), (9, 15)), ((8, 40), (8, TW + 1))):
            worst = max(worst, _run_case(gpu, mode, src, dst, planes, seed=planes))
            worst = max(worst, _run_case(gpu, mode, src, dst, planes, 2, 1, seed=planes + 1))
    print(f"af_resample2d {mode}: worst |err| / bound {worst:.3f}")
    report(f"af_resample2d {mode}: worst |err| / ((Tx + Ty) 2^-24 S) over all shapes, planes, alignments", worst, 1.0, 1.0)


def test_exact_cases(gpu):
    """nearest-exact is the gather of the restatement's indices (and F.interpolate's result), bit for bit; the three torch modes
    at equal size return the input's bits; a constant plane stays constant within the bound."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(3)
    for src, dst in SHAPES:
        x = torch.randn(2, 3, *src, generator=g).to(gpu)
        got = ops.resample2d(x, dst, "nearest-exact")
        iy = torch.tensor(HRf.taps("nearest-exact", src[0], dst[0])[0][:, 0], device=gpu)
        ix = torch.tensor(HRf.taps("nearest-exact", src[1], dst[1])[0][:, 0], device=gpu)
        assert torch.equal(got, x[:, :, iy][:, :, :, ix]), (src, dst)
        assert torch.equal(got, F.interpolate(x, size=dst, mode="nearest-exact")), (src, dst)
    for mode in ("nearest-exact", "bilinear", "bicubic"):
        for hw in ((8, 8), (5, 7), (TH + 1, TW + 1)):
            x = torch.randn(1, 3, *hw, generator=g).to(gpu)
            assert torch.equal(ops.resample2d(x, hw, mode), x), (mode, hw)
    for mode in HRf.MODES:
        T = HRf.TAPS[mode]
        for src, dst in SHAPES:
            x = torch.full((1, 2, *src), 1.7, device=gpu)
            _, wy, _, wx = (t.numpy().astype(np.float64) for t in ops.resample_plan(mode, *src, *dst, device=gpu).tables())
            c = float(np.float32(1.7))
            S = c * np.abs(wy).sum(1)[:, None] * np.abs(wx).sum(1)[None, :]
            exact = c * wy.sum(1)[:, None] * wx.sum(1)[None, :]
            err = np.abs(ops.resample2d(x, dst, mode).cpu().numpy().astype(np.float64) - exact)
            assert (err <= 2 * T * U * S).all(), (mode, src, dst, float((err / S).max() / U))


@pytest.mark.parametrize("mode", HRf.MODES)
def test_batch_split_invariance(gpu, mode):
    """Resampling [4, C, ...] equals the concatenation of resampling its halves, bit for bit (also from unaligned halves)."""
    from adaface_amd import ops
    for src, dst in (((8, 8), (12, 12)), ((5, 7), (9, 15)), ((8, 40), (TH + 1, TW + 1))):
        x = torch.randn(4, 3, *src, generator=torch.Generator().manual_seed(src[1])).to(gpu)
        whole = ops.resample2d(x, dst, mode)
        parts = [ops.resample2d(x[lo:lo + 2].contiguous(), dst, mode) for lo in (0, 2)]
        assert torch.equal(torch.cat(parts), whole), (mode, src, dst)
        odd = [ops.resample2d(_offset_copy(x[lo:lo + 2].cpu(), gpu, 1), dst, mode) for lo in (0, 2)]
        assert torch.equal(torch.cat(odd), whole), (mode, src, dst)


def test_one_launch_per_call_and_refusals(gpu):
    from adaface_amd import _lib, ops
    x = torch.randn(2, 4, 8, 8, device=gpu)
    before = ops.resample2d_launches()
    y = ops.resample2d(x, (16, 16), "bicubic")
    ops.resample2d(torch.randn(8, 3, 16, 16, device=gpu), (24, 24), "lanczos3")
    torch.cuda.synchronize()
    assert ops.resample2d_launches() == before + 2 and tuple(y.shape) == (2, 4, 16, 16)
    assert ops.resample_plan("bicubic", 8, 8, 16, 16, device=gpu) is ops.resample_plan("bicubic", 8, 8, 16, 16, device=gpu)
    with pytest.raises(_lib.AfError, match="alias"):
        ops.resample2d(x, (8, 8), "bilinear", out=x)
    buf = torch.zeros(2 * 4 * 16 * 16 + 64, device=gpu)
    xin = buf[:512].view(2, 4, 8, 8)
    with pytest.raises(_lib.AfError, match="alias"):
        ops.resample2d(xin, (16, 16), "bilinear", out=buf[64:].view(2, 4, 16, 16))       # a partial overlap
    assert ops.resample2d_launches() == before + 2
    with pytest.raises(_lib.AfError, match="upscaling only"):
        ops.resample2d(x, (4, 8), "bilinear")
    for bad in (x.half(), x[:, :, ::2], x[0], x.cpu()):
        with pytest.raises(ValueError, match="resample2d"):
            ops.resample2d(bad, (16, 16), "bilinear")
    with pytest.raises(ValueError, match="out"):
        ops.resample2d(x, (16, 16), "bilinear", out=torch.empty(2, 4, 16, 15, device=gpu))
    with pytest.raises(ValueError, match="mode"):
        ops.resample2d(x, (16, 16), "area")


# ======================================================================================================================
# two passes, tiny model
# ======================================================================================================================
@pytest.fixture(scope="module")
def tiny_model(gpu):
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    model = instantiate_from_config(tiny_config()["model"]).eval()
    sd = O.synth_state_dict(O.unet_param_shapes(O.TINY_UNET), seed=11)
    sd.update(O.synth_state_dict(O.vae_param_shapes(O.TINY_VAE), seed=12))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected
    return model.to(gpu).set_compute_dtype("f32")


@pytest.fixture(scope="module")
def conds(tiny_model, gpu):
    g = dict(np.load(GOLD / "golden_tiny.npz"))
    return (tiny_model.get_learned_conditioning(torch.tensor(g["ddim_c"]).to(gpu)),
            tiny_model.get_learned_conditioning(torch.tensor(g["ddim_uc"]).to(gpu)))


def _sampler(which, model):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.lcm import LCMSampler
    return {"ddim": DDIMSampler, "dpm": DPMSolverSampler, "lcm": LCMSampler}[which](model)


def _first(which, conds, h, w, source, b=1, **extra):
    kw = dict(S=4, batch_size=b, shape=[4, h, w], conditioning=conds[0], unconditional_conditioning=conds[1], guidance_scale=3.0,
              verbose=False, noise_source=source)
    if which == "ddim":
        kw["eta"] = 0.5                                      # (step noise in both passes)
    kw.update(extra)
    return kw


@pytest.mark.parametrize("which", ["ddim", "dpm", "lcm"])
@pytest.mark.parametrize("lat,size", [((8, 8), (16, 16)), ((16, 16), (24, 24))])
def test_two_pass_equals_the_three_calls_by_hand(gpu, report, tiny_model, conds, which, lat, size):
    """hires.two_pass returns the bits of sample, ops.resample2d, sample(x0=, strength=) written out, with the same derived Philox
    source; its latent1 is a plain single-pass run's.  upscale_latent in the three latent modes lies within the kernel's count
    plus the rounding of the two weights to fp32, (Tx + Ty + 2) 2^-24 S, of F.interpolate on the float64 CPU copy of latent1."""
    from adaface_amd import hires, ops
    from adaface_amd.noise import PhiloxNoise
    src = lambda: PhiloxNoise(SEED, sample_ids=[6])
    first = _first(which, conds, *lat, src())
    second = hires.second_kwargs(first, steps=4)
    assert second["noise_source"].seed == src().derive("hires").seed != src().seed
    lat2, lat1 = hires.two_pass(_sampler(which, tiny_model), first, second, size, "latent", strength=0.75)
    lat2, lat1 = lat2.clone(), lat1.clone()
    s = _sampler(which, tiny_model)
    plain, _ = s.sample(**_first(which, conds, *lat, src()))
    assert torch.equal(plain, lat1) and tuple(lat1.shape) == (1, 4, *lat)
    up = ops.resample2d(plain.clone(), size, "bilinear")
    by_hand, _ = s.sample(**{**_first(which, conds, *lat, src().derive("hires")), "shape": [4, *size]}, x0=up, strength=0.75, x_T=None)
    assert torch.equal(by_hand, lat2) and tuple(lat2.shape) == (1, 4, *size) and torch.isfinite(lat2).all()
    other, _ = s.sample(**{**_first(which, conds, *lat, src()), "shape": [4, *size]}, x0=up, strength=0.75, x_T=None)
    assert not torch.equal(other, lat2)                      # (pass one's own source would give another image)
    l64 = lat1.double().cpu()
    for upscaler, mode, tmode in (("latent", "bilinear", "bilinear"), ("latent-bicubic", "bicubic", "bicubic"),
                                  ("latent-nearest", "nearest-exact", "nearest-exact")):
        got = hires.upscale_latent(tiny_model, lat1, size, upscaler).double().cpu().numpy()
        kw = {} if tmode == "nearest-exact" else dict(align_corners=False)
        ref = F.interpolate(l64, size=size, mode=tmode, **kw).numpy()
        iy, wy = (t.numpy() for t in ops.resample_taps(mode, lat[0], size[0]))
        ix, wx = (t.numpy() for t in ops.resample_taps(mode, lat[1], size[1]))
        _, S = HRf.resample_f64(l64.numpy(), iy, wy, ix, wx)
        T = HRf.TAPS[mode]
        err = np.abs(got - ref)
        # (1e-12 max|ref|: the distance of the tables from F.interpolate in float64, tests/test_hires_cpu.py)
        bound = (2 * T + 2) * U * S + 1e-12 * np.abs(ref).max()
        assert (err <= bound).all(), (upscaler, float((err / bound).max()))
        report(f"hires upscale_latent {upscaler} {lat}->{size} [{which}] vs F.interpolate float64: worst |err| / bound",
               float((err / bound).max()), 1.0, 1.0)


def test_pixel_upscaler_hands_pass_two_the_composition(gpu, report, tiny_model, conds):
    """A pixel-bicubic run's pass-two x0 against device decode, float64 F.interpolate on the CPU, clamp, device encode: SAMPLER_TOL
    of max|ref|."""
    from adaface_amd import hires, img2img
    from adaface_amd.noise import PhiloxNoise
    s = _sampler("ddim", tiny_model)
    seen = []
    inner = s.sample

    def rec(**kw):
        seen.append(kw)
        return inner(**kw)
    s.sample = rec
    first = _first("ddim", conds, 8, 8, PhiloxNoise(SEED, sample_ids=[6]), S=2)
    lat2, lat1 = hires.two_pass(s, first, hires.second_kwargs(first), (16, 16), "pixel-bicubic", strength=0.5)
    assert len(seen) == 2 and seen[1]["strength"] == 0.5 and seen[1]["shape"] == [4, 16, 16] and tuple(lat2.shape) == (1, 4, 16, 16)
    x0 = seen[1]["x0"]
    img = tiny_model.decode_first_stage(lat1)
    assert tuple(img.shape) == (1, 3, 64, 64)
    up = F.interpolate(img.double().cpu(), size=(128, 128), mode="bicubic", align_corners=False).clamp(-1.0, 1.0)
    ref = img2img.encode_image(tiny_model, up.float().to(gpu))
    err = (x0 - ref).abs().max().item() / ref.abs().max().item()
    print(f"pixel-bicubic x0 vs decode / float64 interpolate / encode: {err:.3e} of max|ref| {ref.abs().max().item():.3f}")
    report("hires pixel-bicubic pass-two x0 vs decode, float64 F.interpolate, clamp, encode [f32]", err, 1.0, SAMPLER_TOL)
    assert err < SAMPLER_TOL, err
    assert torch.equal(x0, hires.upscale_latent(tiny_model, lat1, (16, 16), "pixel-bicubic"))


class _Standin:
    """apply_model replaced by an element-wise function of (x, t) on the GPU, so that a sample's eps depends on that sample alone
    (tests/test_lcm_gpu.py): eps = sigma_t x + 0.05 sin(3 x), and 0.05 sin(2 x) for the unconditional half."""

    def __init__(self, model):
        self.model = model

    def eps(self, x, t, k):
        return self.model.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1) * x + 0.05 * torch.sin(k * x)

    def __enter__(self):
        object.__setattr__(self.model, "apply_model", lambda x, t, c: self.eps(x, t, 3.0))
        object.__setattr__(self.model, "apply_model_cfg_twin", lambda x, t, twin: torch.cat([self.eps(x, t, 3.0), self.eps(x, t, 2.0)]))
        return self

    def __exit__(self, *exc):
        object.__delattr__(self.model, "apply_model")
        object.__delattr__(self.model, "apply_model_cfg_twin")


@pytest.mark.parametrize("which", ["ddim", "dpm", "lcm"])
def test_both_passes_are_split_invariant(gpu, tiny_model, which):
    """With a PhiloxNoise source, a batch of 4 equals two batches of 2 with first_id 0 and 2, bit for bit, through both passes;
    the same seed again gives the same tensors, seed + 1 others."""
    from adaface_amd import hires
    from adaface_amd.noise import PhiloxNoise

    def run(b, source):
        ctx = torch.zeros(b * 16, 77, 64, device=gpu)
        first = _first(which, (ctx, ctx + 1.0), 8, 8, source, b=b)
        if which == "dpm":
            first["algorithm"] = "sde-dpmsolver++"
        l2, l1 = hires.two_pass(_sampler(which, tiny_model), first, hires.second_kwargs(first), (16, 16), "latent-bicubic", strength=0.75)
        return l2.clone(), l1.clone()
    with _Standin(tiny_model):
        whole = run(4, PhiloxNoise(SEED))
        parts = [run(2, PhiloxNoise(SEED, first_id=lo)) for lo in (0, 2)]
        again = run(4, PhiloxNoise(SEED))
        other = run(4, PhiloxNoise(SEED + 1))
    for k in (0, 1):
        assert torch.isfinite(whole[k]).all() and whole[k].std().item() > 0.1
        assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
        assert torch.equal(again[k], whole[k]) and not torch.equal(other[k], whole[k])
    assert tuple(whole[0].shape) == (4, 4, 16, 16) and not torch.equal(whole[0][0], whole[0][1])


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_pass_two_schedules_start_fresh(gpu, tiny_model, conds, which):
    """The DeepCache and T-GATE logs after two_pass are pass two's own: as long as its executed steps, first entries "full" and None
    with the opt-ins off, "refresh" (never a reuse of pass one's feature) and None with them on."""
    from adaface_amd import hires
    from adaface_amd.noise import PhiloxNoise
    for extra, head in ((dict(), "full"), (dict(deep_cache_interval=2, tgate_step=2), "refresh")):
        s = _sampler(which, tiny_model)
        first = {**_first(which, conds, 8, 8, PhiloxNoise(SEED, sample_ids=[6]), **extra), "eta": 0.0}
        lat2, _ = hires.two_pass(s, first, hires.second_kwargs(first), (16, 16), "latent", strength=0.75)
        assert torch.isfinite(lat2).all()
        assert len(s.deep_cache_log) == len(s.tgate_log) == 3, (s.deep_cache_log, s.tgate_log)      # int(4 * 0.75) executed steps
        assert s.deep_cache_log[0] == head and s.tgate_log[0] is None, (s.deep_cache_log, s.tgate_log)
        if extra:
            assert "replay" in s.tgate_log and s.tgate_log.index("capture") == 1
