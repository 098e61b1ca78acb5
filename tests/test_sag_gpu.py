"""GPU tests of self-attention guidance (af_sag.hip, af_sag_set / af_sag_read, guidance.py) against the float64 restatement of
tests/sag_ref.py.

Kernels: the attention mass against float64 on the same stored operands (three storage types, strided column views of a
[B, N, 3C] buffer, the model's middle-block shapes and a non-power-of-two N), the threshold it implies, bits that depend on
neither the run nor the batch split; the fused degrade element by element within the bound of its counted fp32 roundings, at the
smallest plane (where both edges reflect into the same rows), a non-square one, more than one row band and the real 64 x 64, on
unaligned views, with the aliasing rule and the launch counter.  Model (tiny config, synthetic weights seed 11, f32): the captured
mass against the oracle's middle-block q and k, capture on / off leaves eps bit for bit alone.  Samplers: DDIM and DPM-Solver++
against the restatement driving the oracle, with and without CFG, and every refused combination at sample()."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import dpmpp_ref as R  # noqa: E402
import sag_ref as SR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ROOT / "tests" / "golden"
CFG = O.TINY_UNET
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# the bars tests/test_ops_gpu.py (TOL) and tests/test_fp16_gpu.py (F16_OP_TOL) apply to attention outputs, of max |ref|
ATTN_BAR = {"f32": 2e-4, "bf16": 1.5e-2, "f16": 1.5e-2 / 8}
MASS_SHAPES = [(4, 2, 128), (16, 2, 128), (64, 8, 160), (96, 8, 160)]          # (N, heads, dh)
FWD_TOL_F32 = 2e-4                         # tests/test_model_gpu.py: TOL["f32"], max-abs error / max |ref| of one forward
MASS_TOL = 5 * FWD_TOL_F32                 # the captured mass (mean 1): five times that bar, for the softmax over the block's error
SAMPLER_TOL = 1e-3                         # tests/test_dpm_solver_gpu.py / tests/test_lcm_gpu.py: of max |ref|, f32 mode
SENTINEL = -12345.5
PAD = 8
f32 = lambda v: float(np.float32(v))


# ======================================================================================================================
# the attention-mass kernel
# ======================================================================================================================
_mass_cases = {}


def _mass_case(B, N, heads, dh, dtype):
    """(the [B, N, 3C] buffer as stored in `dtype`, float64 reference mass of its q | k columns).  Normals, plus a per-key score
    offset of +-0.7 through the first dim of every head (q: sqrt(dh), k: +-0.7 exactly), so that the masses fall into two groups
    on either side of the threshold 1.0."""
    key = (B, N, heads, dh, dtype)
    if key not in _mass_cases:
        C = heads * dh
        g = torch.Generator().manual_seed(100 * N + B)
        buf = torch.randn(B, N, 3 * C, generator=g)
        sign = (torch.rand(B, N, 1, generator=g) < 0.5).float() * 2 - 1
        buf[:, :, 0:C:dh] += math.sqrt(dh)
        buf[:, :, C:2 * C:dh] = 0.7 * sign
        stored = buf.to(DT[dtype])
        ref = SR.mass(stored[:, :, :C].float().numpy(), stored[:, :, C:2 * C].float().numpy(), heads)
        _mass_cases[key] = (stored, ref)
    return _mass_cases[key]


def _mass_on_gpu(stored, heads, gpu):
    from adaface_amd import ops
    dev = stored.to(gpu)
    C = dev.shape[2] // 3
    q, k = dev[:, :, :C], dev[:, :, C:2 * C]                  # strided column views, as the model passes them
    assert q.stride() == (dev.shape[1] * 3 * C, 3 * C, 1) and not q.is_contiguous()
    return ops.sag_mass(q, k, heads)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,heads,dh", MASS_SHAPES)
def test_mass_against_float64_on_the_stored_operands(gpu, report, N, heads, dh, B, dtype):
    stored, ref = _mass_case(B, N, heads, dh, dtype)
    got = _mass_on_gpu(stored, heads, gpu).cpu().numpy().astype(np.float64)
    assert got.shape == (B, N) and np.isfinite(got).all()
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    err_sum = float(np.abs(got.sum(axis=1) - N).max())
    print(f"sag mass N={N} h={heads} dh={dh} B={B} [{dtype}]: max err {err:.3e} of max|ref| {scale:.3f}; |sum - N| {err_sum:.3e}")
    report(f"sag mass N{N} h{heads} d{dh} B{B}[{dtype}]", err, scale, ATTN_BAR[dtype] * scale)
    report(f"sag mass N{N} h{heads} d{dh} B{B}: |sum_j mass - N|[{dtype}]", err_sum, float(N), ATTN_BAR[dtype] * N)
    assert err <= ATTN_BAR[dtype] * scale, (err, scale)
    assert err_sum <= ATTN_BAR[dtype] * N, err_sum


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,heads,dh", MASS_SHAPES)
def test_threshold_agrees_with_the_reference(gpu, N, heads, dh, B):
    """mass > 1 equals ref > 1 on every key whose reference mass is further from 1.0 than 100 x the f32 bar of the test above
    (of max |ref|); from the float64 reference alone, at most 5 % of the keys are that close.  fp32 storage is the case the bar
    belongs to; the kernel computes in fp32 from the stored operands whatever their type, so bf16 and fp16 storage are held to
    the same margin."""
    for dtype in ("f32", "bf16", "f16"):
        stored, ref = _mass_case(B, N, heads, dh, dtype)
        margin = 100 * ATTN_BAR["f32"] * float(np.abs(ref).max())
        far = np.abs(ref - 1.0) > margin
        assert 1.0 - far.mean() <= 0.05, (dtype, 1.0 - far.mean())
        assert (ref > 1.0).any() and (ref < 1.0).any()
        got = _mass_on_gpu(stored, heads, gpu).cpu().numpy()
        assert np.array_equal((got > 1.0)[far], (ref > 1.0)[far]), dtype


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("N,heads,dh", MASS_SHAPES)
def test_mass_is_batch_split_invariant(gpu, N, heads, dh, dtype):
    """B = 3 equals B = 1 and B = 2 concatenated, bit for bit; the same call again gives the same bits."""
    stored, _ = _mass_case(3, N, heads, dh, dtype)
    whole = _mass_on_gpu(stored, heads, gpu)
    parts = torch.cat([_mass_on_gpu(stored[:1], heads, gpu), _mass_on_gpu(stored[1:], heads, gpu)])
    assert torch.equal(whole, parts)
    assert torch.equal(_mass_on_gpu(stored, heads, gpu), whole)
    assert not torch.equal(whole[0], whole[1])


def test_mass_scalar_path_and_refusals(gpu):
    """An operand one element off 16-byte alignment takes the element loads and gives the wide path's bits; N above the cap and
    mismatched operands are refused."""
    from adaface_amd import _lib, ops
    stored, _ = _mass_case(3, 96, 8, 160, "bf16")
    C = 8 * 160
    dev = stored.to(gpu)
    wide = ops.sag_mass(dev[:, :, :C], dev[:, :, C:2 * C], 8)
    flat = torch.empty(dev.numel() + 1, device=gpu, dtype=dev.dtype)
    off = flat[1:].view(dev.shape)
    off.copy_(dev)
    assert off.data_ptr() % 16 == 2
    assert torch.equal(ops.sag_mass(off[:, :, :C], off[:, :, C:2 * C], 8), wide)
    big = torch.zeros(1, ops.SAG_MAX_TOKENS + 1, 64, device=gpu)
    with pytest.raises(_lib.AfError, match=r"rc=-1.*256"):
        ops.sag_mass(big, big, 2)
    ok = torch.randn(1, ops.SAG_MAX_TOKENS, 64, device=gpu)
    m = ops.sag_mass(ok, ok, 2)
    assert abs(float(m.mean()) - 1.0) < 1e-5
    with pytest.raises(ValueError, match="sag_mass"):
        ops.sag_mass(ok, ok.half(), 2)
    with pytest.raises(ValueError, match="sag_mass"):
        ops.sag_mass(ok, ok[:, :8], 2)


# ======================================================================================================================
# the degrade kernel
# ======================================================================================================================
DEGRADE_SHAPES = [(8, 8), (16, 16), (8, 24), (64, 64)]
ACP_T = 0.31                               # alphas_cumprod of a middle timestep


def _guarded(shape, gpu, offset=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD + offset,), SENTINEL, device=gpu, dtype=torch.float32)
    return buf, buf[PAD + offset: PAD + offset + n].view(shape)


def _degrade_inputs(H, W, kind, seed):
    """x, e fp32 [2, 4, H, W] and a mass exactly representable and away from 1.0: 1.5 = on, 0.5 = off."""
    g = torch.Generator().manual_seed(seed)
    x, e = torch.randn(2, 4, H, W, generator=g), torch.randn(2, 4, H, W, generator=g)
    n = (H // 8) * (W // 8)
    if kind == "on":
        m = torch.full((2, n), 1.5)
    elif kind == "off":
        m = torch.full((2, n), 0.5)
    else:
        m = torch.where(torch.rand(2, n, generator=g) < 0.5, 1.5, 0.5)
        m[0, 0], m[1, -1] = 1.5, 0.5                         # (both values occur, whatever the draw)
    return x, e, m


def _degrade_case(gpu, H, W, blur_sigma, kind, offset=0, seed=0):
    """One launch against sag_ref.degrade; returns worst err / bound."""
    from adaface_amd import ops
    x, e, m = _degrade_inputs(H, W, kind, seed)
    alpha, sigma = f32(math.sqrt(ACP_T)), f32(math.sqrt(1.0 - ACP_T))
    w = SR.taps(blur_sigma).astype(np.float32).astype(np.float64)
    ref, bound = SR.degrade(x.numpy(), e.numpy(), m.numpy(), alpha, sigma, w)
    if kind == "off":                                        # the plain line, to its five roundings
        plain = alpha * ((x.double() - sigma * e.double()) / alpha) + sigma * e.double()
        assert np.abs(ref - plain.numpy()).max() <= 1e-12
    place = lambda t: _guarded(t.shape, gpu, offset)
    (_, dx), (_, de), (obuf, out) = place(x), place(e), place(x)
    dx.copy_(x)
    de.copy_(e)
    if offset:
        assert dx.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    before = ops.sag_launches()["degrade"]
    got = ops.sag_degrade(dx, de, m.to(gpu), alpha, sigma, blur_sigma, out=out)
    torch.cuda.synchronize()
    assert ops.sag_launches()["degrade"] == before + 1
    assert got.data_ptr() == out.data_ptr()
    host = obuf.cpu().numpy().astype(np.float64)
    lo, n = PAD + offset, x.numel()
    assert (host[:lo] == SENTINEL).all() and (host[lo + n:] == SENTINEL).all(), "wrote outside the output"
    err = np.abs(host[lo: lo + n].reshape(ref.shape) - ref)
    tag = (H, W, blur_sigma, kind, offset)
    assert (err <= bound).all(), (tag, float((err / bound).max()), int(np.argmax(err / bound)))
    if kind != "off":
        on = SR.mask_of(m.numpy(), H, W)
        assert np.abs(ref - (x.double().numpy()))[np.broadcast_to(on, ref.shape)].max() > 0.05, "the blur must matter"
    return float((err / bound).max())


@pytest.mark.parametrize("blur_sigma", [1.0, 2.0])
@pytest.mark.parametrize("H,W", DEGRADE_SHAPES)
def test_degrade_against_float64(gpu, report, H, W, blur_sigma):
    """Every element within ((1 + u)^k - 1) (sum of |terms|), k = 23 under the mask and 5 outside it (the header of
    degrade_kernel), masks all on, all off and mixed; nothing outside the output written; one launch per call."""
    worst = 0.0
    for i, kind in enumerate(("on", "off", "mixed")):
        worst = max(worst, _degrade_case(gpu, H, W, blur_sigma, kind, seed=10 * H + W + i))
    report(f"af_sag_degrade {H}x{W} blur sigma {blur_sigma}: worst |err| / bound over three masks", worst, 1.0, 1.0)


@pytest.mark.parametrize("H,W", [(8, 8), (8, 24), (64, 64)])
def test_degrade_unaligned_views(gpu, report, H, W):
    """x, eps and the output one float off 16-byte alignment."""
    worst = max(_degrade_case(gpu, H, W, 1.0, kind, offset=1, seed=77 + i) for i, kind in enumerate(("on", "mixed")))
    report(f"af_sag_degrade {H}x{W}: unaligned views, worst |err| / bound", worst, 1.0, 1.0)


def test_degrade_refusals_and_split_invariance(gpu):
    from adaface_amd import _lib, ops
    x, e, m = (t.to(gpu) for t in _degrade_inputs(16, 16, "mixed", 5))
    alpha, sigma = f32(math.sqrt(ACP_T)), f32(math.sqrt(1.0 - ACP_T))
    before = ops.sag_launches()["degrade"]
    for out in (x, e):                                       # in place is refused: a band reads its neighbours' rows
        with pytest.raises(_lib.AfError, match=r"rc=-1.*alias"):
            ops.sag_degrade(x, e, m, alpha, sigma, out=out)
    for bad in (dict(alpha=0.0), dict(alpha=-1.0), dict(blur_sigma=0.0), dict(blur_sigma=-1.0)):
        with pytest.raises(_lib.AfError, match="rc=-1"):
            ops.sag_degrade(x, e, m, **{**dict(alpha=alpha, sigma=sigma, blur_sigma=1.0), **bad})
    with pytest.raises(ValueError, match="mass"):
        ops.sag_degrade(x, e, m[:1], alpha, sigma)
    with pytest.raises(ValueError, match="eps"):
        ops.sag_degrade(x, e[:1], m, alpha, sigma)
    with pytest.raises(_lib.AfError, match=r"rc=-1.*multiples of 8"):
        ops.sag_degrade(x[:, :, :12].contiguous(), e[:, :, :12].contiguous(), m[:, :2].contiguous(), alpha, sigma)
    assert ops.sag_launches()["degrade"] == before          # a refused call launches nothing
    # batch split: B = 3 equals B = 1 and B = 2 concatenated, bit for bit; the same call again gives the same bits
    g = torch.Generator().manual_seed(9)
    x3, e3 = torch.randn(3, 4, 16, 24, generator=g).to(gpu), torch.randn(3, 4, 16, 24, generator=g).to(gpu)
    m3 = torch.where(torch.rand(3, 6, generator=g) < 0.5, 1.5, 0.5).to(gpu)
    whole = ops.sag_degrade(x3, e3, m3, alpha, sigma, 2.0)
    parts = torch.cat([ops.sag_degrade(x3[:1], e3[:1], m3[:1], alpha, sigma, 2.0), ops.sag_degrade(x3[1:], e3[1:], m3[1:], alpha, sigma, 2.0)])
    assert torch.equal(whole, parts) and torch.equal(ops.sag_degrade(x3, e3, m3, alpha, sigma, 2.0), whole)
    assert not torch.equal(whole, ops.sag_degrade(x3, e3, m3, alpha, sigma, 1.0))
    # a mass of exactly 1.0 is off, the next float above it is on
    edge = torch.tensor([[1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))]], device=gpu)
    xe, ee = x3[:1, :, :8, :16].contiguous(), e3[:1, :, :8, :16].contiguous()
    got = ops.sag_degrade(xe, ee, edge, alpha, sigma)
    off = ops.sag_degrade(xe, ee, torch.full_like(edge, 0.5), alpha, sigma)
    assert torch.equal(got[..., :8], off[..., :8]) and not torch.equal(got[..., 8:], off[..., 8:])


# ======================================================================================================================
# the model: tiny config, f32
# ======================================================================================================================
def _unet_kwargs(cfg):
    return dict(in_channels=cfg.in_channels, model_channels=cfg.model_channels, out_channels=cfg.out_channels,
                num_res_blocks=cfg.num_res_blocks, attention_resolutions=cfg.attention_resolutions,
                channel_mult=cfg.channel_mult, num_heads=cfg.num_heads, context_dim=cfg.context_dim,
                transformer_depth=cfg.transformer_depth, n_context_layers=cfg.n_context_layers)


@pytest.fixture(scope="module")
def tiny_sd():
    return O.synth_state_dict(O.unet_param_shapes(CFG), seed=11)


@pytest.fixture(scope="module")
def engine(gpu, tiny_sd):
    from adaface_amd.engine import Engine
    eng = Engine(dtype="f32", unet=_unet_kwargs(CFG), vae=None)
    assert eng.load_state_dict(tiny_sd) == []
    yield eng
    eng.close()


@pytest.mark.parametrize("side", [16, 32])
def test_engine_capture_against_the_oracle(gpu, report, engine, tiny_sd, side):
    """set_sag(True), the twin forward, and the mass read back against sag_ref on the oracle's middle-block q and k: below 1e-3
    (five times the 2e-4 f32 model bar; mass has mean 1).  With the capture off eps is bit for bit that of a handle that never
    had it on, and with it on too: the capture only reads."""
    from adaface_amd.engine import Engine
    g = torch.Generator().manual_seed(600 + side)
    c, uc = (torch.randn(16, 77, CFG.context_dim, generator=g) for _ in range(2))
    x, t = torch.randn(1, 4, side, side, generator=g), torch.tensor([500])
    with torch.no_grad():
        eps_ref, q, k = SR.oracle_eps_qk(tiny_sd, CFG, torch.cat([x, x]), torch.cat([t, t]), torch.cat([c, uc]))
    ref = SR.mass(q.numpy(), k.numpy(), CFG.num_heads)
    N = (side // 8) ** 2
    assert ref.shape == (2, N) and (ref > 1.0).any() and (ref < 1.0).any()
    fresh = Engine(dtype="f32", unet=_unet_kwargs(CFG), vae=None)            # never had the capture on
    try:
        assert fresh.load_state_dict(tiny_sd) == []
        fresh.set_context(torch.cat([c, uc]).to(gpu), 2, layerwise=True)
        base = fresh.unet_forward_twin(x.to(gpu), t.to(gpu)).clone()
        assert fresh.sag_state() == {"on": False, "B": 0, "N": 0}
    finally:
        fresh.close()
    engine.set_context(torch.cat([c, uc]).to(gpu), 2, layerwise=True)
    from adaface_amd import ops
    try:
        n0 = ops.sag_launches()["mass"]
        engine.set_sag(True)
        on = engine.unet_forward_twin(x.to(gpu), t.to(gpu)).clone()
        assert ops.sag_launches()["mass"] == n0 + 1
        assert engine.sag_state() == {"on": True, "B": 2, "N": N}
        got = engine.sag_mass().cpu().numpy().astype(np.float64)
        engine.set_sag(False)
        off = engine.unet_forward_twin(x.to(gpu), t.to(gpu)).clone()
        assert ops.sag_launches()["mass"] == n0 + 1          # off: no launch
        assert engine.sag_state() == {"on": False, "B": 2, "N": N}
        # the plain form captures its own batch
        engine.set_context(uc.to(gpu), 1, layerwise=True)
        engine.set_sag(True)
        engine.unet_forward(x.to(gpu), t.to(gpu))
        single = engine.sag_mass().cpu().numpy().astype(np.float64)
    finally:
        engine.set_sag(False)
    assert torch.equal(on, base) and torch.equal(off, base)
    fwd = float((on.cpu() - eps_ref).abs().max() / eps_ref.abs().max())
    err = float(np.abs(got - ref).max())
    err1 = float(np.abs(single - ref[1:]).max())
    print(f"sag capture {side}x{side}: mass err {err:.3e} (plain form {err1:.3e}), mass in [{ref.min():.3f}, {ref.max():.3f}]; eps {fwd:.3e}")
    report(f"tiny_unet twin forward, SAG capture on, eps vs oracle {side}x{side} [f32]", fwd, 1.0, FWD_TOL_F32)
    report(f"tiny_unet SAG captured mass vs sag_ref on the oracle {side}x{side} [f32]", err, 1.0, MASS_TOL)
    report(f"tiny_unet SAG captured mass, plain form, vs sag_ref {side}x{side} [f32]", err1, 1.0, MASS_TOL)
    assert fwd < FWD_TOL_F32, fwd
    assert err < MASS_TOL and err1 < MASS_TOL, (err, err1)


def test_engine_refusals(gpu, engine):
    """What a forward refuses while the capture is on, before any launch; sag_mass without a capture."""
    from adaface_amd import _lib
    from adaface_amd.engine import Engine
    g = torch.Generator().manual_seed(3)
    ctx = torch.randn(32, 77, CFG.context_dim, generator=g).to(gpu)
    x, t = torch.randn(1, 4, 16, 16, generator=g).to(gpu), torch.tensor([500], device=gpu)
    fresh = Engine(dtype="f32", unet=_unet_kwargs(CFG), vae=None)
    try:
        with pytest.raises(_lib.AfError, match="sag_mass"):
            fresh.sag_mass()
    finally:
        fresh.close()
    engine.set_context(ctx, 2, layerwise=True)
    try:
        engine.set_sag(True)
        with pytest.raises(_lib.AfError, match="SAG capture.*T-GATE"):
            engine.unet_forward_twin(x, t, tgate="capture")
        engine.unet_forward_cached(x, t, depth=2, mode="refresh", twin=True)
        with pytest.raises(_lib.AfError, match="SAG capture.*reuse"):
            engine.unet_forward_cached(x, t, depth=2, mode="reuse", twin=True)
        engine.set_pag(("mid",))
        engine.set_context(torch.cat([ctx, ctx[:16]]), 3, layerwise=True)
        with pytest.raises(_lib.AfError, match="SAG capture.*PAG"):
            engine.unet_forward_pag(x, t)
    finally:
        engine.set_pag(())
        engine.set_sag(False)
        engine.unet_cache_invalidate()


# ======================================================================================================================
# the samplers, tiny model
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


X_T_SEED = 2              # a start code for which the reference's masses stay 1e-2 away from the threshold at every step
ORACLE_GUIDANCE = (4.0, 2.0)
SAG_SCALE = 0.75
TS = [1, 251, 501, 751]   # the uniform S = 4 grid


@pytest.fixture(scope="module")
def run_inputs():
    g = dict(np.load(GOLD / "golden_tiny.npz"))
    x_T = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(X_T_SEED))
    return dict(x_T=x_T, c=torch.tensor(g["ddim_c"]), uc=torch.tensor(g["ddim_uc"]))


@pytest.fixture(scope="module")
def oracle_runs(tiny_sd, run_inputs):
    """sag_ref.sample_ref driving the CPU oracle, computed once: S = 4, DDIM and DPM-Solver++(2M), annealed guidance [4, 2] and
    guidance 1 (the single-leg form).  Every step's guide-leg mass keeps 1e-2 from the threshold."""
    acp = R.sd_acp()
    assert list(O.make_ddim_timesteps(4)) == TS == list(R.uniform_grid(4))
    i = run_inputs
    out = {}
    for kind in ("ddim", "dpm"):
        for name, gs in (("cfg", O.guidance_schedule(ORACLE_GUIDANCE, 4)), ("single", [1.0] * 4)):
            lat, masses = SR.sample_ref(kind, tiny_sd, CFG, acp, TS, i["x_T"], i["c"], i["uc"], gs, SAG_SCALE)
            assert len(masses) == 4 and min(float(np.abs(m - 1.0).min()) for m in masses) >= 1e-2, (kind, name)
            out[kind, name] = lat.numpy()
    return out


def _sample(which, model, inputs, gpu, guidance, **extra):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    c, uc = (model.get_learned_conditioning(inputs[k].to(gpu)) for k in ("c", "uc"))
    kw = dict(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=guidance,
              unconditional_conditioning=uc, x_T=inputs["x_T"].to(gpu), **extra)
    if which == "dpm":
        kw["timesteps"] = np.asarray(TS)
    s = (DDIMSampler if which == "ddim" else DPMSolverSampler)(model)
    return s, s.sample(**kw)[0]


@pytest.mark.parametrize("form", ["cfg", "single"])
@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_sampler_matches_restatement_on_the_oracle(gpu, report, tiny_model, run_inputs, oracle_runs, which, form):
    """sample(sag_scale = 0.75) at S = 4 in f32 mode against sag_ref.sample_ref in float64 on the CPU oracle: 1e-3 of max|ref|.
    With CFG a step is one twin call and one single-leg call; with guidance 1 it is two single-leg calls (guidance_log)."""
    ref = oracle_runs[which, form]
    guidance = list(ORACLE_GUIDANCE) if form == "cfg" else 1.0
    from adaface_amd import ops
    n0 = ops.sag_launches()
    s, lat = _sample(which, tiny_model, run_inputs, gpu, guidance, sag_scale=SAG_SCALE)
    n1 = ops.sag_launches()
    err = float(np.abs(lat.cpu().numpy() - ref).max() / np.abs(ref).max())
    print(f"{which} S=4 SAG {form} vs float64 restatement: {err:.3e} of max|ref| {np.abs(ref).max():.3f}")
    report(f"dropin {which} S=4 sag_scale 0.75 ({form}) vs float64 restatement on the oracle [f32]", err, float(np.abs(ref).max()),
           SAMPLER_TOL)
    assert err < SAMPLER_TOL, err
    first = (2, 0.0) if form == "cfg" else (1, 0.0)
    assert s.guidance_log == [first, (1, SAG_SCALE)] * 4
    assert n1["mass"] - n0["mass"] == 4 and n1["degrade"] - n0["degrade"] == 4        # one of each per step
    assert tiny_model.model.diffusion_model.sag is False                                # the capture is off again
    # the guidance matters, or the comparison would mean nothing
    _, plain = _sample(which, tiny_model, run_inputs, gpu, guidance)
    assert float((plain - lat).abs().max()) > 20 * SAMPLER_TOL * float(np.abs(ref).max())


def test_sampler_with_sag_off_is_the_run_without_it(gpu, tiny_model, run_inputs):
    for which in ("ddim", "dpm"):
        _, a = _sample(which, tiny_model, run_inputs, gpu, list(ORACLE_GUIDANCE))
        s, b = _sample(which, tiny_model, run_inputs, gpu, list(ORACLE_GUIDANCE), sag_scale=0.0, sag_blur_sigma=1.0)
        assert torch.equal(a, b) and s.guidance_log == []


def test_plms_runs_and_other_blur_sigma_changes_the_result(gpu, tiny_model, run_inputs):
    from ldm.models.diffusion.plms import PLMSSampler
    c, uc = (tiny_model.get_learned_conditioning(run_inputs[k].to(gpu)) for k in ("c", "uc"))
    kw = dict(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, unconditional_guidance_scale=3.0,
              unconditional_conditioning=uc, x_T=run_inputs["x_T"].to(gpu))
    s = PLMSSampler(tiny_model)
    a, _ = s.sample(sag_scale=SAG_SCALE, **kw)
    assert s.guidance_log == [(2, 0.0), (1, SAG_SCALE)] * 5              # (the first step calls the model twice)
    b, _ = PLMSSampler(tiny_model).sample(sag_scale=SAG_SCALE, sag_blur_sigma=2.0, **kw)
    off, _ = PLMSSampler(tiny_model).sample(**kw)
    assert torch.isfinite(a).all() and not torch.equal(a, b) and not torch.equal(a, off)


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_refused_combinations_raise_at_sample(gpu, tiny_model, run_inputs, which):
    g = list(ORACLE_GUIDANCE)
    run = lambda **kw: _sample(which, tiny_model, run_inputs, gpu, g, sag_scale=SAG_SCALE, **kw)
    try:
        tiny_model.set_pag(("mid",))
        with pytest.raises(NotImplementedError, match="pag_scale"):
            run(pag_scale=3.0)
    finally:
        tiny_model.set_pag(())
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        run(guidance_rescale=0.7)
    with pytest.raises(NotImplementedError, match="tgate_step"):
        run(tgate_step=2)
    with pytest.raises(NotImplementedError, match="deep_cache_interval"):
        run(deep_cache_interval=2)
    try:
        tiny_model.set_regions(torch.ones(2, 2, 16, 16))
        with pytest.raises(NotImplementedError, match="regional"):
            run()
    finally:
        tiny_model.set_regions(None)
    from ldm.modules.diffusionmodules.controlnet import ControlNet
    unet = tiny_model.model.diffusion_model
    try:
        net = ControlNet(image_size=32, use_spatial_transformer=True, hint_channels=3,
                         **{k: v for k, v in _unet_kwargs(CFG).items() if k not in ("n_context_layers", "out_channels")})
        unet.set_control(net, hint=torch.zeros(1, 3, 128, 128))
        with pytest.raises(NotImplementedError, match="ControlNet"):
            run()
    finally:
        unet.set_control(None)
    from ldm.models.diffusion.lcm import LCMSampler
    c, uc = (tiny_model.get_learned_conditioning(run_inputs[k].to(gpu)) for k in ("c", "uc"))
    with pytest.raises(NotImplementedError, match="sag_scale"):
        LCMSampler(tiny_model).sample(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=2.0,
                                      unconditional_conditioning=uc, x_T=run_inputs["x_T"].to(gpu), sag_scale=SAG_SCALE)
    try:
        tiny_model.model.diffusion_model.set_compute_dtype("fp8")
        with pytest.raises(NotImplementedError, match="fp8"):
            run()
    finally:
        tiny_model.model.diffusion_model.set_compute_dtype("f32")
    for bad in (dict(sag_scale=-1.0), dict(sag_scale=SAG_SCALE, sag_blur_sigma=0.0)):
        with pytest.raises(ValueError, match="sag_"):
            _sample(which, tiny_model, run_inputs, gpu, g, **bad)
