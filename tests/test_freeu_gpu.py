"""GPU tests of FreeU (af_freeu.hip, af_set_freeu) against the restatement of tests/freeu_ref.py.

Operator: one site, every storage type and both versions, from 2 x 2 maps to 64 x 64 (the single-launch form up to 256 pixels,
the chunked one above), per element within one storage rounding plus the project's f32 operator bar; the halves FreeU must not
touch come back bit for bit, the result does not depend on the run or on the rest of the batch, and a skip's mean is scaled by
s.  Model (tiny config, synthetic weights seed 11): off is off bit for bit and launch for launch; on, eps against the restated
walk under the bars of tests/test_model_gpu.py / tests/test_fp16_gpu.py; the cached forwards keep their promises with a site as
the kept concatenation; token merging and the fp8 mode compose; once at SD-1.5 widths."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import freeu_ref as FR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = {"f32": 2e-4, "bf16": 3e-2, "f16": 3e-2 / 8}      # tests/test_model_gpu.py; f16: F16_MODEL_TOL of tests/test_fp16_gpu.py
OP_BAR = 2e-4                                           # the project's f32 operator bar, of max |ref|
CFG = O.TINY_UNET
DTYPES = ["f32", "bf16", "f16"]
# (B, Ch, Cs, H, W): 2 x 2 (-1 is the Nyquist bin), non-square, tiles that straddle backbone and skip vectors, 8 x 8, 256 pixels
# (the last single-launch size), 4 chunks, and 16 chunks on one channel vector
OP_SHAPES = [(1, 16, 8, 2, 2), (2, 16, 8, 2, 6), (2, 32, 24, 6, 10), (3, 64, 32, 8, 8), (2, 64, 64, 16, 16), (2, 32, 16, 32, 32),
             (1, 16, 8, 64, 64)]
SETTINGS = {1: (1,) + FR.V1_SD15, 2: (2,) + FR.V2_SD15}


def _stored(t, dtype):
    """t as the storage type holds it, float32"""
    return t.to({"bf16": torch.bfloat16, "f16": torch.float16}[dtype]).float() if dtype != "f32" else t.float()


def _ulp(ref, dtype):
    """one unit in the last place of the storage type at |ref| (float64)"""
    bits = {"bf16": 7, "f16": 10, "f32": 23}[dtype]
    lo = 2.0 ** -14 if dtype == "f16" else 2.0 ** -126                           # (below it the spacing stays that of the last binade)
    e = torch.floor(torch.log2(ref.abs().clamp_min(lo)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - bits)


def _bound(ref, dtype):
    """per element: the single rounding to storage (none for f32) plus the f32 operator bar of max |ref|"""
    b = torch.full_like(ref, OP_BAR * float(ref.abs().max()))
    return b if dtype == "f32" else b + _ulp(ref, dtype)


_op_inputs = {}


def _op_case(shape, dtype):
    """(h, skip) rounded to storage: a per-channel offset of order 3, a low-frequency component, noise."""
    if (shape, dtype) not in _op_inputs:
        B, Ch, Cs, H, W = shape
        g = torch.Generator().manual_seed(300 + Ch + 7 * H + W)
        yy = torch.arange(H, dtype=torch.float32)[:, None] / H
        xx = torch.arange(W, dtype=torch.float32)[None, :] / W

        def make(C):
            off = 3.0 * torch.randn(B, C, 1, 1, generator=g)
            amp = torch.randn(B, C, 1, 1, generator=g)
            ph = torch.rand(B, C, 1, 1, generator=g)
            wave = amp * torch.cos(2 * torch.pi * (yy + ph)) + amp.flip(1) * torch.sin(2 * torch.pi * (xx - yy + ph))
            return _stored(off + wave + 0.5 * torch.randn(B, C, H, W, generator=g), dtype)

        _op_inputs[shape, dtype] = (make(Ch), make(Cs))
    return _op_inputs[shape, dtype]


# ======================================================================================================================
# the operator
# ======================================================================================================================
@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_matches_the_reference(gpu, report, dtype, shape, version):
    from adaface_amd import ops
    B, Ch, Cs, H, W = shape
    h, skip = _op_case(shape, dtype)
    b, s = 1.4, 0.2
    ref_h, ref_s = FR.apply_site(h, skip, version, b, s)
    got_h, got_s = (t.cpu().double() for t in ops.freeu(h.to(gpu), skip.to(gpu), version, b, s, dtype=dtype))
    worst = 0.0
    for name, got, ref in (("backbone", got_h, ref_h), ("skip", got_s, ref_s)):
        assert torch.isfinite(got).all(), name
        margin = (got - ref).abs() / _bound(ref, dtype)
        print(f"freeu v{version} {shape} [{dtype}] {name}: max |got - ref| = {float((got - ref).abs().max()):.3e}, "
              f"{float(margin.max()):.3f} of the bound, max |ref| = {float(ref.abs().max()):.3f}")
        worst = max(worst, float(margin.max()))
    report(f"freeu op v{version} {'x'.join(map(str, shape))}: |got - ref| over (ulp + 2e-4 max|ref|) [{dtype}]", worst, 1.0, 1.0)
    assert worst <= 1.0, worst
    # structure: the upper half of the backbone is never written
    assert torch.equal(got_h[:, Ch // 2:].float(), h[:, Ch // 2:])


@pytest.mark.parametrize("shape", [(3, 64, 32, 8, 8), (2, 32, 16, 32, 32)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_structure(gpu, dtype, shape):
    from adaface_amd import ops
    B, Ch, Cs, H, W = shape
    h, skip = _op_case(shape, dtype)
    hg, sg = h.to(gpu), skip.to(gpu)
    for version in (1, 2):
        # s = 1: the skip's bits stay; b = 1: the backbone's
        oh, os_ = ops.freeu(hg, sg, version, 1.4, 1.0, dtype=dtype)
        assert torch.equal(os_.cpu(), skip) and not torch.equal(oh.cpu(), h)
        oh, os_ = ops.freeu(hg, sg, version, 1.0, 0.2, dtype=dtype)
        assert torch.equal(oh.cpu(), h) and not torch.equal(os_.cpu(), skip)
        oh, os_ = ops.freeu(hg, sg, version, 1.0, 1.0, dtype=dtype)
        assert torch.equal(oh.cpu(), h) and torch.equal(os_.cpu(), skip)
        # run to run
        a = ops.freeu(hg, sg, version, 1.4, 0.2, dtype=dtype)
        b = ops.freeu(hg, sg, version, 1.4, 0.2, dtype=dtype)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # a sample alone, and at position 2 of a batch of 3 (other samples in front of it)
        g = torch.Generator().manual_seed(9)
        h3 = torch.cat([_stored(2 * torch.randn(2, Ch, H, W, generator=g), dtype), h[:1]])
        s3 = torch.cat([_stored(2 * torch.randn(2, Cs, H, W, generator=g), dtype), skip[:1]])
        alone = ops.freeu(hg[:1], sg[:1], version, 1.4, 0.2, dtype=dtype)
        batch = ops.freeu(h3.to(gpu), s3.to(gpu), version, 1.4, 0.2, dtype=dtype)
        assert torch.equal(batch[0][2:], alone[0]) and torch.equal(batch[1][2:], alone[1])


@pytest.mark.parametrize("shape", [(2, 32, 24, 6, 10), (2, 64, 64, 16, 16), (2, 32, 16, 32, 32)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_scales_the_mean_of_the_skip(gpu, report, dtype, shape):
    """The (0, 0) frequency is in the box: the mean of every skip map is multiplied by s.  Bound: every output element is within
    the operator's bound of the exact result, so the mean is within that bound taken at max |ref|."""
    from adaface_amd import ops
    h, skip = _op_case(shape, dtype)
    _, got = ops.freeu(h.to(gpu), skip.to(gpu), 1, 1.2, 0.5, dtype=dtype)
    want = 0.5 * skip.double().mean((-2, -1))
    ref = FR.fourier_filter(skip, 1, 0.5)
    assert float((ref.mean((-2, -1)) - want).abs().max()) < 1e-12               # (the reference itself)
    bound = float(_bound(ref.abs().max().reshape(1), dtype))
    err = float((got.cpu().double().mean((-2, -1)) - want).abs().max())
    report(f"freeu op skip mean, s = 0.5, {'x'.join(map(str, shape))} [{dtype}]", err, 1.0, bound)
    assert err <= bound, (err, bound)


def test_op_refusals(gpu):
    from adaface_amd import ops
    from adaface_amd._lib import AfError
    z = lambda *s: torch.zeros(*s, device=gpu)
    for hs, ss, kw, msg in (((1, 16, 1, 8), (1, 8, 1, 8), {}, "sides"), ((1, 16, 8, 1), (1, 8, 8, 1), {}, "sides"),
                            ((1, 24, 4, 4), (1, 8, 4, 4), {}, "backbone channels"), ((1, 16, 4, 4), (1, 12, 4, 4), {}, "skip channels"),
                            ((1, 16, 4, 4), (1, 8, 4, 4), dict(version=3), "version"), ((1, 16, 4, 4), (1, 8, 4, 4), dict(version=0), "version"),
                            ((1, 16, 4, 4), (1, 8, 4, 4), dict(b=0.9), "outside"), ((1, 16, 4, 4), (1, 8, 4, 4), dict(b=2.5), "outside"),
                            ((1, 16, 4, 4), (1, 8, 4, 4), dict(s=-0.1), "outside"), ((1, 16, 4, 4), (1, 8, 4, 4), dict(s=1.1), "outside")):
        a = dict(version=1, b=1.2, s=0.9)
        a.update(kw)
        with pytest.raises(AfError, match=rf"rc=-1.*{msg}"):
            ops.freeu(z(*hs), z(*ss), a["version"], a["b"], a["s"], dtype="f32")


# ======================================================================================================================
# the model: tiny config, both call forms (maps down to 2 x 2, and non-square down to 4 x 2)
# ======================================================================================================================
FORMS = {"twin1_16x16": (True, 1, 16, 16), "b3_32x16": (False, 3, 32, 16)}      # twin, B of x, H, W


def _unet_kwargs(cfg):
    return dict(in_channels=cfg.in_channels, model_channels=cfg.model_channels, out_channels=cfg.out_channels,
                num_res_blocks=cfg.num_res_blocks, attention_resolutions=cfg.attention_resolutions,
                channel_mult=cfg.channel_mult, num_heads=cfg.num_heads, context_dim=cfg.context_dim,
                transformer_depth=cfg.transformer_depth, n_context_layers=cfg.n_context_layers)


def _rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if not torch.isfinite(got).all():
        return float("inf")
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


@pytest.fixture(scope="module")
def tiny_sd():
    return O.synth_state_dict(O.unet_param_shapes(CFG), seed=11)


@pytest.fixture(scope="module")
def inputs():
    out = {}
    for n, (name, (twin, B, H, W)) in enumerate(FORMS.items()):
        g = torch.Generator().manual_seed(400 + n)
        Bf = 2 * B if twin else B
        out[name] = dict(x=torch.randn(B, 4, H, W, generator=g), t=torch.tensor([981, 500, 1][:B]),
                         ctx=torch.randn(Bf * 16, 77, CFG.context_dim, generator=g), Bf=Bf)
    return out


@pytest.fixture(scope="module")
def engines(gpu, tiny_sd):
    from adaface_amd.engine import Engine
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = Engine(dtype=dtype, unet=_unet_kwargs(CFG), vae=None)
            assert made[dtype].load_state_dict(tiny_sd) == []
        return made[dtype]
    yield get
    for e in made.values():
        e.close()


_ref_cache = {}


def _reference(tiny_sd, inputs, form, freeu):
    """eps of the restated walk, once per (form, setting)"""
    if (form, freeu) not in _ref_cache:
        i = inputs[form]
        rep = (lambda v: torch.cat([v, v])) if FORMS[form][0] else (lambda v: v)
        with torch.no_grad():
            _ref_cache[form, freeu] = FR.unet_forward(tiny_sd, CFG, rep(i["x"]), rep(i["t"]), i["ctx"], freeu=freeu)
    return _ref_cache[form, freeu]


def _forward(eng, inputs, form, gpu):
    twin = FORMS[form][0]
    i = inputs[form]
    eng.set_context(i["ctx"].to(gpu), i["Bf"], layerwise=True)
    x, t = i["x"].to(gpu), i["t"].to(gpu)
    return lambda: (eng.unet_forward_twin if twin else eng.unet_forward)(x, t)


def test_sites_of_the_engine(gpu, engines):
    eng = engines("bf16")
    assert eng.freeu_num_sites() == 10 and eng.freeu_sites() == FR.sites(CFG)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_off_is_off(gpu, tiny_sd, inputs, dtype, form):
    """Never set (a fresh engine, before any set_freeu call), version 0, and version 0 after version 2: the same bits and the
    same launch counters."""
    from adaface_amd import _lib
    from adaface_amd.engine import Engine
    eng = Engine(dtype=dtype, unet=_unet_kwargs(CFG), vae=None)
    assert eng.load_state_dict(tiny_sd) == []
    fwd = _forward(eng, inputs, form, gpu)
    fwd()                                                        # (one-time work of a handle's first forward)
    _lib.plan_counts(reset=True)
    plain = fwd()
    pc_plain = _lib.plan_counts(reset=True)
    eng.set_freeu(0)
    assert torch.equal(fwd(), plain)
    assert _lib.plan_counts(reset=True) == pc_plain
    eng.set_freeu(*SETTINGS[2])
    on = fwd()
    _lib.plan_counts(reset=True)
    eng.set_freeu(0, 1.3, 1.4, 0.9, 0.2)                          # (the numbers of an "off" call do not matter)
    assert torch.equal(fwd(), plain)
    assert _lib.plan_counts(reset=True) == pc_plain
    assert torch.isfinite(on).all() and not torch.equal(on, plain)
    # b = s = 1 is the plain forward too
    eng.set_freeu(1, 1.0, 1.0, 1.0, 1.0)
    assert torch.equal(fwd(), plain)
    eng.close()


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_model_matches_the_reference(gpu, report, engines, inputs, tiny_sd, dtype, form, version):
    eng = engines(dtype)
    try:
        fwd = _forward(eng, inputs, form, gpu)
        eng.set_freeu(0)
        off = fwd()
        err_off = _rel(off, _reference(tiny_sd, inputs, form, None))
        eng.set_freeu(*SETTINGS[version])
        on = fwd()
        assert torch.equal(fwd(), on)                                            # deterministic
        assert torch.isfinite(on).all() and not torch.equal(on, off)
        err = _rel(on, _reference(tiny_sd, inputs, form, SETTINGS[version]))
        print(f"tiny freeu v{version} {form} [{dtype}]: eps err {err:.3e} (FreeU off, same engine and inputs: {err_off:.3e}; bar {TOL[dtype]:.2e})")
        report(f"tiny freeu v{version} {form}: eps vs restated reference [{dtype}]", err, 1.0, TOL[dtype])
        report(f"tiny freeu off {form}: eps vs reference, same inputs [{dtype}]", err_off, 1.0, TOL[dtype])
        assert err < TOL[dtype], (err, err_off)
    finally:
        eng.set_freeu(0)


def test_forward_refuses_a_side_of_one(gpu, engines, inputs):
    """An 8 x 8 latent reaches 1 x 1 at the deepest sites: AF_ERR_INVALID with a message, before anything is launched."""
    from adaface_amd import _lib
    eng = engines("bf16")
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(1, 4, 8, 8, generator=g).to(gpu), torch.tensor([500]).to(gpu)
    eng.set_context(torch.randn(16, 77, CFG.context_dim, generator=g).to(gpu), 1, layerwise=True)
    try:
        eng.set_freeu(*SETTINGS[1])
        _lib.plan_counts(reset=True)
        with pytest.raises(_lib.AfError, match=r"rc=-1.*sides >= 2"):
            eng.unet_forward(x, t)
        assert not any(_lib.plan_counts(reset=True).values())
    finally:
        eng.set_freeu(0)


def test_set_freeu_refusals(gpu, engines):
    from adaface_amd._lib import AfError, check
    eng = engines("bf16")
    for bad in ((3, 1.2, 1.4, 0.9, 0.2), (1, 0.9, 1.4, 0.9, 0.2), (1, 1.2, 2.5, 0.9, 0.2), (2, 1.2, 1.4, -0.5, 0.2), (2, 1.2, 1.4, 0.9, 1.5)):
        with pytest.raises(ValueError):
            eng.set_freeu(*bad)
        with pytest.raises(AfError, match=r"rc=-1.*af_set_freeu"):          # and the library itself
            check(eng._lib.af_set_freeu(eng._h, *[float(v) if i else int(v) for i, v in enumerate(bad)]), "af_set_freeu")
    eng.set_freeu(0, 9.0, 9.0, 9.0, 9.0)                                    # off is always accepted


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cached_forwards_keep_their_promises(gpu, engines, inputs, dtype, depth):
    """depth 2: the kept concatenation (output block 10) is no site; depth 3: it is site 9, whose backbone half is kept scaled
    and whose skip alone is filtered on a reuse step."""
    from adaface_amd._lib import AfError
    eng = engines(dtype)
    assert (12 - depth in [s[0] for s in eng.freeu_sites()]) == (depth == 3)
    try:
        for form, (twin, B, H, W) in FORMS.items():
            eng.set_freeu(*SETTINGS[2])
            fwd = _forward(eng, inputs, form, gpu)
            full = fwd()
            x, t = inputs[form]["x"].to(gpu), inputs[form]["t"].to(gpu)
            assert torch.equal(eng.unet_forward_cached(x, t, depth=depth, mode="refresh", twin=twin), full)
            assert torch.equal(eng.unet_forward_cached(x, t, depth=depth, mode="reuse", twin=twin), full)
            assert torch.equal(eng.unet_forward_cached(x, t, depth=depth, mode="reuse", twin=twin), full)      # (D is not consumed)
            eng.set_freeu(*SETTINGS[2])                                       # the same setting again keeps D
            assert torch.equal(eng.unet_forward_cached(x, t, depth=depth, mode="reuse", twin=twin), full)
            eng.set_freeu(*SETTINGS[1])                                       # a change of the setting drops it
            with pytest.raises(AfError, match="no kept feature"):
                eng.unet_forward_cached(x, t, depth=depth, mode="reuse", twin=twin)
    finally:
        eng.set_freeu(0)


@pytest.mark.parametrize("mode", ["tome", "fp8"])
def test_composition(gpu, tiny_sd, inputs, mode):
    """bf16, token merging 0.5 + FreeU and the fp8 mode + FreeU: finite, deterministic, and not the FreeU-off result."""
    from adaface_amd.engine import Engine
    eng = Engine(dtype="bf16", unet=_unet_kwargs(CFG), vae=None)
    assert eng.load_state_dict(tiny_sd) == []
    if mode == "tome":
        eng.set_tome(0.5)
    else:
        eng.set_fp8(True)
    for form in FORMS:
        fwd = _forward(eng, inputs, form, gpu)
        eng.set_freeu(0)
        off = fwd()
        for version in (1, 2):
            eng.set_freeu(*SETTINGS[version])
            on = fwd()
            assert torch.isfinite(on).all() and torch.equal(fwd(), on) and not torch.equal(on, off)
        eng.set_freeu(0)
        assert torch.equal(fwd(), off)
    eng.close()


def test_sd15_twin_64x64(gpu):
    """SD-1.5 widths, Bf = 2 twin, version 2: the chunked form at C = 320 / 640 and the single-launch form at 1280.  Ten sites,
    finite, the same bits twice, and the plain forward's bits again after version 0."""
    from adaface_amd.engine import Engine
    from adaface_amd.synth import synth_weights_into
    cfg = O.SD15_UNET
    g = torch.Generator().manual_seed(43)
    x = torch.randn(1, 4, 64, 64, generator=g).to(gpu)
    t = torch.randint(0, 1000, (1,), generator=g).to(gpu)
    ctx = torch.randn(2 * 16, 77, cfg.context_dim, generator=g).to(gpu)
    eng = Engine(dtype="bf16", unet=_unet_kwargs(cfg))
    synth_weights_into(eng, O.unet_param_shapes(cfg), seed=42, device=gpu)
    eng.set_context(ctx, 2, layerwise=True)
    plain = eng.unet_forward_twin(x, t)
    eng.set_freeu(*SETTINGS[2])
    assert eng.freeu_sites() == FR.sites(cfg) and eng.freeu_num_sites() == 10
    on = eng.unet_forward_twin(x, t)
    assert torch.isfinite(on).all() and not torch.equal(on, plain)
    assert torch.equal(eng.unet_forward_twin(x, t), on)
    print("sd15 twin Bf=2 64x64 freeu v2: relative deviation from the plain forward", _rel(on, plain))
    eng.set_freeu(0)
    assert torch.equal(eng.unet_forward_twin(x, t), plain)
    eng.close()
