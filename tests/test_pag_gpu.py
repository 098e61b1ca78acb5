"""GPU tests of perturbed-attention guidance and guidance rescale (af_guidance.hip, af_set_pag / af_unet_forward_pag) against the
restatement of tests/pag_ref.py.

Operator: the combine alone per element within the bound of its fp32 roundings, with rescale within the project's f32 operator
bar, on both memory paths, from two elements to more than the real latent; bits that depend on neither the run, the batch nor the
path; the aliasing rule.  Model (tiny config, synthetic weights seed 11): all three legs against the oracle with a perturbing
spatial_transformer under the bars of tests/test_model_gpu.py, with the condition that the reference itself tells PAG from no
PAG; the shared prefix against three full legs; leg identity; off is off; the cached forwards; composition; the samplers
against loops written here; once at SD-1.5 widths."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import pag_ref as PR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = {"f32": 2e-4, "bf16": 3e-2, "f16": 3e-2 / 8}      # tests/test_model_gpu.py; f16: F16_MODEL_TOL of tests/test_fp16_gpu.py
OP_BAR = 2e-4                                           # the project's f32 operator bar, of max |ref|
CFG = O.TINY_UNET
N_SAMPLES = [1, 3]
PER_SAMPLE = [2, 5, 255, 256, 257, 1024, 1027, 16384, 16385]
W_, S_ = 7.5, 3.0


# ======================================================================================================================
# the guidance operator
# ======================================================================================================================
_op_inputs = {}


def _op_case(n, per):
    """(e_c, e_u, e_p) [n, per] fp32: normals with a per-sample scale in [0.5, 3] and a per-sample mean offset of order 0.3"""
    if (n, per) not in _op_inputs:
        g = torch.Generator().manual_seed(500 + 31 * n + per)
        out = []
        for _ in range(3):
            scale = 0.5 + 2.5 * torch.rand(n, 1, generator=g)
            off = 0.3 * torch.randn(n, 1, generator=g)
            out.append((scale * torch.randn(n, per, generator=g) + off).float())
        _op_inputs[n, per] = tuple(out)
    return _op_inputs[n, per]


def _place(t, gpu, offset):
    """t on the GPU, contiguous; offset = 1: its first element one float behind a 16-byte boundary (the scalar path)"""
    buf = torch.empty(t.numel() + 4, device=gpu, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _guide(ec, eu, ep, w, s, phi, gpu, offset=0, return_factor=False, out=None):
    from adaface_amd import ops
    pl = lambda t: None if t is None else _place(t, gpu, offset)
    if out is None:
        out = _place(torch.zeros_like(ec), gpu, offset)
    return ops.guidance(pl(ec), pl(eu), pl(ep), w, s, phi, return_factor=return_factor, out=out)


def _combine_bound(ec, eu, ep, w, s):
    a = lambda t: t.double().abs()
    return 8.0 * 2.0 ** -24 * (a(eu) + abs(w) * (a(ec) + a(eu)) + abs(s) * (a(ec) + a(ep)))


@pytest.mark.parametrize("offset", [0, 1], ids=["wide", "scalar"])
@pytest.mark.parametrize("per", PER_SAMPLE)
@pytest.mark.parametrize("n", N_SAMPLES)
def test_combine_within_its_roundings(gpu, report, n, per, offset):
    ec, eu, ep = _op_case(n, per)
    ref, _ = PR.guidance(ec, eu, ep, W_, S_, 0.0)
    got = _guide(ec, eu, ep, W_, S_, 0.0, gpu, offset).cpu().double()
    margin = float(((got - ref).abs() / _combine_bound(ec, eu, ep, W_, S_)).max())
    print(f"guidance combine {n} x {per} offset {offset}: worst |got - ref| / bound = {margin:.3f}")
    report(f"guidance combine {n}x{per} offset {offset}: |got - ref| over the six-rounding bound", margin, 1.0, 1.0)
    assert margin <= 1.0, margin


@pytest.mark.parametrize("phi", [0.7, 1.0])
@pytest.mark.parametrize("offset", [0, 1], ids=["wide", "scalar"])
@pytest.mark.parametrize("per", PER_SAMPLE)
@pytest.mark.parametrize("n", N_SAMPLES)
def test_rescale_within_the_operator_bar(gpu, report, n, per, offset, phi):
    ec, eu, ep = _op_case(n, per)
    ref, f_ref = PR.guidance(ec, eu, ep, W_, S_, phi)
    got, f = _guide(ec, eu, ep, W_, S_, phi, gpu, offset, return_factor=True)
    got, f = got.cpu().double(), f.cpu().double()
    assert torch.isfinite(got).all() and torch.isfinite(f).all()
    ratio = float((got - ref).abs().max() / (OP_BAR * ref.abs().max()))
    f_err = float(((f - f_ref).abs() / f_ref.abs()).max())
    print(f"guidance rescale {phi} {n} x {per} offset {offset}: max |got - ref| = {ratio:.3e} of the bar, factor rel err {f_err:.3e}")
    report(f"guidance rescale {phi} {n}x{per} offset {offset}: max |got - ref| over 2e-4 max|ref|", ratio, 1.0, 1.0)
    report(f"guidance rescale {phi} {n}x{per} offset {offset}: factor relative error", f_err, 1.0, OP_BAR)
    assert ratio <= 1.0 and f_err <= OP_BAR, (ratio, f_err)


@pytest.mark.parametrize("per", [5, 257, 1024, 1027, 16384])
def test_structure(gpu, per):
    n = 3
    ec, eu, ep = _op_case(n, per)
    for phi in (0.0, 0.7):
        base = _guide(ec, eu, ep, W_, S_, phi, gpu)
        # s = 0 with e_p given is e_p absent
        assert torch.equal(_guide(ec, eu, ep, W_, 0.0, phi, gpu), _guide(ec, eu, None, W_, 0.0, phi, gpu))
        # the wide and the scalar path give an element the same bits; so does another run
        assert torch.equal(_guide(ec, eu, ep, W_, S_, phi, gpu, offset=1), base)
        assert torch.equal(_guide(ec, eu, ep, W_, S_, phi, gpu), base)
        # a sample alone equals the same sample at position 2 of a batch of 3
        alone = _guide(ec[2:], eu[2:], ep[2:], W_, S_, phi, gpu)
        assert torch.equal(alone[0], base[2])
        # in place on e_c
        ecg = _place(ec, gpu, 0)
        from adaface_amd import ops
        ops.guidance(ecg, _place(eu, gpu, 0), _place(ep, gpu, 0), W_, S_, phi, out=ecg)
        assert torch.equal(ecg, base)
        # without an unconditional leg: e_c + s (e_c - e_p)
        ref, _ = PR.guidance(ec, None, ep, 0.0, S_, phi)
        got = _guide(ec, None, ep, 0.0, S_, phi, gpu).cpu().double()
        assert float((got - ref).abs().max()) <= OP_BAR * float(ref.abs().max())
    # w = 1, s = 0, no rescale: e_c to within the bound
    got = _guide(ec, eu, ep, 1.0, 0.0, 0.0, gpu).cpu().double()
    assert bool(((got - ec.double()).abs() <= _combine_bound(ec, eu, ep, 1.0, 0.0)).all())


def test_refusals(gpu):
    from adaface_amd import ops
    from adaface_amd._lib import AfError
    buf = torch.randn(4 * 64, device=gpu)
    ec, eu = buf[:128].view(2, 64), buf[128:].view(2, 64)
    ops.guidance(ec, eu, None, 2.0, 0.0, 0.5, out=ec)                             # exactly e_c: accepted
    for out in (buf[4:132].view(2, 64), buf[64:192].view(2, 64), eu):               # partial overlaps, and e_u itself
        with pytest.raises(AfError, match=r"rc=-1.*overlap"):
            ops.guidance(ec, eu, None, 2.0, 0.0, 0.5, out=out)
    with pytest.raises(AfError, match=r"rc=-1.*overlap"):                           # e_p under the output
        ops.guidance(ec, None, buf[100:228].view(2, 64), 2.0, 1.0, 0.0, out=eu)
    with pytest.raises(AfError, match=r"rc=-1.*per_sample"):
        ops.guidance(buf[:3].view(3, 1), buf[4:7].view(3, 1), None, 2.0, 0.0, 0.0)
    with pytest.raises(AfError, match=r"rc=-1.*rescale"):
        ops.guidance(ec, eu, None, 2.0, 0.0, 1.5)
    with pytest.raises(ValueError):
        ops.guidance(ec, eu[:1], None, 2.0, 0.0, 0.0)


# ======================================================================================================================
# the model: tiny config
# ======================================================================================================================
FORMS = {"b1_16x16": (1, 16, 16), "b2_32x16": (2, 32, 16)}      # B of x, H, W
SITE_SETS = {"mid": ("mid",), "mid+up1": ("mid", "up.blocks.1"), "down2": ("down.blocks.2",)}
SETS_OF = {"f32": ["mid", "mid+up1", "down2"], "bf16": ["mid+up1", "down2"], "f16": ["mid+up1", "down2"]}
MODEL_CASES = [(dt, s) for dt in ("f32", "bf16", "f16") for s in SETS_OF[dt]]


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
    """x, t of one leg; c and uc of B samples (16 layers each); ctx3 = [c; uc; c], ctx2 = [c; uc]"""
    out = {}
    for n, (name, (B, H, W)) in enumerate(FORMS.items()):
        g = torch.Generator().manual_seed(400 + n)
        c = torch.randn(B * 16, 77, CFG.context_dim, generator=g)
        uc = torch.randn(B * 16, 77, CFG.context_dim, generator=g)
        out[name] = dict(x=torch.randn(B, 4, H, W, generator=g), t=torch.tensor([500, 981][:B]), c=c, uc=uc,
                         ctx3=torch.cat([c, uc, c]), ctx2=torch.cat([c, uc]), B=B)
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


def _reference(tiny_sd, inputs, form, sites):
    """eps [3B] of the oracle on [x; x; x], [c; uc; c] with the last third perturbed at `sites` (None: the unpatched oracle)"""
    if (form, sites) not in _ref_cache:
        i = inputs[form]
        B = i["B"]
        x3, t3 = torch.cat([i["x"]] * 3), torch.cat([i["t"]] * 3)
        with torch.no_grad():
            if sites is None:
                _ref_cache[form, sites] = O.unet_forward(tiny_sd, CFG, x3, t3, i["ctx3"])
            else:
                with PR.patched(PR.sites_of(CFG, SITE_SETS[sites]), slice(2 * B, 3 * B)):
                    _ref_cache[form, sites] = O.unet_forward(tiny_sd, CFG, x3, t3, i["ctx3"])
    return _ref_cache[form, sites]


def _pag_forward(eng, inputs, form, gpu):
    i = inputs[form]
    eng.set_context(i["ctx3"].to(gpu), 3 * i["B"], layerwise=True)
    x, t = i["x"].to(gpu), i["t"].to(gpu)
    return lambda: eng.unet_forward_pag(x, t)


def _twin_forward(eng, inputs, form, gpu):
    i = inputs[form]
    eng.set_context(i["ctx2"].to(gpu), 2 * i["B"], layerwise=True)
    return eng.unet_forward_twin(i["x"].to(gpu), i["t"].to(gpu))


def test_sites_and_plan_of_the_engine(gpu, engines):
    from adaface_amd.engine import pag_layout, pag_plan
    eng = engines("bf16")
    lay = pag_layout(_unet_kwargs(CFG))
    try:
        eng.set_pag(())
        sites = eng.pag_sites()
        assert len(sites) == 16 and [s[0] for s in sites] == list(lay["blocks"]) and not any(s[3] for s in sites)
        assert [s[2] for s in sites] == [1, 1, 2, 2, 4, 4, 8, 4, 4, 4, 2, 2, 2, 1, 1, 1] and all(s[1] == 0 for s in sites)
        assert eng.pag_plan() == {"first_block": -1, "two_leg_blocks": 0, "two_leg_blocks_reuse": 0}
        for layers, depth in ((("mid",), 3), (("down.blocks.2",), 3), (("down.blocks.2",), 9), (("up.blocks.1", 3), 2), ((0,), 2)):
            eng.set_pag(layers)
            assert eng.pag_plan(depth) == pag_plan(_unet_kwargs(CFG), layers, depth), (layers, depth)
            assert [i for i, s in enumerate(eng.pag_sites()) if s[3]] == list(PR.sites_of(CFG, layers))
        eng.set_pag(("mid",))
        assert eng.pag_plan(3) == {"first_block": 12, "two_leg_blocks": 12, "two_leg_blocks_reuse": 3}
        eng.set_pag(("down.blocks.2",))
        assert eng.pag_plan()["two_leg_blocks"] == 7
    finally:
        eng.set_pag(())


def test_set_pag_refusals(gpu, engines, inputs):
    import ctypes as C
    from adaface_amd._lib import AfError, check
    eng = engines("bf16")
    for bad in ((16,), (-1,), (3, 3), (0, 6, 0)):
        arr = (C.c_int * len(bad))(*bad)
        with pytest.raises(AfError, match=r"rc=-1.*af_set_pag"):
            check(eng._lib.af_set_pag(eng._h, arr, len(bad)), "af_set_pag")
    for bad in (("middle",), (16,), (True,), (1.5,)):
        with pytest.raises(ValueError, match="PAG"):
            eng.set_pag(bad)
    # no site set, and a batch that is no multiple of three: refused before anything is launched
    from adaface_amd import _lib
    i = inputs["b1_16x16"]
    eng.set_pag(())
    eng.set_context(i["ctx3"].to(gpu), 3, layerwise=True)
    _lib.plan_counts(reset=True)
    with pytest.raises(AfError, match=r"rc=-4.*no site set"):
        eng.unet_forward_pag(i["x"].to(gpu), i["t"].to(gpu))
    out = torch.empty(4, 4, 16, 16, device=gpu)
    x4 = torch.cat([i["x"]] * 4).to(gpu)
    t4 = torch.cat([i["t"]] * 4).to(gpu)
    with pytest.raises(AfError, match=r"rc=-1.*multiple of 3"):
        check(eng._lib.af_unet_forward_pag(eng._h, _lib.ptr(x4), _lib.ptr(t4), _lib.ptr(out), 4, 16, 16, _lib.stream_ptr()), "af_unet_forward_pag")
    assert not any(_lib.plan_counts(reset=True).values())


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype,sites", MODEL_CASES)
def test_model_matches_the_reference(gpu, report, engines, inputs, tiny_sd, dtype, sites, form):
    from adaface_amd import _lib
    eng = engines(dtype)
    B = inputs[form]["B"]
    ref = _reference(tiny_sd, inputs, form, sites)
    # the condition on the inputs: the reference tells PAG from no PAG by more than five bars, and legs 0-1 are the plain oracle's
    dev = _rel(ref[2 * B:], ref[:B])
    assert dev >= 5 * TOL[dtype], (dev, TOL[dtype])
    assert torch.equal(ref[:2 * B], _reference(tiny_sd, inputs, form, None)[:2 * B])
    try:
        eng.set_pag(SITE_SETS[sites])
        fwd = _pag_forward(eng, inputs, form, gpu)
        got = fwd()
        assert torch.equal(fwd(), got)                                            # the same bits twice
        errs = [_rel(got[l * B:(l + 1) * B], ref[l * B:(l + 1) * B]) for l in range(3)]
        _lib.set_knob("pag_share_prefix", 0)
        full = fwd()
        _lib.reset_knobs()
        errs_full = [_rel(full[l * B:(l + 1) * B], ref[l * B:(l + 1) * B]) for l in range(3)]
        share = _rel(got, full)
        twin = _twin_forward(eng, inputs, form, gpu)
        e_twin = _rel(got[:2 * B], twin)
        print(f"tiny pag {sites} {form} [{dtype}]: legs vs reference {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e} (three full legs: "
              f"{errs_full[0]:.3e} {errs_full[1]:.3e} {errs_full[2]:.3e}); shared vs full {share:.3e}; legs 0-1 vs twin {e_twin:.3e}; "
              f"reference leg 2 vs leg 0 {dev:.3e}; bar {TOL[dtype]:.2e}")
        for l in range(3):
            report(f"tiny pag {sites} {form}: leg {l} eps vs perturbed oracle [{dtype}]", errs[l], 1.0, TOL[dtype])
        report(f"tiny pag {sites} {form}: shared prefix vs three full legs [{dtype}]", share, 1.0, TOL[dtype])
        assert max(errs) < TOL[dtype] and max(errs_full) < TOL[dtype], (errs, errs_full)
        assert share < TOL[dtype] and e_twin < TOL[dtype], (share, e_twin)
    finally:
        _lib.reset_knobs()
        eng.set_pag(())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_leg_identity_on_one_token(gpu, engines, dtype):
    """An 8 x 8 latent has one token at the middle block: the identity map IS its attention, so leg 2 must be leg 0 (same
    context, same copy source) while leg 1 (another context) is far from it."""
    eng = engines(dtype)
    g = torch.Generator().manual_seed(77)
    x, t = torch.randn(1, 4, 8, 8, generator=g).to(gpu), torch.tensor([500]).to(gpu)
    c, uc = (torch.randn(16, 77, CFG.context_dim, generator=g) for _ in range(2))
    try:
        eng.set_pag(("mid",))
        eng.set_context(torch.cat([c, uc, c]).to(gpu), 3, layerwise=True)
        e = eng.unet_forward_pag(x, t)
        d20, d10 = _rel(e[2:3], e[0:1]), _rel(e[1:2], e[0:1])
        print(f"leg identity [{dtype}]: leg 2 vs leg 0 {d20:.3e}, leg 1 vs leg 0 {d10:.3e}")
        assert d20 < TOL[dtype] and d10 > 5 * TOL[dtype], (d20, d10)
    finally:
        eng.set_pag(())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_off_is_off(gpu, tiny_sd, inputs, dtype):
    """A fresh engine, set_pag(()), set_pag(("mid",)) then set_pag(()), and sites set without the PAG forward: the plain, twin and
    cached forwards return the same bits and count the same launches."""
    from adaface_amd import _lib
    from adaface_amd.engine import Engine
    eng = Engine(dtype=dtype, unet=_unet_kwargs(CFG), vae=None)
    assert eng.load_state_dict(tiny_sd) == []
    i = inputs["b2_32x16"]
    x, t = i["x"].to(gpu), i["t"].to(gpu)

    def run():
        outs, counts = [], []
        eng.set_context(i["ctx2"][:2 * 16].to(gpu), 2, layerwise=True)
        _lib.plan_counts(reset=True)
        outs.append(eng.unet_forward(x, t))
        counts.append(_lib.plan_counts(reset=True))
        outs.append(eng.unet_forward_cached(x, t, depth=2, mode="refresh"))
        outs.append(eng.unet_forward_cached(x, t, depth=2, mode="reuse"))
        counts.append(_lib.plan_counts(reset=True))
        eng.set_context(i["ctx2"].to(gpu), 4, layerwise=True)
        outs.append(eng.unet_forward_twin(x, t))
        counts.append(_lib.plan_counts(reset=True))
        outs.append(eng.unet_forward_cached(x, t, depth=3, mode="refresh", twin=True))
        outs.append(eng.unet_forward_cached(x, t, depth=3, mode="reuse", twin=True))
        counts.append(_lib.plan_counts(reset=True))
        return outs, counts

    run()                                                        # (one-time work of a handle's first forwards)
    base, base_counts = run()
    for setting in ((), ("mid",), (), ("mid", "up.blocks.1"), ("down.blocks.0",)):
        eng.set_pag(setting)
        outs, counts = run()
        assert all(torch.equal(a, b) for a, b in zip(outs, base)), setting
        assert counts == base_counts, setting
    eng.close()


@pytest.mark.parametrize("sites", ["mid", "down2"])
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cached_forwards_keep_their_promises(gpu, engines, inputs, dtype, depth, sites):
    from adaface_amd._lib import AfError
    eng = engines(dtype)
    try:
        for form in FORMS:
            eng.set_pag(SITE_SETS[sites])
            full = _pag_forward(eng, inputs, form, gpu)()
            x, t = inputs[form]["x"].to(gpu), inputs[form]["t"].to(gpu)
            assert torch.equal(eng.unet_forward_cached(x, t, depth=depth, mode="refresh", twin="pag"), full)
            assert torch.equal(eng.unet_forward_cached(x, t, depth=depth, mode="reuse", twin="pag"), full)
            assert torch.equal(eng.unet_forward_cached(x, t, depth=depth, mode="reuse", twin="pag"), full)
            eng.set_pag(SITE_SETS[sites])                                     # the same set again keeps the feature
            assert torch.equal(eng.unet_forward_cached(x, t, depth=depth, mode="reuse", twin="pag"), full)
            # a reuse asked in another form than the refresh's is refused (the context would not even match: set one that does)
            with pytest.raises(AfError, match="no kept feature"):
                eng.set_context(inputs[form]["ctx3"].to(gpu), 3 * inputs[form]["B"], layerwise=True)
                eng.unet_forward_cached(torch.cat([x] * 3), torch.cat([t] * 3), depth=depth, mode="reuse", twin=False)
            eng.set_pag(("mid", "up.blocks.1"))                               # a change of the set drops it
            with pytest.raises(AfError, match="no kept feature"):
                eng.unet_forward_cached(x, t, depth=depth, mode="reuse", twin="pag")
    finally:
        eng.set_pag(())


@pytest.mark.parametrize("mode", ["freeu", "fp8", "tome"])
def test_composition(gpu, tiny_sd, inputs, mode):
    """bf16, PAG with FreeU v2, with the fp8 mode and with token merging 0.5 at max_downsample 1: finite, deterministic, and not
    the result with PAG's third leg unperturbed (which is leg 0)."""
    from adaface_amd.engine import Engine
    eng = Engine(dtype="bf16", unet=_unet_kwargs(CFG), vae=None)
    assert eng.load_state_dict(tiny_sd) == []
    if mode == "freeu":
        eng.set_freeu(2, 1.3, 1.4, 0.9, 0.2)
    elif mode == "fp8":
        eng.set_fp8(True)
    else:
        eng.set_tome(0.5, 1)
    for form in FORMS:
        B = inputs[form]["B"]
        for sites in (("mid",), ("mid", "up.blocks.1")):
            eng.set_pag(sites)
            fwd = _pag_forward(eng, inputs, form, gpu)
            on = fwd()
            assert torch.isfinite(on).all() and torch.equal(fwd(), on)
            assert _rel(on[2 * B:], on[:B]) > 1e-3, (mode, form, sites)
    eng.close()


def test_tome_at_a_set_site_is_refused(gpu, tiny_sd, inputs):
    from adaface_amd import _lib
    from adaface_amd.engine import Engine
    eng = Engine(dtype="bf16", unet=_unet_kwargs(CFG), vae=None)
    assert eng.load_state_dict(tiny_sd) == []
    eng.set_tome(0.5, 2)
    eng.set_pag(("down.blocks.1",))
    fwd = _pag_forward(eng, inputs, "b1_16x16", gpu)
    _lib.plan_counts(reset=True)
    with pytest.raises(_lib.AfError, match=r"rc=-4.*merges tokens"):
        fwd()
    assert not any(_lib.plan_counts(reset=True).values())
    eng.set_pag(("mid",))                                                     # with max_downsample <= 2 the middle block never merges
    assert torch.isfinite(fwd()).all()
    eng.close()


def test_sd15_64x64(gpu):
    """SD-1.5 widths, bf16, B = 1 (Bf = 3), 64 x 64, the middle block: finite, the same bits twice, leg 2 differs from leg 0,
    legs 0-1 within the bf16 bar of the twin forward, and off again gives the plain bits."""
    from adaface_amd.engine import Engine
    from adaface_amd.synth import synth_weights_into
    cfg = O.SD15_UNET
    g = torch.Generator().manual_seed(43)
    x = torch.randn(1, 4, 64, 64, generator=g).to(gpu)
    t = torch.randint(0, 1000, (1,), generator=g).to(gpu)
    c, uc = (torch.randn(16, 77, cfg.context_dim, generator=g).to(gpu) for _ in range(2))
    eng = Engine(dtype="bf16", unet=_unet_kwargs(cfg))
    synth_weights_into(eng, O.unet_param_shapes(cfg), seed=42, device=gpu)
    eng.set_context(torch.cat([c, uc]), 2, layerwise=True)
    twin = eng.unet_forward_twin(x, t)
    eng.set_pag(("mid",))
    assert eng.pag_plan() == {"first_block": 12, "two_leg_blocks": 12, "two_leg_blocks_reuse": 0}
    eng.set_context(torch.cat([c, uc, c]), 3, layerwise=True)
    e = eng.unet_forward_pag(x, t)
    assert torch.isfinite(e).all() and torch.equal(eng.unet_forward_pag(x, t), e)
    assert not torch.equal(e[2], e[0])
    d = _rel(e[:2], twin)
    print(f"sd15 pag mid Bf=3 64x64: legs 0-1 vs the twin forward {d:.3e}; leg 2 vs leg 0 {_rel(e[2:], e[:1]):.3e}")
    assert d < TOL["bf16"], d
    eng.set_pag(())
    eng.set_context(torch.cat([c, uc]), 2, layerwise=True)
    assert torch.equal(eng.unet_forward_twin(x, t), twin)
    eng.close()


# ======================================================================================================================
# the modules and the samplers: tiny model, f32
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
def run_inputs(gpu, tiny_model):
    g = torch.Generator().manual_seed(600)
    x_T = torch.randn(1, 4, 16, 16, generator=g).to(gpu)
    c = tiny_model.get_learned_conditioning(torch.randn(16, 77, CFG.context_dim, generator=g).to(gpu))
    uc = tiny_model.get_learned_conditioning(torch.randn(16, 77, CFG.context_dim, generator=g).to(gpu))
    return dict(x_T=x_T, c=c, uc=uc)


def _twin(c, uc):
    return (torch.cat([c[0], uc[0]]), list(c[1]) + list(uc[1]), c[2])


def test_leg_identity_through_the_module(gpu, tiny_model):
    """UNetModel.forward(cfg_pag=True) with subject-token conv attention on the cond sample and compel cfg, 8 x 8 latent, middle
    block only (one token there): leg 2 inherits the weighted context and the subject rows, so it is leg 0; leg 1 is not."""
    g = torch.Generator().manual_seed(78)
    x, t = torch.randn(1, 4, 8, 8, generator=g).to(gpu), torch.tensor([500]).to(gpu)
    emb_c = torch.randn(16, 77, CFG.context_dim, generator=g).to(gpu)
    emb_u = torch.randn(16, 77, CFG.context_dim, generator=g).to(gpu)
    c, uc = tiny_model.get_learned_conditioning(emb_c), tiny_model.get_learned_conditioning(emb_u)
    info = dict(c[2], use_conv_attn_kernel_size=3, placeholder2indices={"z": (torch.tensor([0] * 9), torch.arange(1, 10))},
                apply_compel_cfg_prob=1.0, compel_cfg_weight_level_range=(2.0, 2.0),
                empty_context=torch.randn(77, CFG.context_dim, generator=g).to(gpu))
    twin = (torch.cat([c[0], uc[0]]), list(c[1]) + list(uc[1]), info)
    try:
        tiny_model.set_pag(("mid",))
        e = tiny_model.apply_model_cfg_pag(x, t, twin)
        assert tuple(e.shape) == (3, 4, 8, 8) and torch.equal(tiny_model.apply_model_cfg_pag(x, t, twin), e)
        d20, d10 = _rel(e[2:3], e[0:1]), _rel(e[1:2], e[0:1])
        two = tiny_model.apply_model_cfg_twin(x, t, twin)
        d_twin = _rel(e[:2], two)
        # the same call without the subject rows and without the weighting moves leg 0 -- and leg 2 with it
        plain = tiny_model.apply_model_cfg_pag(x, t, _twin(c, uc))
        moved = _rel(e[0:1], plain[0:1])
        print(f"leg identity through the module: leg 2 vs leg 0 {d20:.3e}, leg 1 vs leg 0 {d10:.3e}, legs 0-1 vs twin {d_twin:.3e}, "
              f"leg 0 with vs without conv attention + compel {moved:.3e}")
        assert d20 < TOL["f32"] and d10 > 5 * TOL["f32"] and d_twin < TOL["f32"], (d20, d10, d_twin)
        assert moved > 5 * TOL["f32"] and _rel(plain[2:3], plain[0:1]) < TOL["f32"], moved
    finally:
        tiny_model.set_pag(())


def _guided(model, x, t, twin, w, s, phi):
    from adaface_amd import ops
    b = x.shape[0]
    e = model.apply_model_cfg_pag(x, t, twin)
    return ops.guidance(e[:b], e[b:2 * b], e[2 * b:], w, s, phi)


def _f32(v):
    import numpy as np
    return float(np.float32(float(v)))


def _hand_ddim(model, i, S, gs, pag, adaptive, phi, log):
    import numpy as np
    from adaface_amd import ops
    from ldm.models.diffusion.ddim import DDIMSampler
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    twin, x = _twin(i["c"], i["uc"]), i["x_T"]
    ts = np.flip(s.ddim_timesteps)
    n = len(ts)
    w, delta = gs[0], (gs[0] - gs[1]) / (n - 1)
    for k, step in enumerate(ts):
        idx = n - k - 1
        t = torch.full((x.shape[0],), int(step), device=x.device, dtype=torch.long)
        s_t = PR.pag_scale_at(int(step), pag, adaptive)
        log.append(s_t)
        e = _guided(model, x, t, twin, w, s_t, phi)
        x, _ = ops.ddim_step(x, e, None, w, _f32(s.ddim_alphas[idx]), _f32(s.ddim_alphas_prev[idx]),
                             _f32(s.ddim_sqrt_one_minus_alphas[idx]), 0.0, None, 1.0)
        w = w - delta
    return x


def _hand_plms(model, i, S, w, pag, adaptive, phi, log):
    import numpy as np
    from adaface_amd import ops
    from ldm.models.diffusion.plms import PLMSSampler
    s = PLMSSampler(model)
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    twin, x = _twin(i["c"], i["uc"]), i["x_T"]
    ts = np.flip(s.ddim_timesteps)
    n = len(ts)
    old = []

    def output(xx, step):
        t = torch.full((xx.shape[0],), int(step), device=xx.device, dtype=torch.long)
        s_t = PR.pag_scale_at(int(step), pag, adaptive)
        log.append(s_t)
        return _guided(model, xx, t, twin, w, s_t, phi)

    for k, step in enumerate(ts):
        idx = n - k - 1
        upd = lambda e: ops.ddim_step(x, e, None, 1.0, _f32(s.ddim_alphas[idx]), _f32(s.ddim_alphas_prev[idx]),
                                      _f32(s.ddim_sqrt_one_minus_alphas[idx]), 0.0, None, 1.0)[0]
        e_t = output(x, step)
        if len(old) == 0:
            e_next = output(upd(e_t), ts[min(k + 1, n - 1)])
            e_p = ops.lincomb([(e_t, 0.5), (e_next, 0.5)])
        elif len(old) == 1:
            e_p = ops.lincomb([(e_t, 3 / 2), (old[-1], -1 / 2)])
        elif len(old) == 2:
            e_p = ops.lincomb([(e_t, 23 / 12), (old[-1], -16 / 12), (old[-2], 5 / 12)])
        else:
            e_p = ops.lincomb([(e_t, 55 / 24), (old[-1], -59 / 24), (old[-2], 37 / 24), (old[-3], -9 / 24)])
        x = upd(e_p)
        old.append(e_t)
        if len(old) >= 4:
            old.pop(0)
    return x


def _hand_dpm(model, i, S, gs, pag, adaptive, phi, log, sde=False, seed=0):
    from adaface_amd import ops
    from adaface_amd.ldm.models.diffusion import dpm_solver as D
    acp = model.alphas_cumprod.detach().double().cpu().numpy()
    table = D.dpmpp_schedule(acp, D.dpmpp_timesteps(acp, S), guidance=gs, sde=sde)
    twin, x = _twin(i["c"], i["uc"]), i["x_T"]
    x0_prev = None
    for k, row in enumerate(table):
        t = torch.full((x.shape[0],), int(row[D.COL_T]), device=x.device, dtype=torch.long)
        s_t = PR.pag_scale_at(int(row[D.COL_T]), pag, adaptive)
        log.append(s_t)
        w = float(row[D.COL_G])
        e = _guided(model, x, t, twin, w, s_t, phi)
        xp = x0_prev if row[D.COL_WPREV] != 0.0 else None
        args = (x, e, None, xp, w, _f32(row[D.COL_ALPHA]), _f32(row[D.COL_SIGMA]), _f32(row[D.COL_CX]), _f32(row[D.COL_CD]))
        if sde:
            x, x0_prev = ops.dpmpp_sde_step(*args, _f32(row[D.COL_CN]), _f32(row[D.COL_WCUR]), _f32(row[D.COL_WPREV]), noise=None,
                                            seed=seed, step=k, sample_ids=None, first_id=0)
        else:
            x, x0_prev = ops.dpmpp_step(*args, _f32(row[D.COL_WCUR]), _f32(row[D.COL_WPREV]))
    return x


def _run_sampler(which, model, i, S, gs, **kw):
    from adaface_amd.noise import PhiloxNoise
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    common = dict(S=S, batch_size=1, shape=[4, 16, 16], conditioning=i["c"], unconditional_conditioning=i["uc"], verbose=False,
                  x_T=i["x_T"], eta=0.0)
    if which == "ddim":
        s = DDIMSampler(model)
        return s, s.sample(guidance_scale=list(gs), **common, **kw)[0]
    if which == "plms":
        s = PLMSSampler(model)
        return s, s.sample(unconditional_guidance_scale=gs[0], **common, **kw)[0]
    s = DPMSolverSampler(model)
    if which == "dpm_sde":
        kw = dict(kw, algorithm="sde-dpmsolver++", noise_source=PhiloxNoise(77))
    return s, s.sample(guidance_scale=list(gs), **common, **kw)[0]


def _hand(which, model, i, S, gs, pag, adaptive, phi, log):
    if which == "ddim":
        return _hand_ddim(model, i, S, gs, pag, adaptive, phi, log)
    if which == "plms":
        return _hand_plms(model, i, S, gs[0], pag, adaptive, phi, log)
    return _hand_dpm(model, i, S, list(gs), pag, adaptive, phi, log, sde=which == "dpm_sde", seed=77)


@pytest.mark.parametrize("which", ["ddim", "plms", "dpm", "dpm_sde"])
def test_samplers_equal_a_hand_written_loop(gpu, tiny_model, run_inputs, which):
    """sample(..., pag_scale=3, guidance_rescale=0.7), S = 4, against the loop above: apply_model_cfg_pag,
    ops.guidance and the sampler's own step op, bit for bit; the PAG scale per call follows pag_scale_at, constant and with a
    pag_adaptive_scale that clamps it to 0 from some step on; and all of it differs from the run without PAG."""
    gs = (10.0, 4.0)
    try:
        tiny_model.set_pag(("mid",))
        for adaptive in (0.0, 0.006):
            s, lat = _run_sampler(which, tiny_model, run_inputs, 4, gs, pag_scale=3.0, pag_adaptive_scale=adaptive, guidance_rescale=0.7)
            log = []
            want = _hand(which, tiny_model, run_inputs, 4, gs, 3.0, adaptive, 0.7, log)
            assert torch.isfinite(lat).all() and torch.equal(lat, want), (which, adaptive, _rel(lat, want))
            assert [e[0] for e in s.guidance_log] == [3] * len(log) and [e[1] for e in s.guidance_log] == log
            if adaptive:
                assert log[0] > 0.0 and log[-1] == 0.0 and 0.0 in log[1:], log      # (t = 1: 3 - 0.006 * 999 < 0)
            else:
                assert log == [3.0] * len(log)
        _, off = _run_sampler(which, tiny_model, run_inputs, 4, gs)
        assert not torch.equal(off, lat)
    finally:
        tiny_model.set_pag(())


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_samplers_with_deep_cache(gpu, tiny_model, run_inputs, which):
    """deep_cache_interval = 2 with PAG: refresh / reuse alternate, every call is a three-leg one, finite and deterministic."""
    try:
        tiny_model.set_pag(("mid",))
        kw = dict(pag_scale=3.0, guidance_rescale=0.7, deep_cache_interval=2, deep_cache_depth=2)
        s, a = _run_sampler(which, tiny_model, run_inputs, 4, (10.0, 4.0), **kw)
        n = len(s.deep_cache_log)
        assert n >= 4 and s.deep_cache_log == ["refresh", "reuse"] * (n // 2) + ["refresh"] * (n % 2)
        assert [e[0] for e in s.guidance_log] == [3] * n
        _, b = _run_sampler(which, tiny_model, run_inputs, 4, (10.0, 4.0), **kw)
        assert torch.isfinite(a).all() and torch.equal(a, b)
        _, full = _run_sampler(which, tiny_model, run_inputs, 4, (10.0, 4.0), pag_scale=3.0, guidance_rescale=0.7)
        assert not torch.equal(a, full) and _rel(a, full) < 0.5
    finally:
        tiny_model.set_pag(())


@pytest.mark.parametrize("which", ["ddim", "plms", "dpm"])
def test_rescale_alone_uses_the_twin_forward(gpu, tiny_model, run_inputs, which):
    """guidance_rescale without PAG: the twin forward, ops.guidance without e_p, the step on the combined eps -- by equality with
    a loop that does exactly that (no PAG layer is even set)."""
    from adaface_amd import ops
    assert tiny_model.pag == ()
    s, lat = _run_sampler(which, tiny_model, run_inputs, 4, (10.0, 4.0), guidance_rescale=0.7)
    assert [e[0] for e in s.guidance_log] == [2] * len(s.guidance_log) and len(s.guidance_log) >= 4
    orig = tiny_model.apply_model_cfg_pag

    def twin_as_pag(x, t, twin, deep_cache=None):       # the hand loops above, fed from the twin forward: e_p := e_c, s = 0
        e = tiny_model.apply_model_cfg_twin(x, t, twin)
        return torch.cat([e, e[:x.shape[0]]])
    object.__setattr__(tiny_model, "apply_model_cfg_pag", twin_as_pag)
    try:
        want = _hand(which, tiny_model, run_inputs, 4, (10.0, 4.0), 0.0, 0.0, 0.7, [])
    finally:
        object.__delattr__(tiny_model, "apply_model_cfg_pag")
    assert tiny_model.apply_model_cfg_pag.__func__ is orig.__func__
    assert torch.equal(lat, want), _rel(lat, want)
    _, off = _run_sampler(which, tiny_model, run_inputs, 4, (10.0, 4.0))
    assert not torch.equal(off, lat)
    # the rescaled run's last prediction has the conditional one's deviation when phi = 1 (one direct check of the operator's use)
    e = torch.randn(1, 4, 16, 16, device=gpu)
    out, f = ops.guidance(e, 0.5 * e, None, 4.0, 0.0, 1.0, return_factor=True)
    assert abs(float(out.std() / e.std()) - 1.0) < 1e-5 and abs(float(f) - 1.0 / 2.5) < 1e-5
