"""GPU tests of DeepCache (af_unet_forward_cached): a refresh is the full forward bit for bit; a reuse step at the refresh's
input repeats it bit for bit and at another input matches the restatement of tests/deep_cache_ref.py driving the CPU oracle;
the kept feature survives other work on the handle; skipped blocks launch nothing; every invalid reuse is refused on the host;
and the DDIM / DPM-Solver++ samplers with deep_cache_interval= follow the same restatement step for step.

Tiny config, synthetic weights seed 11, except one SD-1.5-size case.  Bars: TOL of tests/test_model_gpu.py for a forward
(2e-4 f32, 3e-2 bf16, relative to max|reference|) -- the shallow pass is a sub-computation of that forward -- and 1e-3 for a
tiny f32 trajectory, as the drop-in sampler tests."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import deep_cache_ref as DR  # noqa: E402
import dpmpp_ref as R  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ROOT / "tests" / "golden"
TOL = {"f32": 2e-4, "bf16": 3e-2}      # tests/test_model_gpu.py
CFG = O.TINY_UNET
N_IN = 12
# call forms: name -> (twin, B of x, H, W); Bf = 2 B for the twin
FORMS = {"b3_32x16": (False, 3, 32, 16), "twin1_16x16": (True, 1, 16, 16)}


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


def _launches(reset=True):
    """conv / GEMM launches since the last reset: every launch is under exactly one of these counters (_lib.plan_counts)."""
    from adaface_amd import _lib
    pc = _lib.plan_counts(reset=reset)
    return sum(pc[f"tile{i}"] for i in range(6)) + pc["halo"] + pc["fp8"] + pc["up_phase4"]


@pytest.fixture(scope="module")
def tiny_sd():
    return O.synth_state_dict(O.unet_param_shapes(CFG), seed=11)


@pytest.fixture(scope="module")
def inputs():
    """Per call form: (x1, t1) of the refresh, (x2, t2) = x1 + 0.05 noise at other timesteps, the context of the Bf samples."""
    out = {}
    for n, (name, (twin, B, H, W)) in enumerate(FORMS.items()):
        g = torch.Generator().manual_seed(100 + n)
        Bf = 2 * B if twin else B
        x1 = torch.randn(B, 4, H, W, generator=g)
        out[name] = dict(x1=x1, t1=torch.tensor([981, 500, 1][:B]), x2=x1 + 0.05 * torch.randn(B, 4, H, W, generator=g),
                         t2=torch.tensor([947, 466, 34][:B]), ctx=torch.randn(Bf * 16, 77, CFG.context_dim, generator=g), Bf=Bf)
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


_oracle_cache = {}


def _oracle(tiny_sd, inputs, form, k):
    """(eps of the full forward at (x1, t1), eps and last-block tap of the shallow forward at (x2, t2) from the oracle's own D),
    computed once per (form, k)."""
    if (form, k) not in _oracle_cache:
        twin = FORMS[form][0]
        i = inputs[form]
        rep = (lambda v: torch.cat([v, v])) if twin else (lambda v: v)
        taps = {}
        with torch.no_grad():
            full, D = DR.full_forward(tiny_sd, CFG, rep(i["x1"]), rep(i["t1"]), i["ctx"], k)
            shallow = DR.shallow_forward(tiny_sd, CFG, rep(i["x2"]), rep(i["t2"]), i["ctx"], D, k, taps=taps)
        _oracle_cache[form, k] = (full, shallow, taps[f"output_blocks.{N_IN - 1}"])
    return _oracle_cache[form, k]


def _set(eng, inputs, form, gpu):
    i = inputs[form]
    eng.set_context(i["ctx"].to(gpu), i["Bf"], layerwise=True)
    return FORMS[form][0], {k: i[k].to(gpu) for k in ("x1", "t1", "x2", "t2")}


# ======================================================================================================================
# the entry point
# ======================================================================================================================
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_refresh_is_the_full_forward_and_reuse_repeats_it(gpu, report, engines, inputs, tiny_sd, dtype, k, form):
    """Checks 1-3: refresh == unet_forward / unet_forward_twin bit for bit; reuse at the same (x, t) == the same bits, twice,
    and again after a forward of another shape and a refresh-free full forward ran on the handle (the kept feature is neither
    consumed nor in the arena); reuse at (x2, t2) against the restatement fed the oracle's own D, under the full forward's bar."""
    eng = engines(dtype)
    twin, v = _set(eng, inputs, form, gpu)
    plain = (eng.unet_forward_twin if twin else eng.unet_forward)(v["x1"], v["t1"])
    fresh = eng.unet_forward_cached(v["x1"], v["t1"], depth=k, mode="refresh", twin=twin)
    assert torch.equal(fresh, plain)
    again = eng.unet_forward_cached(v["x1"], v["t1"], depth=k, mode="reuse", twin=twin)
    assert torch.equal(again, plain)
    assert torch.equal(eng.unet_forward_cached(v["x1"], v["t1"], depth=k, mode="reuse", twin=twin), plain)
    # other work on the handle: a forward of another shape and batch (the arena is re-planned from offset 0, and grows)
    other = "twin1_16x16" if form == "b3_32x16" else "b3_32x16"
    o_twin, ov = _set(eng, inputs, other, gpu)
    (eng.unet_forward_twin if o_twin else eng.unet_forward)(ov["x2"], ov["t2"])
    _set(eng, inputs, form, gpu)                   # (set_context does not drop the kept feature)
    (eng.unet_forward_twin if twin else eng.unet_forward)(v["x2"], v["t2"])
    assert torch.equal(eng.unet_forward_cached(v["x1"], v["t1"], depth=k, mode="reuse", twin=twin), plain)
    # another input
    ref_full, ref_shallow, _ = _oracle(tiny_sd, inputs, form, k)
    got = eng.unet_forward_cached(v["x2"], v["t2"], depth=k, mode="reuse", twin=twin)
    e_full, e_reuse = _rel(plain, ref_full), _rel(got, ref_shallow)
    report(f"tiny deep_cache k={k} {form}: refresh vs oracle full forward [{dtype}]", e_full, 1.0, TOL[dtype])
    report(f"tiny deep_cache k={k} {form}: reuse at (x2, t2) vs shallow reference [{dtype}]", e_reuse, 1.0, TOL[dtype])
    assert e_full < TOL[dtype], e_full
    assert e_reuse < TOL[dtype], e_reuse
    assert not torch.equal(got, plain)


@pytest.mark.parametrize("k", [1, 3])
def test_kept_feature_survives_a_vae_decode(gpu, tiny_sd, inputs, k):
    """One handle with the U-Net and the VAE decoder (they share the arena): a decode between the refresh and the reuse."""
    from adaface_amd.engine import Engine
    vcfg = O.TINY_VAE
    eng = Engine(dtype="f32", unet=_unet_kwargs(CFG),
                 vae=dict(ch=vcfg.ch, out_ch=vcfg.out_ch, ch_mult=vcfg.ch_mult, num_res_blocks=vcfg.num_res_blocks,
                          z_channels=vcfg.z_channels, embed_dim=vcfg.embed_dim))
    sd = dict(tiny_sd)
    sd.update(O.synth_state_dict(O.vae_param_shapes(vcfg), seed=12))
    assert eng.load_state_dict(sd) == []
    twin, v = _set(eng, inputs, "twin1_16x16", gpu)
    want = eng.unet_forward_cached(v["x1"], v["t1"], depth=k, mode="refresh", twin=twin)
    img = eng.vae_decode(torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(1)).to(gpu))
    assert torch.isfinite(img).all()
    assert torch.equal(eng.unet_forward_cached(v["x1"], v["t1"], depth=k, mode="reuse", twin=twin), want)
    eng.close()


def test_reuse_tap_writes_only_blocks_that_ran(gpu, report, engines, inputs, tiny_sd):
    """f32, k = 2: the tap on output_blocks[n_out - 1] in reuse mode against the reference's; a tap on the middle block, which
    a reuse step skips, leaves its buffer untouched."""
    from adaface_amd._lib import check, ptr
    eng = engines("f32")
    form, k = "b3_32x16", 2
    twin, v = _set(eng, inputs, form, gpu)
    _, _, ref_tap = _oracle(tiny_sd, inputs, form, k)
    eng.unet_forward_cached(v["x1"], v["t1"], depth=k, mode="refresh", twin=twin)
    c, hh, ww = C.c_int(), C.c_int(), C.c_int()
    last, middle = N_IN + 1 + N_IN - 1, N_IN
    try:
        check(eng._lib.af_unet_block_shape(eng._h, last, 32, 16, C.byref(c), C.byref(hh), C.byref(ww)), "af_unet_block_shape")
        buf = torch.full((3, c.value, hh.value, ww.value), -7.5, device=gpu)
        assert tuple(buf.shape) == tuple(ref_tap.shape)
        check(eng._lib.af_unet_set_tap(eng._h, last, ptr(buf)), "af_unet_set_tap")
        eng.unet_forward_cached(v["x2"], v["t2"], depth=k, mode="reuse", twin=twin)
        err = _rel(buf, ref_tap)
        report(f"tiny deep_cache k={k} {form}: reuse tap output_blocks.{N_IN - 1} vs shallow reference [f32]", err, 1.0, TOL["f32"])
        assert err < TOL["f32"], err
        check(eng._lib.af_unet_block_shape(eng._h, middle, 32, 16, C.byref(c), C.byref(hh), C.byref(ww)), "af_unet_block_shape")
        skipped = torch.full((3, c.value, hh.value, ww.value), -7.5, device=gpu)
        check(eng._lib.af_unet_set_tap(eng._h, middle, ptr(skipped)), "af_unet_set_tap")
        eng.unet_forward_cached(v["x2"], v["t2"], depth=k, mode="reuse", twin=twin)
        assert (skipped == -7.5).all()
        eng.unet_forward_cached(v["x2"], v["t2"], depth=k, mode="refresh", twin=twin)       # (a refresh runs it)
        assert (skipped != -7.5).any()
    finally:
        eng._lib.af_unet_set_tap(eng._h, -1, None)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reuse_skips_work(gpu, engines, inputs, dtype):
    """Conv / GEMM launches of one forward: reuse(k=1) < reuse(k=2) < reuse(k=3) < refresh == the plain full forward."""
    eng = engines(dtype)
    twin, v = _set(eng, inputs, "twin1_16x16", gpu)
    _launches()
    eng.unet_forward_twin(v["x1"], v["t1"])
    n_plain = _launches()
    n_refresh, n_reuse = {}, {}
    for k in (1, 2, 3):
        eng.unet_forward_cached(v["x1"], v["t1"], depth=k, mode="refresh", twin=twin)
        n_refresh[k] = _launches()
        eng.unet_forward_cached(v["x2"], v["t2"], depth=k, mode="reuse", twin=twin)
        n_reuse[k] = _launches()
    print(f"conv/GEMM launches [{dtype}]: plain {n_plain}, refresh {n_refresh}, reuse {n_reuse}")
    assert n_plain > 0 and all(n == n_plain for n in n_refresh.values()), (n_plain, n_refresh)
    assert 0 < n_reuse[1] < n_reuse[2] < n_reuse[3] < n_plain, (n_reuse, n_plain)


def test_refusals(gpu, tiny_sd, inputs):
    """Every reuse without a kept feature for exactly its arguments raises AfError on the host; so does a depth outside
    1 .. n_in - 1.  After each refusal a refresh + reuse still works."""
    from adaface_amd._lib import AfError
    from adaface_amd.engine import Engine
    eng = Engine(dtype="f32", unet=_unet_kwargs(CFG))
    assert eng.load_state_dict(tiny_sd) == []
    i3, i1 = inputs["b3_32x16"], inputs["twin1_16x16"]
    x3, t3 = i3["x1"].to(gpu), i3["t1"].to(gpu)
    x1, t1 = i1["x1"].to(gpu), i1["t1"].to(gpu)
    ctx3, ctx2 = i3["ctx"].to(gpu), i1["ctx"].to(gpu)
    fwd = eng.unet_forward_cached

    def refused(*a, **kw):
        with pytest.raises(AfError, match="no kept feature"):
            fwd(*a, mode="reuse", **kw)

    eng.set_context(ctx3, 3, layerwise=True)
    refused(x3, t3, depth=2)                                            # before any refresh
    want = fwd(x3, t3, depth=2, mode="refresh")
    assert torch.equal(fwd(x3, t3, depth=2, mode="reuse"), want)
    refused(x3, t3, depth=3)                                            # another depth
    refused(x3[:, :, :16], t3, depth=2)                                 # another H x W
    eng.set_context(ctx2, 2, layerwise=True)
    refused(x3[:2], t3[:2], depth=2)                                    # another Bf
    want2 = fwd(x3[:2], t3[:2], depth=2, mode="refresh")
    refused(x1, t1, depth=2, twin=True)                                 # the same Bf = 2, H x W differs and twin differs
    refused(x3[:1], t3[:1], depth=2, twin=True)                         # the same Bf, H x W: only twin differs
    assert torch.equal(fwd(x3[:2], t3[:2], depth=2, mode="reuse"), want2)
    name = "model.diffusion_model.out.2.bias"
    eng.load_tensor(name, tiny_sd[name])
    refused(x3[:2], t3[:2], depth=2)                                    # after load_tensor
    fwd(x3[:2], t3[:2], depth=2, mode="refresh")
    eng.unet_cache_invalidate()
    refused(x3[:2], t3[:2], depth=2)                                    # after unet_cache_invalidate
    for depth in (0, N_IN, -1):
        for mode in ("refresh", "reuse"):
            with pytest.raises(AfError, match="depth"):
                fwd(x3[:2], t3[:2], depth=depth, mode=mode)
    with pytest.raises(ValueError):
        fwd(x3[:2], t3[:2], depth=2, mode="keep")
    assert torch.equal(fwd(x3[:2], t3[:2], depth=N_IN - 1, mode="refresh"), want2)
    assert torch.equal(fwd(x3[:2], t3[:2], depth=N_IN - 1, mode="reuse"), want2)
    torch.cuda.synchronize()
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_layerwise_context_and_conv_attention_keep_their_layer(gpu, report, engines, dtype):
    """Subject-token conv attention (ks = 3) on the golden's inputs, k = 2: the transformers that run are CA layers 0, 14, 15
    -- renumbered 0, 1, 2 they would read other context slices.  Reuse at the same input == the full forward bit for bit, which
    itself matches the reference golden."""
    from adaface_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    tiny = dict(np.load(GOLD / "golden_tiny.npz"))
    eng = engines(dtype)
    x, t, ctx = (torch.tensor(tiny[n], device=gpu) for n in ("tiny_x", "tiny_t", "tiny_ctx"))
    spec = UNetModel._conv_attn_spec(3, {"z": (torch.tensor(tiny["tiny_convattn_idx_b"]), torch.tensor(tiny["tiny_convattn_idx_n"]))})
    try:
        eng.set_conv_attn(*spec)
        eng.set_context(ctx, x.shape[0], layerwise=True)
        plain = eng.unet_forward(x, t)
        err = _rel(plain, torch.tensor(tiny["tiny_convattn_eps"]))
        report(f"tiny deep_cache: conv-attention full forward vs reference golden [{dtype}]", err, 1.0, TOL[dtype])
        assert err < TOL[dtype], err
        assert torch.equal(eng.unet_forward_cached(x, t, depth=2, mode="refresh"), plain)
        assert torch.equal(eng.unet_forward_cached(x, t, depth=2, mode="reuse"), plain)
    finally:
        eng.set_conv_attn(0)


# ======================================================================================================================
# samplers, tiny model in f32 mode (the fixtures of tests/test_dpm_solver_gpu.py)
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
def tiny_inputs():
    g = dict(np.load(GOLD / "golden_tiny.npz"))
    gen = torch.Generator().manual_seed(21)
    return dict(x_T=torch.tensor(g["ddim_xT"]), c=torch.tensor(g["ddim_c"]), uc=torch.tensor(g["ddim_uc"]),
                mask=torch.tensor(g["inpaint_mask"]), x0=torch.tensor(g["inpaint_x0"]),
                q_noise=[torch.randn(g["ddim_xT"].shape, generator=gen) for _ in range(10)])


def _conds(model, inputs, gpu):
    return (model.get_learned_conditioning(inputs["c"].to(gpu)), model.get_learned_conditioning(inputs["uc"].to(gpu)))


def _samplers():
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    return {"ddim": DDIMSampler, "dpm": DPMSolverSampler}


class _ReplayedQNoise:
    """model.q_sample with the inpainting blend's noise replaced by the recorded draws, in order"""

    def __init__(self, model, noises):
        self.model, self.noises, self.n = model, noises, 0

    def __enter__(self):
        orig = self.model.q_sample

        def q_sample(x_start, t, noise=None):
            self.n += 1
            return orig(x_start, t, noise=self.noises[self.n - 1])
        object.__setattr__(self.model, "q_sample", q_sample)
        return self

    def __exit__(self, *exc):
        object.__delattr__(self.model, "q_sample")


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_interval_one_is_off(gpu, tiny_model, tiny_inputs, which):
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    kw = dict(S=6, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=[10.0, 4.0],
              unconditional_conditioning=uc, x_T=tiny_inputs["x_T"].to(gpu), eta=0.0)
    lats = []
    for interval in (None, 1):
        s = _samplers()[which](tiny_model)
        lats.append(s.sample(deep_cache_interval=interval, deep_cache_depth=2, **kw)[0].clone())
        assert s.deep_cache_log == ["full"] * 7
    assert torch.equal(lats[0], lats[1])
    s = _samplers()[which](tiny_model)
    on = s.sample(deep_cache_interval=3, **kw)[0]
    assert s.deep_cache_log.count("reuse") == 4 and not torch.equal(on, lats[0])     # (and a real interval is not off)


@pytest.mark.parametrize("inpaint", [False, True])
def test_ddim_sampler_matches_the_oracle(gpu, report, tiny_model, tiny_inputs, tiny_sd, inpaint):
    """S = 6 (7 steps), interval 3, depth 2, guidance [10, 4]: O.ddim_sample driven by the stateful reference callable."""
    i = tiny_inputs
    apply = DR.CachedApplyModel(tiny_sd, CFG, [True, False, False, True, False, False, True], 2)
    kw_ref = dict(mask=i["mask"], x0=i["x0"], q_noise=i["q_noise"]) if inpaint else {}
    with torch.no_grad():
        ref = O.ddim_sample(apply, O.register_schedule(), 6, i["x_T"], i["c"], i["uc"], (10.0, 4.0), **kw_ref)
    want_log = ["refresh", "reuse", "reuse", "refresh", "reuse", "reuse", "refresh"]
    assert apply.log == want_log
    c, uc = _conds(tiny_model, i, gpu)
    kw = dict(mask=i["mask"].to(gpu), x0=i["x0"].to(gpu)) if inpaint else {}
    s = _samplers()["ddim"](tiny_model)
    with _ReplayedQNoise(tiny_model, [t.to(gpu) for t in i["q_noise"]]) as q:
        lat, _ = s.sample(S=6, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=[10.0, 4.0],
                          unconditional_conditioning=uc, x_T=i["x_T"].to(gpu), eta=0.0, deep_cache_interval=3,
                          deep_cache_depth=2, **kw)
    assert q.n == (7 if inpaint else 0)
    err = _rel(lat, ref)
    report(f"dropin DDIMSampler S=6 deep_cache N=3 k=2{' + mask/x0 blend' if inpaint else ''} vs reference on the oracle [f32]",
           err, float(ref.abs().max()), 1e-3)
    assert err < 1e-3, err
    assert s.deep_cache_log == want_log


def test_dpm_solver_sampler_matches_the_oracle(gpu, report, tiny_model, tiny_inputs, tiny_sd):
    """The uniform6 grid of tests/test_dpm_solver_gpu.py (7 steps, mask / x0 blend, guidance [10, 4]) with interval 2, depth 3,
    against dpmpp_ref.sample_ref with the stateful reference callable, under that file's 1e-3."""
    from adaface_amd.ldm.models.diffusion.deep_cache import refresh_steps
    i = tiny_inputs
    ts = R.uniform_grid(6)
    apply = DR.CachedApplyModel(tiny_sd, CFG, refresh_steps(len(ts), 2), 3)
    with torch.no_grad():
        ref, _ = R.sample_ref(apply, R.sd_acp(), ts, i["x_T"], i["c"], i["uc"], O.guidance_schedule((10.0, 4.0), len(ts)),
                              mask=i["mask"], x0=i["x0"], q_noise=i["q_noise"])
    c, uc = _conds(tiny_model, i, gpu)
    s = _samplers()["dpm"](tiny_model)
    with _ReplayedQNoise(tiny_model, [t.to(gpu) for t in i["q_noise"]]):
        lat, _ = s.sample(S=6, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=[10.0, 4.0],
                          unconditional_conditioning=uc, x_T=i["x_T"].to(gpu), eta=0.0, mask=i["mask"].to(gpu),
                          x0=i["x0"].to(gpu), deep_cache_interval=2, deep_cache_depth=3)
    err = _rel(lat, ref)
    report("dropin DPMSolverSampler uniform6 deep_cache N=2 k=3 vs restatement on the oracle [f32]", err, float(ref.abs().max()), 1e-3)
    assert err < 1e-3, err
    assert s.deep_cache_log == apply.log == ["refresh", "reuse", "refresh", "reuse", "refresh", "reuse", "refresh"]


@pytest.mark.parametrize("which", ["ddim", "dpm"])
def test_call_form_change_forces_a_refresh(gpu, tiny_model, tiny_inputs, which):
    """Guidance [3, 1] reaches exactly 1 at the last of the 7 steps: the sampler drops to the single-batch call, for which
    nothing is kept -- with an interval larger than the run that step is a refresh, not a reuse, and nothing raises."""
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    s = _samplers()[which](tiny_model)
    lat, _ = s.sample(S=6, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=[3.0, 1.0],
                      unconditional_conditioning=uc, x_T=tiny_inputs["x_T"].to(gpu), eta=0.0, deep_cache_interval=100,
                      deep_cache_depth=2)
    assert torch.isfinite(lat).all()
    assert s.deep_cache_log == ["refresh"] + ["reuse"] * 5 + ["refresh"]


def test_ddim_decode_takes_the_interval(gpu, tiny_model, tiny_inputs):
    """DDIMSampler.decode (the img2img tail, guidance annealed 4 -> 2): interval 1 is the uncached run bit for bit, interval 2
    alternates, and its first reuse step -- the same call the sampling loop makes -- changes the result."""
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    s = _samplers()["ddim"](tiny_model)
    s.make_schedule(ddim_num_steps=6, ddim_eta=0.0, verbose=False)
    x = tiny_inputs["x_T"].to(gpu)
    kw = dict(guidance_scale=4.0, unconditional_conditioning=uc)
    plain = s.decode(x, c, 4, **kw).clone()
    assert s.deep_cache_log == ["full"] * 4
    assert torch.equal(s.decode(x, c, 4, deep_cache_interval=1, **kw), plain)
    cached = s.decode(x, c, 4, deep_cache_interval=2, deep_cache_depth=3, **kw)
    assert s.deep_cache_log == ["refresh", "reuse", "refresh", "reuse"]
    assert torch.isfinite(cached).all() and not torch.equal(cached, plain)


def test_plms_refuses(gpu, tiny_model, tiny_inputs):
    from ldm.models.diffusion.plms import PLMSSampler
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    kw = dict(S=6, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, unconditional_guidance_scale=3.0,
              unconditional_conditioning=uc, x_T=tiny_inputs["x_T"].to(gpu))
    with pytest.raises(NotImplementedError):
        PLMSSampler(tiny_model).sample(deep_cache_interval=3, **kw)
    a = PLMSSampler(tiny_model).sample(deep_cache_interval=1, **kw)[0]
    assert torch.equal(a, PLMSSampler(tiny_model).sample(**kw)[0])


# ======================================================================================================================
# SD-1.5 size: the large-shape kernels (LDS-halo 3x3, row-panel GEMMs, the one-launch cross-attention layer at 64 x 64) on the
# relocated concatenation buffer
# ======================================================================================================================
def test_sd15_twin_refresh_and_reuse_are_the_full_forward(gpu):
    from adaface_amd import _lib
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
    assert torch.isfinite(plain).all()
    _lib.plan_counts(reset=True)
    assert torch.equal(eng.unet_forward_cached(x, t, depth=2, mode="refresh", twin=True), plain)
    _lib.plan_counts(reset=True)
    again = eng.unet_forward_cached(x, t, depth=2, mode="reuse", twin=True)
    pc = _lib.plan_counts(reset=True)
    print("sd15 twin Bf=2 64x64 reuse k=2 plan counts", pc)
    assert torch.equal(again, plain)
    assert torch.equal(eng.unet_forward_cached(x, t, depth=2, mode="reuse", twin=True), plain)
    eng.close()
