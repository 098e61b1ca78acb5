"""GPU tests of regional prompts (af_set_regions, af_region_attn.hip): the weights kernel against the float64 restatement of
adaface_amd/regions.py; the operator on the fused kernel and on the composition against float64 on the storage-rounded operands
(tests/region_ref.py), its structure (bit-exact), the selection rule under NaN and the segment tail; the model on TINY_UNET
against the patched CPU oracle; the DDIM sampler through LatentDiffusion.set_regions.

Bars: the attention operator's (1.5e-2 bf16, 1.5e-2 / 8 f16, 2e-4 f32 of max|ref| -- the output is a convex combination of
attention outputs, so no wider bar is needed) and the model's (2e-4 f32, 3e-2 bf16, 3.75e-3 f16)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import region_cases as RC  # noqa: E402
import region_ref as RR  # noqa: E402
from adaface_amd import regions as RG  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ROOT / "tests" / "golden"
CFG = O.TINY_UNET
N_SITES = 16


def _rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if not torch.isfinite(got).all():
        return float("inf")
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def _bits(t):
    return t.contiguous().view(torch.uint8)


# ======================================================================================================================
# 1. the weights kernel
# ======================================================================================================================
@pytest.mark.parametrize("kind", ["binary", "random"])
def test_weights_kernel(gpu, report, kind):
    """Bf in {1, 3} x R in {1, 3, 8} x maps 8 x 8, 16 x 24, 64 x 64.  Binary masks: box sums, the scale and the region sum are
    exact in fp32, so the result is within 1 ulp of fp32(a / s) computed in float64.  Random masks: within 160 2^-24 relative
    (63 additions each for the numerator and denominator box sums, 7 for the region sum, the scale and the division).  The
    8 x 8 cell without any weight gives (1, 0, ..) exactly at every level; the active bits are those of the restatement; a
    second run gives the same bits."""
    from adaface_amd import ops
    worst = 0.0
    for Bf in RC.W_BATCHES:
        for R in RC.W_REGIONS:
            for H, W in RC.W_MAPS:
                m = RC.weight_maps(Bf, R, H, W, kind, seed=Bf * 100 + R * 10 + H)
                ref = RG.pyramid(m)
                levels, words = ops.region_weights(m.to(gpu))
                levels2, words2 = ops.region_weights(m.to(gpu))
                for l in range(4):
                    got, want = levels[l].cpu(), ref[l]
                    tag = (kind, Bf, R, H, W, l)
                    assert tuple(got.shape) == tuple(want.shape) and torch.isfinite(got).all(), tag
                    zero = want == 0
                    assert bool((got[zero] == 0).all()), tag
                    if kind == "binary":
                        w32 = want.float()
                        ulp = (torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).double()
                        err = ((got.double() - w32.double()).abs() / ulp)[~zero]
                        bound = 1.0
                    else:
                        err = ((got.double() - want).abs() / want.abs().clamp_min(1e-300))[~zero] / RC.W_REL_BOUND
                        bound = 1.0
                    if err.numel():
                        worst = max(worst, float(err.max()))
                        assert float(err.max()) <= bound, (tag, float(err.max()))
                    c = 8 >> l            # the cell without weight
                    assert bool((got[:, 0, :c, :c] == 1).all()) and bool((got[:, 1:, :c, :c] == 0).all()), tag
                    assert torch.equal(words[l].cpu(), RG.active_pairs(want)), tag
                    assert torch.equal(_bits(levels2[l]), _bits(levels[l])) and torch.equal(words2[l], words[l]), tag
    report(f"af_op_region_weights [{kind}]: worst error / bound ({'1 ulp' if kind == 'binary' else '160 2^-24 relative'})", worst, 1.0, 1.0)


def test_weights_kernel_refuses(gpu):
    from adaface_amd import ops
    from adaface_amd._lib import AfError
    for shape in ((1, 9, 8, 8), (1, 2, 8, 12), (1, 2, 4, 8)):
        with pytest.raises(AfError):
            ops.region_weights(torch.ones(*shape, device=gpu))


# ======================================================================================================================
# 2. the operator
# ======================================================================================================================
def _run(case, dtype, path, gpu, q, k, v, w):
    from adaface_amd import ops
    dh, T, R, Nq, heads, B, slack = case
    o = ops.region_attention(q.to(gpu), k.to(gpu), v.to(gpu), w.to(gpu), heads, R, dtype=dtype, path=path, ld_slack=slack).cpu()
    C = heads * dh
    if slack:
        assert torch.isnan(o[..., C:]).all(), (case, dtype, path, "slack columns were written")
    return o[..., :C]


def _check_case(case, dtype, path, gpu, seed):
    q, k, v, w = RC.op_inputs(case, seed)
    _, _, R, _, heads, _, _ = case
    ref = RR.region_attention(RC.storage_round(q, dtype), RC.storage_round(k, dtype), RC.storage_round(v, dtype), w, heads, R)
    got = _run(case, dtype, path, gpu, q, k, v, w)
    assert torch.isfinite(got).all(), (case, dtype, path)       # (every staged buffer ends in NaN rows: none was read)
    return _rel(got, ref)


@pytest.mark.parametrize("path", ["fused", "composition"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_operator_against_float64(gpu, report, dtype, path):
    """Every case of region_cases.OP_CASES (dh 32 .. 160, T 1 .. 96, R 1 .. 8, Nq 1 .. 257, heads 1 .. 8, B 1 / 3, ld_slack
    0 / 8), staged behind NaN slack columns and 128 NaN tail rows, against float64 on the storage-rounded operands."""
    worst = 0.0
    for i, case in enumerate(RC.OP_CASES):
        err = _check_case(case, dtype, path, gpu, i)
        print(f"region_attention {path} [{dtype}] case {case}: {err:.3e}")
        worst = max(worst, err)
        assert err < RC.OP_TOL[dtype], (case, dtype, path, err)
    report(f"af_op_region_attention {path}: worst of {len(RC.OP_CASES)} cases vs float64 [{dtype}]", worst, 1.0, RC.OP_TOL[dtype])


def test_operator_composition_only_cases(gpu, report):
    """f32 storage and T = 154 (more keys per segment than the fused kernel holds): the planner sends them to the composition,
    and the fused path refuses them."""
    from adaface_amd import ops
    from adaface_amd._lib import AfError
    for i, (dtype, case) in enumerate(RC.COMPOSE_ONLY_CASES):
        assert RG.plan_query(dtype, case[0], case[1], case[2]) == "composition"
        for path in ("auto", "composition"):
            err = _check_case(case, dtype, path, gpu, 50 + i)
            report(f"af_op_region_attention {path} {case} vs float64 [{dtype}]", err, 1.0, RC.OP_TOL[dtype])
            assert err < RC.OP_TOL[dtype], (case, dtype, path, err)
        q, k, v, w = RC.op_inputs(case, 50 + i)
        with pytest.raises(AfError):
            ops.region_attention(q.to(gpu), k.to(gpu), v.to(gpu), w.to(gpu), case[4], case[2], dtype=dtype, path="fused")


def test_operator_planner_path_is_the_fused_kernel(gpu):
    from adaface_amd import _lib
    case = (40, 77, 3, 64, 2, 1, 0)
    q, k, v, w = RC.op_inputs(case, 7)
    n0 = _lib.load().af_region_attn_launches()
    a = _run(case, "bf16", "auto", gpu, q, k, v, w)
    assert _lib.load().af_region_attn_launches() == n0 + 1
    assert torch.equal(a, _run(case, "bf16", "fused", gpu, q, k, v, w))
    _run(case, "bf16", "composition", gpu, q, k, v, w)
    assert _lib.load().af_region_attn_launches() == n0 + 2


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_operator_structure_is_bit_exact(gpu, dtype):
    """Fused path.  All weight on region r == the R = 1 run on that segment alone; a sample alone == the same sample at
    position 2 of a batch of 3; a second run gives the same bits."""
    for case in ((40, 77, 3, 257, 8, 3, 0), (128, 33, 8, 64, 2, 3, 8)):
        dh, T, R, Nq, heads, B, slack = case
        q, k, v, w = RC.op_inputs(case, 11)
        first = _run(case, dtype, "fused", gpu, q, k, v, w)
        assert torch.equal(_bits(first), _bits(_run(case, dtype, "fused", gpu, q, k, v, w)))
        one = (dh, T, R, Nq, heads, 1, slack)
        alone = _run(one, dtype, "fused", gpu, q[2:], k[2:], v[2:], w[2:])
        assert torch.equal(_bits(alone[0]), _bits(first[2])), case
        for r in (0, R - 1):
            wr = torch.zeros_like(w)
            wr[:, r] = 1.0
            got = _run(case, dtype, "fused", gpu, q, k, v, wr)
            seg = (dh, T, 1, Nq, heads, B, slack)
            want = _run(seg, dtype, "fused", gpu, q, k[:, r * T:(r + 1) * T], v[:, r * T:(r + 1) * T], torch.ones(B, 1, Nq))
            assert torch.equal(_bits(got), _bits(want)), (case, r)


@pytest.mark.parametrize("path", ["fused", "composition"])
def test_selection_keeps_nan_regions_out(gpu, path):
    """Region 2's K / V rows are NaN.  w_2 = 0 on (a) the whole first 32-query block and (b) half of the second: those queries
    are finite and bit-equal to the run with a finite region 2; the queries with w_2 > 0 are NaN."""
    case = (40, 77, 3, 64, 2, 1, 0)
    q, k, v, _ = RC.op_inputs(case, 21)
    g = torch.Generator().manual_seed(3)
    a = torch.rand(1, 3, 64, generator=g, dtype=torch.float64) + 0.1
    a[:, 2, :48] = 0.0
    w = RC.normalise(a)
    clean = _run(case, "bf16", path, gpu, q, k, v, w)
    kn, vn = k.clone(), v.clone()
    kn[:, 154:] = float("nan")
    vn[:, 154:] = float("nan")
    got = _run(case, "bf16", path, gpu, q, kn, vn, w)
    assert torch.isfinite(got[:, :48]).all()
    assert torch.equal(_bits(got[:, :48]), _bits(clean[:, :48]))
    assert torch.isnan(got[:, 48:]).all()
    assert torch.isfinite(clean).all()


@pytest.mark.parametrize("path", ["fused", "composition"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_segment_tail_is_masked(gpu, report, dtype, path):
    """T = 77, R = 2, w = (1, 0): the 19 rows behind segment 0's last key are segment 1's FIRST keys, not padding.  They score
    30 above everything in segment 0 (q's first coordinate per head is 4, theirs 7.5 sqrt(dh) + ..), so a kernel that reads
    past key 76 puts all of the softmax on them and fails by order 1."""
    dh, heads = 40, 2
    case = (dh, 77, 2, 64, heads, 1, 0)
    q, k, v, _ = RC.op_inputs(case, 31)
    q = q.reshape(1, 64, heads, dh)
    q[..., 0] = 4.0
    q = q.reshape(1, 64, heads * dh)
    k1 = torch.zeros(19, heads, dh)
    k1[..., 0] = (30.0 + 12.0) * dh ** 0.5 / 4.0            # score 42 against |segment 0 scores| < 12
    k[:, 77:96] = k1.reshape(19, heads * dh)
    v[:, 77:96] = 5.0 + v[:, 77:96]
    w = torch.zeros(1, 2, 64)
    w[:, 0] = 1.0
    ref = RR.region_attention(RC.storage_round(q, dtype), RC.storage_round(k, dtype), RC.storage_round(v, dtype), w, heads, 2)
    s0 = (RC.storage_round(q, dtype).reshape(64, heads, dh).permute(1, 0, 2) @
          RC.storage_round(k, dtype)[0, :77].reshape(77, heads, dh).permute(1, 2, 0)) * dh ** -0.5
    assert float(s0.abs().max()) < 12.0
    got = _run(case, dtype, path, gpu, q, k, v, w)
    err = _rel(got, ref)
    report(f"af_op_region_attention {path}: segment tail, T = 77, the next segment scoring +30 [{dtype}]", err, 1.0, RC.OP_TOL[dtype])
    assert err < RC.OP_TOL[dtype], err


# ======================================================================================================================
# 3. the model
# ======================================================================================================================
FORMS = {"plain1_16x16": (False, 1, 16, 16), "twin1_16x16": (True, 1, 16, 16), "plain2_32x16": (False, 2, 32, 16),
         "twin2_32x16": (True, 2, 32, 16)}


def _unet_kwargs(cfg):
    return dict(in_channels=cfg.in_channels, model_channels=cfg.model_channels, out_channels=cfg.out_channels,
                num_res_blocks=cfg.num_res_blocks, attention_resolutions=cfg.attention_resolutions,
                channel_mult=cfg.channel_mult, num_heads=cfg.num_heads, context_dim=cfg.context_dim,
                transformer_depth=cfg.transformer_depth, n_context_layers=cfg.n_context_layers)


@pytest.fixture(scope="module")
def tiny_sd():
    return O.synth_state_dict(O.unet_param_shapes(CFG), seed=11)


@pytest.fixture(scope="module")
def inputs():
    out = {}
    for n, (name, (twin, B, H, W)) in enumerate(FORMS.items()):
        g = torch.Generator().manual_seed(700 + n)
        Bf = 2 * B if twin else B
        out[name] = dict(x=torch.randn(B, 4, H, W, generator=g), t=torch.tensor([981, 500][:B]),
                         ctx=torch.randn(Bf * 16, 3 * 77, CFG.context_dim, generator=g), Bf=Bf,
                         m=RC.model_maps(B, H, W, 2 if twin else 1))
    return out


_oracle_cache = {}


def _oracle(tiny_sd, inputs, form):
    if form not in _oracle_cache:
        twin, B, H, W = FORMS[form]
        i = inputs[form]
        rep = (lambda v: torch.cat([v, v])) if twin else (lambda v: v)
        with torch.no_grad(), RR.patched(i["m"], 3, (H, W)):
            _oracle_cache[form] = O.unet_forward(tiny_sd, CFG, rep(i["x"]), rep(i["t"]), i["ctx"])
    return _oracle_cache[form]


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


def _forward(eng, inputs, form, gpu, regions=True):
    twin = FORMS[form][0]
    i = inputs[form]
    eng.set_context(i["ctx"].to(gpu), i["Bf"], layerwise=True)
    eng.set_regions(i["m"].to(gpu) if regions else None)
    return (eng.unet_forward_twin if twin else eng.unet_forward)(i["x"].to(gpu), i["t"].to(gpu))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_forward_against_the_patched_oracle(gpu, report, knobs, engines, inputs, tiny_sd, dtype, form):
    """unet_forward / unet_forward_twin (unconditional legs (1, 0, 0)) with R = 3 -- the base, a hard region, a soft overlapping
    region, a gap in the last sample -- at maps down to 2 x 2 (every site has a query tail).  With the default knob and with
    region_fused = 0; on the 16-bit handles the default takes the fused kernel at every site, f32 and the knob none."""
    eng = engines(dtype)
    ref = _oracle(tiny_sd, inputs, form)
    got = _forward(eng, inputs, form, gpu)
    err = _rel(got, ref)
    report(f"tiny regions {form}: forward vs patched oracle [{dtype}]", err, 1.0, RC.MODEL_TOL[dtype])
    st = eng.region_state()
    H, W = FORMS[form][2:]
    assert (st["R"], st["H"], st["W"]) == (3, H, W)
    assert st["fused_sites"] == (0 if dtype == "f32" else N_SITES), st
    assert err < RC.MODEL_TOL[dtype], err
    knobs("region_fused", 0)
    got0 = _forward(eng, inputs, form, gpu)
    err0 = _rel(got0, ref)
    report(f"tiny regions {form}: forward by composition vs patched oracle [{dtype}]", err0, 1.0, RC.MODEL_TOL[dtype])
    assert eng.region_state()["fused_sites"] == 0
    assert err0 < RC.MODEL_TOL[dtype], err0
    eng.set_regions(None)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_off_is_free_and_context_keeps_or_drops(gpu, tiny_sd, inputs, dtype):
    """Regions off again == a forward on a fresh handle, bit for bit.  A set_context of the same shape keeps the regions (and
    the forward repeats), one of another shape drops them."""
    from adaface_amd.engine import Engine
    form = "twin1_16x16"
    fresh = Engine(dtype=dtype, unet=_unet_kwargs(CFG))
    assert fresh.load_state_dict(tiny_sd) == []
    want = _forward(fresh, inputs, form, gpu, regions=False).clone()
    assert fresh.region_state() == {"R": 0, "H": 0, "W": 0, "fused_sites": 0}
    fresh.close()
    eng = Engine(dtype=dtype, unet=_unet_kwargs(CFG))
    assert eng.load_state_dict(tiny_sd) == []
    with_r = _forward(eng, inputs, form, gpu).clone()
    assert not torch.equal(with_r, want)
    i = inputs[form]
    eng.set_context(i["ctx"].to(gpu), i["Bf"], layerwise=True)               # same shape: kept
    assert eng.region_state()["R"] == 3
    assert torch.equal(eng.unet_forward_twin(i["x"].to(gpu), i["t"].to(gpu)), with_r)
    assert torch.equal(_forward(eng, inputs, form, gpu, regions=False), want)
    eng.set_regions(i["m"].to(gpu))
    eng.set_context(i["ctx"][:, :154].contiguous().to(gpu), i["Bf"], layerwise=True)     # another token count: dropped
    assert eng.region_state()["R"] == 0
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_deep_cache_reuse_repeats_its_refresh(gpu, engines, inputs, dtype):
    eng = engines(dtype)
    form = "plain2_32x16"
    want = _forward(eng, inputs, form, gpu).clone()
    i = inputs[form]
    x, t = i["x"].to(gpu), i["t"].to(gpu)
    assert torch.equal(eng.unet_forward_cached(x, t, depth=2, mode="refresh"), want)
    assert torch.equal(eng.unet_forward_cached(x, t, depth=2, mode="reuse"), want)
    eng.set_regions(i["m"].to(gpu))                                          # set_regions drops the kept feature
    from adaface_amd._lib import AfError
    with pytest.raises(AfError, match="no kept feature"):
        eng.unet_forward_cached(x, t, depth=2, mode="reuse")
    eng.set_regions(None)


def test_refusals(gpu, tiny_sd, inputs):
    """Every refusal happens on the host: the launch counters do not move."""
    from adaface_amd import _lib
    from adaface_amd._lib import AfError
    from adaface_amd.engine import Engine
    eng = Engine(dtype="bf16", unet=_unet_kwargs(CFG))
    assert eng.load_state_dict(tiny_sd) == []
    i = inputs["plain2_32x16"]
    x, t, ctx, m = i["x"].to(gpu), i["t"].to(gpu), i["ctx"].to(gpu), i["m"].to(gpu)

    def refused(exc, match, fn, *a, **kw):
        torch.cuda.synchronize()
        before = (_lib.plan_counts(reset=False), _lib.load().af_region_attn_launches())
        with pytest.raises(exc, match=match):
            fn(*a, **kw)
        assert (_lib.plan_counts(reset=False), _lib.load().af_region_attn_launches()) == before

    refused(AfError, "af_set_context", eng.set_regions, m)                               # before any context
    eng.set_context(ctx, 2, layerwise=True)
    refused(AfError, "regions", eng.set_regions, torch.ones(2, 9, 32, 16, device=gpu))   # R > 8
    refused(AfError, "segments", eng.set_regions, torch.ones(2, 2, 32, 16, device=gpu))  # 231 % 2
    refused(AfError, "multiples of 8", eng.set_regions, torch.ones(2, 3, 32, 12, device=gpu))
    refused(AfError, "af_set_context", eng.set_regions, torch.ones(3, 3, 32, 16, device=gpu))   # another batch
    refused(ValueError, "finite", eng.set_regions, -m)
    eng.set_conv_attn(3, [0], [list(range(1, 10))])
    eng.set_context(ctx, 2, layerwise=True)
    refused(AfError, "conv attention", eng.set_regions, m)
    eng.set_conv_attn(0)
    eng.set_context(ctx, 2, layerwise=True)
    eng.set_regions(m)
    assert eng.region_state()["R"] == 3
    refused(AfError, "regions: set for", eng.unet_forward, x[:, :, :16], t)              # another H x W
    refused(AfError, "af_set_context|regions", eng.unet_forward, x[:1], t[:1])           # another batch
    refused(NotImplementedError, "T-GATE", eng.unet_forward, x, t, tgate="capture")
    refused(NotImplementedError, "T-GATE", eng.unet_forward, x, t, tgate="replay")
    eng.set_pag(("mid",))
    refused(NotImplementedError, "PAG", eng.unet_forward_pag, x, t)
    eng.set_pag(())
    refused(NotImplementedError, "ControlNet", eng.set_control, torch.zeros(8, device=gpu, dtype=torch.bfloat16), [1.0], shape=(2, 32, 16))
    refused(NotImplementedError, "conv attention", eng.set_conv_attn, 3, [0], [list(range(1, 10))])
    # ... and the C ABI itself, under the Python checks
    lib, sp = _lib.load(), _lib.stream_ptr()
    out = torch.empty(6, 4, 32, 16, device=gpu)
    x3, t3 = torch.cat([x, x[:1]]), torch.cat([t, t[:1]])
    assert lib.af_tgate_set(eng._h, 1) == 0
    assert lib.af_unet_forward(eng._h, _lib.ptr(x), _lib.ptr(t), _lib.ptr(out), 2, 32, 16, sp) == -4     # AF_ERR_STATE
    assert lib.af_tgate_set(eng._h, 0) == 0
    eng.set_pag(("mid",))
    assert lib.af_unet_forward_pag(eng._h, _lib.ptr(x3), _lib.ptr(t3), _lib.ptr(out), 3, 32, 16, sp) == -4
    eng.set_pag(())
    assert lib.af_unet_forward(eng._h, _lib.ptr(x), _lib.ptr(t), _lib.ptr(out), 2, 16, 16, sp) == -4
    # a context of another batch drops the regions; the old batch's forward then has no context
    eng.set_context(torch.cat([ctx, ctx[:16]]), 3, layerwise=True)
    assert eng.region_state()["R"] == 0
    refused(AfError, "af_set_context", eng.unet_forward, x, t)
    eng.close()


# ======================================================================================================================
# 4. the sampler
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


def test_ddim_sampler_with_regions(gpu, report, tiny_model, tiny_sd):
    """DDIM through LatentDiffusion.set_regions + DDIMSampler.sample against O.ddim_sample over the patched oracle, f32.  S = 4,
    four loop steps: the uniform grid arange(0, 1000, 1000 // S) + 1 has no S with three entries, and S = 3 yields timestep
    1000, which the schedule of 1000 does not hold.  Bar: the larger of the f32 model bar and 4 x the deviation the same
    sampler shows with regions off against the unpatched oracle on the same x_T (the two trajectories amplify round-off
    differently; a missing feature shows 0.2)."""
    from ldm.models.diffusion.ddim import DDIMSampler
    gold = dict(np.load(GOLD / "golden_tiny.npz"))
    x_T, c0, uc0 = torch.tensor(gold["ddim_xT"]), torch.tensor(gold["ddim_c"]), torch.tensor(gold["ddim_uc"])
    g = torch.Generator().manual_seed(41)
    regs = [torch.randn(c0.shape, generator=g) for _ in range(2)]
    both = RG.concat_contexts([c0] + regs, uc0)
    c, uc = both[: c0.shape[0]].contiguous(), both[c0.shape[0]:].contiguous()
    B, H, W = x_T.shape[0], x_T.shape[2], x_T.shape[3]
    m = RC.model_maps(B, H, W, 2)
    sched = O.register_schedule()
    with torch.no_grad():
        plain_ref = O.ddim_sample(lambda x, t, cc: O.unet_forward(tiny_sd, CFG, x, t, cc), sched, 4, x_T, c0, uc0, (10.0, 4.0))
        with RR.patched(m, 3, (H, W)):
            ref = O.ddim_sample(lambda x, t, cc: O.unet_forward(tiny_sd, CFG, x, t, cc), sched, 4, x_T, c, uc, (10.0, 4.0))
    cond = lambda v: tiny_model.get_learned_conditioning(v.to(gpu))
    kw = dict(S=4, batch_size=B, shape=list(x_T.shape[1:]), verbose=False, guidance_scale=[10.0, 4.0], x_T=x_T.to(gpu), eta=0.0)
    off, _ = DDIMSampler(tiny_model).sample(conditioning=cond(c0), unconditional_conditioning=cond(uc0), **kw)
    dev_off = _rel(off, plain_ref)
    tiny_model.set_regions(m)
    try:
        lat, _ = DDIMSampler(tiny_model).sample(conditioning=cond(c), unconditional_conditioning=cond(uc), **kw)
        assert tiny_model.model.diffusion_model.engine(gpu).region_state()["R"] == 3
    finally:
        tiny_model.set_regions(None)
    err = _rel(lat, ref)
    bar = max(RC.MODEL_TOL["f32"], 4.0 * dev_off)
    report("dropin DDIMSampler S=4 regions off vs unpatched oracle [f32]", dev_off, float(plain_ref.abs().max()), RC.MODEL_TOL["f32"])
    report("dropin DDIMSampler S=4 with regions vs patched oracle [f32]", err, float(ref.abs().max()), bar)
    assert err < bar, (err, dev_off)
    assert _rel(off, ref) > 0.05                    # (the bar tells the regional run from the plain one)
    again, _ = DDIMSampler(tiny_model).sample(conditioning=cond(c0), unconditional_conditioning=cond(uc0), **kw)
    assert torch.equal(again, off)                  # (and nothing lingers on the handle)
