"""GPU tests of token merging (af_tome.hip, af_set_tome) against the restatement of tests/tome_ref.py.

Operators: the match is exact on integer operands (both tie rules exercised) and, on Gaussian inputs whose margins are asserted
from the reference alone, picks exactly the reference's targets and cut; merged rows with one member are layernorm_kernel's bits,
group rows the once-rounded mean; unmerge + residual is the once-rounded fp32 sum.  Model (tiny config, synthetic weights seed
11): off is off bit for bit; on, the maps the forward chose are read through the taps, validated against the reference's own
scores and imposed on the reference, whose eps the forward must match under the bars of tests/test_model_gpu.py."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import exact_operands as E  # noqa: E402
import tome_ref as TR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = {"f32": 2e-4, "bf16": 3e-2}      # tests/test_model_gpu.py
CFG = O.TINY_UNET
SHAPES = [(2, 8, 8, 64), (3, 6, 10, 320), (1, 16, 16, 640)]          # (B, H, W, C)
RATIOS = [0.25, 0.5, 0.7, 0.75]
COSINE_SEED = {((2, 8, 8, 64), "bf16"): 1, ((2, 8, 8, 64), "f32"): 1, ((3, 6, 10, 320), "bf16"): 0, ((3, 6, 10, 320), "f32"): 0,
               ((1, 16, 16, 640), "bf16"): 1, ((1, 16, 16, 640), "f32"): 4}


def _stored(t, dtype):
    """t as the storage type holds it, float32"""
    return t.to(torch.bfloat16).float() if dtype == "bf16" else t.float()


def _ulp(ref, dtype):
    """one unit in the last place of the storage type at |ref| (float64)"""
    bits = 7 if dtype == "bf16" else 23
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - bits)


# ======================================================================================================================
# match
# ======================================================================================================================
_exact_cache = {}


def _exact_case(shape):
    """Integer operands in [-3, 3] and the reference's answer per ratio, once per shape; the preconditions under which equality
    is the right test are asserted here, from the reference alone."""
    if shape not in _exact_cache:
        B, H, W, C = shape
        g = torch.Generator().manual_seed(1000 + C + H)
        x = E.int_tensor((B, H * W, C), 1.0, g, lo=-3, hi=3)
        sc = TR.scores(x, H, W, normalize=False)
        assert torch.equal(sc, sc.round()) and float((x.abs().double().sum(-1).max()) * 3) < 2 ** 24      # |dot| < 2^24: exact in fp32
        node_max = sc.max(-1).values
        n_best = (sc == node_max[..., None]).sum(-1)
        assert int((n_best > 1).sum()) > 0, "no src token with a tied maximum"                 # the lowest-d rule is exercised
        srt = torch.sort(node_max, dim=-1, descending=True).values
        cut_ties = 0
        for ratio in RATIOS:
            r = TR.plan(H, W, ratio)[2]
            if 0 < r < srt.shape[1]:
                cut_ties += int((srt[:, r - 1] == srt[:, r]).sum())
        assert cut_ties > 0, "no tie at any cut"                                                # the lower-s rule is exercised
        _exact_cache[shape] = (x, {ratio: TR.match_from_scores(sc, H, W, ratio) for ratio in RATIOS})
    return _exact_cache[shape]


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_match_exact(gpu, dtype, shape, ratio):
    from adaface_amd import ops
    B, H, W, C = shape
    x, refs = _exact_case(shape)
    node_idx, node_max, tmap, _ = refs[ratio]
    g_idx, g_max, g_map = ops.tome_match(x.to(gpu), (H, W), ratio, normalize=False, dtype=dtype)
    assert torch.equal(g_max.cpu().double(), node_max)
    assert torch.equal(g_idx.cpu().long(), node_idx)
    assert torch.equal(g_map.cpu().long(), tmap)
    if ratio == 0.75:
        assert TR.plan(H, W, ratio)[2] == TR.plan(H, W, ratio)[1]          # r = Ns: every src token merged


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_match_cosine(gpu, report, dtype, shape):
    from adaface_amd import ops
    B, H, W, C = shape
    g = torch.Generator().manual_seed(COSINE_SEED[shape, dtype])
    x = _stored(torch.randn(B, H * W, C, generator=g), dtype)
    sc = TR.scores(x, H, W, normalize=True)
    # preconditions, from the reference alone: every src token's two best dst scores and the two sides of every cut are >= 1e-4
    # apart (fp32 accumulation of a cosine is good to about 1e-6)
    top = sc.topk(2, dim=-1).values
    assert float((top[..., 0] - top[..., 1]).min()) >= 1e-4
    srt = torch.sort(top[..., 0], dim=-1, descending=True).values
    for ratio in RATIOS:
        r = TR.plan(H, W, ratio)[2]
        if 0 < r < srt.shape[1]:
            assert float((srt[:, r - 1] - srt[:, r]).min()) >= 1e-4, ratio
    worst = 0.0
    for ratio in RATIOS:
        node_idx, node_max, tmap, _ = TR.match_from_scores(sc, H, W, ratio)
        g_idx, g_max, g_map = ops.tome_match(x.to(gpu), (H, W), ratio, normalize=True, dtype=dtype)
        err = float((g_max.cpu().double() - node_max).abs().max())
        worst = max(worst, err)
        print(f"tome_match cosine {shape} {dtype} ratio {ratio}: max |node_max - ref| = {err:.3e}")
        assert torch.equal(g_idx.cpu().long(), node_idx), ratio
        assert torch.equal(g_map.cpu().long(), tmap), ratio
        assert err <= 1e-5, err
    report(f"tome_match cosine {'x'.join(map(str, shape))} node_max vs fp64 [{dtype}]", worst, 1.0, 1e-5)


def test_match_zero_row_and_refusals(gpu):
    """A zero row has rn = 0: all its scores are 0, so it picks d = 0.  Odd maps and fp16 storage are refused."""
    from adaface_amd import ops
    from adaface_amd._lib import AfError
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 64, 64, generator=g)
    x[0, 1] = 0.0                                                # src ordinal 0
    for dtype in ("bf16", "f32"):
        idx, mx, _ = ops.tome_match(x.to(gpu), (8, 8), 0.5, normalize=True, dtype=dtype)
        assert int(idx[0, 0]) == 0 and float(mx[0, 0]) == 0.0
    with pytest.raises(AfError, match="even"):
        ops.tome_match(torch.randn(1, 63, 64).to(gpu), (7, 9), 0.5)
    with pytest.raises(AfError):
        ops.tome_match(x.to(gpu), (8, 8), 0.5, dtype="f16")
    with pytest.raises(AfError, match="ratio"):
        ops.tome_match(x.to(gpu), (8, 8), 0.8)


# ======================================================================================================================
# merge / unmerge
# ======================================================================================================================
MERGE_HW, MERGE_B, MERGE_RATIO = (16, 16), 3, 0.3                # N = 256 -> r = 76, N' = 180: six row blocks, the last one short


def _merge_case(C, seed):
    H, W = MERGE_HW
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(MERGE_B, H * W, C, generator=g)
    _, _, tmap, _ = TR.match(x, H, W, MERGE_RATIO)
    n_rows = TR.plan(H, W, MERGE_RATIO)[3]
    assert n_rows == 180 and n_rows % 64 != 0
    cnt = torch.zeros(MERGE_B, n_rows, dtype=torch.long).scatter_add_(1, tmap, torch.ones_like(tmap))
    assert int(cnt.min()) == 1 and int(cnt.max()) >= 3           # single rows and groups of several members
    # LayerNorm parameters that keep every output in [2, 14]: no mean of a group comes near zero, where the fp32 LayerNorm
    # arithmetic (relative 1e-6 of values of order 10) would no longer be small against one storage ulp of the result
    gamma = 0.5 + 0.5 * torch.rand(C, generator=g)
    beta = 7.0 + torch.rand(C, generator=g)
    return x, tmap, n_rows, cnt, gamma, beta


@pytest.mark.parametrize("dtype,C", [("bf16", 320), ("bf16", 640), ("f32", 320), ("f32", 64)])
def test_merge_rows(gpu, report, dtype, C):
    from adaface_amd import _lib, ops
    x, tmap, n_rows, cnt, gamma, beta = _merge_case(C, 7)
    x = _stored(x, dtype)
    B, N, _ = x.shape
    assert _lib.norm_plan_query("layernorm", dtype, rows=B * N, C=C)["kernel"] == "wave_row"
    y = ops.tome_merge(x.to(gpu), tmap, n_rows, gamma.to(gpu), beta.to(gpu), dtype=dtype)
    assert torch.equal(y, ops.tome_merge(x.to(gpu), tmap, n_rows, gamma.to(gpu), beta.to(gpu), dtype=dtype))       # run to run
    ln = ops.layer_norm(x.to(gpu), gamma.to(gpu), beta.to(gpu), dtype=dtype).cpu()
    y = y.cpu()
    # rows with one member: the bits layernorm_kernel stores for that token
    first = torch.full((B, n_rows), N, dtype=torch.long).scatter_reduce_(1, tmap, torch.arange(N).expand(B, N), "amin")
    single = cnt == 1
    assert torch.equal(y[single], torch.gather(ln, 1, first[..., None].expand(B, n_rows, C))[single])
    group = ~single
    if dtype == "f32":
        # the f32 LayerNorm output IS the fp32 value the kernel adds: ascending fp32 sum, one division -- reproduced exactly
        acc = torch.zeros(B, n_rows, C)
        for i in range(N):
            acc[torch.arange(B), tmap[:, i]] += ln[:, i]
        assert torch.equal(y[group], (acc / cnt[..., None].float())[group])
    else:
        ref = TR.merge(torch.nn.functional.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5), tmap, n_rows)
        assert float(ref.min()) > 2.0
        err = ((y.double() - ref).abs() / _ulp(ref, dtype))[group]
        print(f"tome_merge LN group rows C={C} [{dtype}]: max error {float(err.max()):.3f} ulp")
        report(f"tome_merge LayerNorm group rows C={C}, in storage ulps [{dtype}]", float(err.max()), 1.0, 1.0)
        assert float(err.max()) <= 1.0
    # without LayerNorm, on integers: the fp32 sums are exact and the mean is rounded once
    xi = E.int_tensor((B, N, C), 1.0, torch.Generator().manual_seed(8), lo=-3, hi=3)
    yi = ops.tome_merge(xi.to(gpu), tmap, n_rows, dtype=dtype).cpu()
    refi = TR.merge(xi.double(), tmap, n_rows)
    assert torch.equal(yi[single], refi[single].float())
    erri = (yi.double() - refi).abs() / _ulp(refi, dtype)
    assert float(erri[refi != 0].max()) <= 1.0 and bool((yi[refi == 0] == 0).all())


@pytest.mark.parametrize("dtype,C", [("bf16", 320), ("f32", 320), ("bf16", 64)])
def test_unmerge_add(gpu, dtype, C):
    from adaface_amd import ops
    x, tmap, n_rows, _, _, _ = _merge_case(C, 9)
    g = torch.Generator().manual_seed(10)
    o = _stored(torch.randn(MERGE_B, n_rows, C, generator=g), dtype)
    res = _stored(x, dtype)
    y = ops.tome_unmerge_add(o.to(gpu), res.to(gpu), tmap, dtype=dtype)
    assert torch.equal(y, ops.tome_unmerge_add(o.to(gpu), res.to(gpu), tmap, dtype=dtype))
    want = _stored(res + TR.unmerge(o, tmap), dtype)              # one fp32 addition (exact IEEE), one rounding
    assert torch.equal(y.cpu(), want)


# ======================================================================================================================
# model
# ======================================================================================================================
FORMS = {"twin1_16x16": (True, 1, 16, 16, 1), "b3_32x16": (False, 3, 32, 16, 2)}      # twin, B of x, H, W, max_downsample
RATIO = 0.5
# the model cases: 0.5 leaves N' = 128 / 256 / 64 rows; 0.7 leaves odd row counts (77 of 256, 154 of 512, 39 of 128) for the
# GEMMs, the attention kernel and the arena plan
MODEL_RATIOS = [0.5, 0.7]


def _tome_maps(eng, forward, Bf, sizes):
    """The token -> merged-row map of every site, int32 [Bf, N_site], through af_tome_set_tap: one forward() per site."""
    from adaface_amd._lib import check, ptr
    out = []
    for site in range(eng.tome_num_sites()):
        buf = torch.full((Bf, int(sizes[site])), -1, device=eng.device, dtype=torch.int32)
        check(eng._lib.af_tome_set_tap(eng._h, site, ptr(buf)), "af_tome_set_tap")
        try:
            forward()
        finally:
            eng._lib.af_tome_set_tap(eng._h, -1, None)
        out.append(buf)
    return out


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
    for n, (name, (twin, B, H, W, _)) in enumerate(FORMS.items()):
        g = torch.Generator().manual_seed(200 + n)
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


def _forward(eng, inputs, form, gpu):
    twin = FORMS[form][0]
    i = inputs[form]
    eng.set_context(i["ctx"].to(gpu), i["Bf"], layerwise=True)
    x, t = i["x"].to(gpu), i["t"].to(gpu)
    return lambda: (eng.unet_forward_twin if twin else eng.unet_forward)(x, t)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_off_is_off(gpu, tiny_sd, inputs, dtype, form):
    """Never set (a fresh engine, before any set_tome call), ratio 0, and ratio 0 after a real ratio: the same bits and the
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
    eng.set_tome(0.0)
    assert torch.equal(fwd(), plain)
    assert _lib.plan_counts(reset=True) == pc_plain
    eng.set_tome(RATIO, FORMS[form][4])
    assert eng.tome_num_sites() == len(TR.site_sizes(CFG, *FORMS[form][2:4], FORMS[form][4]))
    on = fwd()
    _lib.plan_counts(reset=True)
    eng.set_tome(0.0, FORMS[form][4])
    assert eng.tome_num_sites() == 0
    assert torch.equal(fwd(), plain)
    assert _lib.plan_counts(reset=True) == pc_plain
    assert torch.isfinite(on).all() and not torch.equal(on, plain)
    eng.close()


@pytest.mark.parametrize("RATIO", MODEL_RATIOS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_matches_the_reference_with_its_maps(gpu, report, engines, inputs, tiny_sd, dtype, form, RATIO):
    twin, B, H, W, md = FORMS[form]
    i = inputs[form]
    eng = engines(dtype)
    try:
        eng.set_tome(RATIO, md)
        fwd = _forward(eng, inputs, form, gpu)
        eps = fwd()
        assert torch.equal(fwd(), eps)                                           # deterministic
        sizes = TR.site_sizes(CFG, H, W, md)
        maps = [m.cpu() for m in _tome_maps(eng, fwd, i["Bf"], sizes)]
        assert len(maps) == len(sizes) == (5 if md == 1 else 10)
        rep = (lambda v: torch.cat([v, v])) if twin else (lambda v: v)
        log = []
        with torch.no_grad(), TR.patched(RATIO, md, (H, W), maps=maps, log=log):
            ref = O.unet_forward(tiny_sd, CFG, rep(i["x"]), rep(i["t"]), i["ctx"])
        assert len(log) == len(maps)
        differ = 0
        for site, e in enumerate(log):
            h, w = e["hw"]
            assert tuple(maps[site].shape) == (i["Bf"], h * w)
            if dtype == "f32":
                # delta = 1e-3: five times the f32 forward bar of 2e-4 (cosines are <= 1)
                TR.check_map_against_scores(maps[site], e["scores"], h, w, RATIO, 1e-3)
            else:
                TR.check_map_structure(maps[site], h, w, RATIO)
            differ += int((maps[site].long() != e["own_map"]).sum())
        if twin:                                                                 # site 0 ran on the shared half
            assert torch.equal(maps[0][:B], maps[0][B:])
        err = _rel(eps, ref)
        print(f"tiny tome {form} ratio {RATIO} md {md} [{dtype}]: eps err {err:.3e}; {differ} map entries differ from the reference's own choice")
        report(f"tiny tome ratio {RATIO} max_downsample {md} {form}: eps vs reference with the forward's maps [{dtype}]", err, 1.0, TOL[dtype])
        assert err < TOL[dtype], err
    finally:
        eng.set_tome(0.0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cached_refresh_is_the_full_forward(gpu, engines, inputs, dtype):
    eng = engines(dtype)
    try:
        for form, (twin, B, H, W, md) in FORMS.items():
            eng.set_tome(RATIO, md)
            fwd = _forward(eng, inputs, form, gpu)
            full = fwd()
            x, t = inputs[form]["x"].to(gpu), inputs[form]["t"].to(gpu)
            assert torch.equal(eng.unet_forward_cached(x, t, depth=2, mode="refresh", twin=twin), full)
            assert torch.equal(eng.unet_forward_cached(x, t, depth=2, mode="reuse", twin=twin), full)
            # a change of the setting drops the kept feature
            from adaface_amd._lib import AfError
            eng.set_tome(0.25, md)
            with pytest.raises(AfError, match="no kept feature"):
                eng.unet_forward_cached(x, t, depth=2, mode="reuse", twin=twin)
    finally:
        eng.set_tome(0.0)


def test_refused_handles(gpu, tiny_sd):
    from adaface_amd._lib import AfError
    from adaface_amd.engine import Engine
    eng = Engine(dtype="f16", unet=_unet_kwargs(CFG), vae=None)
    with pytest.raises(AfError, match="f16"):
        eng.set_tome(0.5)
    eng.set_tome(0.0)                                                            # (off is always accepted)
    eng.close()
    eng = Engine(dtype="bf16", unet=_unet_kwargs(CFG), vae=None)
    eng.set_fp8(True)
    with pytest.raises(AfError, match="fp8"):
        eng.set_tome(0.5)
    eng.set_fp8(False)
    eng.set_tome(0.5)
    with pytest.raises(AfError, match="token merging"):
        eng.set_fp8(True)
    with pytest.raises(ValueError):
        eng.set_tome(0.9)
    with pytest.raises(ValueError):
        eng.set_tome(0.5, 3)
    eng.close()


def test_sd15_twin_64x64(gpu):
    """SD-1.5 size, Bf = 2 twin, ratio 0.5: finite, the same bits twice, and 2048 of the 3072 src tokens merged at each of the
    five 64 x 64 sites (the MFMA match at C = 320, the row-panel GEMMs on 2048-row samples, the folded norm2 on the unmerge
    launch's statistics)."""
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
    eng.set_tome(0.5)
    assert eng.tome_num_sites() == 5
    fwd = lambda: eng.unet_forward_twin(x, t)
    on = fwd()
    assert torch.isfinite(on).all() and not torch.equal(on, plain)
    assert torch.equal(fwd(), on)
    maps = _tome_maps(eng, fwd, 2, [4096] * 5)
    assert TR.plan(64, 64, 0.5) == (1024, 3072, 2048, 2048)
    for m in maps:
        merged = TR.check_map_structure(m, 64, 64, 0.5)
        assert merged.sum(1).tolist() == [2048, 2048]
    print("sd15 twin Bf=2 64x64 tome 0.5: relative deviation from the un-merged forward", _rel(on, plain))
    eng.set_tome(0.0)
    assert torch.equal(eng.unet_forward_twin(x, t), plain)
    eng.close()
