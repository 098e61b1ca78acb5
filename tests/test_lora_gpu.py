"""GPU tests of the LoRA adapters (af_lora.hip, af_load_tensor_lora, HipModule.set_lora) against tests/lora_ref.py.

Operator (ops.lora_repack), every storage type, the smallest shapes at which each branch can go wrong (padding columns and 3x3
taps, sizes that are no tile multiples, a row offset into a fused buffer with a rank that straddles the chunk, the GEGLU row order
with two adapters, the rank limit, one SD-1.5 width): exact-operand adapters bit for bit against the restated packing, a sentinel
around everything the layout does not own, two runs, and normal operands within the derived per-element bound.
Model (tiny config, synthetic weights seed 11, Bf = 2, 16 x 16): set_lora on a live model against a second model whose state dict
was merged on the CPU, the way back, scales and composition, the partial reload, the oracle under the project's bars, unchanged
launches, an engine rebuild, the text tower and a 3-step DDIM run."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import lora_ref as LR  # noqa: E402
from oracle import clip_oracle as CO  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = {"f32": 2e-4, "bf16": 3e-2, "f16": 3e-2 / 8}      # tests/test_model_gpu.py; f16: F16_MODEL_TOL of tests/test_fp16_gpu.py
DTYPES = ["f32", "bf16", "f16"]
CFG = O.TINY_UNET
PFX = "model.diffusion_model."
SENTINEL = 7.0

# (rows, cin, ks, cin_pad, row_off, rows_total, perm, ranks); every buffer gets 8 columns of slack behind kk * cin_pad and, where
# rows_total is None, two rows behind the weight's
OP_CASES = [(8, 4, 3, 8, 0, None, 0, (1,)), (40, 24, 1, 24, 0, None, 0, (4,)), (64, 64, 1, 64, 64, 192, 0, (33,)),
            (64, 48, 1, 48, 0, None, 1, (8, 3)), (96, 40, 3, 40, 0, None, 0, (16,)), (320, 320, 1, 320, 0, None, 0, (256,)),
            (1280, 320, 3, 320, 0, None, 0, (32,))]
_ids = lambda c: f"{c[0]}x{c[1]}k{c[2]}p{c[3]}o{c[4]}g{c[6]}r{'+'.join(map(str, c[7]))}"
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_cases = {}


def _case(case):
    """base, exact-operand adapters (integers in [-4, 4], s a power of two) and normal ones, once per case"""
    if case not in _cases:
        rows, cin, ks, cin_pad, row_off, rows_total, perm, ranks = case
        g = torch.Generator().manual_seed(1000 + rows + 3 * cin + ks)
        shape = (rows, cin, ks, ks) if ks > 1 else (rows, cin)
        base = 0.1 * torch.randn(shape, generator=g)
        exact, general = [], []
        for i, r in enumerate(ranks):
            dshape = (r,) + shape[1:]
            exact.append((torch.randint(-4, 5, (rows, r), generator=g).float(), torch.randint(-4, 5, dshape, generator=g).float(),
                          2.0 ** (-6 + 3 * i)))
            general.append((torch.randn(rows, r, generator=g), torch.randn(dshape, generator=g), (0.37, -1.3)[i] / r ** 0.5))
        kk = ks * ks
        geom = dict(cin_pad=cin_pad, ldw=kk * cin_pad + 8, row_off=row_off, rows_total=rows_total or row_off + rows + 2, perm=bool(perm))
        _cases[case] = (base, exact, general, geom)
    return _cases[case]


def _run(gpu, base, adapters, geom, dtype):
    from adaface_amd import ops
    buf = torch.full((geom["rows_total"], geom["ldw"]), SENTINEL, dtype=LR.STORAGE[dtype], device=gpu)
    out = ops.lora_repack(base.to(gpu), [(u.to(gpu), d.to(gpu), s) for u, d, s in adapters], dtype=dtype, out=buf, **geom)
    assert out is buf
    return out.cpu()


def _packed(flat, case, geom, fill):
    rows, cin, ks = case[0], case[1], case[2]
    return LR.pack(flat, cin, ks * ks, geom["cin_pad"], geom["ldw"], geom["row_off"], geom["rows_total"], geom["perm"], fill=fill)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(_INT[a.dtype]), b.view(_INT[b.dtype]))


# ======================================================================================================================
# the operator
# ======================================================================================================================
@pytest.mark.parametrize("case", OP_CASES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_exact_operands_bit_for_bit(gpu, dtype, case):
    """Every partial sum is exact and only the additions of the adapters round: the fused result is the restated packing of the
    fp32 merge, bit for bit; the sentinel survives everywhere else; zero adapters give the plain repack; two runs agree."""
    base, exact, _, geom = _case(case)
    st = LR.STORAGE[dtype]
    got = _run(gpu, base, exact, geom, dtype)
    want = _packed(LR.merge32(base, exact).to(st), case, geom, SENTINEL)
    assert _same_bits(got, want), f"{int((got.float() != want.float()).sum())} elements differ"
    assert _same_bits(_run(gpu, base, exact, geom, dtype), got)
    # what the layout does not own: rows outside [row_off, row_off + rows) and the columns beyond kk * cin_pad
    rows, kk = case[0], case[2] ** 2
    owned = torch.zeros(geom["rows_total"], geom["ldw"], dtype=torch.bool)
    owned[geom["row_off"]:geom["row_off"] + rows, :kk * geom["cin_pad"]] = True
    assert (got[~owned].float() == SENTINEL).all() and int((~owned).sum()) >= 8 * geom["rows_total"]
    # zero adapters: the plain repack
    plain = _run(gpu, base, [], geom, dtype)
    assert _same_bits(plain, _packed(base.reshape(rows, -1).to(st), case, geom, SENTINEL))
    assert not _same_bits(plain, got)


@pytest.mark.parametrize("case", OP_CASES, ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_normal_operands_within_the_bound(gpu, report, dtype, case):
    """|got - ref64| <= (R_total + A + 2) 2^-24 (|W| + sum |s| sum |up| |down|) + one storage ulp at |ref|, on EVERY element."""
    base, _, general, geom = _case(case)
    got = _run(gpu, base, general, geom, dtype).double()
    ref, bnd = LR.bound(base, general, dtype)
    refp, bndp = _packed(ref, case, geom, SENTINEL), _packed(bnd, case, geom, 0.0)
    assert got.shape == refp.shape and torch.isfinite(got).all()
    err = (got - refp).abs()
    checked = int((bndp > 0).sum())
    assert checked == case[0] * case[1] * case[2] ** 2                   # no element of the weight is skipped
    worst = float((err[bndp > 0] / bndp[bndp > 0]).max())
    print(f"lora_repack {_ids(case)} [{dtype}]: max |got - ref| = {float(err.max()):.3e}, {worst:.3f} of the bound")
    report(f"lora_repack {_ids(case)}: |got - ref64| over the derived bound [{dtype}]", worst, 1.0, 1.0)
    assert bool((err <= bndp).all()), worst


def test_op_refusals(gpu):
    from adaface_amd import ops
    from adaface_amd._lib import AfError
    z = lambda *s: torch.zeros(*s, device=gpu)
    ok = (z(32, 8), z(8, 16), 1.0)
    with pytest.raises(ValueError, match="adapter 0"):
        ops.lora_repack(z(32, 16), [(z(31, 8), z(8, 16), 1.0)])
    with pytest.raises(ValueError, match="rank 257"):
        ops.lora_repack(z(32, 16), [(z(32, 257), z(257, 16), 1.0)])
    with pytest.raises(AfError, match=r"rc=-1.*at most 8"):
        ops.lora_repack(z(32, 16), [ok] * 9)
    with pytest.raises(AfError, match=r"rc=-1.*do not fit"):
        ops.lora_repack(z(32, 16), [ok], cin_pad=16, ldw=8)
    with pytest.raises(AfError, match=r"rc=-1.*GEGLU"):
        ops.lora_repack(z(48, 16), [(z(48, 8), z(8, 16), 1.0)], perm=True)
    with pytest.raises(AfError, match=r"rc=-1.*finite"):
        ops.lora_repack(z(32, 16), [(z(32, 8), z(8, 16), float("inf"))])
    with pytest.raises(ValueError, match="GPU"):
        ops.lora_repack(torch.zeros(32, 16), [])


# ======================================================================================================================
# the model
# ======================================================================================================================
# a fused q/k/v slot, the hoisted K/V, the permuted GEGLU slot, ff.net.2, proj_in, a ResBlock 3x3 conv, emb_layers.1 -- at the
# outermost level and, for the slots whose shape depends on it, at a deeper one
T = "input_blocks.1.1.transformer_blocks.0"
TARGETS = [f"{T}.attn1.to_q", f"{T}.attn1.to_v", f"{T}.attn2.to_k", f"{T}.attn2.to_v", f"{T}.ff.net.0.proj", f"{T}.ff.net.2",
           "input_blocks.1.1.proj_in", "input_blocks.1.0.in_layers.2", "input_blocks.1.0.emb_layers.1",
           "middle_block.1.transformer_blocks.0.attn2.to_k", "output_blocks.5.1.transformer_blocks.0.ff.net.0.proj",
           "output_blocks.11.1.transformer_blocks.0.attn2.to_out.0", "output_blocks.8.0.out_layers.3"]
TARGETS_B = ["input_blocks.1.1.proj_in", f"{T}.attn1.to_k", "middle_block.2.in_layers.2"]


@pytest.fixture(scope="module")
def tiny_sd():
    return O.synth_state_dict(O.unet_param_shapes(CFG), seed=11)


@pytest.fixture(scope="module")
def shapes(tiny_sd):
    return {k[len(PFX):-len(".weight")]: tuple(v.shape) for k, v in tiny_sd.items() if k.endswith(".weight")}


@pytest.fixture(scope="module")
def inputs(gpu):
    g = torch.Generator().manual_seed(77)
    x, t, ctx = torch.randn(2, 4, 16, 16, generator=g), torch.tensor([981, 300]), torch.randn(2 * 16, 77, CFG.context_dim, generator=g)
    return dict(x=x, t=t, ctx=ctx, xg=x.to(gpu), tg=t.to(gpu), ctxg=ctx.to(gpu))


def _unet(sd, dtype):
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    m = UNetModel(image_size=16, in_channels=CFG.in_channels, model_channels=CFG.model_channels, out_channels=CFG.out_channels,
                  num_res_blocks=CFG.num_res_blocks, attention_resolutions=list(CFG.attention_resolutions),
                  channel_mult=list(CFG.channel_mult), num_heads=CFG.num_heads, use_spatial_transformer=True,
                  context_dim=CFG.context_dim, transformer_depth=CFG.transformer_depth)
    m.load_state_dict({k[len(PFX):]: v for k, v in sd.items() if k.startswith(PFX)}, strict=True)
    return m.set_compute_dtype(dtype)


def _eps(m, inputs):
    return m(inputs["xg"], inputs["tg"], context=inputs["ctxg"], extra_info={"use_layerwise_context": True})


def _close(*models):
    for m in models:
        if m._engine is not None:
            m._engine.close()
            object.__setattr__(m, "_engine", None)


def _rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if not torch.isfinite(got).all():
        return float("inf")
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "fp8"])
def test_live_set_lora_equals_a_fresh_engine_on_merged_weights(gpu, tiny_sd, shapes, inputs, dtype):
    """Exact-operand adapters: the fused load's fp32 value IS the host merge's, so a live model after set_lora and a second
    model that loaded the merged state dict plainly must give the same eps, bit for bit -- a stale LayerNorm-folded twin, fp8
    copy, up-phase pack or hoisted K / V would show here.  Then the way back with the context cache warm."""
    a = LR.exact_adapter(shapes, TARGETS, 4, seed=21)
    live, fresh = _unet(tiny_sd, dtype), _unet(LR.merged_state_dict(tiny_sd, [(a, 1.0)], PFX, exact=True), dtype)
    try:
        base = _eps(live, inputs)                               # (engine built, context hoisted, derived state made)
        sd_before = {k: v.clone() for k, v in live.state_dict().items()}
        live.set_lora([(a, 1.0)])
        assert live.lora_targets() == sorted(TARGETS)
        on = _eps(live, inputs)
        want = _eps(fresh, inputs)
        assert torch.isfinite(on).all() and not torch.equal(on, base)
        assert torch.equal(on, want), _rel(on, want)
        assert all(torch.equal(v, sd_before[k]) for k, v in live.state_dict().items())
        live.clear_lora()
        assert torch.equal(_eps(live, inputs), base)
    finally:
        _close(live, fresh)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_scales_composition_and_partial_reload(gpu, tiny_sd, shapes, inputs, dtype):
    a = LR.exact_adapter(shapes, TARGETS, 4, seed=21)
    b = LR.exact_adapter(shapes, TARGETS_B, 3, seed=22)
    m, both = _unet(tiny_sd, dtype), _unet(LR.merged_state_dict(tiny_sd, [(a, 0.5), (b, 2.0)], PFX, exact=True), dtype)
    try:
        base = _eps(m, inputs)
        m.set_lora([(a, 0.0)])                                  # scale 0: fmaf(0, acc, w) = w
        assert torch.equal(_eps(m, inputs), base)
        m.set_lora([(a, 0.5), (b, 2.0)])
        assert torch.equal(_eps(m, inputs), _eps(both, inputs))
        # swapping set A for set B loads the union of their targets again and nothing else
        m.set_lora([(a, 1.0)])
        eng, calls = m._engine, []
        plain, fused = eng.load_tensor, eng.load_tensor_lora
        eng.load_tensor = lambda name, t: (calls.append(("plain", name, 0)), plain(name, t))[1]
        eng.load_tensor_lora = lambda name, t, ads: (calls.append(("lora", name, len(ads))), fused(name, t, ads))[1]
        m.set_lora([(b, 1.0)])
        del eng.load_tensor, eng.load_tensor_lora
        union = sorted(set(TARGETS) | set(TARGETS_B))
        assert sorted(n for k, n, _ in calls if k == "lora") == [f"{PFX}{n}.weight" for n in union]
        assert {n: c for k, n, c in calls if k == "lora"} == {f"{PFX}{n}.weight": int(n in TARGETS_B) for n in union}
        assert sorted(n for k, n, _ in calls if k == "plain") == [f"{PFX}{n}.weight" for n in union if n not in TARGETS_B]
        only_b = _unet(LR.merged_state_dict(tiny_sd, [(b, 1.0)], PFX, exact=True), dtype)
        try:
            assert torch.equal(_eps(m, inputs), _eps(only_b, inputs))
        finally:
            _close(only_b)
    finally:
        _close(m, both)


_oracle = {}


def _oracle_eps(tiny_sd, inputs, adapters):
    key = "merged" if adapters else "base"
    if key not in _oracle:
        sd = LR.merged_state_dict(tiny_sd, adapters, PFX) if adapters else tiny_sd
        with torch.no_grad():
            _oracle[key] = O.unet_forward(sd, CFG, inputs["x"], inputs["t"], inputs["ctx"])
    return _oracle[key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_matches_the_oracle_on_merged_weights(gpu, report, tiny_sd, inputs, dtype):
    """Normal adapters sized so that the merged delta's rms is a third of the base weight's, against O.unet_forward on the
    CPU-merged (fp64, rounded to fp32) state dict under the project's bars; and, on the CPU references alone, the adapters move
    eps by more than ten times the largest of those bars, so ignoring them cannot pass."""
    a = LR.random_adapter(tiny_sd, PFX, TARGETS, 8, seed=31)
    ref, ref_base = _oracle_eps(tiny_sd, inputs, [(a, 1.0)]), _oracle_eps(tiny_sd, inputs, [])
    effect = _rel(ref, ref_base)
    assert effect > 10 * max(TOL.values()), effect
    m = _unet(tiny_sd, dtype)
    try:
        m.set_lora([(a, 1.0)])
        err = _rel(_eps(m, inputs), ref)
        print(f"tiny lora [{dtype}]: eps err {err:.3e} (bar {TOL[dtype]:.2e}); the adapters move the reference by {effect:.3f}")
        report(f"tiny lora: eps vs oracle on merged weights [{dtype}]", err, 1.0, TOL[dtype])
        assert err < TOL[dtype], err
    finally:
        _close(m)


def test_launches_unchanged_and_engine_rebuild(gpu, tiny_sd, shapes, inputs):
    from adaface_amd import _lib
    a = LR.exact_adapter(shapes, TARGETS, 4, seed=21)
    m = _unet(tiny_sd, "bf16")
    try:
        _eps(m, inputs)
        _lib.plan_counts(reset=True)
        base = _eps(m, inputs)
        pc_base = _lib.plan_counts(reset=True)
        m.set_lora([(a, 1.0)])
        _eps(m, inputs)                                         # (re-hoists the context)
        _lib.plan_counts(reset=True)
        on = _eps(m, inputs)
        assert _lib.plan_counts(reset=True) == pc_base and sum(pc_base.values()) > 0
        # the adapters survive a rebuild of the engine
        m.set_compute_dtype("f32")
        on32 = _eps(m, inputs)
        assert _rel(on32, on) < _rel(on32, base)                # (the f32 engine has them too)
        m.set_compute_dtype("bf16")
        assert torch.equal(_eps(m, inputs), on) and m.lora_targets() == sorted(TARGETS)
    finally:
        _close(m)


def test_text_tower(gpu):
    from adaface_amd.configs import tiny_config
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    sd = {k[len("cond_stage_model."):]: v for k, v in O.synth_state_dict(CO.clip_param_shapes(CO.TINY_CLIP), seed=41).items()}
    kw = tiny_config()["model"]["params"]["cond_stage_config"]["params"]
    names = ["transformer.text_model.encoder.layers.1.self_attn.q_proj", "transformer.text_model.encoder.layers.1.mlp.fc1"]
    a = LR.exact_adapter({n: tuple(sd[n + ".weight"].shape) for n in names}, names, 4, seed=41)
    ids = torch.randint(2, 190, (2, 77), generator=torch.Generator().manual_seed(3))
    live, fresh = FrozenCLIPEmbedder(device=gpu, **kw), FrozenCLIPEmbedder(device=gpu, **kw)
    try:
        live.load_state_dict(sd, strict=True)
        fresh.load_state_dict(LR.merged_state_dict(sd, [(a, 1.0)], "", exact=True), strict=True)
        base = live(ids)
        live.set_lora([(a, 1.0)])
        on = live(ids)
        assert torch.isfinite(on).all() and not torch.equal(on, base) and torch.equal(on, fresh(ids))
        live.clear_lora()
        assert torch.equal(live(ids), base)
        with pytest.raises(KeyError, match="layers.9"):
            live.set_lora([({"transformer.text_model.encoder.layers.9.mlp.fc1": a[names[1]]}, 1.0)])
    finally:
        _close(live, fresh)


def test_ddim_run_with_adapters_equals_the_merged_model(gpu, tiny_sd, shapes):
    """LatentDiffusion.set_lora (what --lora calls) and a short DDIM run with CFG, against the same run on a model that loaded
    the host-merged state dict.  S = 4, the shortest schedule above 3 steps the reference's uniform grid has: 1000 // 3 = 333
    puts S = 3 at timesteps 1, 334, 667, 1000, one beyond the table (make_ddim_sampling_parameters raises IndexError)."""
    from adaface_amd.configs import tiny_config
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.util import instantiate_from_config
    a = LR.exact_adapter(shapes, TARGETS, 4, seed=21)
    g = torch.Generator().manual_seed(5)
    ctx, uctx, x_T = torch.randn(16, 77, 64, generator=g), torch.randn(16, 77, 64, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    outs, models = [], []
    try:
        for merged in (False, True):
            model = instantiate_from_config(tiny_config()["model"]).eval()
            sd = LR.merged_state_dict(tiny_sd, [(a, 1.0)], PFX, exact=True) if merged else tiny_sd
            missing, unexpected = model.load_state_dict(sd, strict=False)
            assert not unexpected
            model = model.to(gpu).set_compute_dtype("bf16")
            models.append(model.model.diffusion_model)
            if not merged:
                assert model.set_lora([({"unet": a, "text": {}}, 1.0)]) is model
            c, uc = model.get_learned_conditioning(ctx.to(gpu)), model.get_learned_conditioning(uctx.to(gpu))
            s, _ = DDIMSampler(model).sample(S=4,conditioning=c, batch_size=1, shape=[4, 16, 16], verbose=False, guidance_scale=4.0,
                                             unconditional_conditioning=uc, eta=0.0, x_T=x_T.to(gpu))
            outs.append(s)
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    finally:
        _close(*models)
