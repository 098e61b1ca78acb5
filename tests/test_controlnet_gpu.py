"""ControlNet on the GPU: the one-launch residual add bit for bit, the control branch and the controlled U-Net against
the restatement of tests/controlnet_ref.py on the CPU oracle, the compositions (DeepCache, FreeU, the samplers) and the refusals.

Bars: TOL of tests/test_model_gpu.py (2e-4 f32, 3e-2 bf16) relative to max|reference|, a eighth of the bf16 bar for fp16 (as
tests/test_fp16_gpu.py), 1e-3 for the tiny f32 sampler trajectories (the drop-in sampler bar).  The operator is exact.
tests/test_controlnet_cpu.py holds the condition that control moves eps by more than ten bf16 bars on these inputs."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from oracle import ldm_oracle as O  # noqa: E402  (the checker, never the thing measured)
import controlnet_ref as R  # noqa: E402
import dpmpp_ref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = {"f32": 2e-4, "bf16": 3e-2, "f16": 3e-2 / 8}
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
CFG = O.TINY_UNET


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


def _counts(reset=True):
    from adaface_amd import _lib
    return _lib.plan_counts(reset=reset)


def _gemms(pc):
    """conv / GEMM launches: every launch is under exactly one of these counters (_lib.plan_counts)."""
    return sum(pc[f"tile{i}"] for i in range(6)) + pc["halo"] + pc["fp8"] + pc["up_phase4"]


# ======================================================================================================================
# 1. the operator
# ======================================================================================================================
SCALES = [1.0, 0.825 ** 5, -0.75, 0.5, 1.3, -0.2, 0.825 ** 12, 2.0, 0.1, -1.0, 0.9, 0.7, 0.3]
SENT = 3.0          # every byte outside the addressed ranges holds this (exact in all three dtypes)


def _op_case(dtype, shapes, Bs, cond_only, ld_mode, misalign, seed):
    """Segments [(rows, C)]: dst k is a channel range [off, off + C) of a [Bd, rows, ld] buffer (ld_mode: "dense" = C, "half0" /
    "half1" = 2 C at offset 0 / C); misalign: both base pointers 4 bytes off a 16-byte boundary.  Returns the full buffers,
    their views, the sources and the expected full buffers (computed on the CPU in the issue's arithmetic)."""
    td = TORCH[dtype]
    g = torch.Generator().manual_seed(seed)
    Bd = 2 * Bs if cond_only else Bs
    shift = 4 // torch.tensor([], dtype=td).element_size() if misalign else 0
    full, views, srcs, want = [], [], [], []
    for k, (rows, C) in enumerate(shapes):
        ld, off = {"dense": (C, 0), "half0": (2 * C, 0), "half1": (2 * C, C)}[ld_mode]
        buf = torch.full((Bd * rows * ld + 64,), SENT, dtype=td)
        body = buf[shift: shift + Bd * rows * ld].view(Bd, rows, ld)
        body[:, :, off: off + C] = torch.randn(Bd, rows, C, generator=g).to(td)
        sbuf = torch.full((Bs * rows * C + 64,), SENT, dtype=td)
        sbody = sbuf[shift: shift + Bs * rows * C].view(Bs, rows, C)
        sbody.copy_(torch.randn(Bs, rows, C, generator=g).to(td))
        exp = buf.clone()
        ebody = exp[shift: shift + Bd * rows * ld].view(Bd, rows, ld)
        d, s = body[:Bs, :, off: off + C], sbody
        ebody[:Bs, :, off: off + C] = (d.float() + s.float() * torch.tensor(SCALES[k], dtype=torch.float32)).to(td)
        full.append((buf, shift, (Bd, rows, ld), off, C))
        srcs.append((sbuf, shift, (Bs, rows, C)))
        want.append(exp)
    return full, srcs, want


def _run_op(gpu, full, srcs, n_scales, cond_only):
    from adaface_amd import ops
    dev_full = [f[0].to(gpu) for f in full]
    dev_src = [s[0].to(gpu) for s in srcs]
    dsts = [b[sh: sh + shp[0] * shp[1] * shp[2]].view(*shp)[:, :, off: off + C] for b, (_, sh, shp, off, C) in zip(dev_full, full)]
    ss = [b[sh: sh + shp[0] * shp[1] * shp[2]].view(*shp) for b, (_, sh, shp) in zip(dev_src, srcs)]
    ops.control_add(dsts, ss, SCALES[:n_scales], cond_only=cond_only)
    torch.cuda.synchronize()
    return [b.cpu() for b in dev_full], [b.cpu() for b in dev_src]


MIXED = [(64, 32), (65, 320), (64, 320), (65, 32)]
OP_CASES = [
    ("mixed4-dense-B1", MIXED, 1, False, "dense", False),
    ("mixed4-half1-B3", MIXED, 3, False, "half1", False),
    ("mixed4-half0-B3-misaligned", MIXED, 3, False, "half0", True),
    ("mixed4-half1-B1-cond-only", MIXED, 1, True, "half1", False),
    ("mixed4-dense-B3-cond-only-misaligned", MIXED, 3, True, "dense", True),
    ("thirteen-half1-B1", (MIXED * 4)[:13], 1, False, "half1", False),
    ("thirteen-dense-B3-cond-only", (MIXED * 4)[:13], 3, True, "dense", False),
    ("one-half1-B3", [(65, 320)], 3, False, "half1", False),
    ("one-dense-B1-misaligned", [(64, 32)], 1, False, "dense", True),
]


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_operator_is_bit_exact_and_touches_nothing_else(gpu, dtype):
    """Every case: the addressed ranges hold exactly (d + s * scale) in fp32, product rounded then sum rounded, rounded once to
    the storage type (computed on the CPU); every other byte of the destination buffers (the other concatenation half, the
    untouched leg of cond_only, the slack around a misaligned view) and every byte of the sources is what it was."""
    from adaface_amd import _lib
    for i, (name, shapes, Bs, cond_only, ld_mode, misalign) in enumerate(OP_CASES):
        full, srcs, want = _op_case(dtype, shapes, Bs, cond_only, ld_mode, misalign, seed=100 + i)
        before = _lib.control_add_launches()
        got, src_after = _run_op(gpu, full, srcs, len(shapes), cond_only)
        assert _lib.control_add_launches() == before + 1, name            # ONE launch, whatever the number of segments
        for k, (g_, w_) in enumerate(zip(got, want)):
            assert torch.equal(g_.view(torch.uint8), w_.view(torch.uint8)), (name, dtype, k)
            assert not torch.equal(w_, full[k][0]), (name, k)             # (the case does change something)
        for k, (a, s) in enumerate(zip(src_after, srcs)):
            assert torch.equal(a.view(torch.uint8), s[0].view(torch.uint8)), (name, dtype, k)


def test_operator_refuses_bad_arguments(gpu):
    from adaface_amd import _lib, ops
    mk = lambda B, rows, C, dt=torch.bfloat16: torch.zeros(B, rows, C, device=gpu, dtype=dt)
    before = (_lib.control_add_launches(), _counts(reset=False))
    with pytest.raises(ValueError, match="dtype"):
        ops.control_add([mk(1, 64, 32)], [mk(1, 64, 32, torch.float16)], [1.0])
    with pytest.raises(ValueError, match="dtype"):
        ops.control_add([mk(1, 64, 32), mk(1, 64, 32, torch.float32)], [mk(1, 64, 32), mk(1, 64, 32, torch.float32)], [1.0, 1.0])
    with pytest.raises(ValueError, match="at most 16"):
        ops.control_add([mk(1, 8, 32) for _ in range(17)], [mk(1, 8, 32) for _ in range(17)], [1.0] * 17)
    for Bs, Bd, co in ((2, 3, False), (2, 4, False), (2, 2, True), (1, 3, True)):
        with pytest.raises(ValueError, match="batch"):
            ops.control_add([mk(Bd, 64, 32)], [mk(Bs, 64, 32)], [1.0], cond_only=co)
    with pytest.raises(ValueError, match="dense"):
        ops.control_add([mk(1, 64, 32)], [mk(1, 64, 64)[:, :, :32]], [1.0])
    with pytest.raises(ValueError):
        ops.control_add([mk(1, 64, 32)], [mk(1, 64, 32)], [1.0, 2.0])
    # ... and the C entry point itself: more than 16 segments, a batch pair that is neither equal nor doubled, a bad dtype
    lib, C = _lib.load(), _lib.C
    d, s = mk(2, 8, 32), mk(1, 8, 32)
    arr = lambda T, v: (T * len(v))(*v)
    P = C.c_void_p

    def call(dt, n, Bs, Bd):
        m = max(n, 1)
        return lib.af_op_control_add(dt, n, arr(P, [d.data_ptr()] * m), arr(P, [s.data_ptr()] * m), arr(C.c_int, [32] * m),
                                     arr(C.c_int, [32] * m), arr(C.c_int64, [8] * m), arr(C.c_float, [1.0] * m), Bs, Bd, None)
    assert call(0, 17, 1, 1) != 0 and call(0, 0, 1, 1) != 0 and call(0, 1, 1, 3) != 0 and call(7, 1, 1, 1) != 0
    assert call(0, 1, 1, 2) == 0                                          # (the valid neighbour of the refused calls)
    torch.cuda.synchronize()
    assert _lib.control_add_launches() == before[0] + 1 and _counts(reset=False) == before[1]


# ======================================================================================================================
# engines, weights, inputs
# ======================================================================================================================
@pytest.fixture(scope="module")
def weights():
    return R.weights(CFG)


def _engines(dtype, weights, cfg=CFG):
    from adaface_amd.engine import Engine
    sd, csd = weights
    eng = Engine(dtype=dtype, unet=_unet_kwargs(cfg))
    assert eng.load_state_dict(sd) == []
    ceng = Engine(dtype=dtype, controlnet={**_unet_kwargs(cfg), "hint_channels": 3})
    assert ceng.load_state_dict(csd) == []
    return eng, ceng


@pytest.fixture(scope="module")
def refs(weights):
    """The reference's control residuals and plain forward for the two forms, computed once and never changed."""
    sd, csd = weights
    out = {}
    for name, (B, H, W, shared) in {"b3_32x16": (3, 32, 16, False), "b2_16x16": (2, 16, 16, True)}.items():
        x, t, ctx, hint = R.case(CFG, B, H, W, shared_hint=shared)
        with torch.no_grad():
            res = R.control_forward(csd, CFG, x, t, ctx, hint)
        out[name] = dict(x=x, t=t, ctx=ctx, hint=hint, res=res, B=B, H=H, W=W)
    return out


def _residuals(ceng, gpu, c, n_blocks=None, ctx=None, B=None):
    """The control engine's residuals for case c as (flat, [NCHW fp32])."""
    B = c["B"] if B is None else B
    ceng.set_context((c["ctx"] if ctx is None else ctx).to(gpu), B, layerwise=True)
    ceng.control_set_hint(c["hint"].to(gpu))
    x = c["x"] if B == c["B"] else torch.cat([c["x"]] * (B // c["B"]))
    t = c["t"] if B == c["B"] else torch.cat([c["t"]] * (B // c["B"]))
    flat = ceng.control_forward(x.to(gpu), t.to(gpu), n_blocks)
    return flat, [r.permute(0, 3, 1, 2).float() for r in ceng.control_residuals(flat, B, c["H"], c["W"], n_blocks)]


# ======================================================================================================================
# 2. hint network and residuals
# ======================================================================================================================
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("form", ["b3_32x16", "b2_16x16"])
def test_control_residuals_against_the_reference(gpu, report, weights, refs, dtype, form):
    """control_set_hint + control_forward: every one of the 13 residuals within TOL of max|that reference residual|; one hint per
    sample on the ragged 32 x 16 batch of 3, a single shared hint on the batch of 2; a truncated run is the prefix, bit for bit."""
    c = refs[form]
    eng, ceng = _engines(dtype, weights)
    try:
        flat, got = _residuals(ceng, gpu, c)
        assert len(got) == 13 and flat.dtype == TORCH[dtype]
        errs = [_rel(g_, r) for g_, r in zip(got, c["res"])]
        for i, e in enumerate(errs):
            report(f"controlnet residual {i} {form} vs reference [{dtype}]", e, float(c["res"][i].abs().max()), TOL[dtype])
        assert max(errs) < TOL[dtype], errs
        flat2, _ = _residuals(ceng, gpu, c)
        assert torch.equal(flat, flat2)                                   # (nothing stale in the arena or the hint feature)
        part, _ = _residuals(ceng, gpu, c, n_blocks=3)
        assert torch.equal(part, flat[: part.numel()])
    finally:
        eng.close()
        ceng.close()


# ======================================================================================================================
# 3. the controlled U-Net
# ======================================================================================================================
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_controlled_unet_plain_and_twin(gpu, report, weights, refs, dtype):
    """Plain form (B = 3, 32 x 16) and twin form (B = 2, 16 x 16; both legs, then cond_only) with the distinct scales
    0.5 + 0.1 i, against the reference's controlled forward fed the reference's residuals.  cond_only: leg 1 is the uncontrolled
    twin forward's leg 1 bit for bit.  The stats report one add launch and n_in + 1 segments."""
    sd, csd = weights
    scales = R.case_scales(CFG)
    eng, ceng = _engines(dtype, weights)
    try:
        # plain
        c = refs["b3_32x16"]
        with torch.no_grad():
            ref = R.controlled_unet_forward(sd, CFG, c["x"], c["t"], c["ctx"], c["res"], scales)
            plain_ref = O.unet_forward(sd, CFG, c["x"], c["t"], c["ctx"])
        flat, _ = _residuals(ceng, gpu, c)
        eng.set_context(c["ctx"].to(gpu), 3, layerwise=True)
        eng.set_control(flat, scales, source=ceng, shape=(3, c["H"], c["W"]))
        eps = eng.unet_forward(c["x"].to(gpu), c["t"].to(gpu))
        assert eng.control_stats() == {"launches": 1, "segments": 13}
        e = _rel(eps, ref)
        report(f"controlnet controlled unet plain B=3 32x16 vs reference [{dtype}]", e, 1.0, TOL[dtype])
        report(f"controlnet (what ignoring control would measure there) [{dtype}]", _rel(eps, plain_ref), 1.0, TOL[dtype])
        assert e < TOL[dtype], e
        assert _rel(eps, plain_ref) > 10 * TOL["bf16"]
        eng.set_control(None)

        # twin, both legs: the control branch on [x; x] with [c; uc]
        c = refs["b2_16x16"]
        uc = torch.randn(c["ctx"].shape, generator=torch.Generator().manual_seed(9))
        x2, t2, ctx2 = torch.cat([c["x"]] * 2), torch.cat([c["t"]] * 2), torch.cat([c["ctx"], uc])
        with torch.no_grad():
            res2 = R.control_forward(csd, CFG, x2, t2, ctx2, c["hint"])
            ref_both = R.controlled_unet_forward(sd, CFG, x2, t2, ctx2, res2, scales)
            ref_cond = R.controlled_unet_forward(sd, CFG, x2, t2, ctx2, c["res"], scales, cond_only=True)
        eng.set_context(ctx2.to(gpu), 4, layerwise=True)
        off = eng.unet_forward_twin(c["x"].to(gpu), c["t"].to(gpu))
        flat2, _ = _residuals(ceng, gpu, c, ctx=ctx2, B=4)
        eng.set_control(flat2, scales, source=ceng, shape=(4, 16, 16))
        both = eng.unet_forward_twin(c["x"].to(gpu), c["t"].to(gpu))
        assert eng.control_stats() == {"launches": 1, "segments": 13}
        flat1, _ = _residuals(ceng, gpu, c)
        eng.set_control(flat1, scales, cond_only=True, source=ceng, shape=(2, 16, 16))
        cond = eng.unet_forward_twin(c["x"].to(gpu), c["t"].to(gpu))
        assert eng.control_stats() == {"launches": 1, "segments": 13}
        e_both, e_cond = _rel(both, ref_both), _rel(cond, ref_cond)
        report(f"controlnet controlled unet twin both legs vs reference [{dtype}]", e_both, 1.0, TOL[dtype])
        report(f"controlnet controlled unet twin cond_only vs reference [{dtype}]", e_cond, 1.0, TOL[dtype])
        assert e_both < TOL[dtype] and e_cond < TOL[dtype], (e_both, e_cond)
        assert torch.equal(cond[2:], off[2:])                             # the unconditional leg: bit for bit
        assert not torch.equal(cond[:2], off[:2]) and not torch.equal(both[2:], off[2:])
    finally:
        eng.close()
        ceng.close()


# ======================================================================================================================
# 4. off is free
# ======================================================================================================================
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_off_is_free(gpu, weights, refs, dtype):
    """eps before set_control and after set_control(None): equal bit for bit, the same launch counters, the same arena.  Outside
    the window the control handle's launch counters do not move."""
    from adaface_amd import _lib
    from ldm.modules.diffusionmodules.controlnet import ControlNet
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    c = refs["b2_16x16"]
    eng, ceng = _engines(dtype, weights)
    try:
        x, t = c["x"].to(gpu), c["t"].to(gpu)
        eng.set_context(c["ctx"].to(gpu), 2, layerwise=True)
        eng.unet_forward(x, t)
        arena = eng.arena_bytes()
        _counts()
        before = eng.unet_forward(x, t)
        pc_before = _counts()
        assert eng.control_stats() == {"launches": 0, "segments": 0}
        flat, _ = _residuals(ceng, gpu, c)
        eng.set_control(flat, R.case_scales(CFG), source=ceng, shape=(2, 16, 16))
        on = eng.unet_forward(x, t)
        eng.set_control(None)
        n_add = _lib.control_add_launches()
        _counts()
        after = eng.unet_forward(x, t)
        pc_after = _counts()
        assert torch.equal(before, after) and not torch.equal(before, on)
        assert pc_before == pc_after and _lib.control_add_launches() == n_add
        assert eng.control_stats() == {"launches": 0, "segments": 0} and eng.arena_bytes() == arena
    finally:
        eng.close()
        ceng.close()
    # the window, through the module: a timestep outside it runs no control kernel at all
    sd, csd = weights
    kw = dict(image_size=32, use_spatial_transformer=True, **{k: v for k, v in _unet_kwargs(CFG).items() if k != "n_context_layers"})
    unet = UNetModel(**kw)
    unet.load_state_dict({k[len(O.UNET_PREFIX):]: v for k, v in sd.items()})
    ckw = {k: v for k, v in kw.items() if k != "out_channels"}
    net = ControlNet(hint_channels=3, **ckw).load_control_state_dict(csd)
    unet.to(gpu).set_compute_dtype(dtype)
    net.to(gpu).set_compute_dtype(dtype)
    info = {"use_layerwise_context": True}
    ctx = c["ctx"].to(gpu)
    plain = unet(x, t, context=ctx, extra_info=dict(info))
    unet.set_control(net, c["hint"].to(gpu), scales=R.case_scales(CFG), t_range=(500, 999))
    inside = unet(x, torch.tensor([901, 650], device=gpu), context=ctx, extra_info=dict(info))
    n_add = _lib.control_add_launches()
    _counts()
    outside = unet(x, t, context=ctx, extra_info=dict(info))              # t = (901, 401): not every t is in the window
    torch.cuda.synchronize()
    pc = _counts()
    assert torch.equal(outside, plain) and _lib.control_add_launches() == n_add and pc == pc_before
    assert torch.isfinite(inside).all()
    unet.set_control(None)
    assert torch.equal(unet(x, t, context=ctx, extra_info=dict(info)), plain)


# ======================================================================================================================
# 5. DeepCache composition, 6. FreeU order
# ======================================================================================================================
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_with_deep_cache(gpu, report, weights, refs, dtype):
    """A refresh (full control) and a reuse step of depth 2 at another (x, t) against the reference composition.  The reuse
    step's control run stops after block 1 and its add has 2 segments."""
    sd, csd = weights
    scales = R.case_scales(CFG)
    c = refs["b2_16x16"]
    k = 2
    g = torch.Generator().manual_seed(77)
    x2 = c["x"] + 0.05 * torch.randn(c["x"].shape, generator=g)
    t2 = c["t"] - 20
    with torch.no_grad():
        ref_full, D = R.controlled_unet_forward(sd, CFG, c["x"], c["t"], c["ctx"], c["res"], scales, keep=k)
        res_k = R.control_forward(csd, CFG, x2, t2, c["ctx"], c["hint"], n_blocks=k)
        ref_reuse = R.controlled_unet_forward(sd, CFG, x2, t2, c["ctx"], res_k, scales, reuse=(D, k))
    eng, ceng = _engines(dtype, weights)
    try:
        eng.set_context(c["ctx"].to(gpu), 2, layerwise=True)
        ceng.set_context(c["ctx"].to(gpu), 2, layerwise=True)
        ceng.control_set_hint(c["hint"].to(gpu))
        _counts()
        flat = ceng.control_forward(c["x"].to(gpu), c["t"].to(gpu))
        pc_full = _counts()
        eng.set_control(flat, scales, source=ceng, shape=(2, 16, 16))
        full = eng.unet_forward_cached(c["x"].to(gpu), c["t"].to(gpu), depth=k, mode="refresh")
        assert eng.control_stats() == {"launches": 1, "segments": 13}
        _counts()
        flat_k = ceng.control_forward(x2.to(gpu), t2.to(gpu), n_blocks=k)
        pc_k = _counts()
        assert 0 < _gemms(pc_k) < _gemms(pc_full), (pc_k, pc_full)
        eng.set_control(flat_k, scales[:k], source=ceng, shape=(2, 16, 16))
        reuse = eng.unet_forward_cached(x2.to(gpu), t2.to(gpu), depth=k, mode="reuse")
        assert eng.control_stats() == {"launches": 1, "segments": k}
        e_full, e_reuse = _rel(full, ref_full), _rel(reuse, ref_reuse)
        report(f"controlnet + deepcache refresh vs reference [{dtype}]", e_full, 1.0, TOL[dtype])
        report(f"controlnet + deepcache reuse depth {k} vs reference [{dtype}]", e_reuse, 1.0, TOL[dtype])
        assert e_full < TOL[dtype] and e_reuse < TOL[dtype], (e_full, e_reuse)
    finally:
        eng.close()
        ceng.close()


def test_freeu_filters_the_controlled_skip(gpu, report, weights, refs):
    """FreeU after the residual add (the controlled skip is what gets filtered), against the reference composition, f32."""
    import freeu_ref
    sd, _ = weights
    scales = R.case_scales(CFG)
    c = refs["b2_16x16"]
    fu = (1,) + freeu_ref.V1_SD15
    with torch.no_grad():
        ref = R.controlled_unet_forward(sd, CFG, c["x"], c["t"], c["ctx"], c["res"], scales, freeu=fu)
        # the other order (filter, then add) is a different function on these inputs: the test can tell them apart
        no_fu = R.controlled_unet_forward(sd, CFG, c["x"], c["t"], c["ctx"], c["res"], scales)
    eng, ceng = _engines("f32", weights)
    try:
        flat, _ = _residuals(ceng, gpu, c)
        eng.set_context(c["ctx"].to(gpu), 2, layerwise=True)
        eng.set_freeu(*fu)
        eng.set_control(flat, scales, source=ceng, shape=(2, 16, 16))
        eps = eng.unet_forward(c["x"].to(gpu), c["t"].to(gpu))
        e = _rel(eps, ref)
        report("controlnet + FreeU v1 (controlled skip, then filter) vs reference [f32]", e, 1.0, TOL["f32"])
        assert e < TOL["f32"], e
        assert _rel(eps, no_fu) > 100 * TOL["f32"]
    finally:
        eng.close()
        ceng.close()


# ======================================================================================================================
# 7. samplers
# ======================================================================================================================
@pytest.fixture(scope="module")
def tiny_model(gpu, weights):
    from adaface_amd.configs import tiny_config
    from ldm.modules.diffusionmodules.controlnet import ControlNet
    from ldm.util import instantiate_from_config
    sd, csd = weights
    model = instantiate_from_config(tiny_config()["model"]).eval()
    full = dict(sd)
    full.update(O.synth_state_dict(O.vae_param_shapes(O.TINY_VAE), seed=12))
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected
    model = model.to(gpu).set_compute_dtype("f32")
    kw = dict(image_size=32, use_spatial_transformer=True, hint_channels=3,
              **{k: v for k, v in _unet_kwargs(CFG).items() if k not in ("n_context_layers", "out_channels")})
    net = ControlNet(**kw).load_control_state_dict(csd).to(gpu).set_compute_dtype("f32")
    return model, net


@pytest.fixture(scope="module")
def sampler_inputs():
    g = torch.Generator().manual_seed(41)
    return dict(x_T=torch.randn(1, 4, 16, 16, generator=g), c=torch.randn(16, 77, CFG.context_dim, generator=g),
                uc=torch.randn(16, 77, CFG.context_dim, generator=g), hint=torch.rand(1, 3, 128, 128, generator=g))


@pytest.mark.parametrize("case", ["ddim", "ddim-window", "dpmpp"])
def test_samplers_follow_the_reference(gpu, report, weights, tiny_model, sampler_inputs, case):
    """Four steps (timesteps 751, 501, 251, 1), f32, annealed guidance [10, 4], control set through UNetModel.set_control: DDIM
    and DPM-Solver++(2M) against the reference loops driving the reference's controlled forward; `ddim-window`: t_range =
    (500, 999) switches control off for the last two steps.  Bar 1e-3 of max|ref|, the drop-in sampler bar."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    sd, csd = weights
    model, net = tiny_model
    i = sampler_inputs
    window = (500, 999) if case == "ddim-window" else (0, 999)
    scales = R.case_scales(CFG)
    apply = R.ControlledApplyModel(sd, csd, CFG, i["hint"], scales, window)
    with torch.no_grad():
        if case == "dpmpp":
            ts = dpmpp_ref.uniform_grid(4)
            ref, _ = dpmpp_ref.sample_ref(apply, dpmpp_ref.sd_acp(), ts, i["x_T"], i["c"], i["uc"], O.guidance_schedule((10.0, 4.0), len(ts)))
        else:
            ref = O.ddim_sample(apply, O.register_schedule(), 4, i["x_T"], i["c"], i["uc"], guidance_scale=(10.0, 4.0))
    assert apply.log == ([True, True, False, False] if case == "ddim-window" else [True] * 4)
    unet = model.model.diffusion_model
    unet.set_control(net, i["hint"].to(gpu), scales=scales, t_range=None if window == (0, 999) else window)
    try:
        c, uc = model.get_learned_conditioning(i["c"].to(gpu)), model.get_learned_conditioning(i["uc"].to(gpu))
        smp = DPMSolverSampler(model) if case == "dpmpp" else DDIMSampler(model)
        lat, _ = smp.sample(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=[10.0, 4.0],
                            unconditional_conditioning=uc, x_T=i["x_T"].to(gpu), eta=0.0)
        unet.set_control(None)
        off, _ = smp.sample(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=[10.0, 4.0],
                            unconditional_conditioning=uc, x_T=i["x_T"].to(gpu), eta=0.0)
    finally:
        unet.set_control(None)
    err = float(np.abs(lat.cpu().numpy() - ref.numpy()).max() / np.abs(ref.numpy()).max())
    report(f"controlnet dropin sampler {case} 4 steps vs reference loop [f32]", err, float(ref.abs().max()), 1e-3)
    assert err < 1e-3, err
    assert _rel(off, ref) > 1e-2                                          # (the uncontrolled run is another trajectory)


# ======================================================================================================================
# 8. SD-1.5 widths
# ======================================================================================================================
SDW_CFG = O.UNetConfig(channel_mult=(1, 2, 4), num_res_blocks=1)      # 320 / 640 / 1280 channels, 8 heads x 40 / 80 / 160, 77 x 768


def test_sd15_widths(gpu, report):
    """model_channels = 320 (the hint ladder 3 -> 16 -> ... -> 256 -> 320, heads of 40 / 80 / 160, the 77 x 768 context), one
    8 x 8 latent with a 64 x 64 hint, B = 1 twin, bf16, on a three-level U-Net with one ResBlock per level (SD-1.5's widths and
    head sizes, not its depth, so that the CPU oracle stays quick).  Residuals and the controlled twin forward at TOL bf16."""
    cfg = SDW_CFG
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=13)
    csd = O.synth_state_dict(R.param_shapes(cfg), seed=33)
    g = torch.Generator().manual_seed(15)
    x, t = torch.randn(1, 4, 8, 8, generator=g), torch.tensor([731])
    ctx2 = torch.randn(2 * 16, 77, cfg.context_dim, generator=g)
    hint = torch.rand(1, 3, 64, 64, generator=g)
    n = R.n_residuals(cfg)
    scales = R.case_scales(cfg)
    x2, t2 = torch.cat([x, x]), torch.cat([t, t])
    with torch.no_grad():
        res = R.control_forward(csd, cfg, x2, t2, ctx2, hint)
        ref = R.controlled_unet_forward(sd, cfg, x2, t2, ctx2, res, scales)
        plain = O.unet_forward(sd, cfg, x2, t2, ctx2)
    eng, ceng = _engines("bf16", (sd, csd), cfg)
    try:
        ceng.set_context(ctx2.to(gpu), 2, layerwise=True)
        ceng.control_set_hint(hint.to(gpu))
        _counts()
        flat = ceng.control_forward(x2.to(gpu), t2.to(gpu))
        print("sd-width control forward plan counts:", _counts())
        got = [r.permute(0, 3, 1, 2).float() for r in ceng.control_residuals(flat, 2, 8, 8)]
        assert len(got) == n == 7 and [r.shape[1] for r in got] == [320, 320, 320, 640, 640, 1280, 1280]
        errs = [_rel(a, b) for a, b in zip(got, res)]
        for i, e in enumerate(errs):
            report(f"controlnet sd-width residual {i} vs reference [bf16]", e, float(res[i].abs().max()), TOL["bf16"])
        eng.set_context(ctx2.to(gpu), 2, layerwise=True)
        eng.set_control(flat, scales, source=ceng, shape=(2, 8, 8))
        eps = eng.unet_forward_twin(x.to(gpu), t.to(gpu))
        assert eng.control_stats() == {"launches": 1, "segments": n}
        e = _rel(eps, ref)
        report("controlnet sd-width controlled twin forward vs reference [bf16]", e, 1.0, TOL["bf16"])
        report("controlnet sd-width (what ignoring control would measure there) [bf16]", _rel(eps, plain), 1.0, TOL["bf16"])
        assert max(errs) < TOL["bf16"], errs
        assert e < TOL["bf16"], e
    finally:
        eng.close()
        ceng.close()


# ======================================================================================================================
# 9. refusals
# ======================================================================================================================
def test_refusals_happen_on_the_host(gpu, weights, refs):
    """cfg_pag / tgate with control, a dtype mismatch between the handles, a hint that is not 8 x the latent, a hint batch that is
    neither 1 nor B: each raises, and no kernel of any counted kind is launched by the refused call."""
    from adaface_amd import _lib
    from ldm.modules.diffusionmodules.controlnet import ControlNet
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    sd, csd = weights
    c = refs["b2_16x16"]
    kw = dict(image_size=32, use_spatial_transformer=True, **{k: v for k, v in _unet_kwargs(CFG).items() if k != "n_context_layers"})
    unet = UNetModel(**kw)
    unet.load_state_dict({k[len(O.UNET_PREFIX):]: v for k, v in sd.items()})
    net = ControlNet(hint_channels=3, **{k: v for k, v in kw.items() if k != "out_channels"}).load_control_state_dict(csd)
    unet.to(gpu).set_compute_dtype("f32")
    net.to(gpu).set_compute_dtype("f32")
    x, t, ctx = c["x"].to(gpu), c["t"].to(gpu), c["ctx"].to(gpu)
    info = {"use_layerwise_context": True}
    hint = c["hint"].to(gpu)
    unet.set_control(net, hint)
    unet(x, t, context=ctx, extra_info=dict(info))                        # (engines built, weights up: what follows launches nothing)
    unet.set_pag(["mid"])
    ctx_twin = torch.cat([ctx, ctx])

    def refused(exc, fn):
        torch.cuda.synchronize()
        before = (_lib.control_add_launches(), _counts(reset=False))
        with pytest.raises(exc):
            fn()
        torch.cuda.synchronize()
        assert (_lib.control_add_launches(), _counts(reset=False)) == before

    refused(NotImplementedError, lambda: unet(x, t, context=ctx_twin, extra_info=dict(info), cfg_pag=True))
    refused(NotImplementedError, lambda: unet(x, t, context=ctx, extra_info=dict(info), tgate="capture"))
    refused(NotImplementedError, lambda: unet(x, t, context=ctx, extra_info=dict(info), tgate="replay"))
    unet.set_pag(None)
    unet.set_control(net, torch.rand(1, 3, 128, 64, device=gpu))
    refused(ValueError, lambda: unet(x, t, context=ctx, extra_info=dict(info)))
    unet.set_control(net, torch.rand(3, 3, 128, 128, device=gpu))
    refused(ValueError, lambda: unet(x, t, context=ctx, extra_info=dict(info)))
    unet.set_control(net, hint)
    net.set_compute_dtype("bf16")
    refused(ValueError, lambda: unet(x, t, context=ctx, extra_info=dict(info)))
    net.set_compute_dtype("f32")
    # ... and below the module, on the handles themselves
    eng, ceng = _engines("f32", weights)
    eng16, _c16 = _engines("bf16", weights)
    try:
        flat, _ = _residuals(ceng, gpu, c)
        eng.set_context(ctx, 2, layerwise=True)
        refused(ValueError, lambda: eng16.set_control(flat, R.case_scales(CFG), source=ceng, shape=(2, 16, 16)))
        refused(ValueError, lambda: eng.set_control(flat, R.case_scales(CFG), source=_c16, shape=(2, 16, 16)))
        refused(ValueError, lambda: eng.set_control(flat[:100], R.case_scales(CFG), source=ceng, shape=(2, 16, 16)))
        eng.set_control(flat, R.case_scales(CFG), source=ceng, shape=(2, 16, 16))
        refused(_lib.AfError, lambda: eng.unet_forward(x, t, tgate="capture"))
        refused(_lib.AfError, lambda: eng.unet_forward(c["x"][:1].to(gpu), c["t"][:1].to(gpu)))          # the layout is for 2 samples
        eng.set_control(flat, R.case_scales(CFG)[:5], source=ceng, shape=(2, 16, 16))
        refused(_lib.AfError, lambda: eng.unet_forward(x, t))                                            # 5 residuals for a full forward
        eng.set_control(flat, R.case_scales(CFG), cond_only=True, source=ceng, shape=(2, 16, 16))
        refused(_lib.AfError, lambda: eng.unet_forward(x, t))                                            # cond_only on the plain form
        refused(_lib.AfError, lambda: ceng.unet_forward(x, t))                                           # a control handle has no decoder
        refused(ValueError, lambda: ceng.control_set_hint(torch.rand(1, 3, 100, 128, device=gpu)))       # sides % 8
        refused(_lib.AfError, lambda: ceng.control_forward(c["x"][:, :, :8].contiguous().to(gpu), t))    # the hint is for 16 x 16
        refused(_lib.AfError, lambda: ceng.set_fp8(True))                                                # fp8 on a control handle
    finally:
        for e in (eng, ceng, eng16, _c16):
            e.close()
