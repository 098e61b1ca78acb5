"""FeedForward scope of the fp8 mode (AF_FP8_SCOPE_FF): norm3 -> e4m3, GEGLU on the fp8 MFMA with e4m3 OUTPUT
(ff_geglu_fp8_kernel), ff.net.2 on the plain fp8 launch.  The reference has no fp8 path: the mode stays PARITY UNPINNED.

Kernel level (af_op_ff_fp8; every reference is a torch restatement on the SAME quantised operands, e4m3 emulated with
torch.float8_e4m3fn, per-row power-of-two weight scales restated as tests/test_fp8_gpu.py does):
  (a) exact probe of the GEGLU bytes: byte equality, no tolerance;
  (b) exact chain: those bytes through ff.net.2 with integer weights and residual, torch.equal against float64;
  (c) Gaussian operands: GEGLU bytes within half an e4m3 step (+ the GELU fit's and the fp32 accumulation's error) of the fp64
      reference, saturation exactly +-448; ff.net.2 within 5e-3 of the output scale of the product of the decoded operands;
  (d) the calibration record of the GEGLU output.
Model level (SD-1.5, synthetic weights, Bf = 16): (e) the scope switches cleanly, (f) the sites and launches of the wide
scope, (g) its accuracy against the f32-mode forward / chain of the same batch at the fp8 mode's stated bars.
"""
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests import exact_operands as X  # noqa: E402
from tests.test_fp8_gpu import FP8_FORWARD_TOL, _e4m3, _quant_w  # noqa: E402

pytestmark = pytest.mark.gpu

E4M3_MAX = 448.0
GELU_FIT_ERR = 1.9e-4          # max |x Phi(x) - gelu_bf16out_f2(x)| over all x (adaface_amd/csrc/af_common.h)


def _bytes(t):
    """float tensor of e4m3-representable values -> its OCP e4m3 bytes"""
    return t.to(torch.float8_e4m3fn).view(torch.uint8)


def _decode(b):
    return b.cpu().view(torch.float8_e4m3fn).double()


def _quant_w2d(w):
    return _quant_w(w[:, :, None, None])[:, :, 0, 0]


# ---------------------------------------------------------------------------------------------------------- (a) + (b)
def probe_operands(M, C, seed):
    """The exact probe of the issue: activation rows with 9-15 entries in {-1, +1} (as e4m3 bytes at shift 0), dense +-1
    value weights, zero gate weights, gate bias 8, value bias 0.  |value| <= 15; the GELU of af_common.h returns
    8 (1 + d), |d| <= 1.5e-5, far below e4m3's half step of 2^-4 relative, so the correct byte is the e4m3 code of
    value * 8 * 2^s whenever that number is representable."""
    g = torch.Generator().manual_seed(seed)
    Fn = 4 * C
    nnz = torch.randint(9, 16, (M,), generator=g)
    order = torch.rand(M, C, generator=g).argsort(dim=1)
    keep = order < nnz[:, None]
    x = torch.where(keep, torch.randint(0, 2, (M, C), generator=g).float() * 2 - 1, torch.zeros(M, C))   # (no -0.0)
    wv = torch.randint(0, 2, (Fn, C), generator=g).float() * 2 - 1
    w1 = torch.cat([wv, torch.zeros(Fn, C)], 0)
    b1 = torch.cat([torch.zeros(Fn), torch.full((Fn,), 8.0)], 0)
    value = x.double() @ wv.double().T + 0.0          # (+ 0.0: a zero is +0, as an fp32 accumulator that started at +0 holds it)
    return {"x": x, "w1": w1, "b1": b1, "value": value, "nnz": keep.sum(1)}


def check_probe_reference(p, shift):
    """Hard asserts on the reference alone; returns the expected bytes."""
    assert int(p["nnz"].min()) >= 9 and int(p["nnz"].max()) <= 15
    assert float(p["value"].abs().max()) <= 15.0
    ref = p["value"] * 8.0 * 2.0 ** shift
    assert float(ref.abs().max()) <= 240.0
    assert torch.equal(ref.float().to(torch.float8_e4m3fn).double(), ref), "value * 8 * 2^s is not exact in e4m3"
    nonzero = float((ref != 0).double().mean())
    distinct = int(torch.unique(ref).numel())
    assert nonzero >= 0.85, nonzero
    assert distinct >= 24, distinct
    return _bytes(ref.float()), nonzero, distinct


def chain_operands(mid, Cout, seed):
    """ff.net.2 on the decoded probe bytes `mid` [M, F] (integers, multiples of 8): weights in {-1, 0, 1}, integer bias and
    residual.  The activation operand is the probe's output and cannot be thinned (90 % non-zero, standard deviation
    8 sqrt(12) = 27.7), so the bf16-exactness of the result (8 significant bits: |sum| <= 256 * 8) is held by the weight
    density instead: K * share * 12 = 40^2 keeps the sum's standard deviation at 40 (x 8), 6.4 sigma inside the range over
    the 1.3 million outputs of the largest case, i.e. share = 128 / K (0.1 / 0.05 / 0.025 at K = 1280 / 2560 / 5120) -- below
    exact_operands.MIN_OPERAND_NONZERO, which assumes operands in {-1, 0, 1} on BOTH sides.  What is asserted for the
    weights in its place: every output sums at least 48 non-zero products (mean 0.9 x 128 = 115, five standard deviations
    of 10 below it, rounded down).  Every other condition of check_exact_case holds as it stands."""
    g = torch.Generator().manual_seed(seed)
    M, K = mid.shape
    share = min(0.3, 128.0 / K)
    w2 = (torch.randint(0, 2, (Cout, K), generator=g).float() * 2 - 1) * (torch.rand(Cout, K, generator=g) < share)
    b2 = X.int_tensor((Cout,), 1.0, g, -8, 8) * 8.0
    r = X.int_tensor((M, Cout), 1.0, g, -16, 16) * 8.0
    ref = X.fp64_ref_linear(mid, w2, b2, r)
    bound = X.absbound_linear(mid, w2, b2, r)
    stats = X.check_exact_case(ref, bound, "fp8", operands=(mid, w2, b2, r), power_operands=(mid, r))
    products = ((mid != 0).double() @ (w2 != 0).double().T).min().item()
    assert products >= 48, products
    return {"w2": w2, "b2": b2, "r": r, "ref": ref, "stats": stats}


@pytest.mark.parametrize("M,C,shift,want_splitk", [
    (2048, 320, 0, False), (2120, 320, 1, False),        # M a multiple of 256 / not
    (1024, 640, -2, False), (1100, 640, 0, False),
    (1024, 1280, 1, True), (1100, 1280, -2, True),       # K = 5120 for ff.net.2, planned over K slices
])
def test_ff_fp8_exact_probe_and_chain(gpu, report, knobs, M, C, shift, want_splitk):
    from adaface_amd import _lib, ops
    knobs("gemm_pp_minfill", 0)                      # (as the fp8 kernel tests: few rows would not fill half the chip)
    p = probe_operands(M, C, seed=M + C + shift + 16)
    want, nonzero, distinct = check_probe_reference(p, shift)
    mid_ref = p["value"] * 8.0                       # what ff.net.2 reads: bytes / 2^shift
    ch = chain_operands(mid_ref, C, seed=M + C + 5)
    x8 = _bytes(p["x"])
    _lib.plan_counts(reset=True)
    out = ops.ff_fp8(None, None, None, p["w1"].to(gpu), p["b1"].to(gpu), ch["w2"].to(gpu), ch["b2"].to(gpu),
                     residual=ch["r"].to(gpu), shift1=0, shift2=shift, x8=x8.to(gpu))
    pc = _lib.plan_counts(reset=True)
    assert pc["ff8"] == 1 and pc["fp8"] == 2, pc
    got = out["mid8"].cpu()
    n_bad = int((got != want).sum())
    print(f"[ff8 probe] M={M} C={C} shift={shift}: {nonzero:.3f} non-zero, {distinct} distinct values, {n_bad} bytes differ; "
          f"ff.net.2 plan {out['plan']}, reference stats {ch['stats']}")
    report(f"ff8 GEGLU exact probe [{M},{C}]x{4 * C} shift {shift}: bytes that differ", float(n_bad), float(want.numel()), 0.0)
    if n_bad:
        idx = (got != want).nonzero()
        first = "; ".join(f"{tuple(int(v) for v in c)}: got {int(got[tuple(c)]):#04x} want {int(want[tuple(c)]):#04x}" for c in idx[:8])
        box = ", ".join(f"axis {a}: [{int(idx[:, a].min())}, {int(idx[:, a].max())}]" for a in range(2))
        raise AssertionError(f"{n_bad} of {want.numel()} GEGLU bytes differ; first: {first}; bounding box: {box}")
    assert out["plan"][0] in (4, 5) and (out["plan"][1] > 1 or not want_splitk), out["plan"]
    X.assert_bit_exact(f"ff8 exact chain ff.net.2 [{M},{4 * C}]->{C} shift {shift}", out["y"], ch["ref"], plan=out["plan"], report=report)


# ------------------------------------------------------------------------------------------------------------- (c)
def _half_step(a):
    """half the e4m3 spacing at magnitude a (3 mantissa bits; subnormal spacing 2^-9)"""
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -6)))
    return torch.maximum(2.0 ** (e - 4), torch.full_like(a, 2.0 ** -10))


def gaussian_case(M, C, Cout, seed, spikes=False):
    g = torch.Generator().manual_seed(seed)
    Fn = 4 * C
    x = torch.randn(M, C, generator=g) * 2.0 + 0.3
    gamma = torch.randn(C, generator=g) * 0.3 + 1.0
    beta = torch.randn(C, generator=g) * 0.2
    xn = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    if spikes:
        at = torch.rand(M, C, generator=g) < 0.002
        xn = torch.where(at, xn + 25.0 * torch.sign(xn), xn)
    s1 = 3
    xq = _e4m3(xn * 2.0 ** s1) / 2.0 ** s1                      # the e4m3 operand the GEGLU reads, decoded
    w1 = torch.randn(2 * Fn, C, generator=g) / math.sqrt(C) * (0.5 + 2.0 * torch.rand(2 * Fn, 1, generator=g))
    b1 = torch.randn(2 * Fn, generator=g) * 0.1
    w2 = torch.randn(Cout, Fn, generator=g) / math.sqrt(Fn) * (0.5 + 2.0 * torch.rand(Cout, 1, generator=g))
    b2 = torch.randn(Cout, generator=g) * 0.1
    r = torch.randn(M, Cout, generator=g).to(torch.bfloat16).float()
    w1q, w2q = _quant_w2d(w1), _quant_w2d(w2)
    xd, wd = xq.double(), w1q.double()
    val = xd @ wd[:Fn].T + b1[:Fn].double()
    gate = xd @ wd[Fn:].T + b1[Fn:].double()
    f = val * F.gelu(gate)                                      # exact (erf) GELU in float64
    # fp32 accumulation over K products (any order): K * 2^-24 of sum |x||w| per pre-activation; through value * gelu(gate)
    # (|gelu'| <= 1.13) it moves f by at most |gelu(gate)| d_val + 1.13 |val| d_gate
    absb = xd.abs() @ wd.abs().T
    d_acc = C * 2.0 ** -24 * absb
    acc_term = F.gelu(gate).abs() * (d_acc[:, :Fn] + b1[:Fn].abs().double() * 2.0 ** -24) + \
        1.13 * val.abs() * (d_acc[:, Fn:] + b1[Fn:].abs().double() * 2.0 ** -24)
    # the GELU fit: 1.9e-4 absolute inside its +-4 clamp; beyond it the fit returns gate (1 + d), |d| <= 1.5e-5
    # (tests/exact_operands.py, GEGLU probes)
    slack = val.abs() * (GELU_FIT_ERR + 1.5e-5 * gate.abs()) + acc_term + f.abs() * 2.0 ** -22     # (+ the epilogue's own fp32 roundings)
    return {"xq": xq, "s1": s1, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "r": r, "w2q": w2q, "f": f, "slack": slack}


def check_geglu_bytes(got8, f, slack, s2):
    """got8 [M, F] bytes against the fp64 reference f at shift s2.  |got - clamp(f 2^s2)| <= half step + 2^s2 slack, and
    what lies beyond the range by more than the slack is exactly +-448.  Returns (worst excess, saturated count)."""
    got = _decode(got8)
    assert torch.isfinite(got).all()
    ref_s = f * 2.0 ** s2
    sl = slack * 2.0 ** s2
    refc = ref_s.clamp(-E4M3_MAX, E4M3_MAX)
    bound = _half_step(refc.abs() + sl) + sl
    excess = float(((got - refc).abs() - bound).max())
    sat = ref_s.abs() > E4M3_MAX + sl
    assert torch.equal(got[sat], torch.sign(ref_s[sat]) * E4M3_MAX)
    return excess, int(sat.sum())


@pytest.mark.parametrize("M,C,Cout", [(2048, 320, 320), (1100, 640, 640), (1024, 1280, 1280)])
def test_ff_fp8_gaussian_operands(gpu, report, knobs, M, C, Cout):
    from adaface_amd import ops
    knobs("gemm_pp_minfill", 0)
    c = gaussian_case(M, C, Cout, seed=M + C)
    amax = float(c["f"].abs().max())
    for s2 in (int(math.floor(math.log2(E4M3_MAX / amax))) - 1, int(math.floor(math.log2(E4M3_MAX / amax))) + 2):
        out = ops.ff_fp8(None, None, None, c["w1"].to(gpu), c["b1"].to(gpu), c["w2"].to(gpu), c["b2"].to(gpu),
                         residual=c["r"].to(gpu), shift1=c["s1"], shift2=s2, x8=_bytes(c["xq"] * 2.0 ** c["s1"]).to(gpu))
        excess, nsat = check_geglu_bytes(out["mid8"], c["f"], c["slack"], s2)
        print(f"[ff8 gaussian] M={M} C={C} s2={s2}: worst excess over the bound {excess:.3e}, {nsat} saturated references")
        report(f"ff8 GEGLU->e4m3 [{M},{C}] shift {s2}: worst excess over half an e4m3 step + fit + accumulation", max(excess, 0.0), 1.0, 0.0)
        assert excess <= 0.0, excess
        mid = _decode(out["mid8"]) / 2.0 ** s2
        ref = mid @ c["w2q"].double().T + c["b2"].double() + c["r"].double()
        scale = float(ref.abs().max())
        err = float((out["y"].cpu().double() - ref).abs().max())
        report(f"ff8 ff.net.2 [{M},{4 * C}]->{Cout} shift {s2} vs product of the decoded operands", err, scale, 5e-3 * scale)
        assert torch.isfinite(out["y"]).all() and err <= 5e-3 * scale, (err, scale)
    assert nsat > 0          # the second shift really saturates (amax * 2^s2 > 448 by construction)


# ------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("M,C", [(2048, 320), (1100, 640)])
def test_ff_fp8_record(gpu, report, knobs, M, C):
    from adaface_amd import ops
    knobs("gemm_pp_minfill", 0)

    def run(c, s2):
        return ops.ff_fp8(None, None, None, c["w1"].to(gpu), c["b1"].to(gpu), c["w2"].to(gpu), c["b2"].to(gpu),
                          residual=c["r"].to(gpu), shift1=c["s1"], shift2=s2, x8=_bytes(c["xq"] * 2.0 ** c["s1"]).to(gpu), record=True)

    c = gaussian_case(M, C, C, seed=M + C + 1)
    amax_ref = float((c["f"].abs() + c["slack"]).max())
    s2 = int(math.floor(math.log2(E4M3_MAX / amax_ref)))           # amax * 2^s2 <= 448: nothing saturates
    o1, o2 = run(c, s2), run(c, s2)
    assert o1["record"] == o2["record"] and torch.equal(o1["mid8"], o2["mid8"]) and torch.equal(o1["y"], o2["y"])
    amax, nsat = o1["record"]
    got = _decode(o1["mid8"])
    assert math.isfinite(amax) and nsat == 0, (amax, nsat)
    # no byte is +-448 unless its reference rounds there
    at_max = got.abs() == E4M3_MAX
    assert bool(((c["f"].abs() * 2.0 ** s2 + c["slack"] * 2.0 ** s2)[at_max] >= 416.0).all())
    assert amax >= float(got.abs().max()) / 2.0 ** s2 * (1 - 2.0 ** -4), (amax, float(got.abs().max()))
    assert abs(amax - float(c["f"].abs().max())) <= float(c["slack"].max()) + 1e-6 * amax_ref
    report(f"ff8 record [{M},{C}]: |amax - reference| / reference", abs(amax - float(c["f"].abs().max())) / amax_ref, 1.0)
    # spikes in the GEGLU's input at the shift calibrated WITHOUT them: some outputs saturate, and the record says so
    sp = gaussian_case(M, C, C, seed=M + C + 1, spikes=True)
    n_over = int((sp["f"].abs() * 2.0 ** s2 > E4M3_MAX + sp["slack"] * 2.0 ** s2).sum())
    assert n_over > 0, "the spiked case does not leave the range: no test of the saturation count"
    o3, o4 = run(sp, s2), run(sp, s2)
    assert o3["record"] == o4["record"] and torch.equal(o3["mid8"], o4["mid8"])
    amax3, nsat3 = o3["record"]
    got3 = _decode(o3["mid8"])
    assert torch.isfinite(got3).all() and torch.isfinite(o3["y"]).all() and math.isfinite(amax3)
    n448 = int((got3.abs() == E4M3_MAX).sum())
    print(f"[ff8 record] M={M} C={C} s2={s2}: amax {amax:.4f} (reference {float(c['f'].abs().max()):.4f}); spiked: amax {amax3:.3f}, "
          f"nsat {nsat3}, bytes at +-448 {n448}, references beyond the range {n_over}")
    assert 0 < nsat3 <= n448, (nsat3, n448)
    assert nsat3 >= n_over


# ----------------------------------------------------------------------------------------------------------- model
def _sd15_inputs(gpu):
    from oracle import ldm_oracle as O
    cfg = O.SD15_UNET
    g = torch.Generator().manual_seed(52)
    x = torch.randn(16, 4, 64, 64, generator=g).to(gpu)
    t = torch.full((16,), 501, dtype=torch.long, device=gpu)
    ctx = torch.randn(16 * 16, 77, cfg.context_dim, generator=g).to(gpu)
    return cfg, x, t, ctx


def _sd15_engine(gpu, mode, ctx):
    from oracle import ldm_oracle as O
    from adaface_amd.engine import Engine
    from adaface_amd.synth import synth_weights_into
    from tests.test_model_gpu import _unet_kwargs
    eng = Engine(dtype=mode, unet=_unet_kwargs(O.SD15_UNET))
    synth_weights_into(eng, O.unet_param_shapes(O.SD15_UNET), seed=51, device=gpu)
    eng.set_context(ctx, 16, layerwise=True)
    return eng


# transformer blocks of the SD-1.5 UNet by level (checkpoint prefixes).  The issue asks for the ten blocks of the 64x64 and 32x32
# levels on the path AND for a level to stay in the scope only if its fp8 pair (LayerNorm pass included) is not slower than
# the bf16 pair.  Measured (scripts/bench_shapes.py --only ff8, profiles/ff8_a0c7710.txt): 64x64 223 us against 192 us -- out, by
# the rule "C >= 512" (AfKnobs::ff8_min_k); 32x32 1.16x, 16x16 1.47x, 8x8 1.32x -- in.  So the path is these eleven blocks.
LEVEL_BLOCKS = {
    64: ("input_blocks.1.1", "input_blocks.2.1", "output_blocks.9.1", "output_blocks.10.1", "output_blocks.11.1"),
    32: ("input_blocks.4.1", "input_blocks.5.1", "output_blocks.6.1", "output_blocks.7.1", "output_blocks.8.1"),
    16: ("input_blocks.7.1", "input_blocks.8.1", "output_blocks.3.1", "output_blocks.4.1", "output_blocks.5.1"),
    8: ("middle_block.1",),
}


def _ff_blocks(names):
    """{block prefix: [its ff site names]} of the sites behind the 60 base ones"""
    out = {}
    for n in names[60:]:
        key = n.split(".transformer_blocks.")[0].split("diffusion_model.")[-1]
        out.setdefault(key, []).append(n)
    return out


def test_sd15_unet_ff_scope_sites_launches_and_switches(gpu, report, tmp_path):
    """(e) scope on, then off: today's fp8 forward bit for bit, 59 launches, the 60 site names as before; fp8 off: bf16 bit
    for bit.  (f) scope on: 92 unique sites, the first 60 the old list, ff8 launches = blocks on the path, fp8 launches =
    59 + 2 x that, both sites of every block on the path reached and no block with one; the path is the eleven blocks of the
    32x32, 16x16 and 8x8 levels (LEVEL_BLOCKS: the 64x64 level measured slower than bf16 and stays there by rule)."""
    from adaface_amd import _lib
    from adaface_amd.fp8_calib import load_scales, save_scales
    cfg, x, t, ctx = _sd15_inputs(gpu)
    eng = _sd15_engine(gpu, "bf16", ctx)
    bf16 = eng.unet_forward(x, t)
    eng.set_fp8(True)
    assert eng.fp8_scope == ("base",)
    names60 = eng.fp8_site_names()
    assert len(names60) == 60
    _lib.plan_counts(reset=True)
    base = eng.unet_forward(x, t)
    pc = _lib.plan_counts(reset=True)
    assert pc["fp8"] == 59 and pc["ff8"] == 0, pc
    # ---- scope on
    eng.set_fp8(True, scope=("base", "ff"))
    assert eng.fp8_scope == ("base", "ff")
    names = eng.fp8_site_names()
    assert len(names) == 92 and len(set(names)) == 92 and names[:60] == names60
    assert sum(n.endswith(".ff.net.0.proj.weight") for n in names[60:]) == 16 and sum(n.endswith(".ff.net.2.weight") for n in names[60:]) == 16
    assert set(eng.fp8_shifts().values()) == {3} and len(eng.fp8_shifts()) == 92
    _lib.plan_counts(reset=True)
    with eng.fp8_record():
        wide = eng.unet_forward(x, t)
        rec = eng.fp8_read_record()
    pc = _lib.plan_counts(reset=True)
    assert torch.isfinite(wide).all() and not torch.equal(wide, base)
    blocks = _ff_blocks(names)
    assert len(blocks) == 16 and all(len(v) == 2 for v in blocks.values())
    reached = {k: [rec[n][0] > 0.0 for n in v] for k, v in blocks.items()}
    assert all(all(v) or not any(v) for v in reached.values()), reached          # a block takes the path as a unit
    on_path = sorted(k for k, v in reached.items() if all(v))
    print(f"[ff8 model] blocks on the FeedForward path: {len(on_path)}: {on_path}; plan counts {pc}")
    assert pc["ff8"] == len(on_path) and pc["fp8"] == 59 + 2 * len(on_path), (pc, on_path)
    assert on_path == sorted(LEVEL_BLOCKS[32] + LEVEL_BLOCKS[16] + LEVEL_BLOCKS[8]), on_path
    assert not any(any(reached[b]) for b in LEVEL_BLOCKS[64])
    assert sum(rec[n][0] > 0.0 for n in names60) == 59                            # the base sites are reached as before
    assert torch.equal(eng.unet_forward(x, t), wide)                              # recording changes nothing
    # the twin forward goes through the same sites
    with eng.fp8_record():
        eng.unet_forward_twin(x[:8].contiguous(), t[:8].contiguous())
        rec_twin = eng.fp8_read_record()
    assert {n for n, (a, _) in rec_twin.items() if a > 0.0} == {n for n, (a, _) in rec.items() if a > 0.0}
    # scale files belong to their scope: a 60-site file is refused under the wide scope and the other way round
    p60, p92 = tmp_path / "s60.json", tmp_path / "s92.json"
    save_scales(p60, {n: 3 for n in names60})
    save_scales(p92, {n: 3 for n in names})
    with pytest.raises(KeyError):
        load_scales(p60, eng.fp8_site_names())
    assert load_scales(p92, eng.fp8_site_names()) == {n: 3 for n in names}
    # calibration covers the new sites
    cal = eng.calibrate_fp8(lambda: eng.unet_forward(x, t), passes=2, headroom=1)
    assert len(cal) == 92 and all(k == 0 for _, _, k in cal.values())
    assert all(cal[n][0] > 0.0 for b in on_path for n in blocks[b])
    assert all(cal[n] == (0.0, 3, 0) for b in LEVEL_BLOCKS[64] for n in blocks[b])    # never reached: the default shift stays
    eng.set_fp8_shifts(None)
    # ---- scope off again
    eng.set_fp8(True, scope=("base",))
    assert eng.fp8_site_names() == names60 and len(eng.fp8_shifts()) == 60
    with pytest.raises(KeyError):
        load_scales(p92, eng.fp8_site_names())
    _lib.plan_counts(reset=True)
    again = eng.unet_forward(x, t)
    pc = _lib.plan_counts(reset=True)
    assert pc["fp8"] == 59 and pc["ff8"] == 0, pc
    assert torch.equal(again, base)
    eng.set_fp8(False)
    assert torch.equal(eng.unet_forward(x, t), bf16)
    # masks without BASE are refused; f32 handles refuse the scope
    with pytest.raises(ValueError):
        eng.set_fp8(True, scope=("ff",))
    with pytest.raises(_lib.AfError):
        _lib.check(eng._lib.af_set_fp8_scope(eng._h, 2), "af_set_fp8_scope")
    eng.close()
    e32 = _sd15_engine(gpu, "f32", ctx)
    with pytest.raises(_lib.AfError):
        _lib.check(e32._lib.af_set_fp8_scope(e32._h, 3), "af_set_fp8_scope")
    e32.close()


def test_sd15_unet_ff_scope_forward_accuracy(gpu, report):
    """(g), per forward: calibrated (two passes, headroom 1) wide scope against the f32-mode forward of the same batch, at the
    fp8 mode's stated bar (8e-2 of max|eps|); the rms ratio beside it; the base scope's numbers of the same run printed."""
    cfg, x, t, ctx = _sd15_inputs(gpu)
    e32 = _sd15_engine(gpu, "f32", ctx)
    f32 = e32.unet_forward(x, t)
    e32.close()
    eng = _sd15_engine(gpu, "bf16", ctx)
    scale, rms32 = f32.abs().max().item(), f32.double().pow(2).mean().sqrt().item()
    fig = {}
    for scope in (("base",), ("base", "ff")):
        eng.set_fp8(True, scope=scope)
        eng.set_fp8_shifts(None)
        cal = eng.calibrate_fp8(lambda: eng.unet_forward(x, t), passes=2, headroom=1)
        assert all(k == 0 for _, _, k in cal.values())
        out = eng.unet_forward(x, t)
        assert torch.isfinite(out).all()
        d = (out - f32).double()
        fig[scope] = (d.abs().max().item() / scale, d.pow(2).mean().sqrt().item() / rms32)
        what = "+".join(scope)
        print(f"[ff8 accuracy] forward, scope {what}, calibrated: max-abs {fig[scope][0]:.3e} of max|eps|, rms ratio {fig[scope][1]:.3e}")
        report(f"sd15_unet Bf=16 fp8 scope {what} calibrated forward vs f32-mode forward (max-abs / max|eps|)", fig[scope][0], scale, FP8_FORWARD_TOL)
        report(f"sd15_unet Bf=16 fp8 scope {what} calibrated forward vs f32-mode forward (rms / rms)", fig[scope][1], rms32, FP8_FORWARD_TOL)
    eng.close()
    e_max, e_rms = fig[("base", "ff")]
    assert e_rms <= FP8_FORWARD_TOL, e_rms
    assert e_max <= FP8_FORWARD_TOL, e_max


@pytest.fixture(scope="module")
def bench_model(gpu):
    from bench import build_model
    return build_model(gpu, "f32")


# the three contexts of tests/test_chained_gpu.py (BASELINE configs 1 / 2 / 4), restated
@pytest.mark.parametrize("workload", ["config1", "config2", "config4"])
def test_config1_shape_chained_error_ff_scope_vs_f32(gpu, report, bench_model, workload):
    """(g), chained: config 1's shape (batch 8 -> CFG batch 16, S = 10 DDIM steps, guidance [10, 4]) in the calibrated wide
    scope against the f32 mode of the same batch, at the fp8 bars of tests/test_chained_gpu.py: first forward <= 8e-2, final
    latent <= 1e-1, rms <= 1e-1, chain gain <= 2.5.  The base scope's numbers of the same run are printed beside them."""
    from adaface_amd import synth
    from adaface_amd.synth import synth_context
    from ldm.models.diffusion.ddim import DDIMSampler
    FWD_BAR, FINAL_BAR, FINAL_RMS_BAR, CHAIN_GAIN = 8e-2, 1e-1, 1e-1, 2.5
    B, S = 8, 10
    model = bench_model
    g = torch.Generator().manual_seed(42)
    x_T = torch.randn(B, 4, 64, 64, generator=g).to(gpu)
    make_ctx = {"config1": synth.synth_context, "config2": synth.synth_context_adaprompt, "config4": synth.synth_context_identity}[workload]
    c_emb = make_ctx(B, seed=100, device=gpu)
    uc_emb = synth_context(B, seed=101, device=gpu, shared=True)
    sampler = DDIMSampler(model)
    t0 = torch.full((B,), 901, dtype=torch.long, device=gpu)

    def chain():
        c = model.get_learned_conditioning(c_emb)
        uc = model.get_learned_conditioning(uc_emb)
        eps_c = model.apply_model(x_T, t0, c)
        lat, _ = sampler.sample(S=S, conditioning=c, batch_size=B, shape=[4, 64, 64], verbose=False,
                                guidance_scale=[10.0, 4.0], unconditional_conditioning=uc, eta=0.0, x_T=x_T)
        torch.cuda.synchronize()
        assert torch.isfinite(lat).all() and torch.isfinite(eps_c).all()
        return eps_c.clone(), lat.clone()

    model.set_compute_dtype("f32")
    out = {"f32": chain()}
    for scope in ("base", "base+ff"):
        model.set_compute_dtype("fp8", fp8_scope=scope)
        cal = model.calibrate_fp8(model.get_learned_conditioning(c_emb), model.get_learned_conditioning(uc_emb), shape=[4, 64, 64],
                                  batch_size=B, S=S, guidance_scale=[10.0, 4.0], x_T=x_T, passes=2, headroom=1)
        assert len(cal) == (60 if scope == "base" else 92) and all(k == 0 for _, _, k in cal.values())
        out[scope] = chain()
    model.set_compute_dtype("f32")
    e_scale, l_scale = out["f32"][0].abs().max().item(), out["f32"][1].abs().max().item()
    l_rms = out["f32"][1].double().pow(2).mean().sqrt().item()
    fig = {}
    for scope in ("base", "base+ff"):
        e1 = (out[scope][0] - out["f32"][0]).abs().max().item() / e_scale
        ef = (out[scope][1] - out["f32"][1]).abs().max().item() / l_scale
        erms = (out[scope][1] - out["f32"][1]).double().pow(2).mean().sqrt().item() / l_rms
        fig[scope] = (e1, ef, erms)
        print(f"[ff8 chained] {workload} scope {scope} calibrated: first forward {e1:.3e}, final {ef:.3e}, rms {erms:.3e}, gain {ef / e1:.2f}")
        report(f"{workload} shape Bf=16: first-forward eps fp8 scope {scope} calibrated vs f32 mode", e1, e_scale, FWD_BAR)
        report(f"{workload} shape Bf=16: final latent after S=10 DDIM steps fp8 scope {scope} calibrated vs f32 mode", ef, l_scale, FINAL_BAR)
        report(f"{workload} shape Bf=16: final latent after S=10 DDIM steps fp8 scope {scope} calibrated vs f32 mode, rms / rms", erms, l_rms, FINAL_RMS_BAR)
    e1, ef, erms = fig["base+ff"]
    assert erms <= FINAL_RMS_BAR, erms
    assert e1 <= FWD_BAR, e1
    assert ef <= FINAL_BAR, ef
    assert ef <= CHAIN_GAIN * e1, (ef, e1)
    assert not torch.equal(out["base+ff"][1], out["base"][1])
