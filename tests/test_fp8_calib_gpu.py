"""Calibrated per-site activation scales of the fp8 mode (af_fp8_* in include/adaface_hip.h) on the GPU.

  operators: the four e4m3 producers with a record (amax, saturated count) at shifts -3 / 0 / 3 / 6; the outlier tensor of
             test_fp8_gpu.py::test_fp8_outlier_channels_saturate_at_56 with the shift its record derives (nothing clips any
             more); the fp8 convolution at other activation shifts;
  model:     invariants of the SD-1.5 UNet (recording changes nothing, shifts reset / save / load, launch counts, the twin
             forward), the user story (weights with outlier channels: the fixed 2^3 breaks the fp8 bar, calibration restores
             it), the chained DDIM run in calibrated fp8, the drop-in classes.
The fp8 mode stays PARITY UNPINNED (the reference computes nothing in fp8); the bars are this package's stated ones.
"""
import math
import struct
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests.test_fp8_gpu import FP8_FORWARD_TOL, _e4m3, _quant_w  # noqa: E402

pytestmark = pytest.mark.gpu

SHIFTS = (-3, 0, 3, 6)
# |amax(kernel) - amax(torch fp32)| / amax(torch): the kernels use exp2 / rcp of the fast transcendental unit and fold
# gamma * rstd before the multiply.  Worst measured over the 32 cases below: see DESIGN.md section 2 (j); the bar is four times
# that, and never looser than 1e-3.  That is about five fp32 ulps, as the bar's rule gives it: a compiler or library change
# that reorders the fused multiply-adds of the affine map or of torch's reference can move the maximum by a few ulps and trip
# this bar with nothing wrong in the record; re-measure before concluding anything else.
AMAX_REL_BAR = 4 * 1.563e-7


def _bits(f):
    return struct.unpack("I", struct.pack("f", f))[0]


def _shift_ref(amax, headroom):
    if not (amax > 0.0) or math.isinf(amax):
        return 3
    m, e = math.frexp(amax)
    return max(-16, min(8, 9 - e - (1 if m > 0.875 else 0) - headroom))


def _half_step_bound(refc, s):
    """Half an e4m3 step around refc (already clamped to +-448 / 2^s): 2^-4 relative, 2^-10 / 2^s absolute in the subnormal
    range, plus the kernels' f32 rounding -- the bound of test_fp8_gpu.py's producer tests with 2^s in place of 2^3."""
    return refc.abs() * (2.0 ** -4) * 1.02 + 2.0 ** -10 / 2.0 ** s + 2e-4


def _check_reference_margins(y, s):
    """The conditions the exact comparisons below rest on, asserted on the torch reference: no element within 1 % of the
    saturation threshold, and 448 / amax more than 1 % away from a power of two."""
    thr = 448.0 / 2.0 ** s
    a = y.abs()
    assert int(((a > thr * 0.99) & (a < thr * 1.01)).sum()) == 0, ("element within 1 % of the threshold", s)
    frac = math.log2(448.0 / a.max().item()) % 1.0
    assert min(frac, 1.0 - frac) > math.log2(1.01), ("448 / amax within 1 % of a power of two", a.max().item())


# seeds chosen (on the CPU, from the torch reference alone) so that _check_reference_margins holds for every shift
GN_CASES = [(2, 320, 64, 64, True, 0), (2, 1280, 8, 8, True, 0), (1, 640, 32, 32, False, 1), (1, 2560, 16, 16, True, 0)]
# LayerNorm: af_launch_layernorm takes layernorm_rowgroup_kernel for bf16 when C / 64 <= 10 and rows >= 8192 (256 workgroups of
# 32 rows), else the wave-per-row layernorm_kernel.  The four shapes of test_layernorm_fp8_output all run the latter (130 rows:
# its ragged last workgroup); (8192, 320) and (8200, 640) run the row-group kernel, 8200 rows with a last workgroup of 8 live rows.
LN_CASES = [(4096, 320, 8), (1024, 640, 0), (256, 1280, 0), (130, 1280, 0), (8192, 320, 4), (8200, 640, 29)]


def _spiked(x, sigma, g, n=40):
    """The inputs of the existing producer tests plus n isolated spikes of 10 .. 120 sigma, either sign: normalised values
    far out in the tail, few enough that the 1 % bands around the thresholds stay empty, so that the saturated counts at
    shifts 3 and 6 are not trivially zero."""
    idx = torch.randperm(x.numel(), generator=g)[:n]
    amp = sigma * (10.0 + 110.0 * torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    x.view(-1)[idx] += amp
    return x


def _gn_inputs(B, C, H, W, silu, seed):
    g = torch.Generator().manual_seed(1000 * seed + C + H)
    x = _spiked(torch.randn(B, C, H, W, generator=g) * 1.7 + 0.4, 1.7, g).to(torch.bfloat16).float()
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    ref = F.group_norm(x, 32, w, b, 1e-5)
    if silu:
        ref = F.silu(ref)
    return x, w, b, ref


def _ln_inputs(rows, C, seed):
    g = torch.Generator().manual_seed(1000 * seed + rows + C)
    x = _spiked(torch.randn(rows, C, generator=g) * 2.0 + 0.3, 2.0, g).to(torch.bfloat16).float()
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    return x, w, b, F.layer_norm(x, (C,), w, b, 1e-5)


def _check_record(report, what, ref, got, rec, rec2, s):
    amax, nsat = rec
    thr = 448.0 / 2.0 ** s
    refc = ref.clamp(-thr, thr)
    excess = ((got - refc).abs() - _half_step_bound(refc, s)).max().item()
    ref_amax = ref.abs().max().item()
    rel = abs(amax - ref_amax) / ref_amax
    ref_nsat = int((ref.abs() > thr).sum())
    print(f"[fp8 record] {what} shift {s}: amax {amax:.6f} ref {ref_amax:.6f} rel {rel:.3e}; nsat {nsat} ref {ref_nsat}; "
          f"half-step excess {excess:.3e}")
    report(f"{what} shift {s}: recorded amax vs torch fp32 (relative)", rel, ref_amax, AMAX_REL_BAR)
    assert torch.isfinite(got).all() and excess <= 0.0, excess
    assert rel <= AMAX_REL_BAR, (amax, ref_amax, rel)
    assert nsat == ref_nsat, (nsat, ref_nsat)
    for headroom in (0, 1):
        assert _shift_ref(amax, headroom) == _shift_ref(ref_amax, headroom)
    assert _bits(rec2[0]) == _bits(amax) and rec2[1] == nsat          # bit-reproducible run to run


@pytest.mark.parametrize("B,C,H,W,silu,seed", GN_CASES)
def test_groupnorm_fp8_record(gpu, report, B, C, H, W, silu, seed):
    """Both GroupNorm kernels (chunked apply / small-map single launch) with the record, shifts -3 / 0 / 3 / 6."""
    from adaface_amd import ops
    x, w, b, ref = _gn_inputs(B, C, H, W, silu, seed)
    xg, wg, bg = x.to(gpu), w.to(gpu), b.to(gpu)
    for s in SHIFTS:
        _check_reference_margins(ref, s)
        y8, rec = ops.group_norm_fp8(xg, wg, bg, eps=1e-5, silu=silu, act_shift=s, record=True)
        y8b, rec2 = ops.group_norm_fp8(xg, wg, bg, eps=1e-5, silu=silu, act_shift=s, record=True)
        plain = ops.group_norm_fp8(xg, wg, bg, eps=1e-5, silu=silu, act_shift=s)
        assert torch.equal(y8, y8b) and torch.equal(y8, plain)          # recording never changes what is written
        got = y8.cpu().view(torch.float8_e4m3fn).float().view(B, H * W, C).permute(0, 2, 1).reshape(B, C, H, W) / 2.0 ** s
        _check_record(report, f"groupnorm->e4m3 C{C} {H}x{W}", ref, got, rec, rec2, s)


@pytest.mark.parametrize("rows,C,seed", LN_CASES)
def test_layernorm_fp8_record(gpu, report, rows, C, seed):
    """Both LayerNorm kernels with the record: the wave-per-row kernel (rows < 8192; 130 rows: ragged last workgroup) and the
    row-group kernel (8192 rows; 8200 rows: lanes past the last row stay for the workgroup reduction and must add nothing)."""
    from adaface_amd import ops
    x, w, b, ref = _ln_inputs(rows, C, seed)
    xg, wg, bg = x.to(gpu), w.to(gpu), b.to(gpu)
    for s in SHIFTS:
        _check_reference_margins(ref, s)
        y8, rec = ops.layer_norm_fp8(xg, wg, bg, act_shift=s, record=True)
        y8b, rec2 = ops.layer_norm_fp8(xg, wg, bg, act_shift=s, record=True)
        plain = ops.layer_norm_fp8(xg, wg, bg, act_shift=s)
        assert torch.equal(y8, y8b) and torch.equal(y8, plain)
        got = y8.cpu().view(torch.float8_e4m3fn).float() / 2.0 ** s
        _check_record(report, f"layernorm->e4m3 [{rows},{C}]", ref, got, rec, rec2, s)


def test_fp8_ops_refuse_shifts_outside_the_range(gpu):
    from adaface_amd import _lib, ops
    x = torch.randn(1, 64, 8, 8).to(gpu)
    w = torch.ones(64).to(gpu)
    for s in (-17, 9):
        with pytest.raises(_lib.AfError):
            ops.group_norm_fp8(x, w, w, act_shift=s)
        with pytest.raises(_lib.AfError):
            ops.layer_norm_fp8(x.reshape(64, 64), w, w, act_shift=s, record=True)
        with pytest.raises(_lib.AfError):
            ops.conv2d_fp8(torch.randn(2, 64, 32, 32).to(gpu), torch.randn(128, 64, 3, 3).to(gpu), act_shift=s)


def test_fp8_outlier_channels_calibrated_do_not_saturate(gpu, report, knobs):
    """The heavy-tailed tensor of test_fp8_gpu.py::test_fp8_outlier_channels_saturate_at_56 (same seed, same construction):
    at the fixed shift 3 the record counts exactly the elements beyond +-56; at the shift the record derives (headroom 1)
    nothing saturates, the producer is within half a step of the UNCLAMPED result, and the convolution of it is within the
    quantisation bound of the unclamped bf16-operand convolution -- the existing test's bound without its clipped-excess term."""
    from adaface_amd import _lib, ops
    knobs("gemm_pp_minfill", 0)
    g = torch.Generator().manual_seed(99)
    B, C, H, W, Cout = 2, 320, 32, 32, 320
    x = torch.randn(B, C, H, W, generator=g)
    chans = (7, 45, 99, 141, 203, 300)
    spikes = torch.rand(B, len(chans), H, W, generator=g) < 0.002
    for i, ch in enumerate(chans):
        x[:, ch] += spikes[:, i] * (150.0 + 250.0 * torch.rand(B, H, W, generator=g)) * (-1 if ch == 99 else 1)
    x = x.to(torch.bfloat16).float()
    gamma = torch.randn(C, generator=g) * 0.2 + 1.0
    beta = torch.randn(C, generator=g) * 0.1
    y = F.silu(F.group_norm(x, 32, gamma, beta, 1e-5))
    n_clip = int((y.abs() > 56.0).sum())
    assert y.abs().max() > 80.0 and n_clip >= 5, (n_clip, y.abs().max().item())
    _check_reference_margins(y, 3)
    xg, gg, bg = x.to(gpu), gamma.to(gpu), beta.to(gpu)
    # fixed scale: the record says what clipped
    _, (amax3, nsat3) = ops.group_norm_fp8(xg, gg, bg, eps=1e-5, silu=True, act_shift=3, record=True)
    assert nsat3 == n_clip, (nsat3, n_clip)
    rel = abs(amax3 - y.abs().max().item()) / y.abs().max().item()
    print(f"[fp8 record] outlier tensor: amax {amax3:.6f} ref {y.abs().max().item():.6f} rel {rel:.3e}; nsat {nsat3} ref {n_clip}")
    assert rel <= AMAX_REL_BAR, rel
    s = _lib.load().af_fp8_shift_for_amax(amax3, 1)
    assert s == _shift_ref(y.abs().max().item(), 1) and s < 3, s
    _check_reference_margins(y, s)
    # derived scale: nothing clips, the bytes follow the unclamped tensor
    y8, (amax_s, nsat_s) = ops.group_norm_fp8(xg, gg, bg, eps=1e-5, silu=True, act_shift=s, record=True)
    assert nsat_s == 0 and _bits(amax_s) == _bits(amax3)
    got = y8.cpu().view(torch.float8_e4m3fn).float().view(B, H * W, C).permute(0, 2, 1).reshape(B, C, H, W) / 2.0 ** s
    excess = ((got - y).abs() - _half_step_bound(y, s)).max().item()
    report(f"fp8 outlier channels at the derived shift {s}: worst excess over half an e4m3 step of the unclamped tensor", max(excess, 0.0), 1.0, 0.0)
    assert torch.isfinite(got).all() and excess <= 0.0, excess
    # consumer: same-operand reference at that shift, kernel bar
    w = torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(C * 9)
    out8 = ops.conv2d_fp8(y.to(gpu), w.to(gpu), act_shift=s).cpu()
    yq = _e4m3(y.to(torch.bfloat16).float() * 2.0 ** s) / 2.0 ** s
    ref_q = F.conv2d(yq.double(), _quant_w(w).double(), padding=1).float()
    scale = ref_q.abs().max().item()
    e_b = (out8 - ref_q).abs().max().item()
    report(f"fp8 conv of the outlier tensor at shift {s} vs same-operand reference", e_b, scale, 5e-3 * scale)
    assert torch.isfinite(out8).all() and e_b <= 5e-3 * scale, (e_b, scale)
    # and against the unclamped bf16-operand convolution: quantisation only, no clipped-excess term
    yb, wb = y.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
    full = F.conv2d(yb, wb, padding=1)
    quant_bound = F.conv2d(yb.abs(), wb.abs(), padding=1) * (2.0 ** -4 + 2.0 ** -4)
    dev = (out8 - full).abs()
    worst = (dev - quant_bound - 5e-3 * scale).max().item()
    report(f"fp8 conv of the outlier tensor at shift {s}: worst deviation from the unclamped bf16 convolution", dev.max().item(), full.abs().max().item())
    report(f"fp8 conv of the outlier tensor at shift {s}: worst excess over the quantisation bound", max(worst, 0.0), 1.0, 0.0)
    assert worst <= 0.0, worst


@pytest.mark.parametrize("B,Cin,H,W,Cout,ks", [
    (2, 320, 64, 64, 320, 3),        # the dominant ResBlock conv
    (4, 320, 32, 32, 640, 1),        # 1x1: plain (no gather) variant
    (16, 1280, 8, 8, 1280, 3),       # M = 1024: sliced K + reduce
])
@pytest.mark.parametrize("s", [-3, 0, 6])
def test_conv2d_fp8_kernel_at_other_shifts(gpu, report, knobs, B, Cin, H, W, Cout, ks, s):
    """The fp8 convolution with an activation scale other than 2^-3 (ConvGemmParams::x_scale_e8 = 127 - s, negative s
    included): inputs of test_conv2d_fp8_kernel scaled by 2^(3 - s), same-operand reference, same 5e-3 bar."""
    from adaface_amd import _lib, ops
    knobs("gemm_pp_minfill", 0)
    g = torch.Generator().manual_seed(Cin + Cout + H + ks + 7)
    x = F.silu(torch.randn(B, Cin, H, W, generator=g) * 1.5) * 2.0 ** (3 - s)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks)
    w = w * (0.25 + 4.0 * torch.rand(Cout, 1, 1, 1, generator=g))
    b = torch.randn(Cout, generator=g) * 0.1
    xq = _e4m3(x.to(torch.bfloat16).float() * 2.0 ** s) / 2.0 ** s
    ref = F.conv2d(xq.double(), _quant_w(w).double(), b.double(), padding=ks // 2).float()
    _lib.plan_counts(reset=True)
    got = ops.conv2d_fp8(x.to(gpu), w.to(gpu), b.to(gpu), act_shift=s).cpu()
    assert _lib.plan_counts(reset=True)["fp8"] == 1
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    report(f"fp8 conv{ks}x{ks} {Cin}->{Cout}@{H}x{W} B{B} act_shift {s} vs same-operand reference", err, scale, 5e-3 * scale)
    assert torch.isfinite(got).all() and err <= 5e-3 * scale, (err, scale)


# ----------------------------------------------------------------------------------------------- model
def _sd15_inputs(gpu):
    from oracle import ldm_oracle as O
    cfg = O.SD15_UNET
    g = torch.Generator().manual_seed(52)
    x = torch.randn(16, 4, 64, 64, generator=g).to(gpu)
    t = torch.full((16,), 501, dtype=torch.long, device=gpu)
    ctx = torch.randn(16 * 16, 77, cfg.context_dim, generator=g).to(gpu)
    return cfg, x, t, ctx


def _sd15_engine(gpu, mode, ctx, weights=None):
    from oracle import ldm_oracle as O
    from adaface_amd.engine import Engine
    from adaface_amd.synth import synth_weights_into
    from tests.test_model_gpu import _unet_kwargs
    eng = Engine(dtype=mode, unet=_unet_kwargs(O.SD15_UNET))
    if weights is None:
        synth_weights_into(eng, O.unet_param_shapes(O.SD15_UNET), seed=51, device=gpu)
    else:
        for name, tns in weights.items():
            eng.load_tensor(name, tns)
    eng.set_context(ctx, 16, layerwise=True)
    return eng


def test_sd15_unet_fp8_calibration_invariants(gpu, report, tmp_path):
    """SD-1.5 UNet, Bf = 16, synthetic weights (as test_sd15_unet_fp8_mode).  All comparisons are torch.equal."""
    from adaface_amd import _lib
    from adaface_amd.fp8_calib import load_scales, save_scales
    cfg, x, t, ctx = _sd15_inputs(gpu)
    eng = _sd15_engine(gpu, "bf16", ctx)
    names = eng.fp8_site_names()
    # 22 ResBlocks x 2 convolutions + 16 transformer blocks; named by the consumer's checkpoint key
    assert len(names) == 60 and len(set(names)) == 60
    assert sum(n.endswith(".in_layers.2.weight") for n in names) == 22 and sum(n.endswith(".out_layers.3.weight") for n in names) == 22
    assert sum(n.endswith(".attn1.to_q.weight") for n in names) == 16
    bf16 = eng.unet_forward(x, t)
    eng.set_fp8(True)
    assert set(eng.fp8_shifts().values()) == {3}
    _lib.plan_counts(reset=True)
    f0 = eng.unet_forward(x, t)
    assert _lib.plan_counts(reset=True)["fp8"] == 59
    eng.set_fp8_shifts(None)
    assert torch.equal(eng.unet_forward(x, t), f0)                      # before any calibration == after a reset
    with eng.fp8_record():
        f_rec = eng.unet_forward(x, t)
        rec_plain = eng.fp8_read_record()
    assert torch.equal(f_rec, f0)                                       # recording changes nothing
    assert torch.equal(eng.unet_forward(x, t), f0)
    reached = {n for n, (amax, _) in rec_plain.items() if amax > 0.0}
    assert len(reached) == 59                                           # the sites of the 59 fp8 launches
    # the twin forward (CFG batch [x; x], context of 16 samples) goes through the same sites
    with eng.fp8_record():
        eng.unet_forward_twin(x[:8].contiguous(), t[:8].contiguous())
        rec_twin = eng.fp8_read_record()
    assert {n for n, (amax, _) in rec_twin.items() if amax > 0.0} == reached
    # two calibrations of the same run: identical amax bits and shifts
    run = lambda: eng.unet_forward(x, t)   # noqa: E731
    cal1 = eng.calibrate_fp8(run, passes=2, headroom=1)
    shifts1 = eng.fp8_shifts()
    eng.set_fp8_shifts(None)
    cal2 = eng.calibrate_fp8(run, passes=2, headroom=1)
    assert eng.fp8_shifts() == shifts1
    assert {n: (_bits(a), s, k) for n, (a, s, k) in cal1.items()} == {n: (_bits(a), s, k) for n, (a, s, k) in cal2.items()}
    assert all(k == 0 for _, _, k in cal1.values())
    assert any(s != 3 for s in shifts1.values())                        # the calibration really moved something
    print("[fp8 calib] synthetic SD-1.5 weights: shifts", sorted(set(shifts1.values())),
          "amax range", min(a for a, _, _ in cal1.values() if a > 0), max(a for a, _, _ in cal1.values()))
    _lib.plan_counts(reset=True)
    f_cal = eng.unet_forward(x, t)
    assert _lib.plan_counts(reset=True)["fp8"] == 59                    # same kernels, other constants
    assert torch.isfinite(f_cal).all() and not torch.equal(f_cal, f0)
    # saved, loaded into a fresh engine with the same weights: same output
    path = tmp_path / "scales.json"
    save_scales(path, shifts1, amax={n: a for n, (a, _, _) in cal1.items()}, headroom=1)
    eng2 = _sd15_engine(gpu, "bf16", ctx)
    eng2.set_fp8(True)
    eng2.set_fp8_shifts(load_scales(path, eng2.fp8_site_names()))
    assert torch.equal(eng2.unet_forward(x, t), f_cal)
    eng2.close()
    # unknown / missing names and shifts outside the range are refused, and leave the shifts alone
    with pytest.raises(KeyError):
        eng.set_fp8_shifts({**{n: 3 for n in names[1:]}, "no.such.weight": 3})
    with pytest.raises(ValueError):
        eng.set_fp8_shifts({**shifts1, names[0]: 9})
    assert eng.fp8_shifts() == shifts1
    # switching fp8 off still restores the bf16 result bit for bit, and back on the calibrated one
    eng.set_fp8(False)
    assert torch.equal(eng.unet_forward(x, t), bf16)
    eng.set_fp8(True)
    assert torch.equal(eng.unet_forward(x, t), f_cal)
    eng.close()
    # an f32 engine has no fp8 sites and says so
    e32 = _sd15_engine(gpu, "f32", ctx)
    f32 = e32.unet_forward(x, t)
    assert e32.fp8_site_names() == []
    with pytest.raises(_lib.AfError):
        e32.fp8_record().__enter__()
    e32.close()
    scale = f32.abs().max().item()
    d_fix = (f0 - f32).abs().max().item() / scale
    d_cal = (f_cal - f32).abs().max().item() / scale
    report("sd15_unet Bf=16 fp8 forward, fixed 2^3, vs f32-mode forward (synthetic weights)", d_fix, scale, FP8_FORWARD_TOL)
    report("sd15_unet Bf=16 fp8 forward, calibrated shifts, vs f32-mode forward (synthetic weights)", d_cal, scale, FP8_FORWARD_TOL)
    print(f"[fp8 calib] synthetic weights: fixed {d_fix:.3e}, calibrated {d_cal:.3e} of max|eps|")
    assert d_cal <= FP8_FORWARD_TOL, d_cal


# The user story's checkpoint: the synthetic weights with outlier channels.  In OUTLIER_BLOCKS ResBlocks the GroupNorm
# gains of OUTLIER_NCH channels of both norms are multiplied by OUTLIER_GAIN, and the matching input-channel weights of the
# consuming convolution divided by it (the f32 result moves little: SiLU is close to linear where the gain matters).
OUTLIER_BLOCKS = ("input_blocks.1.0", "input_blocks.2.0", "input_blocks.4.0", "input_blocks.5.0",
                  "output_blocks.6.0", "output_blocks.8.0", "output_blocks.9.0", "output_blocks.11.0")
OUTLIER_NCH = 16
OUTLIER_GAIN = 48.0


def outlier_weights(gpu, blocks=OUTLIER_BLOCKS, nch=OUTLIER_NCH, gain=OUTLIER_GAIN):
    """(base, modified): the tensors synth_weights_into draws (seed 51), and the ones the construction changes."""
    from oracle import ldm_oracle as O
    shapes = O.unet_param_shapes(O.SD15_UNET)
    g = torch.Generator(device=gpu).manual_seed(51)
    base = {}
    for name in sorted(shapes):                       # (the draw order and scales of adaface_amd.synth.synth_weights_into)
        shp = tuple(shapes[name])
        if len(shp) == 1:
            tns = torch.randn(shp, generator=g, device=gpu)
            tns = 1.0 + 0.1 * tns if name.endswith(".weight") else 0.05 * tns
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            tns = torch.randn(shp, generator=g, device=gpu) * (1.0 / math.sqrt(fan_in))
        base[name] = tns
    mod = {}
    P = "model.diffusion_model."
    for blk in blocks:
        for norm, conv in (("in_layers.0", "in_layers.2"), ("out_layers.0", "out_layers.3")):
            gam, w = base[f"{P}{blk}.{norm}.weight"].clone(), base[f"{P}{blk}.{conv}.weight"].clone()
            C = gam.numel()
            ch = torch.arange(nch, device=gpu) * (C // nch) + 3
            gam[ch] *= gain
            w[:, ch] /= gain
            mod[f"{P}{blk}.{norm}.weight"], mod[f"{P}{blk}.{conv}.weight"] = gam, w
    return base, mod


def test_sd15_unet_outlier_checkpoint_needs_and_gets_calibration(gpu, report):
    """The user story.  On a checkpoint with outlier channels (construction above; parameters and measured deviations in
    DESIGN.md section 2 (j)):
      (i)   the f32-mode forward is finite and its max|eps| within a factor 4 of the unmodified model's;
      (ii)  with the fixed 2^3 the record shows saturated elements in at least eight sites;
      (iii) the fixed-scale fp8 forward EXCEEDS the stated fp8 bar (8e-2 of max|eps|) against the f32-mode forward;
    and after calibrate_fp8 (two passes, headroom 1) no site saturates and the forward is WITHIN the bar."""
    cfg, x, t, ctx = _sd15_inputs(gpu)
    base, mod = outlier_weights(gpu)
    e32 = _sd15_engine(gpu, "f32", ctx, base)
    eps_base = e32.unet_forward(x, t)
    for name, tns in mod.items():
        e32.load_tensor(name, tns)
    e32.set_context(ctx, 16, layerwise=True)
    eps32 = e32.unet_forward(x, t)
    e32.close()
    scale, scale_base = eps32.abs().max().item(), eps_base.abs().max().item()
    print(f"[fp8 outlier model] max|eps| f32: unmodified {scale_base:.4f}, with outlier channels {scale:.4f}")
    assert torch.isfinite(eps32).all() and scale_base / 4 <= scale <= scale_base * 4, (scale, scale_base)          # (i)
    eng = _sd15_engine(gpu, "bf16", ctx, {**base, **mod})
    del base, mod
    eng.set_fp8(True)
    with eng.fp8_record():
        eps_fix = eng.unet_forward(x, t)
        rec = eng.fp8_read_record()
    n_sat_sites = sum(1 for _, k in rec.values() if k > 0)
    d_fix = (eps_fix - eps32).abs().max().item() / scale
    print(f"[fp8 outlier model] fixed 2^3: {n_sat_sites} sites saturate ({sum(k for _, k in rec.values())} elements), "
          f"largest amax {max(a for a, _ in rec.values()):.1f}, deviation {d_fix:.3e} of max|eps|")
    report("sd15_unet outlier checkpoint: fp8 forward, fixed 2^3, vs f32-mode forward", d_fix, scale, FP8_FORWARD_TOL)
    assert n_sat_sites >= 8, n_sat_sites                                                                         # (ii)
    assert torch.isfinite(eps_fix).all() and d_fix > FP8_FORWARD_TOL, d_fix                                      # (iii)
    cal = eng.calibrate_fp8(lambda: eng.unet_forward(x, t), passes=2, headroom=1)
    with eng.fp8_record():
        eps_cal = eng.unet_forward(x, t)
        rec_cal = eng.fp8_read_record()
    eng.close()
    d_cal = (eps_cal - eps32).abs().max().item() / scale
    print(f"[fp8 outlier model] calibrated: shifts {sorted(set(s for _, s, _ in cal.values()))}, "
          f"saturated elements {sum(k for _, k in rec_cal.values())}, deviation {d_cal:.3e} of max|eps|")
    report("sd15_unet outlier checkpoint: fp8 forward, calibrated shifts, vs f32-mode forward", d_cal, scale, FP8_FORWARD_TOL)
    assert all(k == 0 for _, _, k in cal.values()) and all(k == 0 for _, k in rec_cal.values())
    assert torch.isfinite(eps_cal).all() and d_cal <= FP8_FORWARD_TOL, d_cal


def test_config1_shape_chained_error_calibrated_fp8_vs_f32(gpu, report):
    """tests/test_chained_gpu.py's shape (BASELINE config 1: SD-1.5, batch 8 -> CFG batch 16, S = 10 DDIM steps, annealed
    guidance [10, 4], plain context) in CALIBRATED fp8 against the f32 mode, with that file's fp8 bars unchanged.  The
    calibration is LatentDiffusion.calibrate_fp8 with the run's own conditioning.  The fixed-scale numbers of the same run are
    reported beside them; nothing is asserted between the two."""
    from bench import build_model
    from adaface_amd.synth import synth_context
    from ldm.models.diffusion.ddim import DDIMSampler
    from tests.test_chained_gpu import CHAIN_GAIN, FINAL_BAR, FINAL_RMS_BAR, FWD_BAR
    B, S = 8, 10
    model = build_model(gpu, "f32")
    g = torch.Generator().manual_seed(42)
    x_T = torch.randn(B, 4, 64, 64, generator=g).to(gpu)
    c_emb = synth_context(B, seed=100, device=gpu)
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

    out = {"f32": chain()}
    model.set_compute_dtype("fp8")
    out["fp8 fixed"] = chain()
    cal = model.calibrate_fp8(model.get_learned_conditioning(c_emb), model.get_learned_conditioning(uc_emb), shape=[4, 64, 64],
                              batch_size=B, S=S, guidance_scale=[10.0, 4.0], x_T=x_T)
    assert all(k == 0 for _, _, k in cal.values())
    out["fp8 calibrated"] = chain()
    e_scale, l_scale = out["f32"][0].abs().max().item(), out["f32"][1].abs().max().item()
    l_rms = out["f32"][1].double().pow(2).mean().sqrt().item()
    fig = {}
    for mode in ("fp8 fixed", "fp8 calibrated"):
        e1 = (out[mode][0] - out["f32"][0]).abs().max().item() / e_scale
        ef = (out[mode][1] - out["f32"][1]).abs().max().item() / l_scale
        erms = (out[mode][1] - out["f32"][1]).double().pow(2).mean().sqrt().item() / l_rms
        fig[mode] = (e1, ef, erms)
        print(f"[fp8 chained] {mode}: first forward {e1:.3e}, final {ef:.3e}, rms {erms:.3e}, gain {ef / e1:.2f}")
        report(f"config1 shape Bf=16: first-forward eps {mode} vs f32 mode", e1, e_scale, FWD_BAR["fp8"])
        report(f"config1 shape Bf=16: final latent after S=10 DDIM steps {mode} vs f32 mode", ef, l_scale, FINAL_BAR["fp8"])
        report(f"config1 shape Bf=16: final latent after S=10 DDIM steps {mode} vs f32 mode, rms / rms", erms, l_rms, FINAL_RMS_BAR["fp8"])
    e1, ef, erms = fig["fp8 calibrated"]
    assert e1 <= FWD_BAR["fp8"], e1
    assert ef <= FINAL_BAR["fp8"], ef
    assert erms <= FINAL_RMS_BAR["fp8"], erms
    assert ef <= CHAIN_GAIN * e1, (ef, e1)
    assert not torch.equal(out["fp8 calibrated"][1], out["fp8 fixed"][1])


def test_dropin_calibrate_save_load_and_dtype_switches(gpu, knobs, tmp_path):
    """LatentDiffusion.calibrate_fp8 on the tiny model, then a 5-step DDIM sample: finite; save / load reproduces it bit for
    bit; so does fp8 -> bf16 -> fp8 (the engine is rebuilt, the shifts come back from the module) and fp8 -> f32 -> fp8; a
    load_state_dict returns every shift to 3.  (gemm_pp_minfill 0: the tiny model's 16x16 level would otherwise not fill
    the chip and stay on bf16; 32x32 latents at CFG batch 4 give its 128-channel level the 512 rows an fp8 plan needs.)"""
    from oracle import ldm_oracle as O
    from adaface_amd.configs import tiny_config
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.util import instantiate_from_config
    knobs("gemm_pp_minfill", 0)
    model = instantiate_from_config(tiny_config()["model"]).eval()
    sd = O.synth_state_dict(O.unet_param_shapes(O.TINY_UNET), seed=11)
    sd.update(O.synth_state_dict(O.vae_param_shapes(O.TINY_VAE), seed=12))
    sd.update(O.synth_state_dict(O.vae_encoder_param_shapes(O.TINY_VAE), seed=13))
    _, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected
    model = model.to(gpu).set_compute_dtype("fp8")
    unet = model.model.diffusion_model
    g = torch.Generator().manual_seed(5)
    B = 2
    c = model.get_learned_conditioning(model.layerwise_repeat(torch.randn(B, 77, 64, generator=g)).to(gpu))
    uc = model.get_learned_conditioning(model.layerwise_repeat(torch.randn(1, 77, 64, generator=g).expand(B, 77, 64).contiguous()).to(gpu))
    x_T = torch.randn(B, 4, 32, 32, generator=g).to(gpu)

    def sample():
        lat, _ = DDIMSampler(model).sample(S=5, conditioning=c, batch_size=B, shape=[4, 32, 32], verbose=False, guidance_scale=[6.0, 3.0],
                                           unconditional_conditioning=uc, eta=0.0, x_T=x_T)
        assert torch.isfinite(lat).all()
        return lat.clone()

    fixed = sample()
    assert unet.fp8_shifts() is None
    cal = model.calibrate_fp8(c, uc, shape=[4, 32, 32], batch_size=B, S=10, guidance_scale=[6.0, 3.0], x_T=x_T)
    reached = [n for n, (a, _, _) in cal.items() if a > 0.0]
    assert reached, "no fp8 site of the tiny model was reached: the test would show nothing"
    shifts = unet.fp8_shifts()
    assert shifts == {n: s for n, (_, s, _) in cal.items()} and any(s != 3 for s in shifts.values()), shifts
    calibrated = sample()
    assert not torch.equal(calibrated, fixed)
    # fp8 -> bf16 -> fp8 and fp8 -> f32 -> fp8: the engine is rebuilt, the module re-applies the shifts
    for other in ("bf16", "f32"):
        model.set_compute_dtype(other)
        assert not torch.equal(sample(), calibrated)
        model.set_compute_dtype("fp8")
        assert unet._engine is None
        assert torch.equal(sample(), calibrated), other
        assert unet._engine.fp8_shifts() == shifts
    # save; a load_state_dict returns every shift to 3; load brings the calibration back
    path = tmp_path / "tiny_fp8_scales.json"
    model.save_fp8_scales(path)
    model.load_state_dict(sd, strict=False)
    assert unet.fp8_shifts() is None
    assert torch.equal(sample(), fixed)
    assert set(unet._engine.fp8_shifts().values()) == {3}
    model.load_fp8_scales(path)
    assert unet.fp8_shifts() == shifts
    assert torch.equal(sample(), calibrated)
    # a scale file of another model is refused
    from adaface_amd.fp8_calib import save_scales
    save_scales(path, {("x" + n): s for n, s in shifts.items()})
    with pytest.raises(KeyError):
        model.load_fp8_scales(path)
    assert unet.fp8_shifts() == shifts
