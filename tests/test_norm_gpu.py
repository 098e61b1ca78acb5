"""The GroupNorm / LayerNorm kernels of af_norm.hip on every branch, tail and offset tests/norm_cases.py lists, against
F.group_norm / F.layer_norm (and SiLU) in fp64 on inputs already rounded to the storage type.

Every case first asserts that the launch plan (af_norm_plan_query, the plan the launcher follows) is the one the table wrote
out by hand, so the case is known to run the kernel it is there for.  Bounds are the operator bounds of the older tests,
imported, relative to max|reference|: TOL (test_ops_gpu.py) for f32 / bf16, F16_OP_TOL (test_fp16_gpu.py) for f16.

Each shape runs on two inputs:
  plain   randn * 1.7 + 0.4, as the older tests
  loaded  the pixels of the ragged last chunk (the last HW % P pixels; the last pixel where there is no ragged chunk and on the
          small kernel), scaled by sqrt(HW / n_tail): they carry about half of each group's sum of squares.  Before the GPU
          call the test asserts on the reference alone that statistics WITHOUT those pixels put the output at least 10 bounds
          away -- so a kernel that drops the tail (or counts it twice, a change of the same size) cannot pass.  LayerNorm rows
          are independent, so there the rows of the ragged last workgroup are scaled the same way and the precondition is that
          what the stale output buffer holds for them (below) is 10 bounds away.
The op wrappers take the output from an uncleared temporary and a pool may hand back the previous call's buffer, so every
checked call follows a call of the same shape on the NEGATED input: an element the kernel fails to write holds the wrong answer.
Two checked calls must be bit-identical (fixed summation order)."""
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from tests import norm_cases as N            # noqa: E402
from test_ops_gpu import TOL                 # noqa: E402
from test_fp16_gpu import F16_OP_TOL         # noqa: E402

pytestmark = pytest.mark.gpu

PRECONDITION = 10.0   # the loaded tail must move the reference by this many bounds


def _tol(dtype):
    return F16_OP_TOL if dtype == "f16" else TOL[dtype]


def _q(t, dtype):
    """round to the kernel's storage type"""
    return t.to({"bf16": torch.bfloat16, "f16": torch.float16}[dtype]).float() if dtype != "f32" else t.float()


def _dyadic(n, g, lo, hi, step):
    """n values lo + k * step (k random): exact in bf16 / f16 / f32 for the steps used here"""
    return lo + step * torch.randint(0, int(round((hi - lo) / step)) + 1, (n,), generator=g).float()


def _check(report, name, got, ref, dtype):
    """max |got - ref| against the bound relative to max |ref|; ref is fp64"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-12
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs().max().item() if finite else float("inf")
    tol = _tol(dtype) * scale
    report(f"norm {name}[{dtype}]", err, scale, tol)
    assert finite, f"{name}[{dtype}]: non-finite output"
    assert err <= tol, f"{name}[{dtype}]: max abs err {err:.3e} > {_tol(dtype):.2e} * {scale:.3e}"


def _silu64(t):
    return t * torch.sigmoid(t)


# ------------------------------------------------------------------------------------------------------------ GroupNorm
def _gn_ref(x, w, b, eps, silu):
    y = F.group_norm(x.double(), 32, w.double(), b.double(), eps)
    return _silu64(y) if silu else y


def _gn_ref_without_tail(x, w, b, eps, silu, n_tail):
    """the output if the statistics missed the last n_tail pixels"""
    B, C, H, W = x.shape
    xd = x.double().view(B, 32, C // 32, H * W)
    kept = xd[..., : H * W - n_tail]
    mean = kept.mean(dim=(2, 3), keepdim=True)
    var = kept.var(dim=(2, 3), unbiased=False, keepdim=True)
    y = ((xd - mean) / torch.sqrt(var + eps)).view(B, C, H, W) * w.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1)
    return _silu64(y) if silu else y


def _gn_run(gpu, x, w, b, eps, silu, dtype):
    from adaface_amd import ops
    return ops.group_norm(x.to(gpu), w.to(gpu), b.to(gpu), eps=eps, silu=silu, dtype=dtype)


def _gn_checked(gpu, report, name, x, w, b, eps, silu, dtype, ref):
    """negated input first (stale buffers), then the checked call twice"""
    stale = _gn_run(gpu, -x, w, b, eps, silu, dtype)
    del stale
    got = _gn_run(gpu, x, w, b, eps, silu, dtype)
    again = _gn_run(gpu, x, w, b, eps, silu, dtype)
    assert torch.equal(got, again), f"{name}[{dtype}]: two runs differ"
    _check(report, name, got, ref, dtype)
    return got


def _gn_setup(lib, knobs, case, dtype, nosmall):
    """set the knob, assert the plan is the table's, return it"""
    B, C, H, W = case.shape
    if nosmall:
        knobs("gn_small", 0)
    plan = lib.norm_plan_query("groupnorm", dtype, B=B, HW=H * W, C=C)
    assert plan == N.gn_plan(case, dtype, nosmall), (case.shape, dtype, plan)
    return plan


def _gn_tail(case, plan):
    HW = case.shape[2] * case.shape[3]
    return HW % plan["P"] if plan["kernel"] != "small" and HW % plan["P"] else 1


GN_RUN = [p for p in N.gn_params() if p[0].plan != N.REFUSED]


@pytest.mark.parametrize("p", GN_RUN, ids=N.gn_id)
def test_groupnorm(gpu, report, knobs, p):
    from adaface_amd import _lib
    case, dtype, nosmall = p
    plan = _gn_setup(_lib, knobs, case, dtype, nosmall)
    B, C, H, W = case.shape
    HW, n_tail = H * W, _gn_tail(case, plan)
    g = torch.Generator().manual_seed(C + 7 * H + W)
    base = torch.randn(B, C, H, W, generator=g) * 1.7 + 0.4
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    loaded = base.clone()
    loaded.view(B, C, HW)[:, :, HW - n_tail:] *= math.sqrt(HW / n_tail)
    for kind, x in (("plain", _q(base, dtype)), ("loaded", _q(loaded, dtype))):
        if kind == "loaded" and n_tail == HW:
            continue   # (the one-pixel map: its tail is the whole map, the loaded input is the plain one)
        for silu, eps in ((False, 1e-6), (True, 1e-5)):
            ref = _gn_ref(x, w, b, eps, silu)
            name = f"groupnorm {N.gn_id(p)} {plan['kernel']} {kind} silu{int(silu)}"
            if kind == "loaded":
                moved = (_gn_ref_without_tail(x, w, b, eps, silu, n_tail) - ref).abs().max().item()
                bound = _tol(dtype) * ref.abs().max().item()
                report(f"norm {name}: reference without the tail, in bounds", moved / bound, 1.0, PRECONDITION)
                assert moved >= PRECONDITION * bound, (name, moved / bound)
            _gn_checked(gpu, report, name, x, w, b, eps, silu, dtype, ref)


def _case_of(shape):
    return next(c for c in N.GN_CASES if c.shape == shape)


# one chunked + finalize shape, one chunked + fold shape, one small shape (and it again on the chunked path)
SPECIAL_GN = [(c, d, ns) for shape, ns in (((2, 320, 9, 29), False), ((48, 64, 10, 10), False), ((1, 256, 33, 31), False),
                                           ((1, 256, 33, 31), True))
              for c in [_case_of(shape)] for d in c.dtypes]


@pytest.mark.parametrize("p", SPECIAL_GN, ids=N.gn_id)
def test_groupnorm_offset_means(gpu, report, knobs, p):
    """Per-(sample, group) means drawn in [-16, 16] and standard deviations in [0.5, 2]: the statistics are single-pass
    (fp32 partial sums of x and x * x, combined in fp64, var = E[x^2] - mean^2), so this is where cancellation would show.
    Same bounds as everywhere; the measured errors go to the report."""
    from adaface_amd import _lib
    case, dtype, nosmall = p
    plan = _gn_setup(_lib, knobs, case, dtype, nosmall)
    B, C, H, W = case.shape
    g = torch.Generator().manual_seed(31 * C + H)
    mean = (torch.rand(B, 32, 1, 1, generator=g) * 32.0 - 16.0)
    std = (torch.rand(B, 32, 1, 1, generator=g) * 1.5 + 0.5)
    x = _q((torch.randn(B, 32, C // 32, H * W, generator=g) * std + mean).view(B, C, H, W), dtype)
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    for silu, eps in ((False, 1e-6), (True, 1e-5)):
        name = f"groupnorm {N.gn_id(p)} {plan['kernel']} offset means silu{int(silu)}"
        _gn_checked(gpu, report, name, x, w, b, eps, silu, dtype, _gn_ref(x, w, b, eps, silu))


@pytest.mark.parametrize("p", SPECIAL_GN, ids=N.gn_id)
def test_groupnorm_constant_group(gpu, report, knobs, p):
    """One group of the first sample and one of the last are constant at 0.5.  Their sums are exact in fp32 (multiples of 1/4
    far below 2^24), so mean = 0.5 and var = 0 exactly; with eps = 2^-16 rstd is exactly 256, and with gamma a multiple of 1/8
    and beta a multiple of 1/64 the scale gamma * rstd and the shift beta - mean * gamma * rstd are exact too (15 significant
    bits at most), so fma(0.5, scale, shift) is beta with no rounding anywhere: the output must EQUAL beta, in every storage
    type (beta fits bf16).  With SiLU: silu(beta) to the bound.  The other groups meet the reference as usual."""
    from adaface_amd import _lib
    case, dtype, nosmall = p
    plan = _gn_setup(_lib, knobs, case, dtype, nosmall)
    B, C, H, W = case.shape
    cpg, eps = C // 32, 2.0 ** -16
    g = torch.Generator().manual_seed(17 * C + W)
    x = torch.randn(B, C, H, W, generator=g) * 1.7 + 0.4
    spots = [(0, 5), (B - 1, 31)]
    for s, grp in spots:
        x[s, grp * cpg:(grp + 1) * cpg] = 0.5
    x = _q(x, dtype)
    w = _dyadic(C, g, 0.5, 1.5, 1.0 / 8)
    b = _dyadic(C, g, -1.0, 1.0, 1.0 / 64)
    for silu in (False, True):
        name = f"groupnorm {N.gn_id(p)} {plan['kernel']} constant group silu{int(silu)}"
        ref = _gn_ref(x, w, b, eps, silu)
        got = _gn_checked(gpu, report, name, x, w, b, eps, silu, dtype, ref).cpu()
        for s, grp in spots:
            ch = slice(grp * cpg, (grp + 1) * cpg)
            want = b[ch].view(cpg, 1, 1).expand(cpg, H, W)
            if silu:
                err = (got[s, ch].double() - _silu64(want.double())).abs().max().item()
                assert err <= _tol(dtype) * ref.abs().max().item(), (name, s, grp, err)
            else:
                assert torch.equal(got[s, ch], want), (name, s, grp, (got[s, ch] - want).abs().max().item())


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [48, 2592])
def test_groupnorm_refusal_launches_nothing(gpu, dtype, C):
    """C the kernels do not take: AfError, and the output the caller handed over is untouched"""
    from adaface_amd import _lib
    assert _lib.norm_plan_query("groupnorm", dtype, B=1, HW=16, C=C)["kernel"] == "refused"
    x = torch.randn(1, C, 4, 4, device=gpu)
    w, b = torch.ones(C, device=gpu), torch.zeros(C, device=gpu)
    y = torch.full_like(x, 12345.0)
    with pytest.raises(_lib.AfError):
        _lib.check(_lib.load().af_op_groupnorm(_lib.DTYPES[dtype], _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), 1e-5, 1, _lib.ptr(y),
                                               1, C, 4, 4, _lib.stream_ptr()), "af_op_groupnorm")
    torch.cuda.synchronize()
    assert bool((y == 12345.0).all())


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_ref(x, w, b, eps=1e-5):
    return F.layer_norm(x.double(), (x.shape[-1],), w.double(), b.double(), eps)


def _ln_run(gpu, x, w, b, dtype):
    from adaface_amd import ops
    return ops.layer_norm(x.to(gpu), w.to(gpu), b.to(gpu), dtype=dtype)


def _ln_checked(gpu, report, name, x, w, b, dtype, ref):
    stale = _ln_run(gpu, -x, w, b, dtype)
    del stale
    got = _ln_run(gpu, x, w, b, dtype)
    again = _ln_run(gpu, x, w, b, dtype)
    assert torch.equal(got, again), f"{name}[{dtype}]: two runs differ"
    _check(report, name, got, ref, dtype)
    return got


def _ln_setup(lib, case, dtype):
    plan = lib.norm_plan_query("layernorm", dtype, rows=case.rows, C=case.C)
    assert plan == N.ln_plan(case), (case.rows, case.C, dtype, plan)
    return plan


LN_RUN = [p for p in N.ln_params() if p[0].plan != N.LN_REFUSED]


@pytest.mark.parametrize("p", LN_RUN, ids=N.ln_id)
def test_layernorm(gpu, report, p):
    from adaface_amd import _lib
    case, dtype = p
    plan = _ln_setup(_lib, case, dtype)
    rows, C = case.rows, case.C
    n_tail = rows % plan["rows_per_block"] or 1
    g = torch.Generator().manual_seed(rows + C)
    base = torch.randn(rows, C, generator=g) * 1.7 + 0.4
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    loaded = base.clone()
    loaded[rows - n_tail:] *= math.sqrt(rows / n_tail)
    for kind, x in (("plain", _q(base, dtype)), ("loaded", _q(loaded, dtype))):
        ref = _ln_ref(x, w, b)
        name = f"layernorm {N.ln_id(p)} {plan['kernel']} {kind}"
        if kind == "loaded":
            stale = _ln_ref(-x[rows - n_tail:], w, b)      # what the rows hold if the checked call does not write them
            moved = (stale - ref[rows - n_tail:]).abs().max().item()
            bound = _tol(dtype) * ref.abs().max().item()
            report(f"norm {name}: stale tail rows, in bounds", moved / bound, 1.0, PRECONDITION)
            assert moved >= PRECONDITION * bound, (name, moved / bound)
        _ln_checked(gpu, report, name, x, w, b, dtype, ref)


# one shape of each kernel per storage type: (rows, C) of the table
SPECIAL_LN = [(c, d) for c, d in LN_RUN if c.C == 320]


@pytest.mark.parametrize("p", SPECIAL_LN, ids=N.ln_id)
def test_layernorm_offset_means(gpu, report, p):
    """per-row means in [-16, 16], standard deviations in [0.5, 2] (the kernels' variance is two-pass); same bounds"""
    from adaface_amd import _lib
    case, dtype = p
    plan = _ln_setup(_lib, case, dtype)
    rows, C = case.rows, case.C
    g = torch.Generator().manual_seed(3 * rows + C)
    mean = torch.rand(rows, 1, generator=g) * 32.0 - 16.0
    std = torch.rand(rows, 1, generator=g) * 1.5 + 0.5
    x = _q(torch.randn(rows, C, generator=g) * std + mean, dtype)
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = torch.randn(C, generator=g) * 0.2
    _ln_checked(gpu, report, f"layernorm {N.ln_id(p)} {plan['kernel']} offset means", x, w, b, dtype, _ln_ref(x, w, b))


@pytest.mark.parametrize("p", SPECIAL_LN, ids=N.ln_id)
def test_layernorm_constant_and_zero_rows(gpu, report, p):
    """A row constant at 0.5 and an all-zero row, one in the middle of a workgroup's rows and one as the last live row, then
    swapped.  The row sum is exact, so mean is the constant, every difference is 0 and the output must EQUAL beta (a multiple of
    1/64: exact in every storage type); the rows around them meet the reference."""
    from adaface_amd import _lib
    case, dtype = p
    plan = _ln_setup(_lib, case, dtype)
    rows, C = case.rows, case.C
    mid, last = 3 * plan["rows_per_block"] + plan["rows_per_block"] // 2 + 1, rows - 1
    g = torch.Generator().manual_seed(5 * rows + C)
    base = torch.randn(rows, C, generator=g) * 1.7 + 0.4
    w = torch.randn(C, generator=g) * 0.3 + 1.0
    b = _dyadic(C, g, -1.0, 1.0, 1.0 / 64)
    for r_const, r_zero in ((mid, last), (last, mid)):
        x = base.clone()
        x[r_const], x[r_zero] = 0.5, 0.0
        x = _q(x, dtype)
        name = f"layernorm {N.ln_id(p)} {plan['kernel']} constant row {r_const} zero row {r_zero}"
        got = _ln_checked(gpu, report, name, x, w, b, dtype, _ln_ref(x, w, b)).cpu()
        assert torch.equal(got[r_const], b) and torch.equal(got[r_zero], b), name


@pytest.mark.parametrize("C", [2568, 36])
def test_layernorm_refusal_launches_nothing(gpu, C):
    from adaface_amd import _lib
    assert _lib.norm_plan_query("layernorm", "bf16", rows=16, C=C)["kernel"] == "refused"
    x = torch.randn(16, C, device=gpu)
    w, b = torch.ones(C, device=gpu), torch.zeros(C, device=gpu)
    y = torch.full_like(x, 12345.0)
    with pytest.raises(_lib.AfError):
        _lib.check(_lib.load().af_op_layernorm(_lib.DTYPES["bf16"], _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), 1e-5, _lib.ptr(y), 16, C,
                                               _lib.stream_ptr()), "af_op_layernorm")
    torch.cuda.synchronize()
    assert bool((y == 12345.0).all())
