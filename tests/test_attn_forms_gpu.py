"""The forms of AttnParams only the model states, kernel by kernel (ops.attention keyword arguments layout, ld_slack, lse,
batch_window, drop_keys -> af_op_attention_ex).

Every other op-level attention test reaches af_launch_attention through af_op_attention: q, k and v dense with pitch C, no lse,
scale dh^-0.5, the whole batch.  Runner::attn_params (csrc/af_model.hip) never builds that form.  It builds F1 q | k | v as
columns of one [B][N][3C] buffer, F2 k | v as columns of the cached context [B][S][2C] (with the V^T pack made at that pitch),
F3 = F2 with the subject strings' keys dropped and an lse output, F4 = F1 with the causal mask, F5 a window of the batch.  Here
each of them meets each kernel the plan can give it (tests/attn_cases.py holds the tables; tests/test_attn_plan_cpu.py checks
them, the reference and the lse bar on the CPU).

Every case
  * asserts before the launch that af_attn_plan_query names the intended kernel, and after it that the launch counters show
    exactly one launch of that kernel and none of any other;
  * compares the form with the DENSE form bit for bit (torch.equal): same kernel, same knobs, same values -- the kernels'
    arithmetic does not depend on addresses, so a difference is an addressing bug or a result read too early;
  * compares the dense output with the fp64 reference at the bars of tests/test_ops_gpu.py / tests/test_fp16_gpu.py;
  * checks the guards: the op fills every buffer with NaN bytes before the casts, so the window must be finite (no slack column,
    no row behind the operands was read) and slack columns and samples outside the window must still hold the fill.
"""
import functools
import math

import pytest
import torch

import attn_cases as A
import test_fp16_gpu as T16
import test_ops_gpu as T

pytestmark = pytest.mark.gpu

ATTN_KEYS = ("attn_flash", "attn_w4", "attn_ring40", "attn_ring80", "attn_short", "xattn_fused", "conv_attn_short")


def _cmp(report, name, got, ref, dtype):
    """TOL[dtype] of tests/test_ops_gpu.py; fp16: F16_OP_TOL of tests/test_fp16_gpu.py, of max |reference| as well"""
    if dtype != "f16":
        return T._cmp(report, name, got, ref, dtype)
    ref = ref.float()
    scale = ref.abs().max().item() + 1e-12
    err = (got.detach().float().cpu() - ref).abs().max().item() / scale
    report(f"{name}[f16]", err * scale, scale, T16.F16_OP_TOL * scale)
    assert math.isfinite(err) and err <= T16.F16_OP_TOL, f"{name}[f16]: max abs err {err:.3e} of max|ref| > {T16.F16_OP_TOL:.3e}"


@functools.lru_cache(maxsize=None)
def _case_data(c, seed_extra=0, scale_mul=1.0, causal=False, drop=0):
    """operands and the fp64 reference of a case, computed once"""
    q, k, v = A.operands(A.seed_of(c, seed_extra), c.B, c.Nq, c.Nk, c.heads, c.dh, c.dtype)
    scale = scale_mul * c.dh ** -0.5
    o, lse2 = A.ref_attention(q, k[:, :c.Nk - drop], v[:, :c.Nk - drop], c.heads, scale, causal=causal)
    return q, k, v, scale, o, lse2


def _run(gpu, knobs, c, q, k, v, layout, *, scale=None, causal=False, **kw):
    """One launch: the plan is asserted before it, the counters after it.  Returns what ops.attention returns."""
    from adaface_amd import _lib, ops
    for name, val in c.knobs:
        knobs(name, val)
    f = A.op_form(c, layout, kw.get("ld_slack", 0), lse=kw.get("lse", False), causal=causal, drop_keys=kw.get("drop_keys", 0))
    plan = _lib.attn_plan_query(c.dtype, c.dh, c.Nk - kw.get("drop_keys", 0), f["ldq"], f["ldk"], f["ldv"], f["ldo"], causal=causal,
                                lse=kw.get("lse", False), vt_pack=f["vt_pack"])["kernel"]
    assert plan == c.kernel, (plan, c, layout, f)
    _lib.plan_counts(reset=True)
    out = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), c.heads, scale=scale, dtype=c.dtype, causal=causal, layout=layout, **kw)
    torch.cuda.synchronize()
    pc = _lib.plan_counts(reset=True)
    assert {n: pc[n] for n in ATTN_KEYS} == {n: int(n == "attn_" + c.kernel) for n in ATTN_KEYS}, (c, layout, pc)
    return out


def _split(whole, C, window=None):
    """(valid columns of the window's samples, everything else) of the whole pitched output [B, N, C + slack]"""
    B = whole.shape[0]
    b0, nb = (0, B) if window is None else window
    inside = torch.zeros(whole.shape, dtype=torch.bool, device=whole.device)
    inside[b0:b0 + nb, :, :C] = True
    return whole[b0:b0 + nb, :, :C], whole[~inside]


def _assert_guards(name, whole, C, window=None):
    win, rest = _split(whole, C, window)
    assert bool(torch.isfinite(win).all()), f"{name}: NaN in the output: a slack column or a row behind the operands was read"
    assert bool(torch.isnan(rest).all()), f"{name}: {int((~torch.isnan(rest)).sum())} elements outside the output were written"
    return win


def _check_form(gpu, report, knobs, c, layout, ld_slack, name, causal=False):
    q, k, v, scale, ref, _ = _case_data(c, causal=causal)
    C = c.heads * c.dh
    dense = _run(gpu, knobs, c, q, k, v, "dense", causal=causal)
    whole = _run(gpu, knobs, c, q, k, v, layout, causal=causal, ld_slack=ld_slack)
    assert whole.shape == (c.B, c.Nq, C + ld_slack)
    got = _assert_guards(name, whole, C)
    _cmp(report, name + " dense", dense, ref, c.dtype)
    assert torch.equal(got, dense), f"{name}: differs from the dense form, max {(got - dense).abs().max().item():.3e}"


def _ids(cases):
    return [A.case_id(c) for c in cases]


@pytest.mark.parametrize("ld_slack", [0, 8])
@pytest.mark.parametrize("c", A.F1, ids=_ids(A.F1))
def test_f1_qkv_columns(gpu, report, knobs, c, ld_slack):
    """F1: q, k, v are columns 0, C, 2C of one [B][N][3C + slack] buffer, as every self-attention states them"""
    _check_form(gpu, report, knobs, c, "qkv", ld_slack, f"attn forms F1 qkv +{ld_slack} {A.case_id(c)}")


@pytest.mark.parametrize("ld_slack", [0, 8])
@pytest.mark.parametrize("c", A.F2, ids=_ids(A.F2))
def test_f2_context_columns(gpu, report, knobs, c, ld_slack):
    """F2: k, v are columns 0, C of the cached context [B][S][2C + slack]; the V^T pack is made at that pitch"""
    _check_form(gpu, report, knobs, c, "ctx", ld_slack, f"attn forms F2 ctx +{ld_slack} {A.case_id(c)}")


@pytest.mark.parametrize("drop", A.F3_DROP)
@pytest.mark.parametrize("c", A.F3, ids=_ids(A.F3))
def test_f3_lse_with_dropped_keys(gpu, report, knobs, c, drop):
    """F3: conv attention's flash part: the context form over S - groups * ks^2 keys with an lse output.  O is the same call's
    without lse bit for bit, lse is inside 2 E per row (attn_cases.lse_bar) and the same from the dense form bit for bit."""
    q, k, v, scale, ref, lse2 = _case_data(c, seed_extra=drop, drop=drop)
    C = c.heads * c.dh
    name = f"attn forms F3 lse drop{drop} {A.case_id(c)}"
    whole, lse = _run(gpu, knobs, c, q, k, v, "ctx", lse=True, drop_keys=drop)
    plain = _run(gpu, knobs, c, q, k, v, "ctx", drop_keys=drop)
    dense, lse_dense = _run(gpu, knobs, c._replace(Nk=c.Nk - drop), q, k[:, :c.Nk - drop].contiguous(), v[:, :c.Nk - drop].contiguous(),
                            "dense", lse=True)
    got = _assert_guards(name, whole, C)
    assert torch.equal(got, _assert_guards(name + " without lse", plain, C)), f"{name}: O moves with the lse output"
    assert torch.equal(got, dense), f"{name}: O differs from the dense form"
    assert torch.equal(lse, lse_dense), f"{name}: lse differs from the dense form"
    _cmp(report, name + " O", got, ref, c.dtype)
    assert lse.shape == lse2.shape and bool(torch.isfinite(lse).all())
    E = A.lse_bar(q, k[:, :c.Nk - drop], c.heads, scale, c.kernel, c.dtype, lse2)
    ratio = ((lse.double().cpu() - lse2).abs() / (2.0 * E)).max().item()
    report(name + f": worst row |lse - lse2| / (2 E)[{c.dtype}]", ratio, 1.0, 1.0)
    assert ratio <= 1.0, f"{name}: lse leaves 2 E: worst row ratio {ratio:.3f}"


@pytest.mark.parametrize("c", A.F4, ids=_ids(A.F4))
def test_f4_causal_qkv(gpu, report, knobs, c):
    """F4: the CLIP text tower's form, causal on the qkv columns; at T = 300 three workgroups per head, so that the skipped-tile
    predicate runs with blockIdx.x > 0 and waves start past a tile boundary"""
    _check_form(gpu, report, knobs, c, "qkv", 0, f"attn forms F4 causal {A.case_id(c)}", causal=True)


@pytest.mark.parametrize("c,layout,B,window", A.F5, ids=[f"{A.case_id(c)}-{lay}-B{B}-w{w[0]}+{w[1]}" for c, lay, B, w in A.F5])
def test_f5_batch_window(gpu, report, knobs, c, layout, B, window):
    """F5: samples [b0, b0 + nb) of the batch: inside bit-identical to the full-batch run, outside the fill untouched; on the
    short-key kernel the V^T pack pointer moves with the window"""
    c = c._replace(B=B)
    q, k, v, scale, ref, _ = _case_data(c)
    C = c.heads * c.dh
    b0, nb = window
    name = f"attn forms F5 window {b0}+{nb} of {B} {layout} {A.case_id(c)}"
    full = _assert_guards(name + " full", _run(gpu, knobs, c, q, k, v, layout), C)
    got = _assert_guards(name, _run(gpu, knobs, c, q, k, v, layout, batch_window=window), C, window)
    _cmp(report, name + " full batch", full, ref, c.dtype)
    assert torch.equal(got, full[b0:b0 + nb]), f"{name}: differs from the full-batch run"


@pytest.mark.parametrize("c,layout", A.SCALE, ids=[f"{A.case_id(c)}-{lay}" for c, lay in A.SCALE])
def test_scale_is_passed_through(gpu, report, knobs, c, layout):
    """scale = 0.37 dh^-0.5 against the reference at that scale: the kernels fold it into the pre-scaled Q or the exponent"""
    q, k, v, scale, ref, _ = _case_data(c, scale_mul=A.SCALE_MUL)
    name = f"attn forms scale {A.SCALE_MUL} {layout} {A.case_id(c)}"
    got = _assert_guards(name, _run(gpu, knobs, c, q, k, v, layout, scale=scale, ld_slack=8), c.heads * c.dh)
    _cmp(report, name, got, ref, c.dtype)
    base = _case_data(c)[4]
    assert (base - ref).abs().max().item() > 4 * T.TOL["bf16"] * ref.abs().max().item()     # the scale is visible at the bar
