"""The attention launch plan (af_plan_attention through af_attn_plan_query: host code, no GPU) against the table
tests/attn_cases.py writes out by hand, and the checks that make tests/test_attn_forms_gpu.py mean something before it runs:
every GPU case reaches the kernel it names, the derived lse bar is achievable (a CPU emulation of the kernels' roundings stays
inside E on every row) and discriminating (three wrong lse values leave 2 E on every row), and the causal cases tell the mask
from no mask and from an off-by-one mask in every sample and head."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests import attn_cases as A  # noqa: E402

# the op-level bars of tests/test_ops_gpu.py (TOL) and tests/test_fp16_gpu.py (F16_OP_TOL), of max |reference|
from tests.test_fp16_gpu import F16_OP_TOL  # noqa: E402
from tests.test_ops_gpu import TOL  # noqa: E402

OP_TOL = dict(TOL, f16=F16_OP_TOL)


@pytest.fixture
def lib():
    from adaface_amd import _lib
    _lib.load()
    _lib.reset_knobs()
    yield _lib
    _lib.reset_knobs()


def _query(lib, r):
    for k, v in r.knobs.items():
        lib.set_knob(k, v)
    return lib.attn_plan_query(r.dtype, r.dh, r.Nk, r.ldq, r.ldk, r.ldv, r.ldo, causal=r.causal, lse=r.lse, vt_pack=r.pack)["kernel"]


@pytest.mark.parametrize("r", A.PLAN_ROWS, ids=lambda r: r.why)
def test_plan_is_the_hand_written_one(lib, r):
    assert _query(lib, r) == r.kernel, r


def test_table_reaches_every_kernel_and_both_sides_of_every_threshold(lib):
    rows = [(r, _query(lib, r)) for r in A.PLAN_ROWS]
    assert {k for _, k in rows} == set(lib.ATTN_KERNELS)
    assert all(r.kernel == k for r, k in rows)

    def has(kernel, **kw):
        return any(k == kernel and all((r.knobs[a] if a in r.knobs else getattr(r, a)) == v for a, v in kw.items()) for r, k in rows)
    ok = dict(dtype="bf16", causal=False, lse=False)
    # short: 96 / 97 keys, the knob, the pack, the mask, lse, the storage types, the head dims
    assert has("short", Nk=96, pack=True, attn_short=1, **ok) and not has("short", Nk=97)
    assert any(r.Nk == 97 and r.pack and r.knobs["attn_short"] and r.dh in (40, 80) and k != "short" for r, k in rows)
    for off in (dict(attn_short=0), dict(pack=False), dict(causal=True), dict(lse=True), dict(dtype="f32"), dict(dtype="f16"), dict(dh=160)):
        want = dict(dict(dict(ok, pack=True, attn_short=1), Nk=77 if "lse" not in off else 68), **off)
        assert any(all((r.knobs[a] if a in r.knobs else getattr(r, a)) == v for a, v in want.items()) and k != "short" for r, k in rows), off
    assert has("short", dh=40) and has("short", dh=80)
    # ring80: 255 / 256 keys with bit 2 off, bit 2, bit 1, the mask
    assert has("flash", dh=80, Nk=255, attn_ring=3, **ok) and has("ring80", dh=80, Nk=256, attn_ring=3, **ok)
    assert has("ring80", dh=80, Nk=255, attn_ring=7) and has("flash", dh=80, Nk=1024, attn_ring=1) and has("flash", dh=80, Nk=1024, attn_ring=5)
    assert has("ring80", dh=80, attn_ring=2) and has("flash", dh=80, Nk=1024, attn_ring=7, causal=True, dtype="bf16")
    # ring40 / w4: bit 0 on and off, the mask
    assert has("ring40", attn_ring=1) and has("w4", attn_ring=2) and has("w4", attn_ring=6) and has("w4", attn_ring=0)
    assert has("w4", attn_ring=7, causal=True)
    # every storage type on flash, and only bf16 anywhere else
    assert {r.dtype for r, k in rows if k == "flash"} == {"bf16", "f32", "f16"}
    assert {r.dtype for r, k in rows if k not in ("flash", "refused")} == {"bf16"}
    # refusals: a head dim, each pitch, per element size, no key -- and the nearest accepted neighbour of each
    ref = [r for r, k in rows if k == "refused"]
    assert {r.dh for r in ref} >= {48} and any(r.Nk == 0 for r in ref)
    assert any(r.dtype == "bf16" and r.ldk % 8 for r in ref) and any(r.dtype == "f16" and r.ldk % 8 for r in ref)
    assert any(r.dtype == "f32" and r.ldk % 4 for r in ref) and any(r.dtype == "f32" and r.ldk % 8 == 4 and k == "flash" for r, k in rows)
    assert any(r.ldq % 8 for r in ref) and any(r.ldv % 8 for r in ref) and any(r.ldo % 4 for r in ref)
    assert any(r.dtype == "bf16" and r.ldo % 8 == 4 and k != "refused" for r, k in rows)
    assert {r.dh for r, k in rows if k != "refused"} == set(A.DH_LIST)


def test_every_head_dim_in_and_around_the_list(lib):
    """the head dim list itself, every multiple of 8 up to 168: exactly DH_LIST is taken"""
    for dt in ("bf16", "f32", "f16"):
        taken = {dh for dh in range(8, 169, 8) if lib.attn_plan_query(dt, dh, 77, 8 * dh)["kernel"] != "refused"}
        assert taken == set(A.DH_LIST), (dt, taken)


def _gpu_plans():
    out = []
    for fam, cases, layouts in (("F1", A.F1, ("qkv", "dense")), ("F2", A.F2, ("ctx", "dense"))):
        out += [(fam, c, lay, s, {}) for c in cases for lay in layouts for s in ((0, 8) if lay != "dense" else (0,))]
    out += [("F3", c, lay, 0, dict(lse=l, drop_keys=d)) for c in A.F3 for d in A.F3_DROP for lay in ("ctx", "dense") for l in (True, False)]
    out += [("F4", c, lay, 0, dict(causal=True)) for c in A.F4 for lay in ("qkv", "dense")]
    out += [("F5", c, lay, 0, {}) for c, lay, _, _ in A.F5]
    out += [("scale", c, lay, 0, {}) for c, lay in A.SCALE]          # (compared with the reference only: no dense twin)
    return out


@pytest.mark.parametrize("fam,c,layout,slack,kw", _gpu_plans(), ids=lambda v: A.case_id(v) if isinstance(v, A.Case) else str(v))
def test_every_gpu_case_reaches_its_kernel(lib, fam, c, layout, slack, kw):
    """... in the form under test AND in the dense twin it is compared with bit for bit (same kernel, same knobs)"""
    for k, v in c.knobs:
        lib.set_knob(k, v)
    f = A.op_form(c, layout, slack, **kw)
    got = lib.attn_plan_query(c.dtype, c.dh, c.Nk - kw.get("drop_keys", 0), f["ldq"], f["ldk"], f["ldv"], f["ldo"],
                              causal=kw.get("causal", False), lse=kw.get("lse", False), vt_pack=f["vt_pack"])["kernel"]
    assert got == c.kernel, (fam, c, layout, f)


def test_gpu_cases_cover_what_the_forms_are_for():
    """ragged query block, ragged last key tile, more than one workgroup per head where the family asks for it"""
    for fam in (A.F1, A.F2, A.F3, A.F4):
        for key in {(c.kernel, c.dtype) for c in fam}:
            mine = [c for c in fam if (c.kernel, c.dtype) == key]
            assert any(c.Nq % 32 for c in mine), key          # a ragged last wave of queries
            assert any(c.Nk % 64 for c in mine), key          # a ragged last key tile
    assert any(c.Nq > 256 and c.kernel == "ring40" for c in A.F1) and any(c.Nq > 128 and c.kernel == "ring80" for c in A.F1)
    assert any(c.Nq > 256 and c.dtype == dt for c in A.F4 for dt in ("f32",)) and any(c.Nq > 256 and c.dtype == "bf16" for c in A.F4)
    assert any((c.heads * c.B) % 8 == 0 for c in A.F1 if c.kernel == "ring40") and any((c.heads * c.B) % 8 for c in A.F1 if c.kernel == "ring40")
    assert any(c.heads % 4 for c in A.F2 if c.kernel == "short")
    assert {c.kernel for c in A.F1 + A.F2} == {"flash", "w4", "ring40", "ring80", "short"}


def test_counters_and_reset(lib):
    pc = lib.plan_counts(reset=True)
    assert {"attn_flash", "attn_w4", "attn_ring40", "attn_ring80", "attn_short", "xattn_fused", "conv_attn_short"} <= set(pc)
    assert all(lib.plan_counts()[k] == 0 for k in ("attn_flash", "attn_w4", "attn_ring40", "attn_ring80", "attn_short"))
    assert "attn_refused" not in pc


def test_query_rejects_bad_arguments(lib):
    import ctypes as C
    out = C.c_int64()
    with pytest.raises(lib.AfError):
        lib.check(lib.load().af_attn_plan_query(7, 40, 77, 320, 320, 320, 320, 0, C.byref(out)), "af_attn_plan_query")
    with pytest.raises(lib.AfError):
        lib.check(lib.load().af_attn_plan_query(0, 40, 77, 320, 320, 320, 320, 0, None), "af_attn_plan_query")


# ---- the lse bar: achievable and discriminating, on the GPU cases' own operands ----
def _lse_params():
    return [pytest.param(c, d, id=f"{A.case_id(c)}-drop{d}") for c in A.F3 for d in A.F3_DROP]


@pytest.mark.parametrize("c,drop", _lse_params())
def test_lse_bar_is_achievable_and_discriminating(c, drop):
    q, k, v = A.operands(A.seed_of(c, drop), c.B, c.Nq, c.Nk, c.heads, c.dh, c.dtype)
    k = k[:, :c.Nk - drop]
    scale = c.dh ** -0.5
    _, lse2 = A.ref_attention(q, k, v[:, :c.Nk - drop], c.heads, scale)
    E = A.lse_bar(q, k, c.heads, scale, c.kernel, c.dtype, lse2)
    assert E.shape == lse2.shape == (c.B, c.heads, c.Nq) and bool((E > 0).all())
    emu = A.emulate_lse(q, k, c.heads, scale, c.kernel, c.dtype)
    worst = ((emu - lse2).abs() / E).max().item()
    assert worst <= 1.0, worst
    plain = (A.emulate_lse(q, k, c.heads, scale, "flash", "f32") - lse2).abs().max().item()     # fp32 sums alone
    assert plain < 2e-5, plain
    if A.prescaled_q(c.kernel) or A.p_unit(c.kernel, c.dtype, c.dh):      # the emulated roundings really are there
        assert (emu - lse2).abs().max().item() > 5.0 * plain
    for name, wrong in A.wrong_lse(q, k, c.heads, scale, lse2).items():
        ratio = ((wrong - lse2).abs() / (2.0 * E)).min().item()
        assert ratio > 1.0, (name, ratio)


def test_lse_reference_is_the_log2_domain():
    """lse2 against its definition on a case small enough to write out: two keys with scores a, b -> log2(e^a + e^b)"""
    q = torch.tensor([[[1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]])
    k = torch.tensor([[[3.0] + [0.0] * 7, [-1.0] + [0.0] * 7]])
    o, lse2 = A.ref_attention(q, k, k, 1, 0.5)
    import math
    assert abs(lse2.item() - math.log2(math.exp(1.5) + math.exp(-0.5))) < 1e-12
    w = math.exp(1.5) / (math.exp(1.5) + math.exp(-0.5))
    assert abs(o[0, 0, 0].item() - (3.0 * w - 1.0 * (1 - w))) < 1e-12


# ---- the causal cases: no mask and the off-by-one mask move the reference past the bar everywhere ----
@pytest.mark.parametrize("c", A.F4, ids=A.case_id)
def test_causal_cases_tell_the_mask_from_its_neighbours(c):
    q, k, v = A.operands(A.seed_of(c), c.B, c.Nq, c.Nk, c.heads, c.dh, c.dtype)
    ref, _ = A.ref_attention(q, k, v, c.heads, causal=True)
    bar = OP_TOL[c.dtype] * ref.abs().max().item()
    none, _ = A.ref_attention(q, k, v, c.heads)
    ge, _ = A.ref_attention(q, k, v, c.heads, mask="ge")     # (row 0 then sees no key at all: compared from row 1 on)
    for name, wrong, r0 in (("no mask", none, 0), ("j >= i masked", ge, 1)):
        d = (wrong - ref)[:, r0:].abs().view(c.B, c.Nq - r0, c.heads, c.dh).amax(dim=(1, 3))     # [B, H]
        assert bool(torch.isfinite(d).all()) and d.min().item() > bar, (name, d.min().item(), bar)
    # ... and the last rows alone, where the workgroups past the first one and their skipped tiles are
    if c.Nq > 128:
        d = (none - ref)[:, 128:].abs().view(c.B, c.Nq - 128, c.heads, c.dh).amax(dim=(1, 3))
        assert d.min().item() > bar
