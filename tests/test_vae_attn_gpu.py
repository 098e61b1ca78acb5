"""The VAE mid-block attention at operator level (ops.vae_attention -> af_op_vae_attention -> af_vae_attn_core, the function
run_vae_attn calls): the batched scores GEMM on the K third of the qkv tensor (ldw = 3C, pointer offset C, alpha = C^-1/2),
softmax_rows_kernel on scores kept in the storage type, transpose_kernel, the batched P v GEMM over the N positions.

  exact      tests/vae_attn_ref.py's one-hot case, torch.equal over every element of P and of the output, in bf16, fp16 and f32;
             the integer scores case, torch.equal over every stored score (alpha, ldw, the offset, the store's rounding).
  Gaussian   every stage against its fp64 reference from the GPU's own stored input of that stage, elementwise, at a bound
             DERIVED from the formats (one step of the storage type + the worst-case fp32 accumulation error); the output
             against exact attention at the CPU-measured distance of the storage model from it + that bound.
  refusals   N not a multiple of the K tile.

tests/test_vae_attn_cpu.py proves the references.  Every case asserts which kernel ran each GEMM, in one K slice.  The
expectations are read off plan_tiled / rowpanel_kind (csrc/af_conv_gemm.hip), default knobs unless noted:
  * a batched launch (B > 1) is never a ping-pong, 128 x 160 or split-K launch; the cost model (rounds over 256 CUs x tile
    area / efficiency) picks 64 x 64 for N = 576 columns (not a multiple of 128) and 64 x 128 where the columns are;
  * B = 1, <= 1024 rows, K <= 32 tiles: small_m_tile64 -> 64 x 64; with gemm_pp_minfill = 0 the ping-pong 256 x 128 tile
    replaces it (bf16, N % 128 == 0, no K slices: K / 64 < 32);
  * (1, 1920, 512): scores [1920, 512] -> 1920: 180 tiles of 128 x 160 -> gemm_m128_kernel (reported under tile 0);
    P v [1920, 1920] -> 512: 128 x 128 planned for three K slices, run in ONE (the core passes no workspace);
  * (1, 4096, 512) bf16: both on the ping-pong 256 x 128 tile (P v planned for four K slices, run in one); f32: 128 x 128
    and 64 x 128.
"""
import functools

import pytest
import torch

import exact_operands as X
import test_fp16_gpu as T16
import test_ops_gpu as T
import vae_attn_ref as R

pytestmark = pytest.mark.gpu

_onehot = functools.lru_cache(maxsize=2)(lambda shape: R.onehot_case(*shape, seed=R.onehot_seed(*shape)))
W4 = "wave4"


def _run(gpu, q, k, v, dtype):
    from adaface_amd import _lib, ops
    _lib.plan_counts(reset=True)
    r = ops.vae_attention(q.to(gpu), k.to(gpu), v.to(gpu), dtype=dtype, taps=True)
    pc = _lib.plan_counts(reset=True)
    return r, pc


def _assert_plans(name, r, pc, want):
    """want: ((kernel, tile), (kernel, tile)) of the scores and the P v GEMM; one K slice each, two GEMM launches in all"""
    got = r["plans"]
    assert tuple(p[:2] for p in got) == tuple(want) and all(p[2] == 1 for p in got), (name, got, want)
    assert pc["splitk"] == 0 and sum(pc[f"tile{i}"] for i in range(6)) + pc["halo"] == 2, (name, pc)
    assert pc["rowpanel"] == sum(1 for w in want if w[0] == "m128"), (name, pc)


# (B, N, C), storage types, knobs, (scores plan, P v plan)
_T3, _T1, _T0 = (W4, 3), (W4, 1), (W4, 0)
_ALL = ("bf16", "f16", "f32")
_ONEHOT = [
    ((1, 64, 128), _ALL, (), (_T3, _T1)),                          # the tiny model's shape: one tile each
    ((3, 576, 128), _ALL, (), (_T3, _T1)),                         # batched four-wave: 9 x 9 and 9 x 1 tiles per sample
    # ... forced onto 128 x 128 tiles: 576 = 4.5 tiles, ragged rows and ragged K rows, the next sample's K rows behind them
    ((3, 576, 128), _ALL, (("gemm_tile", 0),), (_T0, _T0)),
    ((2, 1024, 512), _ALL, (), (_T1, _T1)),                        # real C; four softmax passes per thread
    ((1, 96, 64), ("f32",), (), (_T3, _T3)),                       # below one tile (96 is not a multiple of 64)
    ((1, 1024, 512), ("bf16",), (("gemm_pp_minfill", 0),), (("pp", 4), ("pp", 4))),
    ((1, 1920, 512), ("bf16",), (), (("m128", 0), _T0)),           # gemm_m128_kernel with alpha != 1
    ((1, 4096, 512), ("bf16",), (), (("pp", 4), ("pp", 4))),       # the production launch
    ((1, 4096, 512), ("f32",), (), (_T0, _T1)),
]
_ONEHOT_PARAMS = [pytest.param(s, dt, kn, want, id=f"{'x'.join(map(str, s))}-{dt}{''.join('-' + k + str(v) for k, v in kn)}")
                  for (s, dts, kn, want) in _ONEHOT for dt in dts]


def test_the_case_list_is_the_one_the_cpu_test_proves():
    assert {s for s, _, _, _ in _ONEHOT} == set(R.ONEHOT_SHAPES)


@pytest.mark.parametrize("shape,dtype,kn,want", _ONEHOT_PARAMS)
def test_onehot_attention_is_bit_exact(gpu, report, knobs, shape, dtype, kn, want):
    """P = 1 / m on the m keys of the query's class and 0 elsewhere, output = (sum v) / m: exact in every storage type, so the
    comparison is torch.equal over every element of P and of the output.  (softmax_rows_kernel: expf(0) = 1, the sum of m ones,
    1.0f / m and 1 * (1 / m) are exact for m a power of two; expf(-2896 ..) = 0.)"""
    for k_, v_ in kn:
        knobs(k_, v_)
    c = _onehot(shape)
    r, pc = _run(gpu, c["q"], c["k"], c["v"], dtype)
    name = f"vae_attn onehot {shape} [{dtype}]{' ' + str(kn) if kn else ''}"
    _assert_plans(name, r, pc, want)
    X.assert_bit_exact(name + " probs", r["probs"], c["ref_probs"], r["plans"], report)
    X.assert_bit_exact(name + " out", r["out"], c["ref_out"], r["plans"], report)


@pytest.mark.parametrize("shape,want", [((2, 576, 256), (_T3, _T1)), ((1, 1024, 1024), (("pp", 4), ("pp", 4)))],
                         ids=["2x576x256", "1x1024x1024"])
def test_int_scores_are_bit_exact(gpu, report, knobs, shape, want):
    """Integer q and k (+-4097 among them, stored as +-4096), alpha = 1/16 and 1/32: the stored score is one round-to-nearest-even
    of an exact fp32 value, compared bit for bit.  Covers alpha, ldw = 3C, the K third's pointer offset and the store."""
    assert shape in R.INT_SCORES_SHAPES
    knobs("gemm_pp_minfill", 0)
    c = R.int_scores_case(*shape, seed=sum(shape))
    r, pc = _run(gpu, c["q"], c["k"], c["v"], "bf16")
    name = f"vae_attn int scores {shape} [bf16]"
    _assert_plans(name, r, pc, want)
    X.assert_bit_exact(name, r["scores"], c["ref_scores"], r["plans"], report)


@functools.lru_cache(maxsize=4)
def _gauss(shape, qscale):
    return R.gaussian_case(*shape, qscale, R.GAUSS_SEED)


@functools.lru_cache(maxsize=8)
def _gauss_model(shape, qscale, dtype):
    """max |storage model - exact| (absolute) and exact attention of the storage-rounded operands, on the CPU"""
    q, k, v = _gauss(shape, qscale)
    rel, _, _, exact = R.model_vs_exact(q, k, v, dtype)
    return rel * float(exact.abs().max()), exact


def _within(report, name, got, ref, bound):
    got = got.detach().cpu().double()
    finite = bool(torch.isfinite(got).all())
    d = (got - ref).abs()
    worst = float((d / bound).max()) if finite else float("inf")
    report(name, float(d.max()) if finite else float("inf"), float(ref.abs().max()), float(bound.max()))
    report(name + " worst |got - ref| / bound", worst, 1.0, 1.0)
    assert finite, f"{name}: non-finite values"
    bad = (d > bound).nonzero()
    assert bad.numel() == 0, (f"{name}: {bad.shape[0]} of {ref.numel()} elements outside the bound, worst {worst:.3f} x; first "
                              f"{[(tuple(int(i) for i in c), float(got[tuple(c)]), float(ref[tuple(c)]), float(bound[tuple(c)])) for c in bad[:4]]}")


@pytest.mark.parametrize("dtype", _ALL)
@pytest.mark.parametrize("qscale", R.GAUSS_QSCALES)
@pytest.mark.parametrize("shape,want", [((2, 576, 128), (_T3, _T1)), ((1, 1024, 512), (_T3, _T3))], ids=["2x576x128", "1x1024x512"])
def test_gaussian_stage_by_stage(gpu, report, shape, want, qscale, dtype):
    """Each tap against the fp64 reference of its stage computed from the GPU's own stored input, rounded once.
    16-bit: |got - ref| <= one step of the storage type at ref + n 2^-24 sum |a||b| (n = C products for the scores, N for P v;
    the softmax: (N + 264) 2^-24 |ref|, vae_attn_ref.SOFTMAX_EXTRA) -- the worst-case fp32 accumulation error plus one rounding
    that may fall the other way; nothing here is tuned.  f32: TOL["f32"] of tests/test_ops_gpu.py of each stage's scale.
    The output against exact attention: the CPU-measured distance of the storage model from it for this very case + the P v
    stage bound."""
    assert shape in R.GAUSS_SHAPES
    q, k, v = _gauss(shape, qscale)
    r, pc = _run(gpu, q, k, v, dtype)
    name = f"vae_attn gaussian {shape} q*{qscale} [{dtype}]"
    _assert_plans(name, r, pc, want)
    qs, ks, vs = (X.roundtrip(t, dtype) for t in (q, k, v))
    sc, pr, out = (r[n].detach().cpu().double() for n in ("scores", "probs", "out"))
    for n, t in (("scores", sc), ("probs", pr), ("out", out)):           # the taps are storage values
        assert torch.equal(X.roundtrip(t, dtype), t), (name, n)
    refs = R.stage_refs(q, k, v, dtype, scores=sc, probs=pr)
    if dtype == "f32":
        tol = T.TOL["f32"]
        bounds = {n: torch.full_like(refs[n], tol * float(refs[n].abs().max())) for n in refs}
    else:
        bounds = {"scores": R.stage_bound_scores(qs, ks, refs["scores"], dtype), "probs": R.stage_bound_probs(refs["probs"], dtype),
                  "out": R.stage_bound_out(pr, vs, refs["out"], dtype)}
    _within(report, name + " scores", sc, refs["scores"], bounds["scores"])
    _within(report, name + " probs", pr, refs["probs"], bounds["probs"])
    _within(report, name + " out", out, refs["out"], bounds["out"])
    dist, exact = _gauss_model(shape, qscale, dtype)
    scale = float(exact.abs().max())
    report(name + " model vs exact (CPU), of max|exact|", dist / scale, 1.0, {"bf16": T.TOL["bf16"], "f16": T16.F16_OP_TOL, "f32": T.TOL["f32"]}[dtype])
    report(name + " out vs exact, of max|exact|", float((out - exact).abs().max()) / scale, 1.0, dist / scale)
    _within(report, name + " out vs exact", out, exact, dist + bounds["out"])


@pytest.mark.parametrize("N,dtype", [(48, "bf16"), (48, "f16"), (48, "f32"), (96, "bf16"), (96, "f16")])
def test_positions_that_are_no_multiple_of_the_k_tile_are_refused(gpu, N, dtype):
    """The P v GEMM contracts over the N positions in whole K tiles (64; f32: 32): AfError with the message, nothing launched."""
    from adaface_amd import _lib, ops
    x = torch.zeros(1, N, 64, device=gpu)
    _lib.plan_counts(reset=True)
    with pytest.raises(_lib.AfError, match=f"{N} positions must be a multiple of {R.BK[dtype]}"):
        ops.vae_attention(x, x, x, dtype=dtype)
    pc = _lib.plan_counts(reset=True)
    assert sum(pc[f"tile{i}"] for i in range(6)) + pc["halo"] == 0, pc
