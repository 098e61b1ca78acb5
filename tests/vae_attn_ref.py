"""fp64 references and case builders for the VAE mid-block attention (ops.vae_attention -> af_vae_attn_core: scores GEMM,
softmax_rows_kernel, transpose_kernel, P v GEMM).  A plain helper: no fixtures, no tests, no GPU imports.

The block keeps its scores in the storage type.  Three references therefore:

  exact_attention   softmax(C^-1/2 q k^T) v in float64, the oracle's formula (oracle/ldm_oracle.py vae_attn);
  stage_refs        every stage in float64 from that stage's STORED input, rounded once to the storage type: what a correct
                    kernel returns up to its fp32 accumulation error (stage_bound_* below);
  storage_model     the chain of the three stage references: what the design computes, roundings included.

Two constructions make the comparison torch.equal instead of a tolerance (tests/test_vae_attn_cpu.py proves the conditions on
the CPU before tests/test_vae_attn_gpu.py relies on them):

  onehot_case       the whole block is exact in bf16, fp16 and f32;
  int_scores_case   the stored score is ONE rounding of an exact integer times a power of two.
"""
import math

import torch

import exact_operands as X

STORAGES = ("bf16", "f16", "f32")
BK = {"bf16": 64, "f16": 64, "f32": 32}           # K tile of the GEMM kernels (bk_of, csrc/af_host.h)
Q_ONEHOT = 32768.0                                 # 2^15: exact in bf16, fp16 and f32
CLASS_PATTERN = (8, 4, 2, 1, 1)                    # the small classes: one group of 16 keys
_MANT = {"bf16": 8, "f16": 11, "f32": 24}          # significant bits
_EMIN = {"bf16": -126, "f16": -14, "f32": -126}    # exponent of the smallest normal number
U32 = 2.0 ** -24                                   # unit roundoff of fp32
# softmax_rows_kernel per element, relative: the argument x - max is rounded once (|x - max| < 128 where exp is not 0: 128 u),
# expf is good to 1 ulp = 2 u, for the numerator and for every term of the sum (2 * 130 u), the sum of n positive terms adds
# (n - 1) u, 1.0f / s and the product u each, and one more for the second-order terms
SOFTMAX_EXTRA = 264


# the cases of tests/test_vae_attn_gpu.py, (B, N, C); tests/test_vae_attn_cpu.py proves the conditions for every one of them
ONEHOT_SHAPES = ((1, 64, 128), (3, 576, 128), (2, 1024, 512), (1, 96, 64), (1, 1024, 512), (1, 1920, 512), (1, 4096, 512))
INT_SCORES_SHAPES = ((2, 576, 256), (1, 1024, 1024))
GAUSS_SHAPES = ((2, 576, 128), (1, 1024, 512))
GAUSS_QSCALES = (1, 8)
GAUSS_SEED = 4
# max |storage_model - exact| / max |exact| of the design on Gaussian operands, a CPU model of the storage roundings:
# (B, N, C, qscale) -> (max |score|, bf16, f16).  Over seeds 0..7 the figures spread by -43 % .. +53 % around these (a maximum
# over 1.5e5 .. 5e5 outputs), so GAUSS_SEED is part of what the +-30 % assertion of tests/test_vae_attn_cpu.py pins.
GAUSS_TABLE = {(2, 576, 128, 1): (5.0, 1.2e-2, 1.3e-3), (2, 576, 128, 8): (40.0, 2.6e-2, 3.0e-3),
               (1, 1024, 512, 1): (5.4, 9.5e-3, 1.3e-3), (1, 1024, 512, 8): (43.0, 3.0e-2, 3.4e-3)}


def onehot_seed(B, N, C):
    return 7 * B + N + C


def alpha_f32(C):
    """1.0f / sqrtf((float)C) as af_vae_attn_core computes it (a power of two for C = 64, 256, 1024)."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(C), dtype=torch.float32)))


def spacing(ref, storage):
    """One step of the storage type at `ref` (float64 tensor): the distance to the next value away from zero."""
    a = ref.abs().double()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -140)))
    e = torch.clamp(e, min=float(_EMIN[storage]))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - (_MANT[storage] - 1))


# ----------------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------------
def exact_attention(q, k, v):
    """softmax(q k^T * C^-0.5, keys) v in float64 on the operands as given; q, k, v [B, N, C]."""
    q, k, v = q.double(), k.double(), v.double()
    w = torch.bmm(q, k.transpose(1, 2)) * (int(q.shape[2]) ** -0.5)
    return torch.bmm(torch.softmax(w, dim=2), v)


def scores_ref(q_st, k_st, storage):
    """The stored scores from the stored q and k: alpha (the kernel's fp32 value) times the fp64 sum, rounded once."""
    return X.roundtrip(torch.bmm(q_st.double(), k_st.double().transpose(1, 2)) * alpha_f32(q_st.shape[2]), storage)


def probs_ref(scores_st, storage):
    return X.roundtrip(torch.softmax(scores_st.double(), dim=2), storage)


def out_ref(probs_st, v_st, storage):
    return X.roundtrip(torch.bmm(probs_st.double(), v_st.double()), storage)


def stage_refs(q, k, v, storage, scores=None, probs=None):
    """{"scores", "probs", "out"}: each stage in float64 from its stored input, rounded once to `storage`.  q, k, v are
    rounded to storage first (as the op casts them).  scores / probs: the stored tensors a kernel produced; given, the NEXT
    stage's reference is computed from them instead of from the previous reference (a GPU tap checks one stage at a time)."""
    qs, ks, vs = (X.roundtrip(t, storage) for t in (q, k, v))
    s = scores_ref(qs, ks, storage)
    p = probs_ref(s if scores is None else scores.double(), storage)
    o = out_ref(p if probs is None else probs.double(), vs, storage)
    return {"scores": s, "probs": p, "out": o}


def storage_model(q, k, v, storage):
    """What the design computes: the chain of the three stage references."""
    return stage_refs(q, k, v, storage)["out"]


def stage_bound_scores(q_st, k_st, ref, storage):
    """|got - ref| of a correct scores GEMM, elementwise: one step of the storage type (the fp32 value may round the other
    way) + the worst-case fp32 accumulation error n u sum |q||k| |alpha| over n = C products (cf. exact_operands.absbound_linear)."""
    n = q_st.shape[2]
    ab = torch.bmm(q_st.double().abs(), k_st.double().abs().transpose(1, 2)) * alpha_f32(n)
    return spacing(ref, storage) + n * U32 * ab


def stage_bound_probs(ref, storage):
    """The same for the softmax over n columns: one step + (n + SOFTMAX_EXTRA) u relative (see SOFTMAX_EXTRA)."""
    return spacing(ref, storage) + (ref.shape[2] + SOFTMAX_EXTRA) * U32 * ref.abs()


def stage_bound_out(probs_st, v_st, ref, storage):
    """The same for the P v GEMM: n = N products."""
    n = probs_st.shape[2]
    return spacing(ref, storage) + n * U32 * torch.bmm(probs_st.double().abs(), v_st.double().abs())


# ----------------------------------------------------------------------------------------------------------------------
# the exact case
# ----------------------------------------------------------------------------------------------------------------------
def class_sizes(N, C):
    """Powers of two from {1, 2, 4, 8, 16} that sum to N: of the N / 16 groups of 16 keys three quarters are one class of 16,
    the others split as CLASS_PATTERN.  N / 8 classes, give or take; at most C."""
    assert N % 16 == 0, N
    groups = N // 16
    n16 = (3 * groups) // 4
    if N == 16:
        n16 = 0
    sizes = [16] * n16
    for _ in range(groups - n16):
        sizes += list(CLASS_PATTERN)
    assert sum(sizes) == N and len(sizes) <= C, (N, C, len(sizes))
    return sizes


def onehot_case(B, N, C, seed):
    """Attention that is exact in every storage type.  Per sample the keys are partitioned into classes (class_sizes), the
    members scattered by a random permutation of all key positions; k_j = the unit vector of its class, q_i = 32768 times the
    unit vector of the class of a random key, v in {+-1, +-2, +-3}.  A matching key scores fl(alpha 32768) >= 1024, every
    other key 0, so exp of the gap is 0 in fp32 and in fp64, P is exactly 1 / m on the m members and the output (sum v) / m.
    Returns q, k, v (float32), ref_probs [B, N, N] and ref_out [B, N, C] (float64, from the construction, not from a
    softmax), cls_k / cls_q (the class of every key / query) and sizes."""
    g = torch.Generator().manual_seed(seed)
    sizes = class_sizes(N, C)
    assert alpha_f32(C) * Q_ONEHOT >= 1024.0, C
    size_t = torch.tensor(sizes)
    cls_sorted = torch.repeat_interleave(torch.arange(len(sizes)), size_t)          # [N]
    q = torch.zeros(B, N, C)
    k = torch.zeros(B, N, C)
    cls_k = torch.zeros(B, N, dtype=torch.long)
    cls_q = torch.zeros(B, N, dtype=torch.long)
    chan = torch.zeros(B, len(sizes), dtype=torch.long)
    for b in range(B):
        cls_k[b, torch.randperm(N, generator=g)] = cls_sorted
        chan[b] = torch.randperm(C, generator=g)[:len(sizes)]                       # which channel is the class's unit vector
        cls_q[b] = cls_k[b, torch.randint(0, N, (N,), generator=g)]
        k[b, torch.arange(N), chan[b, cls_k[b]]] = 1.0
        q[b, torch.arange(N), chan[b, cls_q[b]]] = Q_ONEHOT
    v = torch.randint(1, 4, (B, N, C), generator=g).float() * (torch.randint(0, 2, (B, N, C), generator=g).float() * 2 - 1)
    match = (cls_q.unsqueeze(2) == cls_k.unsqueeze(1))                               # [B, Nq, Nk]
    m = size_t.double()[cls_q]                                                       # [B, Nq]
    ref_probs = match.double() / m.unsqueeze(2)
    ref_out = torch.bmm(match.double(), v.double()) / m.unsqueeze(2)
    return {"q": q, "k": k, "v": v, "ref_probs": ref_probs, "ref_out": ref_out, "cls_k": cls_k, "cls_q": cls_q, "sizes": sizes}


def check_onehot_case(c):
    """The preconditions of the bit-exact comparison, asserted on the case alone (hard asserts, as
    exact_operands.check_exact_case): operands, P and the output are exact in every storage type, enough outputs are non-zero
    and distinct.  Returns the figures."""
    out, p = c["ref_out"], c["ref_probs"]
    for st in STORAGES:
        for name in ("q", "k", "v"):
            assert torch.equal(X.roundtrip(c[name], st), c[name].double()), f"{name} is not exact in {st}"
        assert torch.equal(X.roundtrip(p, st), p), f"P is not exact in {st}"
        assert torch.equal(X.roundtrip(out, st), out), f"the output is not exact in {st}"
    nonzero = float((out != 0).double().mean())
    distinct = int(torch.unique(out).numel())
    assert nonzero >= X.MIN_NONZERO_OUTPUTS, f"only {nonzero:.3f} of the outputs are non-zero"
    assert distinct >= X.MIN_DISTINCT_OUTPUTS, f"only {distinct} distinct output values"
    return {"nonzero": nonzero, "distinct": distinct, "classes": len(c["sizes"])}


# ----------------------------------------------------------------------------------------------------------------------
# exact scores
# ----------------------------------------------------------------------------------------------------------------------
def int_scores_case(B, N, C, seed, storage="bf16"):
    """q, k integers in {-1, 0, 1} at exact_operands.density_for(C), about one q in 64 replaced by +-4097
    (exact_operands.add_wide: stored as +-4096 in bf16, exact in f32), C in {64, 256, 1024} so that alpha is a power of two:
    sum q k over the STORED operands is an integer below 2^24, exact in fp32 in any order, alpha times it is exact, and the
    stored score is one rounding of that.  v: small integers.  Returns q, k, v and ref_scores (float64)."""
    assert C in (64, 256, 1024), C
    a = alpha_f32(C)
    assert math.log2(a) == round(math.log2(a)), a
    g = torch.Generator().manual_seed(seed)
    d = X.density_for(C)
    q = X.add_wide(X.int_tensor((B, N, C), d, g), g)
    k = X.int_tensor((B, N, C), d, g)
    v = X.int_tensor((B, N, C), 1.0, g, -3, 3)
    qs, ks = X.roundtrip(q, storage), X.roundtrip(k, storage)
    s = torch.bmm(qs, ks.transpose(1, 2))
    bound = torch.bmm(qs.abs(), ks.abs().transpose(1, 2))
    assert float(bound.max()) < X.TWO24, float(bound.max())
    assert torch.equal(s, s.round())
    ref = X.roundtrip(s * a, storage)
    return {"q": q, "k": k, "v": v, "ref_scores": ref, "exact_scores": s * a}


def gaussian_case(B, N, C, qscale, seed):
    """q, k, v ~ N(0, 1), q times qscale (float32; the caller rounds to a storage type)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, N, C, generator=g) * float(qscale)
    k = torch.randn(B, N, C, generator=g)
    v = torch.randn(B, N, C, generator=g)
    return q, k, v


def model_vs_exact(q, k, v, storage):
    """max |storage_model - exact| / max |exact| on the storage-rounded operands, max |score|, and the two outputs."""
    qs, ks, vs = (X.roundtrip(t, storage) for t in (q, k, v))
    ex = exact_attention(qs, ks, vs)
    mo = storage_model(q, k, v, storage)
    smax = float((torch.bmm(qs, ks.transpose(1, 2)) * (int(q.shape[2]) ** -0.5)).abs().max())
    return float((mo - ex).abs().max() / ex.abs().max()), smax, mo, ex


# ----------------------------------------------------------------------------------------------------------------------
# the mistakes a kernel could make, applied to the exact case's reference (tests/test_vae_attn_cpu.py)
# ----------------------------------------------------------------------------------------------------------------------
def mistaken_outputs(c, drop):
    """{"drop_tail": the last `drop` keys missing from the P v contraction, "next_sample": sample b reads K / V of sample
    b + 1 (B > 1 only), "transposed": P^T v} for a one-hot case, each [B, N, C] float64."""
    p, v = c["ref_probs"], c["v"].double()
    N = p.shape[1]
    out = {"drop_tail": torch.bmm(p[:, :, :N - drop], v[:, :N - drop]), "transposed": torch.bmm(p.transpose(1, 2), v)}
    if p.shape[0] > 1:
        out["next_sample"] = exact_attention(c["q"], torch.roll(c["k"], -1, 0), torch.roll(c["v"], -1, 0))
    return out


def changed_row_share(a, b):
    """Per sample: the share of query rows in which a and b differ somewhere."""
    return (a != b).any(dim=2).double().mean(dim=1)


def drop_floor(T, N):
    """What the share of rows a dropped tile of T keys changes is asserted against: 25 %, or half of what counting allows where
    that is less -- T keys lie in at most T classes of at most 16 of the N keys each, so they reach at most 16 T / N of the
    queries (N = 4096: 25 % for T = 64, 12.5 % for T = 32)."""
    return min(0.25, 8.0 * T / N)
