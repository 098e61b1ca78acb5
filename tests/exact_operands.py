"""Operands for which floating point is exact, and the oracle that goes with them (a plain helper: no fixtures, no tests).

With small-integer activations, weights, bias and residual every product of a GEMM / convolution is an integer and every
partial sum -- in ANY summation order, tile shape, K slicing or MFMA shape -- is an integer bounded by
sum |x||w| + |b| + |r|.  While that bound is below 2^24 an fp32 accumulator holds every partial sum exactly, and while the
result is representable in the storage type (bf16: an 8-bit integer times a power of two) the store is exact too.  The
float64 reference is then not close to what a correct kernel returns, it IS what a correct kernel returns: the comparison
is torch.equal, and one dropped, doubled or misplaced product at one output fails it.

The preconditions (check_exact_case) are computed on the CPU from the operands and the fp64 reference alone, never from
the output under test, and are hard asserts.  If a shape breaks one, change the operands (density, value range), not the
condition.
"""
import math

import torch
import torch.nn.functional as F

TWO24 = float(2 ** 24)
MIN_NONZERO_OUTPUTS = 0.90      # share of outputs that are non-zero
MIN_DISTINCT_OUTPUTS = 40       # distinct output values
MIN_OPERAND_NONZERO = 0.20      # share of non-zero entries of each operand (0.22 at K = 23040: 0.33 kept x 2/3 of {-1, 0, 1})
WIDE_VALUE = 4097.0             # 13 significant bits: not a bf16 value, not a 10-bit-mantissa MFMA operand
CARRIER_X = 2.0
CARRIER_W3 = 128.0              # 3x3: nine taps x 2 x 128 = 2304 between the first and the last chunk (bf16 spacing there: 16)
CARRIER_W1 = 1024.0             # one tap (1x1, linear): 2 x 1024 = 2048


def int_tensor(shape, density, gen, lo=-1, hi=1):
    """Uniform integers in [lo, hi] (float32), each kept with probability `density`, the rest zero."""
    v = torch.randint(lo, hi + 1, tuple(shape), generator=gen).float()
    if density >= 1.0:
        return v
    keep = torch.rand(tuple(shape), generator=gen) < density
    return v * keep


def density_for(K, alpha=1.0):
    """Keep probability that holds the output's standard deviation near 33 for any K with operands in {-1, 0, 1}
    (variance K * (d * 2/3)^2 = 1100), so that bf16 (integers up to 256) stores every output exactly.  A launch with
    |alpha| > 1 multiplies that deviation, so its operands are thinned by 1 / |alpha| (density, never a mask)."""
    return min(1.0, math.sqrt(1100.0 / (K * 4.0 / 9.0))) / max(1.0, abs(alpha))


ALPHAS = (0.5, -2.0)            # powers of two: alpha * (an integer below 2^24) is exact in fp32


def rowbias_rows(B, N):
    """The per-sample bias row of the exact cases, [B, N]: small integers, and any two samples fewer than 17 apart (the
    samples of one tile are at most four apart) differ in EVERY column, so a row taken from the wrong sample shows at every
    output of that sample."""
    b = torch.arange(B).view(B, 1)
    n = torch.arange(N).view(1, N)
    return (((7 * b + 3 * n) % 17) - 8).float()


def out_hw(H, W, ks, stride, up, pad=None):
    """Output map of a convolution; pad None = ks // 2 on every side, pad 0 (3x3, stride 2, even maps) = one row / column of
    zeros below and to the right only: (H + 1 - 3) // 2 + 1."""
    hi, wi = H << int(up), W << int(up)
    if pad == 0 and ks == 3:
        assert stride == 2 and not up and H % 2 == 0 and W % 2 == 0, (H, W, stride, up)
        return (hi + 1 - ks) // stride + 1, (wi + 1 - ks) // stride + 1
    assert pad is None or pad == ks // 2, pad
    return (hi + 2 * (ks // 2) - ks) // stride + 1, (wi + 2 * (ks // 2) - ks) // stride + 1


def roundtrip(t, storage):
    """t through the kernel's storage type and back, in float64."""
    if storage in ("bf16", "fp8"):
        return t.to(torch.float32).to(torch.bfloat16).double()
    if storage == "f32":
        return t.to(torch.float32).double()
    if storage == "f16":
        return t.to(torch.float32).to(torch.float16).double()
    raise ValueError(storage)


def fp64_ref_conv(x, w, b=None, r=None, stride=1, up=False, rowbias=None, alpha=1.0, pad=None):
    """alpha * F.conv2d(nearest-2x(x) if up else x, w, None, stride, padding) + b [+ rowbias[sample]] [+ r] in float64.
    pad None: ks // 2 on every side; pad 0: F.pad(x, (0, 1, 0, 1)), zeros below and to the right only."""
    xi = x.double()
    if up:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    if pad == 0 and w.shape[-1] == 3:
        xi, padding = F.pad(xi, (0, 1, 0, 1)), 0
    else:
        assert pad is None or pad == w.shape[-1] // 2, pad
        padding = w.shape[-1] // 2
    y = F.conv2d(xi, w.double(), None, stride=stride, padding=padding)
    if alpha != 1.0:
        y = y * float(alpha)
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    if rowbias is not None:
        y = y + rowbias.double().view(rowbias.shape[0], -1, 1, 1)
    return y if r is None else y + r.double()


def fp64_ref_linear(x, w, b=None, r=None, alpha=1.0):
    """alpha * F.linear(x, w) + b [+ r] in float64."""
    y = F.linear(x.double(), w.double(), None)
    if alpha != 1.0:
        y = y * float(alpha)
    if b is not None:
        y = y + b.double()
    return y if r is None else y + r.double()


def _abs(t):
    return None if t is None else t.abs()


def absbound_conv(x, w, b=None, r=None, stride=1, up=False, rowbias=None, alpha=1.0, pad=None):
    """|alpha| conv(|x|, |w|) + |b| + |rowbias| + |r|: what any partial sum of any summation order is bounded by."""
    return fp64_ref_conv(x.abs(), w.abs(), _abs(b), _abs(r), stride, up, _abs(rowbias), abs(alpha), pad)


def absbound_linear(x, w, b=None, r=None, alpha=1.0):
    return fp64_ref_linear(x.abs(), w.abs(), _abs(b), _abs(r), abs(alpha))


def check_exact_case(ref, absbound, storage, operands=(), power_operands=None):
    """The preconditions under which torch.equal against `ref` is the right test, asserted on the reference alone.
    operands: every tensor the kernel reads (None entries are ignored); power_operands: the ones whose share of non-zero
    entries is asserted (default: all of them).  Returns the figures it checked."""
    out_storage = "bf16" if storage == "fp8" else storage
    ops = [t for t in operands if t is not None]
    for i, t in enumerate(ops):                                                  # 1. operands exact in the storage type
        assert torch.equal(roundtrip(t, storage), t.double()), f"operand {i} is not exact in {storage}"
    mx = float(absbound.max())
    assert mx < TWO24, f"sum |x||w| + |b| + |r| reaches {mx:.0f} >= 2^24: fp32 partial sums are not exact"    # 2.
    assert torch.equal(roundtrip(ref, out_storage), ref), f"the reference is not exact in {out_storage}"       # 3.
    nonzero = float((ref != 0).double().mean())                                  # 4. power
    distinct = int(torch.unique(ref).numel())
    assert nonzero >= MIN_NONZERO_OUTPUTS, f"only {nonzero:.3f} of the outputs are non-zero"
    assert distinct >= MIN_DISTINCT_OUTPUTS, f"only {distinct} distinct output values"
    shares = []
    for i, t in enumerate(ops if power_operands is None else [t for t in power_operands if t is not None]):
        share = float((t != 0).double().mean())
        shares.append(share)
        assert share >= MIN_OPERAND_NONZERO, f"operand {i}: only {share:.3f} of its entries are non-zero"
    return {"absbound": mx, "max_abs_ref": float(ref.abs().max()), "nonzero": nonzero, "distinct": distinct,
            "operand_nonzero": shares}


def assert_bit_exact(name, got, ref, plan=None, report=None):
    """torch.equal(got, ref) over EVERY element.  On failure the message gives the number of mismatching elements, the
    first coordinates with got / ref, the bounding box of the mismatches per axis and the plan (tile, K slices, halo)."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    bad = ~(got == ref)                       # (NaN != anything: a non-finite output is a mismatch)
    n_bad = int(bad.sum())
    scale = float(ref.abs().max())
    if n_bad:
        d = (got - ref).abs()
        err = float(torch.nan_to_num(d, nan=float("inf"))[bad].max())
    else:
        err = 0.0
    if report is not None:
        report(name, err, scale, 0.0)
    if not n_bad:
        return
    idx = bad.nonzero()
    first = "; ".join(f"{tuple(int(v) for v in c)}: got {float(got[tuple(c)])!r} ref {float(ref[tuple(c)])!r}" for c in idx[:8])
    box = ", ".join(f"axis {a}: [{int(idx[:, a].min())}, {int(idx[:, a].max())}]" for a in range(idx.shape[1]))
    raise AssertionError(f"{name}: {n_bad} of {ref.numel()} elements differ from the exact reference (max |diff| {err:g}); "
                         f"first: {first}; bounding box: {box}; plan (tile, K slices, halo): {plan}")


# ----------------------------------------------------------------------------------------------------------------------
# operand builders
# ----------------------------------------------------------------------------------------------------------------------
def add_wide(x, gen, share=1.0 / 64):
    """About one activation in 64 becomes +-4097 (13 significant bits).  With weights in {-1, 0, 1} every product is still an
    exact integer, but only with true fp32 operands: a path that narrows them to bf16 (4097 -> 4096) or to a 10-bit-mantissa
    MFMA format returns something else."""
    at = torch.rand(x.shape, generator=gen) < share
    sign = torch.randint(0, 2, x.shape, generator=gen).float() * 2 - 1
    return torch.where(at, sign * WIDE_VALUE, x)


def add_carrier(x, w):
    """The cancelling carrier.  x: [B, C, ...] activations (or [M, K] rows), w: [N, C, ...] weights, C >= 128.  One channel of
    the first 64-channel chunk and one of the last hold x = 2 everywhere; their weights are +A and -A on every tap of every
    output channel (A = 128 for 3x3, 1024 for one tap).  The two cancel exactly, at the zero-padded border too, so they add
    nothing to the reference -- but between the first and the last chunk every partial sum carries +-2304 (+-2048), where
    bf16 spacing is 16: an accumulator, a transposition tile or a split-K slab narrower than fp32 loses the small terms.
    Where K is sliced the two channels lie in different slices."""
    C = x.shape[1]
    assert C >= 128 and w.shape[1] == C
    c0, c1 = 5, C - 7
    taps = 1
    for s in w.shape[2:]:
        taps *= s
    a = CARRIER_W3 if taps > 1 else CARRIER_W1
    x, w = x.clone(), w.clone()
    x[:, c0] = CARRIER_X
    x[:, c1] = CARRIER_X
    w[:, c0] = a
    w[:, c1] = -a
    return x, w


def conv_case(B, Cin, H, W, Cout, ks, stride, up, bias, res, seed, storage="bf16", wide=False, carrier=False, rowbias=False,
              alpha=1.0, pad=None):
    """Integer operands, fp64 reference and |.| bound of one convolution case; the preconditions are asserted before it
    returns.  K = 64 without a bias widens the operand range to [-2, 2] (the shortest K is where the power conditions are
    tightest).  rowbias: the per-sample row rowbias_rows(B, Cout) ("rb"); alpha in ALPHAS (or 1) scales the convolution before
    the bias; pad 0: bottom / right padding (out_hw)."""
    assert alpha == 1.0 or alpha in ALPHAS, alpha
    g = torch.Generator().manual_seed(seed)
    K = Cin * ks * ks
    d = density_for(K, alpha)
    lo, hi = (-2, 2) if (K <= 64 and not bias) else (-1, 1)
    x = int_tensor((B, Cin, H, W), d, g, lo, hi)
    w = int_tensor((Cout, Cin, ks, ks), d, g, lo, hi)
    b = int_tensor((Cout,), 1.0, g, -8, 8) if bias else None
    if wide:
        x = add_wide(x, g)
    if carrier:
        x, w = add_carrier(x, w)
    ho, wo = out_hw(H, W, ks, stride, up, pad)
    r = int_tensor((B, Cout, ho, wo), 1.0, g, -16, 16) if res else None
    rb = rowbias_rows(B, Cout) if rowbias else None
    ref = fp64_ref_conv(x, w, b, r, stride, up, rb, alpha, pad)
    bound = absbound_conv(x, w, b, r, stride, up, rb, alpha, pad)
    stats = check_exact_case(ref, bound, storage, operands=(x, w, b, r, rb))
    return {"x": x, "w": w, "b": b, "r": r, "rb": rb, "alpha": alpha, "pad": pad, "ref": ref, "absbound": bound, "stats": stats}


def add_rowbias(c, storage="bf16"):
    """A convolution case with the per-sample row added to it: same operands, reference + rowbias[sample]; the preconditions
    are asserted again on the new reference (one fp64 convolution serves the case with and without the row)."""
    assert c["rb"] is None
    B, N = c["ref"].shape[:2]
    rb = rowbias_rows(B, N)
    ref = c["ref"] + rb.double().view(B, N, 1, 1)
    bound = c["absbound"] + rb.double().abs().view(B, N, 1, 1)
    stats = check_exact_case(ref, bound, storage, operands=(c["x"], c["w"], c["b"], c["r"], rb))
    return dict(c, rb=rb, ref=ref, absbound=bound, stats=stats)


def linear_case(M, K, N, bias, res, seed, storage="bf16", wide=False, carrier=False, alpha=1.0):
    """The same for F.linear: x [M, K], w [N, K]; the carrier's "channels" are K columns."""
    assert alpha == 1.0 or alpha in ALPHAS, alpha
    g = torch.Generator().manual_seed(seed)
    d = density_for(K, alpha)
    lo, hi = (-2, 2) if (K <= 64 and not bias) else (-1, 1)
    x = int_tensor((M, K), d, g, lo, hi)
    w = int_tensor((N, K), d, g, lo, hi)
    b = int_tensor((N,), 1.0, g, -8, 8) if bias else None
    r = int_tensor((M, N), 1.0, g, -16, 16) if res else None
    if wide:
        x = add_wide(x, g)
    if carrier:
        x, w = add_carrier(x, w)
    ref = fp64_ref_linear(x, w, b, r, alpha)
    bound = absbound_linear(x, w, b, r, alpha)
    stats = check_exact_case(ref, bound, storage, operands=(x, w, b, r))
    return {"x": x, "w": w, "b": b, "r": r, "alpha": alpha, "ref": ref, "absbound": bound, "stats": stats}


# ----------------------------------------------------------------------------------------------------------------------
# GEGLU probes.  gelu is not exact, and the kernels do not compute erf-GELU: csrc/af_common.h gives the bf16 kernels two
# fitted forms (gelu_bf16out_f, gelu_bf16out_f2) and the f32 kernels the Abramowitz-Stegun erf (erf_as_f).  But for an
# argument g >= 8 every form returns g (1 + d) with |d| <= 1.5e-5 (tests/test_exact_operands_cpu.py restates them in float32
# and asserts it), half a bf16 ulp is 2^-9, so a representable product v * g stores as v * g; the erf form returns g itself,
# so the f32 kernels' output is v * g as well.
# ----------------------------------------------------------------------------------------------------------------------
GEGLU_GATE_VALUES = (8.0, 16.0, 32.0)
GEGLU_VALUE_BIASES = (1.0, -1.0, 2.0, -2.0)


def geglu_value_probe(M, K, N, seed, storage="bf16", wide=False, alpha=1.0):
    """Gate weight rows zero, gate bias 8 / 16 / 32 cycling with the column; value rows and value bias the signed integer
    operands above.  Expected: (alpha x @ Wv.T + bv) * g_n.  Isolates the value half of the GEMM, the value | gate interleave and
    the bias permutation.  Returns x [M, K], w [2N, K] (value rows first, as torch's chunk(2) reads them), b [2N], ref [M, N]."""
    g = torch.Generator().manual_seed(seed)
    d = density_for(K, alpha)
    x = int_tensor((M, K), d, g)
    wv = int_tensor((N, K), d, g)
    bv = int_tensor((N,), 1.0, g, -8, 8)
    if wide:
        x = add_wide(x, g)
    gate = torch.tensor(GEGLU_GATE_VALUES)[torch.arange(N) % len(GEGLU_GATE_VALUES)]
    w = torch.cat([wv, torch.zeros(N, K)], 0)
    b = torch.cat([bv, gate], 0)
    val = fp64_ref_linear(x, wv, bv, None, alpha)      # (alpha scales both halves; the gate rows are zero)
    ref = val * gate.double()
    bound = absbound_linear(x, wv, bv, None, alpha) * gate.double()
    stats = check_exact_case(ref, bound, storage, operands=(x, w, b), power_operands=(x, wv, bv))
    return {"x": x, "w": w, "b": b, "ref": ref, "absbound": bound, "stats": stats}


def geglu_gate_probe(M, K, N, seed, storage="bf16"):
    """Value weight rows zero, value bias +-1 / +-2 cycling with the column; gate rows and x in {0, 1} with a density that
    puts the gate pre-activation g near min(60, K / 2), gate bias integers in [0, 8].  Asserted on the reference: every g is
    an integer >= 8 and v * g is exact in the storage type.  Expected: v_n * g.  One product dropped from or added to the
    gate half moves g by one and fails the case."""
    g = torch.Generator().manual_seed(seed)
    d = math.sqrt(min(60.0, K / 2.0) / K)
    x = int_tensor((M, K), d, g, 1, 1)
    wg = int_tensor((N, K), d, g, 1, 1)
    bg = int_tensor((N,), 1.0, g, 0, 8)
    v = torch.tensor(GEGLU_VALUE_BIASES)[torch.arange(N) % len(GEGLU_VALUE_BIASES)]
    w = torch.cat([torch.zeros(N, K), wg], 0)
    b = torch.cat([v, bg], 0)
    gate = fp64_ref_linear(x, wg, bg)
    assert float(gate.min()) >= 8.0 and torch.equal(gate, gate.round()), float(gate.min())
    ref = v.double() * gate
    stats = check_exact_case(ref, gate * 2.0, storage, operands=(x, w, b), power_operands=(x, wg, v))
    return {"x": x, "w": w, "b": b, "ref": ref, "absbound": gate * 2.0, "gate": gate, "stats": stats}
