"""fp64 references, derived error bounds, cases and a CPU emulation of the LayerNorm-folded GEMM chain (ops.ln_chain ->
af_op_ln_chain: producer GEMM with ln_stats_out, ln_fold_kernel, ln_finalize_kernel, consumer GEMM with the LNMODE 1 epilogue).
A plain helper: no fixtures, no tests, no GPU imports.  Every function works on the device its tensors live on.

Each stage is compared with a float64 evaluation of that stage ALONE, from the output the previous stage RETURNED, so a stage
that fails while the ones before it hold names its kernel.  u32 = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16 unit roundoff:
8 significant bits, round to nearest even).  A sum of n fp32 terms in any order is off by at most (n - 1) u32 sum |x_i| to first
order; the bounds below round that up to n (which pays for the second-order terms at these n).

S0  producer output   t vs t64 = a Wp^T + b + r:  ub |t64| + (1 + ub) (Kp + 2) u32 (|a| |Wp|^T + |b| + |r|)
    Kp products accumulated in fp32, one addition each for bias and residual, one rounding to bf16.

S1  fold (ln_fold_kernel, one wave per weight row: a per-lane sum over k = lane, lane + 64, ..., then a 6-level butterfly)
    Wf     == bf16(W * gamma): the fp32 product rounded to nearest even, bit for bit (torch: (W * gamma).bfloat16())
    colsum vs the fp64 row sums of the RETURNED Wf:  (ceil(C / 64) + 6) u32 sum_k |Wf|
    biasf  vs sum_k W beta + b:  (ceil(C / 64) + 7) u32 (sum_k |W| |beta| + |b|)   (one rounding per product more)

S2  partial sums (LNMODE 2 epilogues): slab q of row m holds (sum, sum of squares) of the stored t[m, 80 q : 80 q + 80], q =
    2 * (column tile) + wave group -- on the ping-pong kernel and gemm_m128_kernel ("slab80").  The row-panel producer
    (rowpanel_kernel, af_conv_gemm.hip) has no second wave group: slab 2 k holds all 160 columns of column tile k and slab
    2 k + 1 is written as exactly (0, 0), so that ln_finalize_kernel sums the same number of parts ("tile160").  LAYOUT_OF maps
    the planned producer kernel to its layout; the sums over all slabs of a row are the same quantity either way.
    n values per slab (80 or 160), every lane sums its 4 n / 16 values in order, then two butterfly levels:
    n u32 sum |t| for the sum, (n + 1) u32 sum t^2 for the sum of squares (one rounding per square more).

S3  finalize (ln_finalize_kernel and ln_mu_rstd, af_device.h; P slabs, the sums taken in slab order starting from 0):
      s1 = sum_q p1_q: (P - 1) roundings, |s1 - S1| <= (P - 1) u32 A, A = sum_q |p1_q|;  mu = s1 * fl(1 / C): two more,
      |mu - mu64| <= (P + 2) u32 A / C                                  (A >= |S1|; the + 1 pays for second order)
      E2 = fl(s2 * fl(1 / C)), all p2_q >= 0: |E2 - E2_64| <= (P + 1) u32 E2_64
      mu * mu: |fl(mu^2) - mu64^2| <= 2 |mu64| (P + 2) u32 A / C + u32 mu64^2   (fused into the subtraction: less)
      var = max(E2 - mu^2, 0), one rounding, relative to var <= E2;  var + eps, one rounding
      |d(var + eps)| <= u32 [(P + 2) E2_64 + 2 (P + 2) |mu64| A / C + mu64^2] + u32 (var64 + eps) =: D
      rstd = v_rsq_f32(var + eps), 1 ulp = 2^-23 relative:  with x = D / (var64 + eps) <= 0.01,
      |rstd / rstd64 - 1| <= 0.505 x + 2^-22                            (|(1 + x)^-1/2 - 1| <= x / 2 * (1 + x) there)
    This is the E[x^2] - mu^2 cancellation: the bound scales with E[x^2] / (var + eps), which the cases cap at 8.

S4  consumer, linear part, from the returned t, stats, Wf, colsum, biasf:  y64 = rstd (t Wf^T - mu colsum) + biasf
      lin = rstd (C + 4) u32 (|t| |Wf|^T + |mu| |colsum|) + 4 u32 |biasf|;   bound = ub |y64| + (1 + ub) lin
    A consumer that finalises its own rows (row-panel kernels, gemm_m128_kernel) never stores its (mu, rstd): the returned ones
    are ln_finalize_kernel's.  Its mu is the same product; its rstd comes from the same partial sums in the same order but with
    the variance contracted as hipcc chose in that kernel (rowpanel_kernel: fma(-mu, mu, fl(s2 / C)); ln_finalize_kernel:
    fma(s2, 1 / C, -fl(mu mu)); af_device.h).  Both are inside the S3 bound r3 of rstd64, so they are within 2 r3 of each other:
      lin += 2 r3 |y64 - biasf|   for such a consumer.

S4g GEGLU consumer: out = bf16(val * gelu(gate)), val and gate the fp32 values of S4 (not rounded in between), columns
    [0, N) and [N, 2 N) in the weight's own row order.  The epilogue's GELU is gelu_bf16out_f2 (af_common.h): x Phi(x) with
    Phi ~ 0.5 + xc q(xc^2), xc = clamp(x, +-4), q of degree 6.  GELU is 1.13-Lipschitz (max of Phi(x) + x phi(x), at x = sqrt 2:
    1.1290).  With Bv, Bg the `lin` bounds of value and gate and G the formula's allowance:
      err = |gelu(g64)| Bv + (|v64| + Bv) (1.13 Bg + G) + 2 u32 |out64|;   bound = ub |out64| + (1 + ub) err
    G = 2 * GELU_FIT_ERR.  GELU_FIT_ERR = 1.88e-4 is the measured maximum of |formula in fp32 - erf GELU in fp64| over
    [-GATE_RANGE, GATE_RANGE] = [-8, 8] on 2^21 + 1 equidistant points (measure_gelu_fit: 1.879e-4, reached at x = -3.665;
    tests/test_ln_fold_cpu.py repeats the measurement and checks that the gates of every case stay inside the range).

E   end to end: y_folded and y_plain vs fp64 LN(t) W^T + b (GEGLU applied), both under the bf16 bar of tests/test_ops_gpu.py
    relative to max |ref|.  No assertion of one against the other.
"""
import math

import torch

U32 = 2.0 ** -24
UB = 2.0 ** -8
EPS = 1e-5
RATIO_CAP = 8.0             # E[x^2] / (var + eps) of every row of the fp64 reference of t
GELU_LIPSCHITZ = 1.13
GELU_FIT_ERR = 1.88e-4
GATE_RANGE = 8.0
SLAB = 80
# statistics layout by the producer's planned kernel (ops.GEMM_KERNELS names)
LAYOUT_OF = {"pp": "slab80", "m128": "slab80", "rowpanel": "tile160"}

# The chains of tests/test_ln_fold_gpu.py: name -> (M, Kp, C, N, producer bias, residual, geglu).  The smallest shapes at which
# the planner folds at all: the row-panel kernels need M >= 128 * 256 rows at C = 320 and 16384 at C = 640; 32868 leaves 100 of
# 256 rows in the last panel.  expected kernels: EXPECT[name] = (producer, consumer) as (kernel name, row-panel kind).
CHAINS = {
    "64_rp_bias_res__n960":   (32768, 320, 320, 960, True, True, False),
    "64_rp_bare__n320":       (32768, 320, 320, 320, False, False, False),
    "64_ff2_pp__geglu1280":   (32768, 1280, 320, 1280, True, True, True),
    "64_rp_bias_res__geglu":  (32768, 320, 320, 1280, True, True, True),
    "64_tail_rp__geglu1280":  (32868, 320, 320, 1280, True, True, True),
    "32_m128_res__n1920":     (16384, 640, 640, 1920, True, True, False),
    "32_ff2_pp__n640":        (16384, 2560, 640, 640, True, True, False),
    "32_m128_res__geglu2560": (16384, 640, 640, 2560, False, True, True),
    "32_ff2_pp__n1920":       (16384, 2560, 640, 1920, False, True, False),
}
EXPECT = {
    "64_rp_bias_res__n960":   (("rowpanel", 2), ("rowpanel", 2)),
    "64_rp_bare__n320":       (("rowpanel", 2), ("rowpanel", 2)),
    "64_ff2_pp__geglu1280":   (("pp", 0), ("rowpanel", 1)),
    "64_rp_bias_res__geglu":  (("rowpanel", 2), ("rowpanel", 1)),
    "64_tail_rp__geglu1280":  (("rowpanel", 2), ("rowpanel", 1)),
    "32_m128_res__n1920":     (("m128", 0), ("rowpanel", 5)),
    "32_ff2_pp__n640":        (("pp", 0), ("m128", 0)),
    "32_m128_res__geglu2560": (("m128", 0), ("rowpanel", 4)),
    "32_ff2_pp__n1920":       (("pp", 0), ("rowpanel", 5)),
}
# (M, Kp, C, N) of a chain the operator refuses: ff.net.2 of the 16x16 level, [4096, 5120] -> 1280, plans K slices that the
# 128 x 160 tile GEMM drops, and no LayerNorm epilogue with them -- the reason that level does not fold.  ([4096, 1280] -> 1280
# alone does plan one.)
REFUSED = (4096, 5120, 1280, 1280)


def chain_seed(name):
    return 1000 + sorted(CHAINS).index(name)


def rb(x):
    """x rounded to bf16 (nearest even), as float32"""
    return x.float().bfloat16().float()


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def make_case(M, Kp, C, N, bias, res, geglu, seed, device="cpu"):
    """The inputs of one chain, bf16-representable where the kernels store bf16.  t = a Wp^T (+ b) (+ r) has rows of standard
    deviation sigma_m = 1 (every 7th row: 0.05, so that eps matters) around a row mean drawn uniformly from [-2 sigma_m,
    2 sigma_m] (so that mu * colsum matters): column 0 of a holds the mean and meets a column of ones in Wp, the other columns
    are Gaussian.  gamma = 1 + 0.2 randn, beta = 0.2 randn, consumer weight randn / sqrt(C)."""
    g = torch.Generator(device=device).manual_seed(seed)

    def randn(*s):
        return torch.randn(*s, generator=g, device=device)

    rows = torch.arange(M, device=device)
    sigma = torch.where(rows % 7 == 6, 0.05, 1.0).float()
    off = (torch.rand(M, generator=g, device=device) * 4 - 2) * sigma
    share = math.sqrt(0.5) if res else 1.0           # the residual carries half of the variance
    a = randn(M, Kp) * (sigma * share / math.sqrt(Kp - 1)).unsqueeze(1)
    a[:, 0] = off
    wp = randn(C, Kp)
    wp[:, 0] = 1.0
    rows_c = 2 * N if geglu else N
    c = {"M": M, "Kp": Kp, "C": C, "N": N, "geglu": geglu, "eps": EPS, "sigma": sigma, "off": off,
         "a": rb(a), "wp": rb(wp), "bp": 0.05 * randn(C) if bias else None,
         "res": rb(randn(M, C) * (sigma * share).unsqueeze(1)) if res else None,
         "gamma": 1 + 0.2 * randn(C), "beta": 0.2 * randn(C),
         "wc": rb(randn(rows_c, C) / math.sqrt(C)), "bc": 0.1 * randn(rows_c)}
    return c


def named_case(name, device="cpu", M=None):
    """CHAINS[name] (M overridden: the CPU test checks the same distribution on fewer rows)"""
    M0, Kp, C, N, bias, res, geglu = CHAINS[name]
    return make_case(M or M0, Kp, C, N, bias, res, geglu, chain_seed(name), device)


def _d(x):
    return None if x is None else x.double()


def t_exact(c):
    """(t64, magnitude) of the producer: a Wp^T + b + r in float64 and |a| |Wp|^T + |b| + |r|"""
    a, wp = c["a"].double(), c["wp"].double()
    t = a @ wp.T
    mag = a.abs() @ wp.abs().T
    if c["bp"] is not None:
        t = t + c["bp"].double()
        mag = mag + c["bp"].double().abs()
    if c["res"] is not None:
        t = t + c["res"].double()
        mag = mag + c["res"].double().abs()
    return t, mag


def input_conditions(c, t64=None):
    """{"ratio": max over rows of E[x^2] / (var + eps) of t64, "offset": max |row mean| / sigma, "small_rows": share of rows
    with sigma 0.05, "eps_share": max eps / (var + eps)}"""
    t = t_exact(c)[0] if t64 is None else t64
    mu = t.mean(1)
    var = t.var(1, unbiased=False)
    e2 = (t * t).mean(1)
    sg = c["sigma"].double()
    return {"ratio": float((e2 / (var + c["eps"])).max()), "offset": float((mu.abs() / sg).max()),
            "offset_mean": float((mu.abs() / sg).mean()), "small_rows": float((sg < 0.1).double().mean()),
            "eps_share": float((c["eps"] / (var + c["eps"])).max())}


# ----------------------------------------------------------------------------------------------------------------------
# stage references: each returns (|got - ref|, bound), elementwise float64
# ----------------------------------------------------------------------------------------------------------------------
def s0(c, t, exact=None):
    t64, mag = t_exact(c) if exact is None else exact
    return (t.double() - t64).abs(), UB * t64.abs() + (1 + UB) * (c["Kp"] + 2) * U32 * mag


def s1_wf_ref(c):
    return (c["wc"].float() * c["gamma"].float()).bfloat16().float()


def s1_colsum(c, Wf, colsum):
    w = Wf.double()
    return (colsum.double() - w.sum(1)).abs(), (math.ceil(c["C"] / 64) + 6) * U32 * w.abs().sum(1)


def s1_biasf(c, biasf):
    w, beta = c["wc"].double(), c["beta"].double()
    ref, mag = w @ beta, w.abs() @ beta.abs()
    if c["bc"] is not None:
        ref, mag = ref + c["bc"].double(), mag + c["bc"].double().abs()
    return (biasf.double() - ref).abs(), (math.ceil(c["C"] / 64) + 7) * U32 * mag


def s2_ref(t, slabs, layout):
    """(ref [slabs, M, 2], magnitude [slabs, M, 2], values per slab) of the partial sums of the stored t"""
    t = t.double()
    M, C = t.shape
    assert slabs * SLAB == C, (slabs, C)
    n = SLAB if layout == "slab80" else 2 * SLAB
    x = t.reshape(M, C // n, n)
    ref = torch.stack([x.sum(2), (x * x).sum(2)], dim=2).permute(1, 0, 2)       # [C / n, M, 2]
    mag = torch.stack([x.abs().sum(2), (x * x).sum(2)], dim=2).permute(1, 0, 2)
    if layout == "tile160":                                                      # (slab 2 k: the tile, slab 2 k + 1: zeros)
        z = torch.zeros_like(ref)
        ref = torch.stack([ref, z], dim=1).reshape(slabs, M, 2)
        mag = torch.stack([mag, z], dim=1).reshape(slabs, M, 2)
    else:
        assert layout == "slab80", layout
    return ref, mag, n


def s2(t, parts, layout):
    ref, mag, n = s2_ref(t, parts.shape[0], layout)
    k = torch.tensor([n, n + 1], dtype=torch.float64, device=t.device)
    return (parts.double() - ref).abs(), k * U32 * mag


def s3_ref(c, parts):
    """(mu64, rstd64, bound of |mu - mu64|, bound of |rstd / rstd64 - 1|) from the returned partial sums (see the module text)"""
    p = parts.double()
    P, Cn, eps = p.shape[0], c["C"], c["eps"]
    A = p[:, :, 0].abs().sum(0) / Cn
    mu = p[:, :, 0].sum(0) / Cn
    e2 = p[:, :, 1].sum(0) / Cn
    var = torch.clamp(e2 - mu * mu, min=0.0)
    rstd = (var + eps) ** -0.5
    D = U32 * ((P + 2) * e2 + 2 * (P + 2) * mu.abs() * A + mu * mu) + U32 * (var + eps)
    x = D / (var + eps)
    assert float(x.max()) <= 0.01, float(x.max())
    return mu, rstd, (P + 2) * U32 * A, 0.505 * x + 2.0 ** -22


def s3(c, parts, stats):
    """((|mu - mu64|, bound), (|rstd / rstd64 - 1|, bound))"""
    mu, rstd, bmu, brs = s3_ref(c, parts)
    st = stats.double()
    return ((st[:, 0] - mu).abs(), bmu), ((st[:, 1] / rstd - 1).abs(), brs)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def s4_lin(c, t, stats, Wf, colsum, biasf, own_parts=None):
    """(y64, lin): the consumer's fp32 values before GEGLU and rounding, and their error bound.  own_parts: the partial sums
    of a consumer that finalises its own rows (see S4 in the module text)"""
    t, w, st = t.double(), Wf.double(), stats.double()
    mu, rstd = st[:, 0:1], st[:, 1:2]
    cs, bf = colsum.double().unsqueeze(0), biasf.double().unsqueeze(0)
    y = rstd * (t @ w.T - mu * cs) + bf
    lin = rstd * (c["C"] + 4) * U32 * (t.abs() @ w.abs().T + mu.abs() * cs.abs()) + 4 * U32 * bf.abs()
    if own_parts is not None:
        lin = lin + 2 * s3_ref(c, own_parts)[3].unsqueeze(1) * (y - bf).abs()
    return y, lin


def s4(c, t, stats, Wf, colsum, biasf, y, own_parts=None):
    """(|y - ref|, bound) of the folded consumer, GEGLU included where the case has it"""
    y64, lin = s4_lin(c, t, stats, Wf, colsum, biasf, own_parts)
    if not c["geglu"]:
        return (y.double() - y64).abs(), UB * y64.abs() + (1 + UB) * lin
    N = c["N"]
    v, g, bv, bg = y64[:, :N], y64[:, N:], lin[:, :N], lin[:, N:]
    gg = gelu64(g)
    out = v * gg
    err = gg.abs() * bv + (v.abs() + bv) * (GELU_LIPSCHITZ * bg + 2 * GELU_FIT_ERR) + 2 * U32 * out.abs()
    return (y.double() - out).abs(), UB * out.abs() + (1 + UB) * err


def gate_max(c, t, stats, Wf, colsum, biasf):
    return float(s4_lin(c, t, stats, Wf, colsum, biasf)[0][:, c["N"]:].abs().max())


def e2e_ref(c, t):
    """fp64 LN(t) W^T + b of the stored t (GEGLU applied)"""
    t = t.double()
    mu = t.mean(1, keepdim=True)
    var = t.var(1, unbiased=False, keepdim=True)
    ln = (t - mu) / torch.sqrt(var + c["eps"]) * c["gamma"].double() + c["beta"].double()
    y = ln @ c["wc"].double().T
    if c["bc"] is not None:
        y = y + c["bc"].double()
    if c["geglu"]:
        y = y[:, :c["N"]] * gelu64(y[:, c["N"]:])
    return y


def ratio(err_bound):
    """max err / bound; where the bound is 0 the error must be 0 (inf otherwise)"""
    err, bound = err_bound
    r = torch.where(bound > 0, err / torch.clamp(bound, min=1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    r = torch.where(torch.isnan(err), torch.full_like(r, float("inf")), r)
    return float(r.max())


def outside(err_bound):
    """bool tensor: elements outside their bound"""
    err, bound = err_bound
    return (err > bound) | torch.isnan(err)


def check_chain(c, r, layout, exact=None, own_stats=False):
    """Every stage of one chain result r (ops.ln_chain's or emulate's dict): {stage: worst error / bound} -- a stage holds when
    its figure is <= 1 -- and "wf_equal", "e_folded", "e_plain" (relative to max |ref|), "gate_max".  own_stats: the consumer
    finalised its own rows from the partial sums (a row-panel or 128 x 160 tile launch)."""
    out = {"s0": ratio(s0(c, r["t"], exact)),
           "wf_equal": bool(torch.equal(r["Wf"], s1_wf_ref(c))),
           "s1_colsum": ratio(s1_colsum(c, r["Wf"], r["colsum"])),
           "s1_biasf": ratio(s1_biasf(c, r["biasf"])),
           "s2": ratio(s2(r["t"], r["parts"], layout))}
    m, s = s3(c, r["parts"], r["stats"])
    out["s3_mu"], out["s3_rstd"] = ratio(m), ratio(s)
    out["s4"] = ratio(s4(c, r["t"], r["stats"], r["Wf"], r["colsum"], r["biasf"], r["y_folded"], r["parts"] if own_stats else None))
    ref = e2e_ref(c, r["t"])
    scale = float(ref.abs().max())
    out["e_folded"] = float((r["y_folded"].double() - ref).abs().max()) / scale
    out["e_plain"] = float((r["y_plain"].double() - ref).abs().max()) / scale
    out["gate_max"] = gate_max(c, r["t"], r["stats"], r["Wf"], r["colsum"], r["biasf"]) if c["geglu"] else 0.0
    return out


STAGES = ("s0", "s1_colsum", "s1_biasf", "s2", "s3_mu", "s3_rstd", "s4")


def stage(c, r, layout, name):
    """(|got - ref|, bound) of one of STAGES"""
    if name == "s0":
        return s0(c, r["t"])
    if name == "s1_colsum":
        return s1_colsum(c, r["Wf"], r["colsum"])
    if name == "s1_biasf":
        return s1_biasf(c, r["biasf"])
    if name == "s2":
        return s2(r["t"], r["parts"], layout)
    if name in ("s3_mu", "s3_rstd"):
        return s3(c, r["parts"], r["stats"])[name == "s3_rstd"]
    assert name == "s4", name
    return s4(c, r["t"], r["stats"], r["Wf"], r["colsum"], r["biasf"], r["y_folded"])


def share_outside(c, r, layout, name):
    """The share of the stage's rows (s1: weight rows, i.e. output columns; s2: rows of t, any slab; s4: rows of y, any column)
    with an element outside its bound"""
    o = outside(stage(c, r, layout, name))
    if name == "s2":
        o = o.any(dim=2).any(dim=0)
    elif o.dim() == 2:
        o = o.any(dim=1)
    return float(o.double().mean())


# ----------------------------------------------------------------------------------------------------------------------
# the epilogue's GELU formula
# ----------------------------------------------------------------------------------------------------------------------
def gelu_fit32(x):
    """gelu_bf16out_f2 (csrc/af_common.h) in float32"""
    x = x.float()
    xc = x.clamp(-4.0, 4.0)
    s = xc * xc
    q = s * 2.27794120e-08 + (-1.59850396e-06)
    for k in (4.79536935e-05, -8.13999317e-04, 8.77231965e-03, -6.45729896e-02, 3.97883296e-01):
        q = q * s + k
    return x * (xc * q + 0.5)


def measure_gelu_fit(points=2 ** 21 + 1):
    """(max |gelu_fit32 - erf GELU in float64| over [-GATE_RANGE, GATE_RANGE], the x where it is reached)"""
    x = torch.linspace(-GATE_RANGE, GATE_RANGE, points, dtype=torch.float64).float()
    e = (gelu_fit32(x).double() - gelu64(x.double())).abs()
    i = int(e.argmax())
    return float(e[i]), float(x[i])


# ----------------------------------------------------------------------------------------------------------------------
# CPU emulation of the chain in float32, bf16 rounding where the kernels round; and the mistakes a kernel could make
# ----------------------------------------------------------------------------------------------------------------------
VARIANTS = ("colsum_unrounded", "biasf_no_wbeta", "stats_unrounded", "slabs_wrong_order", "var_n_minus_1", "eps_dropped",
            "mu_neighbour_row", "geglu_unpermuted")
# the stage each mistake must leave the bound of, and the least share of that stage's rows / columns outside it
VARIANT_STAGE = {"colsum_unrounded": ("s1_colsum", 0.90), "biasf_no_wbeta": ("s1_biasf", 0.90), "stats_unrounded": ("s2", 0.90),
                 "slabs_wrong_order": ("s2", 0.90), "var_n_minus_1": ("s3_rstd", 0.90), "eps_dropped": ("s3_rstd", 0.10),
                 "mu_neighbour_row": ("s4", 0.90), "geglu_unpermuted": ("s4", 0.90)}


def _lane_strided_sum32(x):
    """ln_fold_kernel's row sum: lane l adds columns l, l + 64, ... in order, then the xor butterfly 32, 16, .., 1"""
    rows, K = x.shape
    n = math.ceil(K / 64)
    xp = torch.zeros(rows, n * 64)
    xp[:, :K] = x
    acc = torch.zeros(rows, 64)
    for i in range(n):
        acc = acc + xp[:, i * 64:(i + 1) * 64]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, idx ^ o]
    return acc[:, 0]


def _slab_sums32(x, xsq_src=None):
    """An LNMODE 2 epilogue's (sum, sum of squares) of x [M, w]: the lanes of a row hold columns 16 i + 4 h + e (h = lane / 16),
    each sums its values over (i, e) in order, then the butterfly over h (xor 16, xor 32)"""
    M, w = x.shape
    x4 = x.reshape(M, w // 16, 4, 4)
    ps, pq = torch.zeros(M, 4), torch.zeros(M, 4)
    for i in range(w // 16):
        for e in range(4):
            v = x4[:, i, :, e]
            ps = ps + v
            pq = pq + v * v
    idx = torch.arange(4)
    for o in (1, 2):
        ps = ps + ps[:, idx ^ o]
        pq = pq + pq[:, idx ^ o]
    return ps[:, 0], pq[:, 0]


def emulate(c, layout, variant=None):
    """The chain on the CPU with the kernels' arithmetic: the dict ops.ln_chain returns (no guards, no plans).  variant: one of
    VARIANTS, the named mistake built in."""
    assert variant is None or variant in VARIANTS, variant
    Cn, N, eps = c["C"], c["N"], c["eps"]
    f = torch.float32
    t32 = c["a"].float() @ c["wp"].float().T
    if c["bp"] is not None:
        t32 = t32 + c["bp"].float()
    if c["res"] is not None:
        t32 = t32 + c["res"].float()
    t = rb(t32)
    # fold
    w, gamma, beta = c["wc"].float(), c["gamma"].float(), c["beta"].float()
    prod = w * gamma
    Wf = rb(prod)
    colsum = _lane_strided_sum32(prod if variant == "colsum_unrounded" else Wf)
    biasf = torch.zeros(w.shape[0]) if variant == "biasf_no_wbeta" else _lane_strided_sum32(w * beta)
    if c["bc"] is not None:
        biasf = biasf + c["bc"].float()
    # partial sums
    n = SLAB if layout == "slab80" else 2 * SLAB
    src = t32 if variant == "stats_unrounded" else t
    slabs = Cn // SLAB
    parts = torch.zeros(slabs, t.shape[0], 2)
    for k in range(Cn // n):
        s1, s2_ = _slab_sums32(src[:, k * n:(k + 1) * n])
        q = k if layout == "slab80" else 2 * k
        parts[q, :, 0], parts[q, :, 1] = s1, s2_
    if variant == "slabs_wrong_order":
        parts = parts.roll(1, 0)
    # finalize
    inv = torch.tensor(1.0, dtype=f) / torch.tensor(float(Cn), dtype=f)
    s1, s2_ = torch.zeros(t.shape[0]), torch.zeros(t.shape[0])
    for q in range(slabs):
        s1 = s1 + parts[q, :, 0]
        s2_ = s2_ + parts[q, :, 1]
    mu = s1 * inv
    var = torch.clamp(s2_ * inv - mu * mu, min=0.0)
    if variant == "var_n_minus_1":
        var = var * (Cn / (Cn - 1.0))
    rstd = torch.rsqrt(var if variant == "eps_dropped" else var + eps)
    stats = torch.stack([mu, rstd], dim=1)
    # consumer
    mu_used = mu.roll(-1) if variant == "mu_neighbour_row" else mu
    acc = t @ Wf.T
    y32 = (acc - mu_used.unsqueeze(1) * colsum.unsqueeze(0)) * rstd.unsqueeze(1) + biasf.unsqueeze(0)
    # the unfolded route: LayerNorm in fp32 on the stored t, stored as bf16, then the plain GEMM
    tm = t.mean(1, keepdim=True)
    tv = t.var(1, unbiased=False, keepdim=True)
    ln = rb((t - tm) * torch.rsqrt(tv + eps) * gamma + beta)
    p32 = ln @ w.T
    if c["bc"] is not None:
        p32 = p32 + c["bc"].float()
    if c["geglu"]:
        if variant == "geglu_unpermuted":   # the kernel pairs rows 32 k + i (value) and 32 k + 16 + i (gate) of an unpacked weight
            idx = torch.arange(N)
            vi, gi = (idx // 16) * 32 + idx % 16, (idx // 16) * 32 + 16 + idx % 16
            y32 = y32[:, vi] * gelu_fit32(y32[:, gi])
        else:
            y32 = y32[:, :N] * gelu_fit32(y32[:, N:])
        p32 = p32[:, :N] * gelu_fit32(p32[:, N:])
    return {"Wf": Wf, "colsum": colsum, "biasf": biasf, "t": t, "parts": parts, "stats": stats, "y_folded": rb(y32),
            "y_plain": rb(p32)}
