"""The exact-operand oracle (tests/exact_operands.py) checked without a GPU.

Two things are shown here.  (1) The oracle does not fail a correct kernel: fp32 evaluations of the integer operands in three
different summation orders equal the fp64 reference bit for bit, also after a bf16 round trip of the output.  (2) It
catches single-site mistakes: each mistake below, injected into that CPU evaluation, makes assert_bit_exact raise and name
the site -- while the max-abs criterion of tests/test_ops_gpu.py::_cmp accepts the first one on that test's own Gaussian
operands.  (3) The float32 restatement of the three GELU forms of csrc/af_common.h keeps v * g exact over the whole range
the GEGLU probes use, so the probes' exactness follows from the formulas and not from the kernels' output.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_operands as X

SHAPES = [   # B, Cin, H, W, Cout, ks, stride, up, bias, res
    (1, 128, 12, 10, 24, 3, 1, False, True, True),
    (2, 64, 9, 7, 20, 3, 2, False, True, False),
    (1, 128, 6, 5, 16, 3, 1, True, True, False),
    (2, 192, 8, 8, 12, 1, 1, False, True, True),
]


def _finish(y, c):
    if c["b"] is not None:
        y = y + c["b"].view(1, -1, 1, 1)
    if c["r"] is not None:
        y = y + c["r"]
    assert y.dtype == torch.float32
    return y


def _eval_plain(c, stride, up):
    xi = F.interpolate(c["x"], scale_factor=2.0, mode="nearest") if up else c["x"]
    return _finish(F.conv2d(xi, c["w"], None, stride=stride, padding=c["w"].shape[-1] // 2), c)


def _slabs(c, stride, up, chunk=64):
    xi = F.interpolate(c["x"], scale_factor=2.0, mode="nearest") if up else c["x"]
    Cin = xi.shape[1]
    return [F.conv2d(xi[:, s:s + chunk], c["w"][:, s:s + chunk], None, stride=stride, padding=c["w"].shape[-1] // 2)
            for s in range(0, Cin, chunk)]


def _eval_slices_reversed(c, stride, up, chunk=32):
    """K cut into channel slices, the slabs summed in reverse order."""
    slabs = _slabs(c, stride, up, chunk)
    y = torch.zeros_like(slabs[0])
    for s in reversed(slabs):
        y = y + s
    return _finish(y, c)


def _eval_taps_outermost(c, stride, up):
    xi = F.interpolate(c["x"], scale_factor=2.0, mode="nearest") if up else c["x"]
    ks = c["w"].shape[-1]
    pad = ks // 2
    xp = F.pad(xi, (pad, pad, pad, pad))
    Ho = (xi.shape[2] + 2 * pad - ks) // stride + 1
    Wo = (xi.shape[3] + 2 * pad - ks) // stride + 1
    y = torch.zeros(xi.shape[0], c["w"].shape[0], Ho, Wo)
    for ky in range(ks):
        for kx in range(ks):
            win = xp[:, :, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            y = y + torch.einsum("bchw,oc->bohw", win, c["w"][:, :, ky, kx])
    return _finish(y, c)


@pytest.mark.parametrize("storage,wide", [("bf16", False), ("f32", True)])
@pytest.mark.parametrize("carrier", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_evaluation_in_any_order_equals_the_fp64_reference(shape, carrier, storage, wide):
    """No false alarm: plain F.conv2d in fp32, K slices summed in reverse, taps outermost -- all three equal the fp64
    reference bit for bit, with and without the cancelling carrier, with the wide (+-4097) f32 operands, and after a bf16
    round trip of the output in the bf16 cases."""
    B, Cin, H, W, Cout, ks, stride, up, bias, res = shape
    if carrier and Cin < 128:
        Cin = 128
    c = X.conv_case(B, Cin, H, W, Cout, ks, stride, up, bias, res, seed=Cin + Cout + H, storage=storage, wide=wide, carrier=carrier)
    for name, y in (("plain", _eval_plain(c, stride, up)), ("slices reversed", _eval_slices_reversed(c, stride, up)),
                    ("taps outermost", _eval_taps_outermost(c, stride, up))):
        X.assert_bit_exact(name, y, c["ref"], None)
        if storage == "bf16":
            X.assert_bit_exact(name + " -> bf16", y.to(torch.bfloat16).float(), c["ref"], None)


def test_fp32_linear_in_any_order_equals_the_fp64_reference():
    """The same for F.linear: one matmul, and 32-column K slices summed in reverse; the K = 64 case without bias uses [-2, 2]."""
    for (M, K, N, bias, res, carrier) in [(70, 64, 48, False, False, False), (33, 320, 64, True, True, True), (200, 64, 192, True, False, False)]:
        c = X.linear_case(M, K, N, bias, res, seed=M + K + N, carrier=carrier)
        y = c["x"] @ c["w"].t()
        y2 = sum((c["x"][:, s:s + 32] @ c["w"][:, s:s + 32].t() for s in reversed(range(0, K, 32))), torch.zeros(M, N))
        for yy in (y, y2):
            if bias:
                yy = yy + c["b"]
            if res:
                yy = yy + c["r"]
            X.assert_bit_exact("linear", yy.to(torch.bfloat16).float(), c["ref"], None)


def test_table_of_the_smallest_shapes_keeps_the_power_conditions():
    """The shortest K is where the power conditions are tightest: the three small shapes the GPU file uses, built here so that
    a precondition failure shows up without a GPU."""
    assert X.linear_case(200, 64, 192, True, False, seed=1)["stats"]["distinct"] >= 40
    assert X.linear_case(333, 128, 4, True, False, seed=2)["stats"]["nonzero"] >= 0.9
    assert X.conv_case(2, 64, 16, 16, 160, 1, 1, False, True, False, seed=3)["stats"]["distinct"] >= 40
    assert X.conv_case(1, 4, 64, 64, 320, 3, 1, False, True, False, seed=4)["stats"]["distinct"] >= 40
    assert abs(X.density_for(23040) - 0.3277) < 1e-3 and X.density_for(960) == 1.0


def _case():
    B, Cin, H, W, Cout = 1, 128, 12, 10, 24
    c = X.conv_case(B, Cin, H, W, Cout, 3, 1, False, True, True, seed=77)
    return c, _eval_plain(c, 1, False)


def _raises_naming(got, ref, *needles, plan=(0, 1, 0)):
    with pytest.raises(AssertionError) as ei:
        X.assert_bit_exact("injected", got, ref, plan)
    msg = str(ei.value)
    for n in needles:
        assert n in msg, (n, msg)
    return msg


def test_one_dropped_product_at_one_output_is_reported():
    """One (channel, tap) product missing at one output: one mismatch, named by coordinate, bounding box and plan."""
    c, y = _case()
    b, o, oy, ox, ch, ky, kx = 0, 7, 5, 4, 0, 0, 2
    while c["x"][b, ch, oy + ky - 1, ox + kx - 1] * c["w"][o, ch, ky, kx] == 0:
        ch += 1
    y[b, o, oy, ox] -= c["x"][b, ch, oy + ky - 1, ox + kx - 1] * c["w"][o, ch, ky, kx]
    msg = _raises_naming(y.to(torch.bfloat16).float(), c["ref"], "1 of ", f"({b}, {o}, {oy}, {ox})",
                         f"axis 1: [{o}, {o}]", f"axis 2: [{oy}, {oy}]", f"axis 3: [{ox}, {ox}]", "(0, 1, 0)")
    assert "got" in msg and "ref" in msg


def test_one_tap_of_one_channel_read_from_the_wrong_pixel_at_a_corner_is_reported():
    """Output (0, 0) reads its top-left tap from the zero padding; the mistake reads the row's last pixel instead (a halo
    column that wraps)."""
    c, y = _case()
    b, o, ch = 0, 3, 0
    W = c["x"].shape[3]
    while c["x"][b, ch, 0, W - 1] * c["w"][o, ch, 0, 0] == 0:
        ch += 1
    y[b, o, 0, 0] += c["x"][b, ch, 0, W - 1] * c["w"][o, ch, 0, 0]
    _raises_naming(y.to(torch.bfloat16).float(), c["ref"], "1 of ", f"({b}, {o}, 0, 0)", "axis 2: [0, 0]", "axis 3: [0, 0]")


def test_bias_off_by_one_at_one_column_is_reported():
    """One output channel gets its neighbour's bias: every pixel of that channel differs, the box names the column."""
    c, y = _case()
    o = 0
    while c["b"][o] == c["b"][o + 1]:
        o += 1
    y[:, o] += c["b"][o + 1] - c["b"][o]
    H, W = y.shape[2:]
    _raises_naming(y.to(torch.bfloat16).float(), c["ref"], f"{H * W} of ", f"axis 1: [{o}, {o}]", f"axis 2: [0, {H - 1}]")


def test_one_k_slice_slab_rounded_to_bf16_is_reported_with_the_carrier():
    """Two 64-channel K slices; the carrier's +2304 sits in the first slab and its -2304 in the second.  With fp32 slabs the
    sum is exact; with ONE slab stored as bf16 (spacing 16 at 2304) the small terms are lost.  Without the carrier the
    same rounding goes unnoticed, because a slab of small integers is exact in bf16: that is what the carrier is for."""
    B, Cin, H, W, Cout = 1, 128, 12, 10, 24
    for carrier in (False, True):
        c = X.conv_case(B, Cin, H, W, Cout, 3, 1, False, True, True, seed=78, carrier=carrier)
        slabs = _slabs(c, 1, False, 64)
        assert len(slabs) == 2
        X.assert_bit_exact("fp32 slabs", _finish(slabs[0] + slabs[1], c), c["ref"], None)
        y = _finish(slabs[0].to(torch.bfloat16).float() + slabs[1], c)
        if carrier:
            assert float(slabs[0].abs().max()) > 2048
            msg = _raises_naming(y, c["ref"], "elements differ")
            assert int(msg.split(":")[1].split(" of ")[0]) > y.numel() // 2          # (most outputs lose their low bits)
        else:
            assert float(slabs[0].abs().max()) <= 256
            X.assert_bit_exact("bf16 slab, no carrier: exact, hence unseen", y, c["ref"], None)


def test_one_operand_truncated_to_bf16_is_reported_in_an_f32_case():
    """The wide operands of the f32 cases: 4097 is 4096 in bf16, so a path that narrows the activations returns another
    integer wherever such an activation meets a non-zero weight."""
    c = X.conv_case(1, 128, 12, 10, 24, 3, 1, False, True, True, seed=79, storage="f32", wide=True)
    assert int((c["x"].abs() == X.WIDE_VALUE).sum()) > 100
    X.assert_bit_exact("f32 operands", _eval_plain(c, 1, False), c["ref"], None)
    narrowed = dict(c, x=c["x"].to(torch.bfloat16).float())
    _raises_naming(_eval_plain(narrowed, 1, False), c["ref"], "elements differ")
    with pytest.raises(AssertionError):                      # and the wide operands are no bf16 case: precondition 1 says so
        X.check_exact_case(c["ref"], c["absbound"], "bf16", operands=(c["x"],))


def test_the_gaussian_max_abs_bar_accepts_one_dropped_product():
    """The gap the exact tests close.  tests/test_ops_gpu.py::test_conv2d's ResBlock case (2x320x32x32 -> 320, bias +
    residual, its own seed and Gaussian operands) under that file's own criterion _cmp: max-abs <= 1.5e-2 * max|ref|
    = 0.098 absolute, while a perfect kernel's bf16 output rounding is 0.0156 and one product |x||w| is about 0.019.  Asserted
    first, from the operands: the dropped product plus the rounding stays below the bar.  Then: _cmp accepts the output with
    that product missing -- and on integer operands of the same shape assert_bit_exact does not."""
    import math
    from test_ops_gpu import TOL, _cmp, _q
    B, Cin, H, W, Cout, ks = 2, 320, 32, 32, 320, 3
    g = torch.Generator().manual_seed(Cin + Cout + H + ks)
    x = _q(torch.randn(B, Cin, H, W, generator=g), "bf16")
    w = _q(torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks), "bf16")
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(x, w, b, padding=1)
    r = _q(torch.randn(ref.shape, generator=g), "bf16")
    ref = ref + r
    scale = ref.abs().max().item()
    bar = TOL["bf16"] * scale
    sg = torch.Generator().manual_seed(2024)                                    # the seeded site
    bi, o, oy, ox, ch = (int(torch.randint(0, n, (1,), generator=sg)) for n in (B, Cout, H - 2, W - 2, Cin))
    oy, ox = oy + 1, ox + 1
    prod = (x[bi, ch, oy, ox] * w[o, ch, 1, 1]).item()                          # the centre tap of channel ch
    ulp_half = 2.0 ** (math.floor(math.log2(scale)) - 8)                         # half a bf16 step at the top of the range
    assert 0.0 < abs(prod) and abs(prod) + ulp_half < bar, (prod, ulp_half, bar)
    wrong = ref.clone()
    wrong[bi, o, oy, ox] -= prod
    got = wrong.to(torch.bfloat16).float()
    assert got[bi, o, oy, ox] != ref.to(torch.bfloat16).float()[bi, o, oy, ox] or abs(prod) < ulp_half
    lines = []
    _cmp(lambda *a: lines.append(a), "gap", got, ref, "bf16")                   # accepted: no AssertionError
    assert lines and lines[0][1] <= bar
    c = X.conv_case(B, Cin, H, W, Cout, ks, 1, False, True, True, seed=5)
    y = _eval_plain(c, 1, False)
    chi = ch
    while c["x"][bi, chi, oy, ox] * c["w"][o, chi, 1, 1] == 0:
        chi = (chi + 1) % Cin
    y[bi, o, oy, ox] -= c["x"][bi, chi, oy, ox] * c["w"][o, chi, 1, 1]
    _raises_naming(y.to(torch.bfloat16).float(), c["ref"], "1 of ", f"({bi}, {o}, {oy}, {ox})")


# ----------------------------------------------------------------------------------------------------------------------
# The three GELU forms of csrc/af_common.h restated in float32.  fma(a, b, c) is one rounding of the exact a * b + c: float64
# holds the product of two float32 values exactly and the sum to far below a float32 ulp.  v_rcp_f32 / v_exp_f32 are
# approximations (1 ulp), but for g >= 8 their arguments are 1 + 2^-70 = 1.0f and below 2^-46: rcp(1.0f) is 1.0f and the
# exponential vanishes against 1.0f on any implementation, so the claim does not rest on how numpy rounds them.
# ----------------------------------------------------------------------------------------------------------------------
f32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _gelu_erf_f(x):
    ax = np.abs(x * f32(0.70710678118654752440))
    t = f32(1.0) / _fma(ax, f32(0.3275911), f32(1.0))
    poly = _fma(t, f32(1.061405429), f32(-1.453152027))
    poly = _fma(poly, t, f32(1.421413741))
    poly = _fma(poly, t, f32(-0.284496736))
    poly = _fma(poly, t, f32(0.254829592))
    poly = poly * t
    e = np.exp2(f32(-1.44269504088896340736) * ax * ax).astype(f32)
    r = _fma(-poly, e, f32(1.0))
    erf = np.copysign(r, x)
    return f32(0.5) * x * (f32(1.0) + erf)


def _gelu_bf16out_f(x):
    u = x * _fma(x * x, f32(-0.07068715223 * 1.44269504089), f32(-1.59748341624 * 1.44269504089))
    return x * (f32(1.0) / (f32(1.0) + np.exp2(u).astype(f32)))


def _gelu_bf16out_f2(x):
    xc = np.clip(x, f32(-4.0), f32(4.0))
    s = xc * xc
    q = s * f32(2.27794120e-08) + f32(-1.59850396e-06)
    for cf in (4.79536935e-05, -8.13999317e-04, 8.77231965e-03, -6.45729896e-02, 3.97883296e-01):
        q = q * s + f32(cf)           # (contracted to an fma or not: both are tried below)
    ph = xc * q + f32(0.5)
    return x * ph


def _gelu_bf16out_f2_fma(x):
    xc = np.clip(x, f32(-4.0), f32(4.0))
    s = xc * xc
    q = _fma(s, f32(2.27794120e-08), f32(-1.59850396e-06))
    for cf in (4.79536935e-05, -8.13999317e-04, 8.77231965e-03, -6.45729896e-02, 3.97883296e-01):
        q = _fma(q, s, f32(cf))
    ph = _fma(xc, q, f32(0.5))
    return x * ph


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def test_gelu_forms_keep_v_times_g_exact_over_the_probes_range():
    """What both GEGLU probes rest on: for every integer gate g in 8..256 each form returns g (1 + d) with |d| <= 1.5e-5 (the
    erf form of the f32 kernels: g itself), and bf16(v * form(g)) == v * g for every representable v * g the probes can
    produce: v in {+-1, +-2} (gate probe), every integer v in [-256, 256] with g in {8, 16, 32} (value probe)."""
    g = np.arange(8, 257, dtype=f32)
    forms = {"gelu_erf_f": _gelu_erf_f, "gelu_bf16out_f": _gelu_bf16out_f, "gelu_bf16out_f2": _gelu_bf16out_f2,
             "gelu_bf16out_f2 (fma)": _gelu_bf16out_f2_fma}
    for name, form in forms.items():
        y = form(g)
        assert y.dtype == f32
        d = np.abs(y.astype(np.float64) / g.astype(np.float64) - 1.0).max()
        assert d <= 1.5e-5, (name, d)
        if name == "gelu_erf_f":
            assert np.array_equal(y, g), name                  # the f32 kernels store v * g with no rounding to hide behind
        n_pairs = 0
        for v in X.GEGLU_VALUE_BIASES:                          # gate probe
            exact = v * g.astype(np.float64)
            rep = _bf16(exact) == exact
            assert np.array_equal(_bf16(f32(v) * y)[rep], exact[rep]), (name, v)
            n_pairs += int(rep.sum())
        assert n_pairs >= 4 * 120
        for gv in X.GEGLU_GATE_VALUES:                          # value probe
            v = np.arange(-256, 257, dtype=f32)
            yg = form(np.full_like(v, gv))
            exact = v.astype(np.float64) * gv
            assert np.array_equal(_bf16(exact), exact)
            assert np.array_equal(_bf16(v * yg), exact), (name, gv)
            if name == "gelu_erf_f":
                assert np.array_equal((v * yg).astype(np.float64), exact)


def test_geglu_probes_meet_their_preconditions():
    """Both probes build (their preconditions are asserted inside) at K = 64, 320 and 1280; the silenced half is really zero."""
    for (M, K, N) in [(70, 64, 256), (300, 320, 128), (256, 1280, 64)]:
        p = X.geglu_value_probe(M, K, N, seed=M + K)
        assert p["w"][N:].abs().max() == 0 and set(p["b"][N:].tolist()) == set(X.GEGLU_GATE_VALUES)
        q = X.geglu_gate_probe(M, K, N, seed=M + K)
        assert q["w"][:N].abs().max() == 0 and float(q["gate"].min()) >= 8 and float(q["ref"].abs().max()) <= 512


# ----------------------------------------------------------------------------------------------------------------------
# The launch forms of tests/test_launch_forms_gpu.py: per-sample bias row, alpha, bottom / right padding.  For every such case
# the fp64 reference must DIFFER from what each plausible wrong kernel returns -- computed here from the same operands -- in
# every sample the mistake touches; otherwise the GPU comparison could not fail.
# ----------------------------------------------------------------------------------------------------------------------
FORM_CASES = [   # B, Cin, H, W, Cout, stride, rowbias, alpha, pad  (3x3, bias + residual)
    (4, 64, 16, 8, 16, 1, True, 1.0, None),       # two images per 256-row tile
    (4, 64, 8, 16, 16, 1, True, 1.0, None),
    (8, 64, 4, 16, 16, 1, True, 1.0, None),       # four images per tile
    (5, 64, 12, 12, 16, 1, True, 1.0, None),      # 144-row samples under 256-row tiles: a tile straddles samples in mid-row
    (4, 64, 8, 8, 16, 1, True, 1.0, None),        # 64-row samples: four per tile
    (2, 64, 32, 8, 16, 1, True, 1.0, None),       # one image per tile: the tile's first sample IS the sample
    (4, 128, 16, 8, 16, 1, True, 0.5, None),
    (4, 128, 16, 8, 16, 1, True, -2.0, None),
    (2, 64, 12, 12, 24, 1, False, 0.5, None),
    (2, 64, 12, 12, 24, 1, False, -2.0, None),
    (2, 128, 16, 16, 16, 2, False, 1.0, 0),       # bottom / right padding
    (1, 128, 12, 20, 24, 2, True, 1.0, 0),
    (2, 64, 12, 20, 16, 2, True, -2.0, 0),
]


def _rows(t):
    """[B, C, H, W] -> [B * H * W, C], the GEMM's row order"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _form_case(case, storage="bf16"):
    B, Cin, H, W, Cout, stride, rowbias, alpha, pad = case
    c = X.conv_case(B, Cin, H, W, Cout, 3, stride, False, True, True, seed=sum(int(abs(v or 0) * 2) for v in case), storage=storage,
                    rowbias=rowbias, alpha=alpha, pad=pad)
    conv = X.fp64_ref_conv(c["x"], c["w"], None, None, stride, False, None, 1.0, pad)
    return c, conv


def _samples_differing(a, b, B):
    """the samples in which [B, ...] tensors a and b differ somewhere"""
    return {i for i in range(B) if not torch.equal(a[i], b[i])}


def _with_rowbias_of(c, sample_of_row):
    """the reference with row m taking its bias row from sample sample_of_row[m] instead of its own"""
    B, N, Ho, Wo = c["ref"].shape
    own = torch.arange(B * Ho * Wo) // (Ho * Wo)
    rows = _rows(c["ref"]) - c["rb"].double()[own] + c["rb"].double()[sample_of_row]
    return rows.view(B, Ho, Wo, N).permute(0, 3, 1, 2), {int(s) for s in own[sample_of_row != own].unique()}


@pytest.mark.parametrize("case", FORM_CASES, ids=["-".join(str(v) for v in c) for c in FORM_CASES])
def test_launch_form_references_differ_from_every_wrong_kernel(case):
    B, Cin, H, W, Cout, stride, rowbias, alpha, pad = case
    c, conv = _form_case(case)
    ref = c["ref"]
    Ho, Wo = ref.shape[2:]
    X.assert_bit_exact("the parts add up", float(alpha) * conv + c["b"].double().view(1, -1, 1, 1)
                       + (c["rb"].double().view(B, -1, 1, 1) if rowbias else 0) + c["r"].double(), ref, None)
    m = torch.arange(B * Ho * Wo)
    if rowbias:
        # the row of the tile's first sample applied to the whole 256-row tile
        wrong, touched = _with_rowbias_of(c, (m // 256 * 256) // (Ho * Wo))
        if Ho * Wo < 256:
            assert len(touched) >= B // 2                       # (several samples per tile: at least every second one is wrong)
        elif Ho * Wo % 256 == 0:
            assert not touched                                  # (a tile inside one sample: this mistake cannot show, others can)
        assert _samples_differing(wrong, ref, B) == touched, (case, touched)
        for s in touched:                                       # ... in EVERY column of every row that took the wrong row
            rows_w, rows_r = _rows(wrong[s:s + 1]), _rows(ref[s:s + 1])
            bad_rows = (rows_w != rows_r).any(1)
            assert bool((rows_w != rows_r)[bad_rows].all())
        # the row indexed by m / Wo instead of m / (Ho * Wo)
        wrong, touched = _with_rowbias_of(c, (m // Wo) % B)
        assert len(touched) >= B - 1, touched
        assert _samples_differing(wrong, ref, B) == touched, (case, touched)
    if alpha != 1.0:
        dropped = ref + (1.0 - float(alpha)) * conv
        assert _samples_differing(dropped, ref, B) == set(range(B)), case
        after_bias = float(alpha) * (conv + c["b"].double().view(1, -1, 1, 1)) + (c["rb"].double().view(B, -1, 1, 1) if rowbias else 0) + c["r"].double()
        assert _samples_differing(after_bias, ref, B) == set(range(B)), case
    if pad == 0:
        sym = X.fp64_ref_conv(c["x"], c["w"], c["b"], c["r"], stride, False, c["rb"], alpha, None)
        assert sym.shape == ref.shape
        assert _samples_differing(sym, ref, B) == set(range(B)), case
        assert float((sym != ref).double().mean()) > 0.5        # (every window moves by one pixel: most outputs change)


def test_rowbias_rows_differ_between_samples_of_a_tile_in_every_column():
    rb = X.rowbias_rows(32, 1280)
    assert float(rb.abs().max()) <= 8 and torch.equal(rb, rb.round())
    for d in range(1, 17):
        assert bool((rb[d:] != rb[:-d]).all()), d


def test_launch_form_cases_are_exact_in_every_storage_type():
    """alpha in {0.5, -2} and the bias row keep every case exact: the operand density is lowered by 1 / |alpha| (density_for), the
    preconditions are asserted inside conv_case / linear_case; an fp32 evaluation equals the fp64 reference bit for bit."""
    for storage, wide in (("bf16", False), ("f16", False), ("f32", True)):
        for alpha in X.ALPHAS:
            c = X.conv_case(2, 128, 12, 12, 24, 3, 1, False, True, True, seed=5, storage=storage, wide=wide, rowbias=True, alpha=alpha)
            y = F.conv2d(c["x"], c["w"], None, padding=1) * alpha + c["b"].view(1, -1, 1, 1) + c["rb"].view(2, -1, 1, 1) + c["r"]
            assert y.dtype == torch.float32
            X.assert_bit_exact(f"fp32 evaluation alpha {alpha} [{storage}]", y, c["ref"], None)
            lc = X.linear_case(130, 320, 64, True, True, seed=6, storage=storage, wide=wide, alpha=alpha)
            X.assert_bit_exact(f"fp32 linear alpha {alpha} [{storage}]", (lc["x"] @ lc["w"].t()) * alpha + lc["b"] + lc["r"], lc["ref"], None)
        c = X.conv_case(2, 128, 12, 20, 24, 3, 2, False, True, True, seed=7, storage=storage, wide=wide, rowbias=True, pad=0)
        assert tuple(c["ref"].shape) == (2, 24, 6, 10)
        y = F.conv2d(F.pad(c["x"], (0, 1, 0, 1)), c["w"], c["b"], stride=2) + c["rb"].view(2, -1, 1, 1) + c["r"]
        X.assert_bit_exact(f"fp32 evaluation bottom/right padding [{storage}]", y, c["ref"], None)
    p = X.geglu_value_probe(300, 320, 128, seed=9, alpha=0.5)
    q = X.geglu_value_probe(300, 320, 128, seed=9, alpha=-2.0)
    assert p["stats"]["distinct"] >= 40 and q["stats"]["distinct"] >= 40
