"""Operator-level wrappers over the C ABI (af_op_* in include/adaface_hip.h).

Same names / argument meaning as the torch.nn.functional calls the reference makes on
the hot path, operating on fp32 CUDA(HIP) tensors in the reference's
layouts.  `dtype` selects the kernels' storage/MFMA type: "bf16", "f32" or "f16".
Used by the parity tests and by nobody on the hot path (the model executors call the
same kernels internally with no conversions).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import DTYPES, check, ptr, stream_ptr


def _dev_f32(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError("adaface_amd.ops: tensors must live on the GPU (no CPU path)")
    return t.contiguous().float()


def conv2d(x, weight, bias=None, stride=1, padding=None, upsample=False, residual=None, dtype="bf16", rowbias=None, alpha=1.0,
           ld_slack=0):
    """alpha * F.conv2d(F.interpolate(x, 2, 'nearest') if upsample else x, weight, None, stride, padding) + bias
    [+ rowbias[b]] [+ residual].  padding=0 on a 3x3 / stride-2 convolution of an even map pads below and to the right only
    (F.pad(x, (0, 1, 0, 1)), the VAE encoder's Downsample).  rowbias: [B, Cout], the per-sample row the ResBlocks add.
    ld_slack > 0 (a multiple of 8) widens every row pitch by that many elements (NaN in the operands' slack, a sentinel in the
    output buffer before the launch) and returns (y, slack): slack [B * Ho * Wo, ld_slack] is what the output buffer's slack
    columns hold after the launch (OUTPUT_SENTINEL if nothing wrote there)."""
    lib = _lib.load()
    x, weight = _dev_f32(x), _dev_f32(weight)
    B, Cin, H, W = x.shape
    Cout, Cin2, ks, ks2 = weight.shape
    if Cin2 != Cin or ks != ks2:
        raise ValueError(f"conv2d: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
    pad = ks // 2 if padding is None else padding
    up = 1 if upsample else 0
    Hi, Wi = H << up, W << up
    if pad == 0 and ks == 3:   # bottom / right only
        Ho, Wo = (Hi + 1 - ks) // stride + 1, (Wi + 1 - ks) // stride + 1
    else:
        Ho, Wo = (Hi + 2 * pad - ks) // stride + 1, (Wi + 2 * pad - ks) // stride + 1
    b = None if bias is None else _dev_f32(bias)
    r = None if residual is None else _dev_f32(residual)
    if rowbias is None and alpha == 1.0 and ld_slack == 0 and pad == ks // 2:
        y = torch.empty(B, Cout, Ho, Wo, device=x.device, dtype=torch.float32)
        check(lib.af_op_conv2d(DTYPES[dtype], ptr(x), ptr(weight), ptr(b), ptr(r), ptr(y), B, Cin, H, W, Cout, ks, stride,
                               pad, up, stream_ptr()), "af_op_conv2d")
        return y
    rb = None if rowbias is None else _dev_f32(rowbias)
    if rb is not None and tuple(rb.shape) != (B, Cout):
        raise ValueError(f"conv2d: rowbias {tuple(rb.shape)} is not [{B}, {Cout}]")
    co4 = (Cout + 3) // 4 * 4
    y = torch.empty((B * Ho * Wo, co4 + ld_slack) if ld_slack else (B, Cout, Ho, Wo), device=x.device, dtype=torch.float32)
    check(lib.af_op_conv2d_ex(DTYPES[dtype], ptr(x), ptr(weight), ptr(b), ptr(r), ptr(rb), float(alpha), ptr(y), B, Cin, H, W, Cout,
                              ks, stride, pad, up, ld_slack, stream_ptr()), "af_op_conv2d_ex")
    if not ld_slack:
        return y
    return y[:, :Cout].reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2).contiguous(), y[:, co4:].contiguous()


OUTPUT_SENTINEL = 49152.0   # 3 * 2^14: what conv2d / linear leave in the output buffer before the launch (af_ops.hip)


FP8_ACT_SHIFT = 3   # fp8 activations hold value * 2^s; s = 3 until a site is calibrated (AF_FP8_SHIFT_DEFAULT, adaface_hip.h)


def _fp8_record(rec):
    """The two 32-bit words an af_op_*_fp8_rec call wrote -> (amax: float, nsat: int)."""
    words = rec.cpu()
    return float(words.view(torch.float32)[0]), int(words[1]) & 0xFFFFFFFF


def conv2d_fp8(x, weight, bias=None, stride=1, upsample=False, residual=None, act_shift=FP8_ACT_SHIFT):
    """conv2d with both operands quantised to OCP e4m3 as the UNet's fp8 mode does (x * 2^act_shift saturating, weight
    rows scaled by a power of two), bf16 bias / residual / output.  Raises AfError when the shape has no fp8 plan."""
    lib = _lib.load()
    x, weight = _dev_f32(x), _dev_f32(weight)
    B, Cin, H, W = x.shape
    Cout, Cin2, ks, ks2 = weight.shape
    if Cin2 != Cin or ks != ks2:
        raise ValueError(f"conv2d_fp8: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
    pad, up = ks // 2, 1 if upsample else 0
    Hi, Wi = H << up, W << up
    Ho, Wo = (Hi + 2 * pad - ks) // stride + 1, (Wi + 2 * pad - ks) // stride + 1
    y = torch.empty(B, Cout, Ho, Wo, device=x.device, dtype=torch.float32)
    b = None if bias is None else _dev_f32(bias)
    r = None if residual is None else _dev_f32(residual)
    check(lib.af_op_conv2d_fp8(ptr(x), ptr(weight), ptr(b), ptr(r), ptr(y), B, Cin, H, W, Cout, ks, stride, pad, up,
                               act_shift, stream_ptr()), "af_op_conv2d_fp8")
    return y


def group_norm_fp8(x, weight, bias, eps=1e-5, silu=False, act_shift=FP8_ACT_SHIFT, record=False):
    """GroupNorm(32) [+ SiLU] written as e4m3 bytes of result * 2^act_shift: uint8 [B, H*W, C] (NHWC).
    record=True: returns (bytes, (amax, nsat)), the calibration record of the call: the largest |result| the kernel saw and
    the number of elements with |result * 2^act_shift| > 448."""
    lib = _lib.load()
    x = _dev_f32(x)
    B, Cn, H, W = x.shape
    y = torch.empty(B, H * W, Cn, device=x.device, dtype=torch.uint8)
    if record:
        rec = torch.zeros(2, device=x.device, dtype=torch.int32)
        check(lib.af_op_groupnorm_fp8_rec(ptr(x), ptr(_dev_f32(weight)), ptr(_dev_f32(bias)), eps, 1 if silu else 0, ptr(y), B,
                                          Cn, H, W, act_shift, ptr(rec), stream_ptr()), "af_op_groupnorm_fp8_rec")
        return y, _fp8_record(rec)
    check(lib.af_op_groupnorm_fp8(ptr(x), ptr(_dev_f32(weight)), ptr(_dev_f32(bias)), eps, 1 if silu else 0, ptr(y), B, Cn,
                                  H, W, act_shift, stream_ptr()), "af_op_groupnorm_fp8")
    return y


def layer_norm_fp8(x, weight, bias, eps=1e-5, act_shift=FP8_ACT_SHIFT, record=False):
    """LayerNorm over the last dim written as e4m3 bytes of result * 2^act_shift: uint8, same shape as x.
    record=True: returns (bytes, (amax, nsat)) as group_norm_fp8."""
    lib = _lib.load()
    x = _dev_f32(x)
    Cn = x.shape[-1]
    rows = x.numel() // Cn
    y = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    if record:
        rec = torch.zeros(2, device=x.device, dtype=torch.int32)
        check(lib.af_op_layernorm_fp8_rec(ptr(x), ptr(_dev_f32(weight)), ptr(_dev_f32(bias)), eps, ptr(y), rows, Cn, act_shift,
                                          ptr(rec), stream_ptr()), "af_op_layernorm_fp8_rec")
        return y, _fp8_record(rec)
    check(lib.af_op_layernorm_fp8(ptr(x), ptr(_dev_f32(weight)), ptr(_dev_f32(bias)), eps, ptr(y), rows, Cn, act_shift,
                                  stream_ptr()), "af_op_layernorm_fp8")
    return y


def ff_fp8(x, ln_weight, ln_bias, w1, b1, w2, b2, residual=None, shift1=FP8_ACT_SHIFT, shift2=FP8_ACT_SHIFT, eps=1e-5,
           x8=None, record=False):
    """One FeedForward as the fp8 mode's FF scope runs it (af_op_ff_fp8): LayerNorm -> e4m3 * 2^shift1 -> GEGLU (w1 [2F, C]:
    value rows then gate rows, b1) on the fp8 MFMA -> e4m3 * 2^shift2 -> w2 [Cout, F], b2, + residual -> bf16.
    x8: uint8 [M, C] of raw e4m3 bytes that replace the LayerNorm output (x / ln_weight / ln_bias may then be None).
    Returns {"y": fp32 [M, Cout] (bf16 values), "mid8": uint8 [M, F] (the GEGLU bytes), "plan": (tile, splitk) of the second
    GEMM, "record": (amax, nsat) of the GEGLU output when record=True}."""
    import ctypes as C
    lib = _lib.load()
    w1, w2 = _dev_f32(w1), _dev_f32(w2)
    F2, Cn = w1.shape
    Cout, Fn = w2.shape
    if F2 != 2 * Fn:
        raise ValueError(f"ff_fp8: w1 {tuple(w1.shape)} / w2 {tuple(w2.shape)}")
    if x8 is not None:
        x8 = x8.contiguous()
        assert x8.dtype == torch.uint8 and x8.shape[-1] == Cn
        M, dev = x8.numel() // Cn, x8.device
        xf = g = b = None
    else:
        xf, g, b = _dev_f32(x), _dev_f32(ln_weight), _dev_f32(ln_bias)
        M, dev = xf.numel() // Cn, xf.device
    b1 = None if b1 is None else _dev_f32(b1)
    b2 = None if b2 is None else _dev_f32(b2)
    r = None if residual is None else _dev_f32(residual)
    y = torch.empty(M, Cout, device=dev, dtype=torch.float32)
    mid = torch.empty(M, Fn, device=dev, dtype=torch.uint8)
    rec = torch.zeros(2, device=dev, dtype=torch.int32) if record else None
    plan = (C.c_int * 2)()
    check(lib.af_op_ff_fp8(ptr(xf), ptr(x8), ptr(g), ptr(b), eps, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(r), M, Cn, Fn, Cout,
                           shift1, shift2, ptr(rec), ptr(y), ptr(mid), plan, stream_ptr()), "af_op_ff_fp8")
    out = {"y": y, "mid8": mid, "plan": (int(plan[0]), int(plan[1]))}
    if record:
        out["record"] = _fp8_record(rec)
    return out


def linear(x, weight, bias=None, residual=None, geglu=False, dtype="bf16", alpha=1.0, ld_slack=0):
    """alpha * F.linear(x, weight) + bias [+ residual] over the last dim; geglu=True applies GEGLU (attention.py:32-45) to the
    projection.  ld_slack > 0: wide rows as conv2d, returns (y, slack) with slack [M, ld_slack]."""
    lib = _lib.load()
    x, weight = _dev_f32(x), _dev_f32(weight)
    K = x.shape[-1]
    M = x.numel() // K
    rows = weight.shape[0]
    N = rows // 2 if geglu else rows
    b = None if bias is None else _dev_f32(bias)
    r = None if residual is None else _dev_f32(residual)
    if alpha == 1.0 and ld_slack == 0:
        y = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
        check(lib.af_op_linear(DTYPES[dtype], ptr(x), ptr(weight), ptr(b), ptr(r), ptr(y), M, K, N, 1 if geglu else 0,
                               stream_ptr()), "af_op_linear")
        return y
    no4 = (N + 3) // 4 * 4
    y = torch.empty((M, no4 + ld_slack) if ld_slack else (*x.shape[:-1], N), device=x.device, dtype=torch.float32)
    check(lib.af_op_linear_ex(DTYPES[dtype], ptr(x), ptr(weight), ptr(b), ptr(r), float(alpha), ptr(y), M, K, N, 1 if geglu else 0,
                              ld_slack, stream_ptr()), "af_op_linear_ex")
    if not ld_slack:
        return y
    return y[:, :N].reshape(*x.shape[:-1], N).contiguous(), y[:, no4:].contiguous()


def group_norm(x, weight, bias, eps=1e-5, silu=False, dtype="bf16"):
    """F.group_norm(x, 32, weight, bias, eps) (+ SiLU)."""
    lib = _lib.load()
    x = _dev_f32(x)
    B, Cn, H, W = x.shape
    y = torch.empty_like(x)
    check(lib.af_op_groupnorm(DTYPES[dtype], ptr(x), ptr(_dev_f32(weight)), ptr(_dev_f32(bias)), eps, 1 if silu else 0,
                              ptr(y), B, Cn, H, W, stream_ptr()), "af_op_groupnorm")
    return y


def conv_gn(x, w, b, gamma, beta, eps=1e-5, silu=True, residual=None):
    """conv3x3 (stride 1, bf16) then GroupNorm(32)(+SiLU) with the statistics summed in the convolution's epilogue
    (af_op_conv_gn).  Returns (conv output, GroupNorm output)."""
    lib = _lib.load()
    x = _dev_f32(x)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    h = torch.empty(B, Cout, H, W, device=x.device, dtype=torch.float32)
    y = torch.empty_like(h)
    check(lib.af_op_conv_gn(ptr(x), ptr(_dev_f32(w)), ptr(_dev_f32(b)) if b is not None else None,
                            ptr(_dev_f32(residual)) if residual is not None else None, ptr(_dev_f32(gamma)), ptr(_dev_f32(beta)),
                            eps, 1 if silu else 0, ptr(h), ptr(y), B, Cin, H, W, Cout, stream_ptr()), "af_op_conv_gn")
    return h, y


def gn_conv1x1(x, gamma, beta, w, bias=None, eps=1e-6):
    """GroupNorm(32) + 1x1 convolution (SpatialTransformer.norm + proj_in) in bf16, both ways (af_op_gn_conv1x1): returns
    (plain, fused) = (apply pass + GEMM, row-panel GEMM with the GroupNorm in its prologue), each [B, N, H, W]."""
    lib = _lib.load()
    x = _dev_f32(x)
    B, Cn, H, W = x.shape
    N = w.shape[0]
    y0 = torch.empty(B, N, H, W, device=x.device, dtype=torch.float32)
    y1 = torch.empty_like(y0)
    check(lib.af_op_gn_conv1x1(ptr(x), ptr(_dev_f32(gamma)), ptr(_dev_f32(beta)), eps, ptr(_dev_f32(w.reshape(N, Cn))),
                               ptr(_dev_f32(bias)) if bias is not None else None, ptr(y0), ptr(y1), B, Cn, H, W, N, stream_ptr()),
          "af_op_gn_conv1x1")
    return y0, y1


LN_CHAIN_PARTS_CAP = 20     # statistics slabs ln_chain leaves room for: 16 of C = 1280 and spare ones that must stay unwritten
LN_CHAIN_GUARD_ROWS = 256   # rows behind the M valid ones of t and y: one row panel


def geglu_row_perm(rows):
    """Row of output feature n of a GEGLU projection [2 N, K] (value rows, then gate rows) in the kernels' repacked weight:
    value / gate groups of 16 interleaved (geglu_perm, csrc/af_common.h).  A LongTensor p with packed[p[n]] = w[n]."""
    n = torch.arange(rows)
    half = rows // 2
    j = torch.where(n < half, n, n - half)
    return (j // 16) * 32 + torch.where(n < half, 0, 16) + (j % 16)


def ln_chain(a, wp, gamma, beta, wc, bp=None, res=None, bc=None, eps=1e-5, geglu=False, dtype="bf16", parts_n=0):
    """One producer GEMM -> LayerNorm -> consumer GEMM pair with the LayerNorm folded into the GEMMs, as the transformer blocks
    run it in bf16 (af_op_ln_chain), every intermediate returned.  a [M, Kp], wp [C, Kp], bp [C], res [M, C], gamma / beta [C],
    wc [N, C] ([2 N, C] with geglu), bc [N] ([2 N]).  Returns a dict of fp32 tensors:
      Wf [rows, C], colsum [rows], biasf [rows]  the folded consumer weight, its row sums and W beta + b, in wc's row order
      t [M, C]            the producer's stored output;  t_guard: the LN_CHAIN_GUARD_ROWS rows behind it
      parts [slabs, M, 2] (sum, sum of squares) per statistics slab;  parts_spare: the slabs behind them (NaN unless written)
      stats [M, 2]        (mu, rstd) from ln_finalize_kernel
      y_folded, y_plain [M, N]  the folded consumer / LayerNorm launch + plain GEMM;  y_folded_guard, y_plain_guard
    and plans = two dicts (kernel by its GEMM_KERNELS name, rowpanel, tile, splitk, ln_slabs) of the producer and the folded
    consumer.  AfError where a launch plans no LayerNorm epilogue, for parts_n > 0 that is not the producer's slab count and
    for a dtype other than bf16."""
    lib = _lib.load()
    M, Kp = a.shape
    Cn = wp.shape[0]
    rows = wc.shape[0]
    N = rows // 2 if geglu else rows
    if wp.shape[1] != Kp or wc.shape[1] != Cn or (res is not None and tuple(res.shape) != (M, Cn)):
        raise ValueError(f"ln_chain: a {tuple(a.shape)}, wp {tuple(wp.shape)}, wc {tuple(wc.shape)} do not chain")
    plans = (C.c_int * 10)()
    dev, G, cap = a.device, LN_CHAIN_GUARD_ROWS, LN_CHAIN_PARTS_CAP
    f = dict(device=dev, dtype=torch.float32)
    wf, cs, bf = torch.empty(rows, Cn, **f), torch.empty(rows, **f), torch.empty(rows, **f)
    t, parts, stats = torch.empty(M + G, Cn, **f), torch.empty(cap, M, 2, **f), torch.empty(M, 2, **f)
    y1, y0 = torch.empty(M + G, N, **f), torch.empty(M + G, N, **f)
    opt = lambda v: None if v is None else ptr(_dev_f32(v))   # noqa: E731
    check(lib.af_op_ln_chain(DTYPES[dtype], ptr(_dev_f32(a)), ptr(_dev_f32(wp)), opt(bp), opt(res), ptr(_dev_f32(gamma)),
                             ptr(_dev_f32(beta)), eps, ptr(_dev_f32(wc)), opt(bc), M, Kp, Cn, N, int(geglu), parts_n, cap, G,
                             ptr(wf), ptr(cs), ptr(bf), ptr(t), ptr(parts), ptr(stats), ptr(y1), ptr(y0), plans, stream_ptr()),
          "af_op_ln_chain")
    pl = tuple(dict(kernel=GEMM_KERNELS.get(int(plans[5 * i]), int(plans[5 * i])), rowpanel=int(plans[5 * i + 1]),
                    tile=int(plans[5 * i + 2]), splitk=int(plans[5 * i + 3]), ln_slabs=int(plans[5 * i + 4])) for i in range(2))
    if geglu:   # back to wc's row order
        p = geglu_row_perm(rows).to(dev)
        wf, cs, bf = wf[p], cs[p], bf[p]
    slabs = pl[0]["ln_slabs"]
    return {"Wf": wf, "colsum": cs, "biasf": bf, "t": t[:M], "t_guard": t[M:], "parts": parts[:slabs], "parts_spare": parts[slabs:],
            "stats": stats, "y_folded": y1[:M], "y_folded_guard": y1[M:], "y_plain": y0[:M], "y_plain_guard": y0[M:], "plans": pl}


def layer_norm(x, weight, bias, eps=1e-5, dtype="bf16"):
    lib = _lib.load()
    x = _dev_f32(x)
    Cn = x.shape[-1]
    y = torch.empty_like(x)
    check(lib.af_op_layernorm(DTYPES[dtype], ptr(x), ptr(_dev_f32(weight)), ptr(_dev_f32(bias)), eps, ptr(y),
                              x.numel() // Cn, Cn, stream_ptr()), "af_op_layernorm")
    return y


def tome_match(x, hw, ratio, normalize=True, dtype="bf16"):
    """Token-merging match on x [B, H*W, C] (hw = (H, W), both even): (node_idx int32 [B, Ns], node_max fp32 [B, Ns],
    map int32 [B, H*W]) -- per src token the lowest best dst ordinal and its score (cosine, or the plain dot product with
    normalize=False), and the merged row of every token when r = min(Ns, int(N * ratio)) src tokens are merged."""
    lib = _lib.load()
    x = _dev_f32(x)
    B, N, Cn = x.shape
    H, W = hw
    if H * W != N:
        raise ValueError(f"tome_match: {H} x {W} map, {N} tokens")
    Nd, Ns, _, _ = _lib.tome_plan_query(H, W, ratio)
    node_idx = torch.empty(B, Ns, device=x.device, dtype=torch.int32)
    node_max = torch.empty(B, Ns, device=x.device, dtype=torch.float32)
    tmap = torch.empty(B, N, device=x.device, dtype=torch.int32)
    check(lib.af_op_tome_match(DTYPES[dtype], ptr(x), B, H, W, Cn, float(ratio), 1 if normalize else 0, ptr(node_idx),
                               ptr(node_max), ptr(tmap), stream_ptr()), "af_op_tome_match")
    return node_idx, node_max, tmap


def tome_merge(x, tmap, n_rows, weight=None, bias=None, eps=1e-5, dtype="bf16"):
    """Rows of the merged sequence [B, n_rows, C]: row j = the mean over the tokens i with tmap[b, i] = j of LayerNorm(x[b, i])
    (weight = None: of x[b, i]), summed in fp32 in ascending i and rounded once."""
    lib = _lib.load()
    x = _dev_f32(x)
    B, N, Cn = x.shape
    tmap = tmap.to(device=x.device, dtype=torch.int32).contiguous()
    y = torch.empty(B, int(n_rows), Cn, device=x.device, dtype=torch.float32)
    check(lib.af_op_tome_merge(DTYPES[dtype], ptr(x), ptr(_dev_f32(weight)) if weight is not None else None,
                               ptr(_dev_f32(bias)) if bias is not None else None, eps, ptr(tmap), B, N, int(n_rows), Cn, ptr(y),
                               stream_ptr()), "af_op_tome_merge")
    return y


def tome_unmerge_add(o, res, tmap, dtype="bf16"):
    """res [B, N, C] + o [B, N', C] gathered by tmap [B, N], in fp32, rounded once."""
    lib = _lib.load()
    o, res = _dev_f32(o), _dev_f32(res)
    B, N, Cn = res.shape
    tmap = tmap.to(device=res.device, dtype=torch.int32).contiguous()
    y = torch.empty_like(res)
    check(lib.af_op_tome_unmerge_add(DTYPES[dtype], ptr(o), ptr(res), ptr(tmap), B, N, o.shape[1], Cn, ptr(y), stream_ptr()),
          "af_op_tome_unmerge_add")
    return y


def freeu(h, skip, version, b, s, dtype="bf16"):
    """FreeU on one concatenation, h [B, Ch, H, W] and skip [B, Cs, H, W] (Ch % 16 == 0, Cs % 8 == 0, H, W >= 2): the first
    Ch / 2 channels of h times b (version 1) or times (b - 1) * mhat + 1 (version 2), skip + (s - 1) * its part at the
    frequencies {-1, 0}^2; fp32 arithmetic on the values stored as `dtype`, rounded once.  Returns (h', skip') in fp32."""
    lib = _lib.load()
    h, skip = _dev_f32(h), _dev_f32(skip)
    B, Ch, H, W = h.shape
    if skip.shape[0] != B or tuple(skip.shape[2:]) != (H, W):
        raise ValueError(f"freeu: h {tuple(h.shape)} and skip {tuple(skip.shape)} do not concatenate")
    h_out, skip_out = torch.empty_like(h), torch.empty_like(skip)
    check(lib.af_op_freeu(DTYPES[dtype], ptr(h), ptr(skip), B, Ch, skip.shape[1], H, W, int(version), float(b), float(s),
                          ptr(h_out), ptr(skip_out), stream_ptr()), "af_op_freeu")
    return h_out, skip_out


STORAGE_TORCH = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}


def _rows_ld(name, t, shape):
    """Row stride (elements) of a [B', N, C] device view whose rows are C contiguous elements ld apart, samples N * ld apart."""
    if not t.is_cuda or tuple(t.shape) != tuple(shape):
        raise ValueError(f"tgate_add: {name} must be a device tensor of shape {tuple(shape)}, got {tuple(t.shape)}")
    ld = t.stride(1) if t.shape[1] > 1 else (t.stride(0) // max(t.shape[1], 1) if t.shape[0] > 1 else t.shape[2])
    if t.stride(2) != 1 or ld < t.shape[2] or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * ld):
        raise ValueError(f"tgate_add: {name} has strides {t.stride()}: rows must be contiguous and evenly spaced")
    return int(ld)


def tgate_add(t1, src, legs=1, cache=False, stats_parts=0, out=None, cache_out=None):
    """The T-GATE add (af_op_tgate_add) on the caller's own buffers, all of one storage dtype (bf16, fp16 or f32), nothing
    converted or copied: t2 = t1 + src for [legs * B, N, C] views (rows of C contiguous elements, any row stride and alignment),
    fp32 add, rounded once; cache: also the mean of src over the legs (1 or 2; sample b with b + B), [B, N, C]; stats_parts > 0:
    also fp32 [stats_parts, legs * B * N, 2], the sum and the sum of squares of every t2 row's rounded values in part 0.
    out: where t2 goes (may be src itself); cache_out: where the mean goes.  Returns (t2, cache or None, stats or None)."""
    lib = _lib.load()
    names = {v: k for k, v in STORAGE_TORCH.items()}
    if t1.dtype not in names or src.dtype != t1.dtype:
        raise ValueError(f"tgate_add: storage dtypes {t1.dtype} / {src.dtype}")
    if legs not in (1, 2) or t1.dim() != 3 or t1.shape[0] % legs:
        raise ValueError(f"tgate_add: {legs} legs for a batch of {tuple(t1.shape)}")
    LB, N, Cn = t1.shape
    B = LB // legs
    ld1, lds = _rows_ld("t1", t1, t1.shape), _rows_ld("src", src, t1.shape)
    if out is None:
        out = torch.empty(LB, N, Cn, device=t1.device, dtype=t1.dtype)
    ld2 = _rows_ld("out", out, t1.shape)
    if cache and cache_out is None:
        cache_out = torch.empty(B, N, Cn, device=t1.device, dtype=t1.dtype)
    ldc = 0
    if cache_out is not None:
        if cache_out.dtype != t1.dtype:
            raise ValueError("tgate_add: cache_out has another dtype")
        ldc = _rows_ld("cache_out", cache_out, (B, N, Cn))
    stats = torch.empty(int(stats_parts), LB * N, 2, device=t1.device, dtype=torch.float32) if stats_parts > 0 else None
    check(lib.af_op_tgate_add(DTYPES[names[t1.dtype]], ptr(t1), ptr(src), ptr(out), ptr(cache_out), ptr(stats), int(stats_parts),
                              int(legs), B, N, Cn, ld1, lds, ld2, ldc, stream_ptr()), "af_op_tgate_add")
    return out, cache_out, stats


def control_add(dsts, srcs, scales, cond_only=False):
    """The ControlNet residual add (af_op_control_add) on the caller's own buffers, in place, ONE launch for all segments:
    dsts[k] [Bd, P_k, C_k] (rows of C_k contiguous elements, any row stride and alignment: a channel range of a wider buffer)
    += scales[k] * srcs[k] [Bs, P_k, C_k] (dense), fp32 product rounded, fp32 sum rounded, then the storage rounding.  Bd = Bs,
    or cond_only: Bd = 2 Bs and only the samples < Bs are touched.  All of one storage dtype (bf16, fp16 or f32); at most 16
    segments.  Nothing outside the addressed channel ranges is read or written.  Returns dsts."""
    lib = _lib.load()
    names = {v: k for k, v in STORAGE_TORCH.items()}
    dsts, srcs, scales = list(dsts), list(srcs), [float(v) for v in scales]
    n = len(dsts)
    if not (n == len(srcs) == len(scales)) or n < 1:
        raise ValueError(f"control_add: {n} dsts, {len(srcs)} srcs, {len(scales)} scales")
    if n > _lib.CONTROL_MAX_SEGMENTS:
        raise ValueError(f"control_add: {n} segments (at most {_lib.CONTROL_MAX_SEGMENTS})")
    dt = dsts[0].dtype
    if dt not in names or any(t.dtype != dt for t in dsts + srcs):
        raise ValueError(f"control_add: one storage dtype for every operand, got {sorted({str(t.dtype) for t in dsts + srcs})}")
    if any(t.dim() != 3 for t in dsts + srcs):
        raise ValueError("control_add: operands are [B, P, C] views")
    Bs, Bd = srcs[0].shape[0], dsts[0].shape[0]
    if Bd != (2 * Bs if cond_only else Bs):
        raise ValueError(f"control_add: dst batch {Bd} for a src batch of {Bs} (cond_only={bool(cond_only)})")
    lds = []
    for k, (d, s) in enumerate(zip(dsts, srcs)):
        if s.shape[0] != Bs or d.shape[0] != Bd or tuple(s.shape[1:]) != tuple(d.shape[1:]):
            raise ValueError(f"control_add: segment {k}: dst {tuple(d.shape)} against src {tuple(s.shape)}")
        if not s.is_cuda or not s.is_contiguous():
            raise ValueError(f"control_add: segment {k}: src must be a dense device tensor (strides {s.stride()})")
        lds.append(_rows_ld(f"dsts[{k}]", d, d.shape))
    P = _lib.C.c_void_p
    check(lib.af_op_control_add(DTYPES[names[dt]], n, (P * n)(*[d.data_ptr() for d in dsts]), (P * n)(*[s.data_ptr() for s in srcs]),
                                (_lib.C.c_int * n)(*[int(d.shape[2]) for d in dsts]), (_lib.C.c_int * n)(*lds),
                                (_lib.C.c_int64 * n)(*[int(d.shape[1]) for d in dsts]), (_lib.C.c_float * n)(*scales),
                                int(Bs), int(Bd), stream_ptr()), "af_op_control_add")
    return dsts


def lora_repack(base, adapters=(), cin_pad=None, ldw=None, row_off=0, rows_total=None, perm=False, dtype="bf16", out=None):
    """The weight repack with LoRA adapters merged (af_op_lora_repack): base [rows, cin(, ks, ks)] fp32 and adapters
    [(up [rows, r(, 1, 1)], down [r, cin(, ks, ks)], s)] (at most 8, r <= 256) -> the packed buffer [rows_total, ldw] in the storage
    type `dtype`, element (row_off + perm(o), tap * cin_pad + c) = base[o, c, tap] + sum_a s_a * (up_a @ down_a)[o, c * ks^2 + tap],
    formed in fp32 and rounded once; columns cin <= c < cin_pad are zeros.  perm: the GEGLU row order.  Defaults: cin_pad = cin,
    ldw = ks^2 * cin_pad, rows_total = row_off + rows.  out: a buffer of that shape and type to write into (what the kernel does
    not own keeps its content); otherwise a zero-filled one."""
    from .lora import check_lora_pair
    lib = _lib.load()
    base = _dev_f32(base)
    rows, cin = base.shape[0], base.shape[1]
    ks = base.shape[2] if base.dim() == 4 else 1
    cin_pad = cin if cin_pad is None else int(cin_pad)
    ldw = ks * ks * cin_pad if ldw is None else int(ldw)
    rows_total = row_off + rows if rows_total is None else int(rows_total)
    if row_off < 0 or row_off + rows > rows_total:
        raise ValueError(f"lora_repack: rows {row_off} .. {row_off + rows} outside a buffer of {rows_total}")
    if out is None:
        out = torch.zeros(rows_total, ldw, device=base.device, dtype=STORAGE_TORCH[dtype])
    elif tuple(out.shape) != (rows_total, ldw) or out.dtype != STORAGE_TORCH[dtype] or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"lora_repack: out must be a contiguous device tensor [{rows_total}, {ldw}] of {STORAGE_TORCH[dtype]}")
    adapters = list(adapters)
    n = len(adapters)
    ups, downs = [], []
    for i, (up, down, _s) in enumerate(adapters):
        check_lora_pair(f"adapter {i}", tuple(base.shape), tuple(up.shape), tuple(down.shape))
        ups.append(_dev_f32(up))
        downs.append(_dev_f32(down))
    arr = lambda t, vals: (t * max(n, 1))(*vals)
    check(lib.af_op_lora_repack(DTYPES[dtype], ptr(base), rows, cin, cin_pad, ks, ldw, int(row_off), 1 if perm else 0, n,
                                arr(C.c_void_p, [u.data_ptr() for u in ups]), arr(C.c_void_p, [d.data_ptr() for d in downs]),
                                arr(C.c_int, [int(d.shape[0]) for d in downs]), arr(C.c_float, [float(a[2]) for a in adapters]),
                                ptr(out), stream_ptr()), "af_op_lora_repack")
    return out


ATTN_LAYOUTS = {"dense": 0, "qkv": 1, "ctx": 2}     # AF_ATTN_* (include/adaface_hip.h)


def attention(q, k, v, heads, scale=None, dtype="bf16", causal=False, nan_guard=False, *, layout="dense", ld_slack=0, lse=False,
              batch_window=None, drop_keys=0):
    """softmax(q k^T * scale) v per head; q [B,N,heads*dh], k/v [B,S,heads*dh] (attention.py:197-243).  causal: query i
    attends to keys <= i (the CLIP text tower's mask).  nan_guard (tests): K / V sit in front of 128 rows of NaNs.

    The keyword-only arguments state the forms of AttnParams only the model builds (af_op_attention_ex); with all of them at
    their defaults the call is af_op_attention as before and returns o [B,N,heads*dh].  With any of them set:
      layout        "dense": three buffers; "qkv": q | k | v as columns of one [B][N][3C] buffer (self-attention, N == S);
                    "ctx": k | v as columns of one [B][S][2C] buffer, the cached context, from which the short-key kernel's V^T
                    pack is made (bf16, dh 40 / 80, <= 96 keys, no mask, no lse); "qkv" makes no pack, as the model's
                    self-attention has none
      ld_slack      elements (a multiple of 8) added to every row pitch, the output's included
      lse           also return the log2-domain log-sum-exp of the scaled scores, fp32 [B, heads, N]; no V^T pack is made
      batch_window  (b0, nb): samples [b0, b0 + nb) run, every pointer moved by b0 samples
      drop_keys     the last drop_keys key rows are left out (the batch stride stays S rows)
    and the return value is the WHOLE pitched output [B, N, heads*dh + ld_slack] (or the pair (o, lse)): every input buffer, the
    output and lse hold NaN bytes before the launch, so slack columns and samples outside the window read NaN unless the kernel
    wrote there, and a NaN inside the window is a read of a slack column or of a row behind the operands."""
    lib = _lib.load()
    q, k, v = _dev_f32(q), _dev_f32(k), _dev_f32(v)
    B, Nq, Cn = q.shape
    Nk = k.shape[1]
    dh = Cn // heads
    scale = dh ** -0.5 if scale is None else scale
    flags = (1 if causal else 0) | (2 if nan_guard else 0)
    if layout == "dense" and ld_slack == 0 and not lse and batch_window is None and drop_keys == 0:
        o = torch.empty_like(q)
        check(lib.af_op_attention(DTYPES[dtype], ptr(q), ptr(k), ptr(v), ptr(o), B, Nq, Nk, heads, dh, scale, flags, stream_ptr()),
              "af_op_attention")
        return o
    b0, nb = (0, -1) if batch_window is None else batch_window
    o = torch.empty(B, Nq, Cn + ld_slack, dtype=torch.float32, device=q.device)
    l = torch.empty(B, heads, Nq, dtype=torch.float32, device=q.device) if lse else None
    check(lib.af_op_attention_ex(DTYPES[dtype], ptr(q), ptr(k), ptr(v), ptr(o), ptr(l), B, Nq, Nk, heads, dh, scale, flags,
                                 ATTN_LAYOUTS[layout], int(ld_slack), int(b0), int(nb), int(drop_keys), stream_ptr()),
          "af_op_attention_ex")
    return (o, l) if lse else o


REGION_PATHS = {"auto": 0, "composition": 1, "fused": 2}


def region_weights(m):
    """af_op_region_weights (region_weights_kernel): m [Bf, R, H, W] >= 0 -> (list of the four pyramid levels, fp32
    [Bf, R, H >> l, W >> l]; list of the active-region words per level, int64 [Bf, ceil(N_l / 32)])."""
    from .regions import level_offsets
    lib = _lib.load()
    m = _dev_f32(m)
    Bf, R, H, W = m.shape
    w_off, b_off, n_w, n_b = level_offsets(Bf, R, H, W)
    pyr = torch.full((max(n_w, 1),), float("nan"), dtype=torch.float32, device=m.device)
    bits = torch.full((max(n_b, 1),), -1, dtype=torch.int32, device=m.device)
    check(lib.af_op_region_weights(ptr(m), Bf, R, H, W, ptr(pyr), ptr(bits), stream_ptr()), "af_op_region_weights")
    levels, words = [], []
    for l in range(4):
        h, w = H >> l, W >> l
        nblk = (h * w + 31) // 32
        levels.append(pyr[w_off[l]: w_off[l] + Bf * R * h * w].reshape(Bf, R, h, w))
        words.append(bits[b_off[l]: b_off[l] + Bf * nblk].reshape(Bf, nblk).long() & 0xFFFFFFFF)
    return levels, words


def region_attention(q, k, v, w, heads, R, scale=None, dtype="bf16", path="auto", ld_slack=0):
    """af_op_region_attention: o(p) = sum over {r : w_r(p) > 0} of w_r(p) softmax(q_p K_r^T scale) V_r per head.  q [B, Nq, C],
    k / v [B, R T, C] (R segments of T keys), w [B, R, Nq] (normalised weights: a level of the pyramid).  path: "auto" (the
    planner), "composition" (R attention launches + the combine) or "fused" (region_attn_kernel).  Returns the whole pitched
    output [B, Nq, C + ld_slack]: every staged buffer holds NaN bytes wherever no operand is, as ops.attention's keyword forms."""
    lib = _lib.load()
    q, k, v, w = _dev_f32(q), _dev_f32(k), _dev_f32(v), _dev_f32(w)
    B, Nq, Cn = q.shape
    if k.shape[1] % R or tuple(w.shape) != (B, R, Nq) or k.shape != v.shape:
        raise ValueError(f"region_attention: k {tuple(k.shape)}, w {tuple(w.shape)} for {R} regions and {Nq} queries")
    T = k.shape[1] // R
    dh = Cn // heads
    scale = dh ** -0.5 if scale is None else scale
    o = torch.empty(B, Nq, Cn + ld_slack, dtype=torch.float32, device=q.device)
    check(lib.af_op_region_attention(DTYPES[dtype], ptr(q), ptr(k), ptr(v), ptr(w), ptr(o), B, Nq, R, T, heads, dh, scale,
                                     REGION_PATHS[path], int(ld_slack), stream_ptr()), "af_op_region_attention")
    return o


CONV_ATTN_PATHS = {"auto": 0, "merge": 1, "one_pass": 2}


def conv_attn_key_order(n_keys, token_idx, ks):
    """Key order of conv attention, as af_set_context lays the cached key list out: the subject tokens at the tail, the other
    tokens first in their own order, then string by string in the order given (each string's ks^2 positions in the
    reference's tap order).  token_idx: list of strings, each ks^2 distinct positions in [0, n_keys); no position twice.
    Returns the list `order` with new row r = old row order[r]."""
    nt = ks * ks
    groups = [[int(t) for t in g] for g in token_idx]
    if ks not in (2, 3, 4):
        raise ValueError(f"conv attention: kernel size {ks} (the reference has 2, 3 and 4)")
    if not groups or any(len(g) != nt for g in groups):
        raise ValueError(f"conv attention: every subject string needs ks^2 = {nt} token positions")
    flat = [t for g in groups for t in g]
    if any(t < 0 or t >= n_keys for t in flat):
        raise ValueError(f"conv attention: token position outside [0, {n_keys})")
    if len(set(flat)) != len(flat):
        raise ValueError("conv attention: a token position appears twice")
    if len(flat) >= n_keys:
        raise ValueError("conv attention: no ordinary key left")
    subj = set(flat)
    return [t for t in range(n_keys) if t not in subj] + flat


def conv_attention(q, k, v, heads, hw, ks, token_idx, scale=None, dtype="bf16", path="auto"):
    """Cross-attention with subject-token convolutional attention (attention.py:208-216, ldm/util.py:701-879): the score
    columns of the ks^2 tokens of every subject string in token_idx are replaced by the shifted ks x ks conv maps of q with
    their keys, then softmax over all keys and the product with v.  q [B, H*W, heads*dh] with hw = (H, W), k / v
    [B, S, heads*dh]; every sample carries all strings.  path: "auto" = the UNet planner's choice, "merge" = flash attention
    + the subj_scores / merge kernels, "one_pass" = conv map + the short-key kernel (AfError where the shape has none)."""
    lib = _lib.load()
    q, k, v = _dev_f32(q), _dev_f32(k), _dev_f32(v)
    B, N, Cn = q.shape
    Nk = k.shape[1]
    Hh, Ww = hw
    if Hh * Ww != N:
        raise ValueError(f"conv_attention: hw {hw} does not match {N} queries")
    dh = Cn // heads
    scale = dh ** -0.5 if scale is None else scale
    order = torch.tensor(conv_attn_key_order(Nk, token_idx, ks), device=q.device)
    k, v = k[:, order].contiguous(), v[:, order].contiguous()
    o = torch.empty_like(q)
    check(lib.af_op_conv_attention(DTYPES[dtype], ptr(q), ptr(k), ptr(v), ptr(o), B, Hh, Ww, Nk, heads, dh, scale, ks,
                                   len(token_idx), CONV_ATTN_PATHS[path], stream_ptr()), "af_op_conv_attention")
    return o


GEMM_KERNELS = {1: "wave4", 2: "halo4", 3: "pp", 4: "pp_fp8", 5: "halo8", 6: "s8", 7: "up_phase4", 8: "rowpanel", 9: "m128"}


def vae_attention(q, k, v, dtype="bf16", taps=False):
    """The VAE mid-block attention between its qkv convolution and proj_out (model.py:179-242; af_op_vae_attention): one head
    over C channels, softmax(C^-1/2 q k^T) v with q, k, v [B, N, C]; the scores are stored in `dtype` before the softmax, as the
    VAE executors keep them.  Returns out [B, N, C].  taps=True: a dict of out, scores and probs ([B, N, N]: the stored scores
    before the softmax and P after it, storage values as fp32) and plans = ((kernel, tile, splitk) of the scores GEMM, the
    same of the P v GEMM), kernel by its GEMM_KERNELS name.  AfError where N is not a multiple of the K tile."""
    import ctypes as C
    lib = _lib.load()
    q, k, v = _dev_f32(q), _dev_f32(k), _dev_f32(v)
    if q.dim() != 3 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError(f"vae_attention: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} must all be [B, N, C]")
    B, N, Cn = q.shape
    o = torch.empty_like(q)
    sc = torch.empty(B, N, N, device=q.device, dtype=torch.float32) if taps else None
    pr = torch.empty(B, N, N, device=q.device, dtype=torch.float32) if taps else None
    plans = (C.c_int * 6)()
    check(lib.af_op_vae_attention(DTYPES[dtype], ptr(q), ptr(k), ptr(v), ptr(o), B, N, Cn, ptr(sc), ptr(pr), plans, stream_ptr()),
          "af_op_vae_attention")
    if not taps:
        return o
    return {"out": o, "scores": sc, "probs": pr,
            "plans": tuple((GEMM_KERNELS.get(int(plans[3 * i]), int(plans[3 * i])), int(plans[3 * i + 1]), int(plans[3 * i + 2]))
                           for i in range(2))}


def xattn_fused(x, gamma, beta, wq, kv, wo, bo, eps=1e-5):
    """One cross-attention layer of a 64x64-level BasicTransformerBlock in ONE kernel (bf16; attention.py:172-257, 279):
    y = x + to_out(softmax(to_q(LayerNorm(x)) K^T / sqrt(40)) V) with x [B, N, 320], kv [B, S, 640] = the context's K | V
    projections.  Returns (y, parts) with parts [4, B * N, 2] = the LayerNorm partial sums (sum, sum of squares) of the stored
    rows, as the next consumer reads them."""
    lib = _lib.load()
    x = _dev_f32(x)
    B, N, Cn = x.shape
    S = kv.shape[1]
    xb = x.to(torch.bfloat16).float().reshape(B * N, Cn)            # statistics of the rows the kernel reads
    mu = xb.mean(dim=1)
    var = (xb * xb).mean(dim=1) - mu * mu
    stats = torch.stack([mu, torch.rsqrt(var.clamp_min(0) + eps)], dim=1).contiguous()
    y = torch.empty_like(x)
    parts = torch.empty(4, B * N, 2, device=x.device, dtype=torch.float32)
    check(lib.af_op_xattn_fused(ptr(x), ptr(stats), ptr(_dev_f32(gamma)), ptr(_dev_f32(beta)), ptr(_dev_f32(wq)), ptr(_dev_f32(kv)),
                                ptr(_dev_f32(wo)), ptr(_dev_f32(bo)), ptr(y), ptr(parts), B, N, S, stream_ptr()), "af_op_xattn_fused")
    return y, parts


def timestep_embedding(t, dim, dtype="f32"):
    lib = _lib.load()
    t = t.contiguous().long()
    y = torch.empty(t.shape[0], dim, device=t.device, dtype=torch.float32)
    check(lib.af_op_timestep_embedding(DTYPES[dtype], ptr(t), ptr(y), t.shape[0], dim, stream_ptr()),
          "af_op_timestep_embedding")
    return y


def ddim_step(x, e_cond, e_uncond, guidance, a_t, a_prev, sqrt_one_minus_at, sigma_t=0.0, noise=None, temperature=1.0):
    """CFG combine + DDIM update (ddim.py:260,279-295); returns (x_prev, pred_x0)."""
    lib = _lib.load()
    x, e_cond = _dev_f32(x), _dev_f32(e_cond)
    eu = None if e_uncond is None else _dev_f32(e_uncond)
    nz = None if noise is None else _dev_f32(noise)
    x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
    check(lib.af_ddim_step(ptr(x), ptr(e_cond), ptr(eu), ptr(nz), x.numel(), float(guidance), float(a_t), float(a_prev),
                           float(sqrt_one_minus_at), float(sigma_t), float(temperature), ptr(x_prev), ptr(pred_x0),
                           stream_ptr()), "af_ddim_step")
    return x_prev, pred_x0


def dpmpp_coeffs(acp_t, acp_prev, h_last=0.0):
    """af_dpmpp_coeffs (host only, no GPU): the eight doubles (alpha_t, sigma_t, c_x, c_d, w_cur, w_prev, h, r) of one
    DPM-Solver++(2M) step from alphas_cumprod acp_t to acp_prev; h_last <= 0: a first-order step."""
    import ctypes
    out = (ctypes.c_double * 8)()
    check(_lib.load().af_dpmpp_coeffs(float(acp_t), float(acp_prev), float(h_last), out), "af_dpmpp_coeffs")
    return tuple(float(v) for v in out)


def dpmpp_step(x, e_cond, e_uncond, x0_prev, guidance, alpha_t, sigma_t, c_x, c_d, w_cur=1.0, w_prev=0.0, x_next=None,
               x0_out=None, want_x0=True):
    """CFG combine + one DPM-Solver++(2M) step (af_dpmpp_step); returns (x_next, x0).  e_uncond None: no guidance; x0_prev
    None: a first-order step.  x_next / x0_out: fp32 contiguous tensors to write into (x_next may be x itself), allocated when
    None; want_x0=False with x0_out None skips the x0 write and returns (x_next, None)."""
    lib = _lib.load()
    x, e_cond = _dev_f32(x), _dev_f32(e_cond)
    eu = None if e_uncond is None else _dev_f32(e_uncond)
    xp = None if x0_prev is None else _dev_f32(x0_prev)
    for name, t in (("e_cond", e_cond), ("e_uncond", eu), ("x0_prev", xp)):
        if t is not None and t.numel() != x.numel():
            raise ValueError(f"dpmpp_step: {name} has {t.numel()} elements, x has {x.numel()}")
    for name, t in (("x_next", x_next), ("x0_out", x0_out)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == x.numel()):
            raise ValueError(f"dpmpp_step: {name} must be a contiguous fp32 GPU tensor of x's size")
    if x_next is None:
        x_next = torch.empty_like(x)
    if x0_out is None and want_x0:
        x0_out = torch.empty_like(x)
    check(lib.af_dpmpp_step(ptr(x), ptr(e_cond), ptr(eu), ptr(xp), x.numel(), float(guidance), float(alpha_t), float(sigma_t),
                            float(c_x), float(c_d), float(w_cur), float(w_prev), ptr(x_next), ptr(x0_out), stream_ptr()),
          "af_dpmpp_step")
    return x_next, x0_out


def philox4x32_10(ctr, key):
    """af_philox4x32_10 (host only, no GPU): the four output words of Philox4x32-10 for a 4-word counter and a 2-word key."""
    import ctypes
    c = (ctypes.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in ctr])
    k = (ctypes.c_uint32 * 2)(*[int(v) & 0xFFFFFFFF for v in key])
    out = (ctypes.c_uint32 * 4)()
    check(_lib.load().af_philox4x32_10(c, k, out), "af_philox4x32_10")
    return tuple(int(v) for v in out)


def philox_randn(n_samples, per_sample, seed, stream, step, sample_ids=None, first_id=0, device=None, out=None):
    """af_philox_randn: fp32 normals [n_samples, per_sample] of the samples sample_ids (an int64 GPU tensor; None:
    first_id + i) under the keying contract of csrc/af_philox.h.  out: a contiguous fp32 GPU tensor (or view) of
    n_samples * per_sample elements to write into."""
    n_samples, per_sample = int(n_samples), int(per_sample)
    if out is None:
        out = torch.empty(n_samples, per_sample, device=device, dtype=torch.float32)
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n_samples * per_sample):
        raise ValueError("philox_randn: out must be a contiguous fp32 GPU tensor of n_samples * per_sample elements")
    if sample_ids is not None and not (sample_ids.is_cuda and sample_ids.dtype == torch.int64 and sample_ids.is_contiguous()
                                       and sample_ids.numel() >= n_samples):
        raise ValueError("philox_randn: sample_ids must be a contiguous int64 GPU tensor of at least n_samples elements")
    check(_lib.load().af_philox_randn(ptr(out), n_samples, per_sample, ptr(sample_ids), int(first_id),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(step), stream_ptr()), "af_philox_randn")
    return out


def dpmpp_sde_coeffs(acp_t, acp_prev, h_last=0.0):
    """af_dpmpp_sde_coeffs (host only, no GPU): the nine doubles (alpha_t, sigma_t, c_x, c_d, c_n, w_cur, w_prev, h, r) of one
    DPM-Solver++(2M) SDE step from alphas_cumprod acp_t to acp_prev; h_last <= 0: a first-order step."""
    import ctypes
    out = (ctypes.c_double * 9)()
    check(_lib.load().af_dpmpp_sde_coeffs(float(acp_t), float(acp_prev), float(h_last), out), "af_dpmpp_sde_coeffs")
    return tuple(float(v) for v in out)


def dpmpp_sde_step(x, e_cond, e_uncond, x0_prev, guidance, alpha_t, sigma_t, c_x, c_d, c_n, w_cur=1.0, w_prev=0.0, noise=None,
                   seed=0, step=0, sample_ids=None, first_id=0, x_next=None, x0_out=None, want_x0=True):
    """CFG combine + one DPM-Solver++(2M) SDE step (af_dpmpp_sde_step); returns (x_next, x0).  noise: the z to use (x's
    size); None: z is generated inside the kernel from (seed, sample id, stream 1, step, element), x's dim 0 being the
    samples (ids: sample_ids, an int64 GPU tensor, or first_id + i).  The other arguments as dpmpp_step."""
    lib = _lib.load()
    x, e_cond = _dev_f32(x), _dev_f32(e_cond)
    eu = None if e_uncond is None else _dev_f32(e_uncond)
    xp = None if x0_prev is None else _dev_f32(x0_prev)
    nz = None if noise is None else _dev_f32(noise)
    for name, t in (("e_cond", e_cond), ("e_uncond", eu), ("x0_prev", xp), ("noise", nz)):
        if t is not None and t.numel() != x.numel():
            raise ValueError(f"dpmpp_sde_step: {name} has {t.numel()} elements, x has {x.numel()}")
    for name, t in (("x_next", x_next), ("x0_out", x0_out)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == x.numel()):
            raise ValueError(f"dpmpp_sde_step: {name} must be a contiguous fp32 GPU tensor of x's size")
    n_samples = x.shape[0] if x.dim() > 0 else 1
    if sample_ids is not None and not (sample_ids.is_cuda and sample_ids.dtype == torch.int64 and sample_ids.is_contiguous()
                                       and sample_ids.numel() >= n_samples):
        raise ValueError("dpmpp_sde_step: sample_ids must be a contiguous int64 GPU tensor of at least x.shape[0] elements")
    if x_next is None:
        x_next = torch.empty_like(x)
    if x0_out is None and want_x0:
        x0_out = torch.empty_like(x)
    check(lib.af_dpmpp_sde_step(ptr(x), ptr(e_cond), ptr(eu), ptr(xp), x.numel(), float(guidance), float(alpha_t), float(sigma_t),
                                float(c_x), float(c_d), float(w_cur), float(w_prev), ptr(x_next), ptr(x0_out), float(c_n), ptr(nz),
                                x.numel() // n_samples, ptr(sample_ids), int(first_id), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step),
                                stream_ptr()), "af_dpmpp_sde_step")
    return x_next, x0_out


def lcm_coeffs(acp_t, acp_prev, acp_s=0.0, t=0, timestep_scaling=10.0, sigma_data=0.5):
    """af_lcm_coeffs (host only, no GPU): the seven doubles (alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n) of one consistency
    step from alphas_cumprod acp_t to acp_prev (1.0: the final step, which returns the denoised sample).  acp_s <= 0: LCM, with
    the boundary condition of integer timestep t; acp_s > 0: TCD with alphas_cumprod acp_s at the intermediate timestep."""
    import ctypes
    out = (ctypes.c_double * 7)()
    check(_lib.load().af_lcm_coeffs(float(acp_t), float(acp_prev), float(acp_s), int(t), float(timestep_scaling),
                                    float(sigma_data), out), "af_lcm_coeffs")
    return tuple(float(v) for v in out)


def lcm_step(x, e_cond, e_uncond, guidance, alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n, noise=None, seed=0, step=0,
             sample_ids=None, first_id=0, x_next=None, d_out=None, want_d=True):
    """CFG combine + one LCM / TCD step (af_lcm_step), one launch; returns (x_next, D) with D = k_out x0 + k_skip x the denoised
    sample and x_next = c_x x + c_0 x0 + c_n z.  e_uncond None: no guidance.  c_n == 0: no noise is read or generated; otherwise
    noise is the z to use (x's size), or None: z is generated inside the kernel from (seed, sample id, stream 1, step, element),
    x's dim 0 being the samples (ids: sample_ids, an int64 GPU tensor, or first_id + i).  x_next / d_out: fp32 contiguous tensors
    to write into (x_next may be x itself, d_out neither), allocated when None; want_d=False with d_out None skips the D write."""
    lib = _lib.load()
    x, e_cond = _dev_f32(x), _dev_f32(e_cond)
    eu = None if e_uncond is None else _dev_f32(e_uncond)
    nz = None if noise is None else _dev_f32(noise)
    for name, t in (("e_cond", e_cond), ("e_uncond", eu), ("noise", nz)):
        if t is not None and t.numel() != x.numel():
            raise ValueError(f"lcm_step: {name} has {t.numel()} elements, x has {x.numel()}")
    for name, t in (("x_next", x_next), ("d_out", d_out)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == x.numel()):
            raise ValueError(f"lcm_step: {name} must be a contiguous fp32 GPU tensor of x's size")
    n_samples = x.shape[0] if x.dim() > 0 else 1
    if sample_ids is not None and not (sample_ids.is_cuda and sample_ids.dtype == torch.int64 and sample_ids.is_contiguous()
                                       and sample_ids.numel() >= n_samples):
        raise ValueError("lcm_step: sample_ids must be a contiguous int64 GPU tensor of at least x.shape[0] elements")
    if x_next is None:
        x_next = torch.empty_like(x)
    if d_out is None and want_d:
        d_out = torch.empty_like(x)
    check(lib.af_lcm_step(ptr(x), ptr(e_cond), ptr(eu), x.numel(), float(guidance), float(alpha_t), float(sigma_t), float(k_out),
                          float(k_skip), float(c_x), float(c_0), float(c_n), ptr(x_next), ptr(d_out), ptr(nz),
                          x.numel() // n_samples, ptr(sample_ids), int(first_id), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step),
                          stream_ptr()), "af_lcm_step")
    return x_next, d_out


def lcm_step_launches() -> int:
    """Launches of the LCM / TCD step kernel since the library was loaded (not part of plan_counts)."""
    return int(_lib.load().af_lcm_step_launches())


SAG_MAX_TOKENS = 256   # the attention-mass kernel's cap on N (csrc/af_sag.hip)


def sag_taps(sigma=1.0):
    """af_sag_taps (host only, no GPU): the nine Gaussian taps of self-attention guidance's blur, as doubles summing to 1."""
    import ctypes
    out = (ctypes.c_double * 9)()
    check(_lib.load().af_sag_taps(float(sigma), out), "af_sag_taps")
    return tuple(float(v) for v in out)


def sag_mass(q, k, heads):
    """af_op_sag_mass: the attention mass per key, fp32 [B, N] = mean over heads of the column sums of
    softmax(q k^T dh^-0.5).  q, k: [B, N, heads * dh] GPU tensors of one storage dtype (bf16, fp16 or f32), nothing converted;
    column views of a wider [B, N, ld] buffer are taken as they are (unit column stride, rows ld apart, samples N * ld apart)."""
    names = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
    if q.dtype not in names or k.dtype != q.dtype or not (q.is_cuda and k.is_cuda):
        raise ValueError(f"sag_mass: storage dtypes {q.dtype} / {k.dtype} (GPU tensors of one of bf16, fp16, f32)")
    if q.dim() != 3 or k.shape != q.shape or q.shape[2] % int(heads):
        raise ValueError(f"sag_mass: q {tuple(q.shape)} / k {tuple(k.shape)} for {heads} heads")
    B, N, Cn = (int(v) for v in q.shape)
    lds = []
    for name, t in (("q", q), ("k", k)):
        sb, sr, sc = t.stride()
        if sc != 1 or sr < Cn or (B > 1 and sb != N * sr):
            raise ValueError(f"sag_mass: {name} has strides {t.stride()}: rows must be contiguous and evenly spaced")
        lds.append(int(sr))
    out = torch.empty(B, N, device=q.device, dtype=torch.float32)
    part = torch.empty(B, int(heads), N, device=q.device, dtype=torch.float32)      # the per-head column sums (kernel scratch)
    check(_lib.load().af_op_sag_mass(DTYPES[names[q.dtype]], ptr(q), ptr(k), ptr(out), ptr(part), B, N, int(heads), Cn // int(heads),
                                     lds[0], lds[1], stream_ptr()), "af_op_sag_mass")
    return out


def sag_degrade(x, eps, mass, alpha, sigma, blur_sigma=1.0, out=None):
    """af_sag_degrade, one launch on fp32 latents [B, C, H, W]: x0 = (x - sigma eps) / alpha, its nine-tap Gaussian blur under
    reflect padding where mass [B, (H / 8)(W / 8)] > 1 (each cell an 8 x 8 block), re-noised: alpha d + sigma eps.  out: a
    contiguous fp32 GPU tensor of x's size that overlaps no input; allocated when None."""
    for name, t in (("x", x), ("eps", eps), ("mass", mass)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"sag_degrade: {name} must be a contiguous fp32 GPU tensor")
    if x.dim() != 4 or eps.shape != x.shape:
        raise ValueError(f"sag_degrade: x {tuple(x.shape)} / eps {tuple(eps.shape)} ([B, C, H, W] both)")
    B, Cn, H, W = (int(v) for v in x.shape)
    if mass.numel() != B * (H // 8) * (W // 8):
        raise ValueError(f"sag_degrade: mass has {mass.numel()} values, x needs {B} x {(H // 8) * (W // 8)}")
    if out is None:
        out = torch.empty_like(x)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape):
        raise ValueError("sag_degrade: out must be a contiguous fp32 GPU tensor of x's shape")
    check(_lib.load().af_sag_degrade(ptr(x), ptr(eps), ptr(mass), ptr(out), B, Cn, H, W, float(alpha), float(sigma), float(blur_sigma),
                                     stream_ptr()), "af_sag_degrade")
    return out


def sag_launches() -> dict:
    """Launches of the two self-attention-guidance kernels since the library was loaded (not part of plan_counts)."""
    lib = _lib.load()
    return {"mass": int(lib.af_sag_mass_launches()), "degrade": int(lib.af_sag_degrade_launches())}


RESAMPLE_MODES = {"nearest-exact": 0, "bilinear": 1, "bicubic": 2, "lanczos3": 3}   # AF_RESAMPLE_* (include/adaface_hip.h)
RESAMPLE_MAX_TAPS = 7      # AF_RESAMPLE_MAX_TAPS
RESAMPLE_TILE = (16, 64)   # the kernel's output tile, rows x columns (TH, TW of csrc/af_resample.hip)


def _resample_mode(mode):
    if mode not in RESAMPLE_MODES:
        raise ValueError(f"resample: mode {mode!r} (one of {', '.join(RESAMPLE_MODES)})")
    return RESAMPLE_MODES[mode]


def resample_taps(mode, n_in, n_out):
    """af_resample_taps (host only, no GPU): the tap table of one axis, (idx int64 [n_out, taps], w float64 [n_out, taps]);
    unused taps carry weight 0 and a valid index."""
    import ctypes
    n = max(int(n_out), 1) * RESAMPLE_MAX_TAPS
    idx, w, taps = (ctypes.c_int32 * n)(), (ctypes.c_double * n)(), ctypes.c_int()
    check(_lib.load().af_resample_taps(_resample_mode(mode), int(n_in), int(n_out), idx, w, ctypes.byref(taps)), "af_resample_taps")
    t = taps.value
    return (torch.tensor(idx[:n_out * t], dtype=torch.int64).view(n_out, t),
            torch.tensor(w[:n_out * t], dtype=torch.float64).view(n_out, t))


class _ResamplePlan:
    """An af_resample_plan: the tables of one (mode, H, W, Ho, Wo) on the current device; freed with the object."""

    def __init__(self, mode, H, W, Ho, Wo):
        self.shape = (int(H), int(W), int(Ho), int(Wo))
        self.handle = C.c_void_p()
        lib = _lib.load()
        self._destroy = lib.af_resample_plan_destroy      # (held here: module globals may be gone when the last plan is collected)
        check(lib.af_resample_plan_create(_resample_mode(mode), *self.shape, C.byref(self.handle)), "af_resample_plan_create")

    def tables(self):
        """The plan's own tables as the kernel reads them: (iy int32 [Ho, T], wy fp32 [Ho, T], ix [Wo, T], wx [Wo, T]), host."""
        _, _, Ho, Wo = self.shape
        taps = C.c_int()
        lib = _lib.load()
        check(lib.af_resample_plan_tables(self.handle, C.byref(taps), None, None, None, None), "af_resample_plan_tables")
        t = taps.value
        iy, wy = torch.empty(Ho, t, dtype=torch.int32), torch.empty(Ho, t, dtype=torch.float32)
        ix, wx = torch.empty(Wo, t, dtype=torch.int32), torch.empty(Wo, t, dtype=torch.float32)
        check(lib.af_resample_plan_tables(self.handle, C.byref(taps), ptr(iy), ptr(wy), ptr(ix), ptr(wx)), "af_resample_plan_tables")
        return iy, wy, ix, wx

    def __del__(self):
        destroy, handle = getattr(self, "_destroy", None), getattr(self, "handle", None)
        if destroy is not None and handle:
            self.handle = None
            destroy(handle)


_resample_plans = {}


def resample_plan(mode, H, W, Ho, Wo, device=None):
    """The cached plan of (mode, H, W, Ho, Wo, device); made on first use (needs the GPU: the plan owns device tables)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (mode, int(H), int(W), int(Ho), int(Wo), device.index)
    if key not in _resample_plans:
        with torch.cuda.device(device):
            _resample_plans[key] = _ResamplePlan(mode, H, W, Ho, Wo)
    return _resample_plans[key]


def resample2d(x, size, mode, out=None):
    """af_resample2d, one launch: [B, C, H, W] fp32 on the GPU -> [B, C, size[0], size[1]] under `mode` (RESAMPLE_MODES; upscaling
    only).  Any 4-byte alignment of x's and out's storage; out: a contiguous fp32 GPU tensor of the result's shape that does not
    overlap x, allocated when None."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4):
        raise ValueError("resample2d: x must be a contiguous fp32 GPU tensor [B, C, H, W]")
    B, Cn, H, W = (int(v) for v in x.shape)
    Ho, Wo = int(size[0]), int(size[1])
    plan = resample_plan(mode, H, W, Ho, Wo, x.device)
    if out is None:
        out = torch.empty(B, Cn, Ho, Wo, device=x.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, Cn, Ho, Wo)
              and out.device == x.device):
        raise ValueError(f"resample2d: out must be a contiguous fp32 GPU tensor of shape {(B, Cn, Ho, Wo)} on x's device")
    if B * Cn == 0:
        return out
    with torch.cuda.device(x.device):
        check(_lib.load().af_resample2d(plan.handle, ptr(x), ptr(out), B * Cn, stream_ptr()), "af_resample2d")
    return out


def resample2d_launches() -> int:
    """Launches of the resampling kernel since the library was loaded (not part of plan_counts)."""
    return int(_lib.load().af_resample2d_launches())


STREAM_QSAMPLE = 2    # noise.STREAM_QSAMPLE (csrc/af_philox.h), stated here because noise.py imports this module


def noise_blend(x, x0, keep, sa, s1, noise=None, seed=0, stream=STREAM_QSAMPLE, step=0, sample_ids=None, first_id=0, out=None):
    """af_noise_blend, one launch on fp32 latents [B, C, ...]: q = sa * x0 + s1 * z, then out = q * keep + (1 - keep) * x, every
    product and sum rounded on its own -- the bits of LatentDiffusion.q_sample followed by the samplers' blend line.
    keep: [B, 1 or C, ...] (1 = take the noised x0), or None: out = q, the stochastic encode (x may then be None).
    noise: the z to use (x0's size); None: z is generated inside the kernel from (seed, sample id, stream, step, element), the
    bits philox_randn gives (ids: sample_ids, an int64 GPU tensor, or first_id + i).  s1 == 0: no noise is read or generated.
    out: a contiguous fp32 GPU tensor of x0's size to write into, which may be x itself (no other overlap); allocated when None."""
    lib = _lib.load()
    x0 = _dev_f32(x0)
    if x0.dim() < 2:
        raise ValueError("noise_blend: x0 must be [B, C, ...]")
    B, Cc = x0.shape[0], x0.shape[1]
    HW = x0.numel() // max(B * Cc, 1)
    xx = None if x is None else _dev_f32(x)
    nz = None if noise is None else _dev_f32(noise)
    for name, t in (("x", xx), ("noise", nz)):
        if t is not None and t.shape != x0.shape:
            raise ValueError(f"noise_blend: {name} has shape {tuple(t.shape)}, x0 has {tuple(x0.shape)}")
    kc, kp = 1, None
    if keep is not None:
        if xx is None:
            raise ValueError("noise_blend: a keep mask needs x, the latent to blend into")
        if keep.dim() != x0.dim() or keep.shape[1] not in (1, Cc) or keep.shape[2:] != x0.shape[2:] or keep.shape[0] not in (1, B):
            raise ValueError(f"noise_blend: keep has shape {tuple(keep.shape)}; [B, 1 or C, ...] of x0's {tuple(x0.shape)} expected")
        kc = int(keep.shape[1])
        kp = _dev_f32(keep if keep.shape[0] == B else keep.expand(B, *keep.shape[1:]))
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x0.shape):
        raise ValueError("noise_blend: out must be a contiguous fp32 GPU tensor of x0's shape")
    if sample_ids is not None and not (sample_ids.is_cuda and sample_ids.dtype == torch.int64 and sample_ids.is_contiguous()
                                       and sample_ids.numel() >= B):
        raise ValueError("noise_blend: sample_ids must be a contiguous int64 GPU tensor of at least x0.shape[0] elements")
    if out is None:
        out = torch.empty_like(x0)
    check(lib.af_noise_blend(ptr(xx), ptr(x0), ptr(kp), kc, ptr(nz), B, Cc, HW, float(sa), float(s1), ptr(sample_ids),
                             int(first_id), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(step), ptr(out), stream_ptr()),
          "af_noise_blend")
    return out


def guidance(e_c, e_u, e_p, w, s, rescale=0.0, return_factor=False, out=None):
    """af_guidance: e = e_u + w (e_c - e_u) + s (e_c - e_p), then guidance rescale e (phi f + 1 - phi) with
    f = std(e_c) / std(e) per sample (dim 0 of e_c; unbiased).  e_u None: no w term; e_p None (or s = 0): no s term; rescale 0:
    no statistics.  out: a contiguous fp32 GPU tensor of e_c's size to write into, which may be e_c itself (no other overlap).
    return_factor (rescale > 0): also the applied f, [n_samples].  The sampler steps then take the result as e_cond with
    e_uncond None."""
    lib = _lib.load()
    e_c = _dev_f32(e_c)
    eu = None if e_u is None else _dev_f32(e_u)
    ep = None if e_p is None else _dev_f32(e_p)
    for name, t in (("e_u", eu), ("e_p", ep)):
        if t is not None and t.numel() != e_c.numel():
            raise ValueError(f"guidance: {name} has {t.numel()} elements, e_c has {e_c.numel()}")
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == e_c.numel()):
        raise ValueError("guidance: out must be a contiguous fp32 GPU tensor of e_c's size")
    if return_factor and not float(rescale) > 0.0:
        raise ValueError("guidance: the factor exists only with rescale > 0")
    n_samples = e_c.shape[0] if e_c.dim() > 1 else 1
    if out is None:
        out = torch.empty_like(e_c)
    factor = torch.empty(n_samples, device=e_c.device, dtype=torch.float32) if return_factor else None
    check(lib.af_guidance(ptr(e_c), ptr(eu), ptr(ep), n_samples, e_c.numel() // max(n_samples, 1), float(w), float(s),
                          float(rescale), ptr(out), ptr(factor), stream_ptr()), "af_guidance")
    return (out, factor) if return_factor else out


def lincomb(terms, cfg=False):
    """sum_i w_i * x_i over up to four (tensor, weight) pairs; cfg=True: terms = [(e_cond, g), (e_uncond, _)] ->
    e_uncond + g * (e_cond - e_uncond)."""
    lib = _lib.load()
    xs = [_dev_f32(t) for t, _ in terms]
    ws = [float(w) for _, w in terms]
    while len(xs) < 4:
        xs.append(None)
        ws.append(0.0)
    out = torch.empty_like(xs[0])
    check(lib.af_lincomb(ptr(out), out.numel(), ptr(xs[0]), ws[0], ptr(xs[1]), ws[1], ptr(xs[2]), ws[2], ptr(xs[3]), ws[3],
                         1 if cfg else 0, stream_ptr()), "af_lincomb")
    return out


def to_uint8(img):
    """clamp((img+1)/2,0,1)*255 -> uint8 HWC (stable_txt2img.py:715,764-765)."""
    lib = _lib.load()
    img = _dev_f32(img)
    B, Cn, H, W = img.shape
    if Cn != 3:
        raise ValueError("to_uint8 expects [B,3,H,W]")
    y = torch.empty(B, H, W, 3, device=img.device, dtype=torch.uint8)
    check(lib.af_to_uint8(ptr(img), ptr(y), B, H, W, stream_ptr()), "af_to_uint8")
    return y
