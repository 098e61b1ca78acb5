"""Reference restatement of the seed-stable noise and of DPM-Solver++(2M) SDE for the tests, written from the papers and the
issue's contract, not from the product code:

  * Philox4x32-10: Salmon, Moraes, Dror, Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3" (SC'11), section 3.3 / table 2:
    ten rounds of  (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  the key bumped by the
    Weyl constants between rounds.  Integer arithmetic in numpy uint64.
  * keying: key = (seed lo, seed hi), counter = (g, (step << 8) | stream, id lo, id hi), element e -> group e // 4, lane e % 4.
  * bits -> normals, float64: u = ((r_even >> 9) + 0.5) 2^-23, v = (r_odd >> 8) 2^-24, rho = sqrt(-2 ln u),
    (rho cos 2 pi v, rho sin 2 pi v) for the pairs (r0, r1), (r2, r3).
  * the SDE solver (Lu et al. 2022, DPM-Solver++, the stochastic multistep form):
        x' = (sigma_s / sigma_t) e^-h x + alpha_s (1 - e^-2h) D + sigma_s sqrt(1 - e^-2h) z
    with D of the deterministic 2M solver (tests/dpmpp_ref.py), coefficients in mpmath at 50 digits.
"""
import sys
from pathlib import Path

import mpmath
import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import dpmpp_ref as R  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

U = 2.0 ** -24
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
STREAM_XT, STREAM_STEP, STREAM_QSAMPLE = 0, 1, 2
SDE_COEF_NAMES = ("alpha_t", "sigma_t", "c_x", "c_d", "c_n", "w_cur", "w_prev", "h", "r")

KNOWN_ANSWERS = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ------------------------------------------------------------------ the generator --------------------------------------
def philox4x32_10(ctr, key):
    """ctr: four arrays (or ints) of 32-bit words, key: two; broadcast against each other.  Returns four uint64 arrays of
    32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    k = [np.asarray(v, dtype=np.uint64) & MASK for v in key]
    c = list(np.broadcast_arrays(*c))
    for rnd in range(10):
        p0 = np.uint64(M0) * c[0]            # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        if rnd < 9:
            k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return c


def group_bits(seed, sample_id, stream, step, groups):
    """The [len(groups), 4] words of the groups `groups` of one sample."""
    assert 0 <= step < 1 << 24 and 0 <= stream < 256 and sample_id >= 0
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = np.asarray(groups, dtype=np.uint64)
    out = philox4x32_10((g, (step << 8) | stream, sample_id & 0xFFFFFFFF, sample_id >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=-1)


def uniforms(bits):
    """(u, v) in float64 for the pairs of a [G, 4] word array: [G, 2] each."""
    b = bits.astype(np.uint64)
    u = ((b[:, 0::2] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    v = (b[:, 1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u, v


def normals(seed, ids, stream, step, per_sample):
    """(z, rho), float64 [len(ids), per_sample]: the normals of the contract and the Box-Muller radius behind each."""
    gps = (per_sample + 3) // 4
    zs, rhos = [], []
    for sid in ids:
        u, v = uniforms(group_bits(seed, int(sid), stream, step, np.arange(gps)))
        rho = np.sqrt(-2.0 * np.log(u))
        z = np.stack([rho * np.cos(2.0 * np.pi * v), rho * np.sin(2.0 * np.pi * v)], axis=-1)   # [G, pair, (cos, sin)]
        zs.append(z.reshape(-1)[:per_sample])
        rhos.append(np.repeat(rho.reshape(-1), 2)[:per_sample])
    return np.stack(zs), np.stack(rhos)


# ------------------------------------------------------------------ coefficients ---------------------------------------
def sde_coeffs_mp(acp_t, acp_prev, h_last):
    """The nine coefficients at 50 digits from two exact doubles (h_last <= 0: first order)."""
    with mpmath.workdps(50):
        a_t, a_p = mpmath.mpf(acp_t), mpmath.mpf(acp_prev)
        alpha_t, sigma_t = mpmath.sqrt(a_t), mpmath.sqrt(1 - a_t)
        alpha_p, sigma_p = mpmath.sqrt(a_p), mpmath.sqrt(1 - a_p)
        h = mpmath.log(alpha_p / sigma_p) - mpmath.log(alpha_t / sigma_t)
        if h_last > 0:
            r = mpmath.mpf(h_last) / h
            w_cur, w_prev = 1 + 1 / (2 * r), -1 / (2 * r)
        else:
            r, w_cur, w_prev = mpmath.mpf(0), mpmath.mpf(1), mpmath.mpf(0)
        e2 = 1 - mpmath.exp(-2 * h)
        return (alpha_t, sigma_t, sigma_p / sigma_t * mpmath.exp(-h), alpha_p * e2, sigma_p * mpmath.sqrt(e2), w_cur, w_prev, h, r)


def sde_coeffs_f64(acp_t, acp_prev, h_last):
    return tuple(float(v) for v in sde_coeffs_mp(acp_t, acp_prev, h_last))


def sde_schedule_f64(acp, ts, order=2, lower_order_final=True):
    out, h_last = [], 0.0
    for t, a_t, a_p, second in R.steps(acp, ts, order, lower_order_final):
        c = sde_coeffs_f64(a_t, a_p, h_last if second else 0.0)
        out.append((t, c))
        h_last = c[7]
    return out


def ddim_sigma_eta1(a_t, a_prev):
    """DDIM's sigma at eta = 1 (Song et al. 2021, eq. 16): sqrt((1 - a_prev) / (1 - a_t)) sqrt(1 - a_t / a_prev)."""
    return np.sqrt((1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev))


# ------------------------------------------------------------------ one step in float64, with its bound ----------------
def sde_step_f64(x, e_c, e_u, x0_prev, z, rho, g, alpha_t, sigma_t, c_x, c_d, c_n, w_cur=1.0, w_prev=0.0, normal_bar=0.0,
                 extra_x0_roundings=0, extra_update_roundings=0):
    """dpmpp_ref.step_f64 with the noise term: x' = c_x x + c_d D + c_n z on float64 copies, scalars as given.  Returns
    (x_next, x0, bound_x_next, bound_x0).  Roundings on x_next's longest path, counted from dpmpp_sde_step_kernel
    (af_philox.hip) as if nothing were fused: D's count (dpmpp_ref.step_f64), c_d D (1), + c_x x (1), + c_n z (1): D + 3.
    The device's z differs from the float64 z by at most normal_bar * max(rho, 2^-10): that times |c_n| is added; the product
    c_n z and its add are covered by the term |c_n z| in the sum of terms."""
    x, e_c, z = np.asarray(x, np.float64), np.asarray(e_c, np.float64), np.asarray(z, np.float64)
    k = extra_x0_roundings
    if e_u is None:
        e, t_e = e_c, np.abs(e_c)
    else:
        e_u = np.asarray(e_u, np.float64)
        e = e_u + g * (e_c - e_u)
        t_e = np.abs(e_u) + abs(g) * (np.abs(e_c) + np.abs(e_u))
        k += 3
    x0 = (x - sigma_t * e) / alpha_t
    t_x0 = (np.abs(x) + sigma_t * t_e) / alpha_t
    k_x0 = k + 3
    if x0_prev is None:
        d, t_d, k_d = x0, t_x0, k_x0
    else:
        x0_prev = np.asarray(x0_prev, np.float64)
        d = w_cur * x0 + w_prev * x0_prev
        t_d = abs(w_cur) * t_x0 + abs(w_prev) * np.abs(x0_prev)
        k_d = k_x0 + 2
    x_next = c_x * x + c_d * d + c_n * z
    t_xn = abs(c_x) * np.abs(x) + abs(c_d) * t_d + abs(c_n) * np.abs(z)
    k_xn = k_d + 3 + extra_update_roundings
    bound = ((1 + U) ** k_xn - 1) * t_xn + abs(c_n) * normal_bar * np.maximum(np.asarray(rho, np.float64), 2.0 ** -10)
    return x_next, x0, bound, ((1 + U) ** k_x0 - 1) * t_x0


# ------------------------------------------------------------------ a whole run in float64 on the CPU -------------------
def sde_sample_ref(apply_model, acp, ts, x_T, cond, uncond, guidance, seed, ids, order=2, lower_order_final=True, mask=None,
                   x0=None, temperature=1.0):
    """The SDE sampler loop in float64 around a model called in fp32 (the oracle's UNet), with the reference normals: step
    noise from stream 1 and the blend's q_sample noise from stream 2, both at step = the loop index; x_T None: stream 0, step 0.
    One model call on cat[x, x] with cat[cond, uncond] (cond first), e = e_u + g (e_c - e_u).  Returns (latent, timesteps)."""
    shape = tuple(x_T.shape) if x_T is not None else None
    per = int(np.prod(shape[1:]))
    draw = lambda stream, step: torch.tensor(normals(seed, ids, stream, step, per)[0]).reshape(shape)
    img = x_T.double()
    b = shape[0]
    hist, called = None, []
    for i, (t, c) in enumerate(sde_schedule_f64(acp, ts, order, lower_order_final)):
        tt = torch.full((b,), t, dtype=torch.long)
        called.append(t)
        if mask is not None:
            noisy = np.sqrt(acp[t]) * x0.double() + np.sqrt(1.0 - acp[t]) * draw(STREAM_QSAMPLE, i)
            img = noisy * mask.double() + (1.0 - mask.double()) * img
        e_c, e_u = apply_model(torch.cat([img.float()] * 2), torch.cat([tt] * 2), torch.cat([cond, uncond])).double().chunk(2)
        e = e_u + guidance[i] * (e_c - e_u)
        alpha_t, sigma_t, c_x, c_d, c_n, w_cur, w_prev = c[:7]
        pred = (img - sigma_t * e) / alpha_t
        d = pred if w_prev == 0.0 else w_cur * pred + w_prev * hist
        img = c_x * img + c_d * d + c_n * temperature * draw(STREAM_STEP, i)
        hist = pred
    return img, called
