"""Reference restatement of LCM / TCD few-step sampling for the tests, in float64 numpy, written from the papers and not from
the product code:

  * Luo, Tan, Huang, Li, Zhao, "Latent Consistency Models" (2023), Algorithm 3 (multistep latent consistency sampling), with the
    boundary condition of Song, Dhariwal, Chen, Sutskever, "Consistency Models" (ICML 2023), section 3:
        x0 = (x - sigma_t eps) / alpha_t,   tau = t * timestep_scaling,
        f(x, t) = c_skip x + c_out x0,  c_skip = sd^2 / (tau^2 + sd^2),  c_out = tau / sqrt(tau^2 + sd^2)
        x_prev = sqrt(acp_prev) f + sqrt(1 - acp_prev) z;   the last step returns f.
    The grid: the distillation's k = T // original_steps spaced timesteps (i + 1) k - 1, descending, thinned to the S entries at
    floor(linspace(0, original_steps, S, endpoint=False)).
  * Zheng, Ma, Peng, Chen, Fu, "Trajectory Consistency Distillation" (2024), Algorithm 4 (strategic stochastic sampling):
        s = floor((1 - gamma) t_prev),   x_s = sqrt(acp_s) x0 + sqrt(1 - acp_s) eps           (the deterministic move to s)
        x_prev = sqrt(acp_prev / acp_s) x_s + sqrt(1 - acp_prev / acp_s) z;   the last step returns x0.
  * the guidance-scale embedding of the LCM authors' code (w_embedding): the sinusoid of (w - 1) 1000 with frequencies
    exp(-ln(10000) i / (half - 1)), laid out [sin | cos].

THE IDENTITIES the coefficient tests check, with x' = c_x x + c_0 x0 + c_n z and x = alpha x0* + sigma e*:
  TCD, not the last step:  c_x alpha + c_0 = sqrt(acp_prev)               (an exact x0 prediction is carried to the next level)
                           (c_x sigma)^2 + c_n^2 = 1 - acp_prev           (and so is the marginal variance)
  LCM, not the last step:  c_n^2 = 1 - acp_prev                           (the re-noising is q(x_prev | D) exactly)
                           c_x = sqrt(acp_prev) k_skip,  c_0 = sqrt(acp_prev) k_out,  k_skip + k_out^2 = 1
                                                                          (the boundary condition's own identity)
  last step, both:         (c_x, c_0, c_n) = (k_skip, k_out, 0).
"""
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import philox_ref as P  # noqa: E402

U = 2.0 ** -24          # unit roundoff of fp32
COEF_NAMES = ("alpha_t", "sigma_t", "k_out", "k_skip", "c_x", "c_0", "c_n")
GRIDS = {4: [999, 759, 499, 259], 8: [999, 879, 759, 639, 499, 379, 259, 139], 2: [999, 499], 1: [999]}


# ------------------------------------------------------------------ grid -------------------------------------------
def grid(S, original_steps=50, T=1000):
    """The S timesteps, DESCENDING (the order they are taken in)."""
    k = T // original_steps
    origin = [(i + 1) * k - 1 for i in range(original_steps)][::-1]
    return [origin[int(math.floor(j * original_steps / S))] for j in range(S)]


def steps(acp, ts_desc, gamma=None):
    """[(t, acp_t, acp_prev, acp_s or None, s or None)] in the order the steps are taken; the last one has acp_prev = 1 (and, for
    TCD, acp_s = 1): it returns the denoised sample."""
    out = []
    n = len(ts_desc)
    for i, t in enumerate(ts_desc):
        final = i == n - 1
        t_prev = 0 if final else int(ts_desc[i + 1])
        a_prev = 1.0 if final else float(acp[t_prev])
        if gamma is None:
            out.append((int(t), float(acp[t]), a_prev, None, None))
        else:
            s = int(math.floor((1.0 - gamma) * t_prev))
            out.append((int(t), float(acp[t]), a_prev, 1.0 if final else float(acp[s]), s))
    return out


# ------------------------------------------------------------------ one step, as the papers write it ---------------
def _step_from_x0(x, x0, eps, z, acp_t, acp_prev, acp_s, t, timestep_scaling, sigma_data):
    """(x_prev, denoised) from the predicted x0 on: every line as in the algorithms above; acp_s None: LCM."""
    if acp_s is None:
        tau = t * timestep_scaling
        c_skip = sigma_data ** 2 / (tau ** 2 + sigma_data ** 2)
        c_out = tau / math.sqrt(tau ** 2 + sigma_data ** 2)
        den = c_skip * x + c_out * x0
        if acp_prev == 1.0:
            return den, den
        return math.sqrt(acp_prev) * den + math.sqrt(1.0 - acp_prev) * z, den
    den = x0
    if acp_prev == 1.0:
        return den, den
    x_s = math.sqrt(acp_s) * x0 + math.sqrt(1.0 - acp_s) * eps
    ratio = acp_prev / acp_s
    return math.sqrt(ratio) * x_s + math.sqrt(1.0 - ratio) * z, den


def step_direct(x, eps, z, acp_t, acp_prev, acp_s, t, timestep_scaling=10.0, sigma_data=0.5):
    """(x_prev, denoised) of one step from the model's eps; acp_s None: LCM.  acp_prev == 1: the last step."""
    alpha, sigma = math.sqrt(acp_t), math.sqrt(1.0 - acp_t)
    x0 = (x - sigma * eps) / alpha
    return _step_from_x0(x, x0, eps, z, acp_t, acp_prev, acp_s, t, timestep_scaling, sigma_data)


def coeffs_f64(acp_t, acp_prev, acp_s, t, timestep_scaling=10.0, sigma_data=0.5):
    """(alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n) read off the step, which is linear in (x, x0, z) once eps is written as
    (x - alpha x0) / sigma: the coefficient of a variable is the step's value with that variable 1 and the others 0 (x0 handed
    over as given, so that no cancellation enters)."""
    alpha, sigma = math.sqrt(acp_t), math.sqrt(1.0 - acp_t)
    at = lambda x, x0, z: _step_from_x0(x, x0, (x - alpha * x0) / sigma, z, acp_t, acp_prev, acp_s, t, timestep_scaling, sigma_data)
    (c_x, k_skip), (c_0, k_out), (c_n, _) = at(1.0, 0.0, 0.0), at(0.0, 1.0, 0.0), at(0.0, 0.0, 1.0)
    return (alpha, sigma, k_out, k_skip, c_x, c_0, c_n)


def schedule_f64(acp, ts_desc, gamma=None):
    """[(t, coefficients)] of a whole run."""
    return [(t, coeffs_f64(a_t, a_p, a_s, t)) for t, a_t, a_p, a_s, _ in steps(acp, ts_desc, gamma)]


# ------------------------------------------------------------------ the guidance-scale embedding -------------------
def w_embedding(w, dim):
    """[dim] float64: [sin((w - 1) 1000 f_i) | cos(...)], f_i = exp(-ln(10000) i / (half - 1)), zero-padded to an odd dim."""
    half = dim // 2
    out = np.zeros(dim)
    for i in range(half):
        a = (w - 1.0) * 1000.0 * math.exp(-math.log(10000.0) * i / (half - 1))
        out[i], out[half + i] = math.sin(a), math.cos(a)
    return out


# ------------------------------------------------------------------ one step in float64, with its fp32 rounding bound
def step_f64(x, e_c, e_u, z, rho, g, alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n, normal_bar=0.0):
    """One step on float64 copies of fp32 data with the scalars AS GIVEN (pass them already rounded to fp32 to model the kernel).
    Returns (x_next, d, bound_x_next, bound_d): bound = ((1 + u)^k - 1) * (sum of the absolute values of the terms that form the
    output), k the number of fp32 roundings on the output's longest path as lcm_step_kernel's header (af_lcm.hip) counts them:

        e = e_u + g (e_c - e_u)      sub, mul, add            3     (no e_u: e = e_c, 0)
        x0 = (x - sigma_t e) / alpha mul, sub, division      +3  => x0: 6 with guidance, 3 without
        D = k_out x0 + k_skip x      mul, add                +2  => d_out: 8 / 5
        x' = c_0 x0 + c_x x + c_n z  mul, add, add           +3  => x_next: 9 / 6;  c_n == 0: mul, add, +2 => 8 / 5

    (a fused multiply-add rounds once where this counts two, so contraction only helps).  z None (c_n == 0): no noise term.  The
    device's z differs from the float64 z by at most normal_bar * max(rho, 2^-10): that times |c_n| is added, as
    philox_ref.sde_step_f64 does."""
    x, e_c = np.asarray(x, np.float64), np.asarray(e_c, np.float64)
    if e_u is None:
        e, t_e, k = e_c, np.abs(e_c), 0
    else:
        e_u = np.asarray(e_u, np.float64)
        e = e_u + g * (e_c - e_u)
        t_e = np.abs(e_u) + abs(g) * (np.abs(e_c) + np.abs(e_u))
        k = 3
    x0 = (x - sigma_t * e) / alpha_t
    t_x0 = (np.abs(x) + sigma_t * t_e) / alpha_t
    k_x0 = k + 3
    d = k_out * x0 + k_skip * x
    t_d = abs(k_out) * t_x0 + abs(k_skip) * np.abs(x)
    x_next = c_x * x + c_0 * x0
    t_xn = abs(c_x) * np.abs(x) + abs(c_0) * t_x0
    k_xn = k_x0 + 2
    extra = 0.0
    if c_n != 0.0:
        z = np.asarray(z, np.float64)
        x_next = x_next + c_n * z
        t_xn = t_xn + abs(c_n) * np.abs(z)
        k_xn += 1
        if normal_bar > 0.0:      # (a z handed in as fp32 data carries no error of its own, and needs no rho)
            extra = abs(c_n) * normal_bar * np.maximum(np.asarray(rho, np.float64), 2.0 ** -10)
    return x_next, d, ((1 + U) ** k_xn - 1) * t_xn + extra, ((1 + U) ** (k_x0 + 2) - 1) * t_d


# ------------------------------------------------------------------ a whole run in float64 on the CPU ---------------
def sample_ref(apply_model, acp, ts_desc, x_T, cond, uncond, guidance, seed, ids, gamma=None, temperature=1.0):
    """The sampler loop in float64 around a model called in fp32 (the oracle's UNet), written with step_direct and the reference
    normals of tests/philox_ref.py (stream 1, step = the loop index).  One model call on cat[x, x] with cat[cond, uncond] (cond
    first), e = e_u + g (e_c - e_u); uncond None: one call, no guidance.  Returns (latent, [denoised of each step], timesteps)."""
    shape = tuple(x_T.shape)
    per = int(np.prod(shape[1:]))
    b = shape[0]
    img = x_T.double()
    dens, called = [], []
    for i, (t, a_t, a_p, a_s, _) in enumerate(steps(acp, ts_desc, gamma)):
        tt = torch.full((b,), t, dtype=torch.long)
        called.append(t)
        if uncond is None:
            e = apply_model(img.float(), tt, cond).double()
        else:
            e_c, e_u = apply_model(torch.cat([img.float()] * 2), torch.cat([tt] * 2), torch.cat([cond, uncond])).double().chunk(2)
            e = e_u + guidance[i] * (e_c - e_u)
        z = temperature * torch.tensor(P.normals(seed, ids, P.STREAM_STEP, i, per)[0]).reshape(shape)
        img, den = step_direct(img, e, z, a_t, a_p, a_s, t)
        dens.append(den)
    return img, dens, called
