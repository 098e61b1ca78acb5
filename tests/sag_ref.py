"""Reference restatement of self-attention guidance for the tests, in float64 numpy, written from the paper and not from the
product code: Hong, Lee, Jang, Kim, "Improving Sample Quality of Diffusion Models Using Self-Attention Guidance" (ICCV 2023),
section 4 and Algorithm 1, with the constants of its public pipeline (kernel size 9, blur sigma 1, mask threshold 1.0).

Per sampler step at timestep t, alpha = sqrt(acp_t), sigma = sqrt(1 - acp_t):

    mass[b, j] = sum_i (1 / heads) sum_h softmax_j(q_bhi . k_bhj dh^-0.5)       the middle block's first self-attention; mean_j = 1
    mask       = mass_g > 1.0, reshaped (H / 8, W / 8), every cell an 8 x 8 block of the H x W latent, all channels
    x0         = (x - sigma e_g) / alpha                                         g = the unconditional leg under CFG, else the only leg
    blur       = 9-tap separable Gaussian of x0 per plane, w_i ~ exp(-0.5 ((i - 4) / s)^2) normalised, reflect padding of 4
    x_deg      = alpha (mask ? blur : x0) + sigma e_g
    e_d        = model(x_deg, t, the guide leg's conditioning)
    e          = e_u + w (e_c - e_u) + scale (e_u - e_d)      with CFG;      e = e_c + scale (e_c - e_d)      without
"""
import math
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import dpmpp_ref as R  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

U = 2.0 ** -24          # unit roundoff of fp32
K_BLUR = 23             # fp32 roundings on the longest path of a blurred output element (the header of degrade_kernel, af_sag.hip)
K_PLAIN = 5             # ... of an element outside the mask


# ------------------------------------------------------------------ taps, mass, mask --------------------------------
def taps(sigma=1.0):
    w = np.array([math.exp(-0.5 * ((i - 4) / sigma) ** 2) for i in range(9)], np.float64)
    return w / w.sum()


def mass(q, k, heads):
    """q, k [B, N, heads * dh] (any float array) -> float64 [B, N]."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    B, N, C = q.shape
    dh = C // heads
    qh = q.reshape(B, N, heads, dh).transpose(0, 2, 1, 3)
    kh = k.reshape(B, N, heads, dh).transpose(0, 2, 1, 3)
    s = np.einsum("bhid,bhjd->bhij", qh, kh) * dh ** -0.5
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    return p.mean(axis=1).sum(axis=1)


def mask_of(m, H, W):
    """mass [B, (H / 8)(W / 8)] -> bool [B, 1, H, W]."""
    m = np.asarray(m)
    cells = (m > 1.0).reshape(m.shape[0], 1, H // 8, W // 8)
    return np.repeat(np.repeat(cells, 8, axis=2), 8, axis=3)


# ------------------------------------------------------------------ the degraded input ------------------------------
def blur(x0, w):
    """The separable 9-tap filter of every [.., H, W] plane under reflect padding of 4 (np.pad(mode="reflect"))."""
    pad = [(0, 0)] * (x0.ndim - 2)
    p = np.pad(x0, pad + [(0, 0), (4, 4)], mode="reflect")
    h = sum(w[t] * p[..., :, t: t + x0.shape[-1]] for t in range(9))
    p = np.pad(h, pad + [(4, 4), (0, 0)], mode="reflect")
    return sum(w[t] * p[..., t: t + x0.shape[-2], :] for t in range(9))


def degrade(x, e, m, alpha, sigma, w):
    """(x_deg, bound) in float64 on copies of fp32 data, the scalars and taps AS GIVEN (pass them rounded to fp32 to model the
    kernel).  bound = ((1 + u)^k - 1) * (sum of the absolute values of the terms that form the element): k = 23 where the mask is
    on (x0 3, each pass 9, alpha d and the last sum 2), 5 where it is off; the method of lcm_ref.step_f64."""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    w = np.asarray(w, np.float64)
    H, W = x.shape[-2:]
    x0 = (x - sigma * e) / alpha
    t_x0 = (np.abs(x) + abs(sigma) * np.abs(e)) / alpha
    on = mask_of(m, H, W)
    d = np.where(on, blur(x0, w), x0)
    t_d = np.where(on, blur(t_x0, np.abs(w)), t_x0)
    out = alpha * d + sigma * e
    terms = alpha * t_d + abs(sigma) * np.abs(e)
    k = np.where(on, K_BLUR, K_PLAIN)
    return out, ((1 + U) ** k - 1) * terms


def combine(e_c, e_u, e_d, w, scale):
    if e_u is None:
        return e_c + scale * (e_c - e_d)
    return e_u + w * (e_c - e_u) + scale * (e_u - e_d)


# ------------------------------------------------------------------ the oracle's middle-block q and k ---------------
def oracle_eps_qk(sd, cfg, x, t, ctx):
    """(eps, q, k) of the CPU oracle's forward: q, k [B, N, C] of middle_block.1.transformer_blocks.0.attn1, rebuilt from the
    output of the last input block with the oracle's own layers."""
    P = O.UNET_PREFIX
    tp = {}
    eps = O.unet_forward(sd, cfg, x, t, ctx, taps=tp)
    n_in = len(O._unet_layout(cfg)[0])
    h = tp[f"input_blocks.{n_in - 1}"]
    emb = O._lin(sd, P + "time_embed.2", F.silu(O._lin(sd, P + "time_embed.0", O.timestep_embedding(t, cfg.model_channels))))
    h = O.resblock(sd, P + "middle_block.0", h, emb)
    p = P + "middle_block.1"
    B, C, Hh, Ww = h.shape
    g = O._conv(sd, p + ".proj_in", O._gn(sd, p + ".norm", h, 1e-6), pad=0)
    tok = g.permute(0, 2, 3, 1).reshape(B, Hh * Ww, C)
    n1 = O._ln(sd, p + ".transformer_blocks.0.norm1", tok)
    a = p + ".transformer_blocks.0.attn1"
    return eps, O._lin(sd, a + ".to_q", n1), O._lin(sd, a + ".to_k", n1)


def guided_eps(sd, cfg, x, t, cond, uncond, w, scale, blur_sigma, acp_t, rec=None):
    """The combined eps of one step in float64 around the oracle called in fp32; x float64 [B, C, H, W], t an integer.  rec (a
    list): the guide leg's mass of the step is appended."""
    b = x.shape[0]
    H, W = x.shape[-2:]
    tt = torch.full((b,), int(t), dtype=torch.long)
    alpha, sigma = math.sqrt(acp_t), math.sqrt(1.0 - acp_t)
    with torch.no_grad():
        if uncond is None:
            e, q, k = oracle_eps_qk(sd, cfg, x.float(), tt, cond)
            e_c, e_u, e_g = e.double(), None, e.double()
            g_ctx = cond
        else:
            e, q, k = oracle_eps_qk(sd, cfg, torch.cat([x.float()] * 2), torch.cat([tt] * 2), torch.cat([cond, uncond]))
            e_c, e_u = e.double().chunk(2)
            e_g, q, k, g_ctx = e_u, q[b:], k[b:], uncond
        m = mass(q.numpy(), k.numpy(), cfg.num_heads)
        if rec is not None:
            rec.append(m)
        x_deg, _ = degrade(x.numpy(), e_g.numpy(), m, alpha, sigma, taps(blur_sigma))
        e_d = O.unet_forward(sd, cfg, torch.from_numpy(x_deg).float(), tt, g_ctx).double()
    return combine(e_c, e_u, e_d, w, scale)


# ------------------------------------------------------------------ whole runs in float64 on the CPU ----------------
def sample_ref(kind, sd, cfg, acp, ts, x_T, cond, uncond, guidance, scale, blur_sigma=1.0):
    """kind "ddim": the eta = 0 DDIM update on the ascending timesteps ts (the last step goes to acp[0], as the reference's
    sampling parameters do); kind "dpm": DPM-Solver++(2M) with dpmpp_ref.schedule_f64's coefficients.  guidance: one value per
    step; uncond None or a guidance of 1: the single-leg form.  Returns (latent float64, [guide-leg mass of each step])."""
    img = x_T.double()
    masses = []
    ts = [int(v) for v in ts]
    n = len(ts)
    leg = lambda g: None if (uncond is None or g == 1.0) else uncond
    if kind == "ddim":
        for i in range(n):
            t = ts[n - 1 - i]
            a_t, a_p = float(acp[t]), float(acp[ts[n - 2 - i]] if i < n - 1 else acp[0])
            e = guided_eps(sd, cfg, img, t, cond, leg(guidance[i]), guidance[i], scale, blur_sigma, a_t, masses)
            x0 = (img - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
            img = math.sqrt(a_p) * x0 + math.sqrt(1.0 - a_p) * e
        return img, masses
    if kind != "dpm":
        raise ValueError(kind)
    hist = None
    for i, (t, c) in enumerate(R.schedule_f64(acp, ts)):
        e = guided_eps(sd, cfg, img, t, cond, leg(guidance[i]), guidance[i], scale, blur_sigma, float(acp[t]), masses)
        alpha_t, sigma_t, c_x, c_d, w_cur, w_prev = c[:6]
        pred = (img - sigma_t * e) / alpha_t
        d = pred if w_prev == 0.0 else w_cur * pred + w_prev * hist
        img = c_x * img + c_d * d
        hist = pred
    return img, masses
