"""GPU tests of the DPM-Solver++(2M) sampler: af_dpmpp_step element by element against float64 with a counted rounding bound,
its first-order form against af_ddim_step, a closed form for a constant data prediction, and DPMSolverSampler on the tiny model
against the restatement of tests/dpmpp_ref.py driving the CPU oracle, against DDIMSampler at order 1, in the throughput modes
and twice for determinism."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import dpmpp_ref as R  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ROOT / "tests" / "golden"
SENTINEL = -12345.5
PAD = 8                                    # guard floats in front of and behind every output (32 bytes: keeps 16-byte alignment)
f32 = lambda v: float(np.float32(v))


# ======================================================================================================================
# kernel
# ======================================================================================================================
@pytest.fixture(scope="module")
def coef_sets():
    """Three steps' coefficients from af_dpmpp_coeffs, rounded to fp32 as the sampler hands them over: the smallest-h and the
    largest-h step of the S = 20 uniform-t grid and a middle step of the S = 10 logSNR grid, second-order weights from the h
    of the step before (the step after for a grid's first step)."""
    from adaface_amd import ops
    acp = R.sd_acp()
    out = []
    for ts, pick in ((R.uniform_grid(20), "min"), (R.uniform_grid(20), "max"), (R.logsnr_grid(acp, 10), 4)):
        st = R.steps(acp, ts)
        hs = [ops.dpmpp_coeffs(a_t, a_p, 0.0)[6] for _, a_t, a_p, _ in st]
        i = int(np.argmin(hs)) if pick == "min" else int(np.argmax(hs)) if pick == "max" else pick
        _, a_t, a_p, _ = st[i]
        c = ops.dpmpp_coeffs(a_t, a_p, hs[i - 1] if i > 0 else hs[i + 1])
        assert c[5] != 0.0 and c[6] == hs[i]
        out.append(tuple(f32(v) for v in c[:6]))
    assert out[0] != out[1]
    return out


def _guarded(n, gpu, offset=0):
    """an n-element fp32 view with PAD sentinel floats on either side, `offset` floats off 16-byte alignment"""
    buf = torch.full((n + 2 * PAD + offset,), SENTINEL, device=gpu, dtype=torch.float32)
    return buf, buf[PAD + offset: PAD + offset + n]


def _inputs(n, seed, gpu, offset=0):
    g = torch.Generator().manual_seed(seed)
    host = [torch.randn(n + offset, generator=g) for _ in range(4)]       # x, e_c, e_u, x0_prev
    dev = [h.to(gpu)[offset:] for h in host]
    for d in dev:
        assert d.data_ptr() % 16 == (4 * offset) % 16
    return [h[offset:].numpy() for h in host], dev


def _run_case(gpu, n, coef, cfg, ms, want_x0, offset=0, alias=False, seed=0):
    from adaface_amd import ops
    (x, ec, eu, xp), (dx, dec, deu, dxp) = _inputs(n, seed, gpu, offset)
    g = 7.5
    alpha_t, sigma_t, c_x, c_d, w_cur, w_prev = coef
    ref_xn, ref_x0, b_xn, b_x0 = R.step_f64(x, ec, eu if cfg else None, xp if ms else None, g, alpha_t, sigma_t, c_x, c_d,
                                            w_cur, w_prev)
    if alias:
        xbuf, dx_view = _guarded(n, gpu, offset)
        dx_view.copy_(dx)
        dx, nbuf, nview = dx_view, xbuf, dx_view
    else:
        nbuf, nview = _guarded(n, gpu, offset)
    hbuf, hview = _guarded(n, gpu, offset) if want_x0 else (None, None)
    got_xn, got_x0 = ops.dpmpp_step(dx, dec, deu if cfg else None, dxp if ms else None, g, alpha_t, sigma_t, c_x, c_d, w_cur,
                                    w_prev, x_next=nview, x0_out=hview, want_x0=want_x0)
    torch.cuda.synchronize()
    assert got_xn.data_ptr() == nview.data_ptr() and (got_x0 is None) == (not want_x0)
    tag = (n, cfg, ms, want_x0, offset, alias)
    worst = 0.0
    for buf, ref, bound in ((nbuf, ref_xn, b_xn), (hbuf, ref_x0, b_x0)):
        if buf is None:
            continue
        host = buf.cpu().numpy().astype(np.float64)
        lo = PAD + offset
        assert (host[:lo] == SENTINEL).all() and (host[lo + n:] == SENTINEL).all(), ("wrote outside [0, n)", tag)
        err = np.abs(host[lo: lo + n] - ref)
        assert (err <= bound).all(), (tag, float((err / bound).max()), int(np.argmax(err / bound)))
        worst = max(worst, float((err / bound).max()))
    return worst


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 2 * 4 * 8 * 8, 8 * 4 * 64 * 64 + 3])
def test_step_kernel_against_float64(gpu, report, coef_sets, n):
    """Every element of x_next and x0_out within k 2^-24 (sum of |terms|), k counted from the kernel source (dpmpp_ref.step_f64:
    10 / 8 / 7 / 5 roundings for x_next with guidance + history / guidance / history / neither, 6 / 3 for x0_out); nothing
    outside [0, n) written.  {guidance} x {history} x {x0_out wanted}, the three coefficient sets in turn."""
    worst, k = 0.0, 0
    for cfg in (True, False):
        for ms in (True, False):
            for want_x0 in (True, False):
                worst = max(worst, _run_case(gpu, n, coef_sets[k % 3], cfg, ms, want_x0, seed=n + k))
                k += 1
    report(f"af_dpmpp_step n={n}: worst |err| / bound over 8 argument forms", worst, 1.0, 1.0)


@pytest.mark.parametrize("n", [5, 257, 2 * 4 * 8 * 8])
def test_step_kernel_unaligned_views_and_in_place(gpu, report, coef_sets, n):
    """Every view one float off 16-byte alignment (the scalar path), and x_next aliasing x (aligned: the 16-byte path, where
    a lane's four loads precede its stores)."""
    w1 = max(_run_case(gpu, n, coef_sets[i % 3], True, True, True, offset=1, seed=50 + i) for i in range(3))
    w2 = max(_run_case(gpu, n, coef_sets[i % 3], i != 1, i != 2, True, alias=True, seed=60 + i) for i in range(3))
    w3 = _run_case(gpu, n, coef_sets[0], True, True, True, offset=1, alias=True, seed=70)
    report(f"af_dpmpp_step n={n}: unaligned views / in place, worst |err| / bound", max(w1, w2, w3), 1.0, 1.0)


def test_step_refuses_history_aliases_on_the_device(gpu):
    """x0_out that is x0_prev, x or x_next is refused on the host with a message; so is a history of another size."""
    from adaface_amd import _lib, ops
    x, e, h, out = (torch.randn(64, device=gpu) for _ in range(4))
    step = lambda **kw: ops.dpmpp_step(x, e, None, kw.pop("x0_prev", h), 1.0, 0.8, 0.6, 0.9, 0.1, 1.5, -0.5, **kw)
    for kw in (dict(x0_out=h), dict(x0_out=x), dict(x_next=out, x0_out=out)):
        with pytest.raises(_lib.AfError, match="alias"):
            step(**kw)
    with pytest.raises(ValueError):
        step(x0_prev=h[:32])
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["min_h", "max_h", "last"])
def test_first_order_step_equals_ddim_step(gpu, report, which):
    """Order 1 is DDIM with eta = 0: af_dpmpp_step (no history) against af_ddim_step on the same inputs and the same fp32
    (a_t, a_prev).  The two evaluate different but equal formulas, so not bit-equal: each stays within its own rounding bound
    of the common exact value.  af_dpmpp_step: its 8 / 6 roundings plus the fp32 roundings of the scalars it is handed
    (sigma_t, alpha_t on x0's path, c_d on the way to x_next); af_ddim_step: 10 / 7 (dpmpp_ref.ddim_step_f64) plus the one of
    sqrt(1 - a_t), which it is handed."""
    from adaface_amd import ops
    acp = R.sd_acp()
    st = R.steps(acp, R.uniform_grid(20))
    hs = [R.coeffs_f64(a_t, a_p, 0.0)[6] for _, a_t, a_p, _ in st]
    i = {"min_h": int(np.argmin(hs)), "max_h": int(np.argmax(hs)), "last": len(st) - 1}[which]
    a_t, a_prev = st[i][1], st[i][2]                     # fp32 values already (the model's table)
    assert f32(a_t) == a_t and f32(a_prev) == a_prev
    s1m = f32(np.sqrt(1.0 - a_t))
    c64 = ops.dpmpp_coeffs(a_t, a_prev, 0.0)
    c32 = [f32(v) for v in c64[:4]]
    n, g = 8 * 4 * 16 * 16 + 1, 7.5
    (x, ec, eu, _), (dx, dec, deu, _) = _inputs(n, 17, gpu)
    worst = 0.0
    for cfg in (True, False):
        xn, x0 = ops.dpmpp_step(dx, dec, deu if cfg else None, None, g, *c32)
        xp, p0 = ops.ddim_step(dx, dec, deu if cfg else None, g, a_t, a_prev, s1m)
        ref_xn, ref_x0, b_xn, b_x0 = R.step_f64(x, ec, eu if cfg else None, None, g, *c64[:4], extra_x0_roundings=2,
                                                extra_update_roundings=1)
        ref_xp, ref_p0, t_xp, t_p0, k_xp, k_p0 = R.ddim_step_f64(x, ec, eu if cfg else None, g, a_t, a_prev, np.sqrt(1.0 - a_t))
        # the identity itself, in float64 (the e coefficient sigma_prev - alpha_prev sigma_t / alpha_t cancels a digit or two)
        assert (np.abs(ref_xn - ref_xp) <= 1e-13 * t_xp).all() and (np.abs(ref_x0 - ref_p0) <= 1e-13 * t_p0).all()
        d_xp, d_p0 = ((1 + R.U) ** (k_xp + 1) - 1) * t_xp, ((1 + R.U) ** (k_p0 + 1) - 1) * t_p0
        for got, other, bound in ((xn, xp, b_xn + d_xp), (x0, p0, b_x0 + d_p0)):
            err = (got.double() - other.double()).abs().cpu().numpy()
            assert (err <= bound).all(), (which, cfg, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    report(f"af_dpmpp_step order 1 vs af_ddim_step ({which} of S=20): worst |diff| / bound", worst, 1.0, 1.0)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("split", [False, True])
def test_constant_data_prediction_is_integrated_exactly(gpu, report, order, split):
    """If the model's data prediction is the same tensor c at every step, every order of the solver is exact: after the last
    step x = alpha_end c + (sigma_end / sigma_start) (x_start - alpha_start c), whatever the grid (w_cur + w_prev = 1 and the
    c_x telescope).  Seven steps over the explicit non-uniform grid [1, 40, 200, 333, 600, 800, 981]; eps = (x - alpha_t c) /
    sigma_t is formed in float64 from the kernel's own x and rounded to fp32, with guidance as e_c = e + d, e_u = e + g d /
    (g - 1), for which e_u + g (e_c - e_u) = e.  The closed form needs no restatement of the solver.
    Bound: E_{i+1} = c_x E_i + b_i over the seven steps (the data prediction does not depend on x, so an error carried in x
    is only multiplied by c_x < 1; the total is below the sum of the seven b_i), b_i the per-step bound of
    test_step_kernel_against_float64, where a step's bound counts three more roundings on x0's path (the rounding of eps
    and of the scalars sigma_t, alpha_t, against the closed form's exact ones), one more for c_d, and at order 2
    |c_d w_prev| times the previous step's x0 bound, for the history it reads."""
    from adaface_amd import ops
    from adaface_amd.ldm.models.diffusion import dpm_solver as D
    acp = R.sd_acp()
    ts = np.asarray([1, 40, 200, 333, 600, 800, 981])
    tab = D.dpmpp_schedule(acp, ts, order=order, lower_order_final=False)
    n, g = 2 * 4 * 8 * 8 + 3, 7.5
    rng = np.random.default_rng(5)
    c = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    delta = rng.standard_normal(n)
    x = torch.randn(n, generator=torch.Generator().manual_seed(6)).to(gpu)
    x_start = x.cpu().numpy().astype(np.float64)
    hist = [torch.empty(n, device=gpu) for _ in range(2)]
    total, b_x0_prev, x0_prev = np.zeros(n), np.zeros(n), None
    for i, row in enumerate(tab):
        alpha_t, sigma_t, c_x, c_d, w_cur, w_prev = row[D.COL_ALPHA: D.COL_WPREV + 1]
        xh = x.cpu().numpy().astype(np.float64)
        e = (xh - alpha_t * c) / sigma_t
        e_c, e_u = (e + delta, e + g * delta / (g - 1.0)) if split else (e, None)
        e_c32 = e_c.astype(np.float32)
        e_u32 = None if e_u is None else e_u.astype(np.float32)
        second = w_prev != 0.0
        assert second == (order == 2 and i > 0)
        c32 = [f32(v) for v in (alpha_t, sigma_t, c_x, c_d, w_cur, w_prev)]
        _, _, b_xn, b_x0 = R.step_f64(xh, e_c32, e_u32, x0_prev.cpu().numpy() if second else None, g, *c32,
                                      extra_x0_roundings=3, extra_update_roundings=1)
        total = c32[2] * total + b_xn + (abs(c32[3] * c32[5]) * b_x0_prev if second else 0.0)
        b_x0_prev = b_x0
        x, x0_prev = ops.dpmpp_step(x, torch.tensor(e_c32, device=gpu), None if e_u32 is None else torch.tensor(e_u32, device=gpu),
                                    x0_prev if second else None, g, *c32, x_next=x, x0_out=hist[i % 2])
    a_end, a_start = acp[0], acp[981]
    want = np.sqrt(a_end) * c + np.sqrt((1.0 - a_end) / (1.0 - a_start)) * (x_start - np.sqrt(a_start) * c)
    err = np.abs(x.cpu().numpy().astype(np.float64) - want)
    report(f"DPM-Solver++ order {order}{' CFG split' if split else ''}: constant x0 over 7 steps, worst |err| / bound",
           float((err / total).max()), 1.0, 1.0)
    assert (err <= total).all(), (float((err / total).max()), float(err.max()))
    assert float(np.abs(x0_prev.cpu().numpy() - c).max()) < 1e-3     # the history holds c itself


# ======================================================================================================================
# sampler, tiny model
# ======================================================================================================================
@pytest.fixture(scope="module")
def tiny_model(gpu):
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    model = instantiate_from_config(tiny_config()["model"]).eval()
    sd = O.synth_state_dict(O.unet_param_shapes(O.TINY_UNET), seed=11)
    sd.update(O.synth_state_dict(O.vae_param_shapes(O.TINY_VAE), seed=12))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected
    return model.to(gpu).set_compute_dtype("f32")


@pytest.fixture(scope="module")
def tiny_inputs():
    g = dict(np.load(GOLD / "golden_tiny.npz"))
    gen = torch.Generator().manual_seed(21)
    return dict(x_T=torch.tensor(g["ddim_xT"]), c=torch.tensor(g["ddim_c"]), uc=torch.tensor(g["ddim_uc"]),
                mask=torch.tensor(g["inpaint_mask"]), x0=torch.tensor(g["inpaint_x0"]),
                q_noise=[torch.randn(g["ddim_xT"].shape, generator=gen) for _ in range(10)])


@pytest.fixture(scope="module")
def oracle_runs(tiny_inputs):
    """The restatement driving the CPU oracle's UNet, computed once: S = 6 on the uniform-t grid (7 steps) with the inpainting
    blend, S = 10 on the logSNR grid; annealed guidance [10, 4], second order, lower_order_final."""
    cfg = O.TINY_UNET
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=11)
    apply = lambda x, t, c: O.unet_forward(sd, cfg, x, t, c)
    acp = R.sd_acp()
    i = tiny_inputs
    out = {}
    for name, ts, inpaint in (("uniform6", R.uniform_grid(6), True), ("logsnr10", R.logsnr_grid(acp, 10), False)):
        gs = O.guidance_schedule((10.0, 4.0), len(ts))
        kw = dict(mask=i["mask"], x0=i["x0"], q_noise=i["q_noise"]) if inpaint else {}
        with torch.no_grad():
            lat, called = R.sample_ref(apply, acp, ts, i["x_T"], i["c"], i["uc"], gs, **kw)
        out[name] = (lat.numpy(), called, len(ts))
    return out


def _conds(model, inputs, gpu):
    return (model.get_learned_conditioning(inputs["c"].to(gpu)), model.get_learned_conditioning(inputs["uc"].to(gpu)))


@pytest.mark.parametrize("case", ["uniform6", "logsnr10"])
def test_sampler_matches_restatement_on_the_oracle(gpu, report, tiny_model, tiny_inputs, oracle_runs, case):
    """DPMSolverSampler.sample in f32 mode (annealed guidance [10, 4], cond / uncond pair, fixed x_T; uniform6 also mask / x0
    with the q_sample noise replayed) against dpmpp_ref.sample_ref on the CPU oracle: 1e-3 of max|ref|, the drop-in sampler bar
    (DDIM measures 3.9e-6 there, PLMS 1.5e-6)."""
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    ref, ref_calls, n = oracle_runs[case]
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    S, skip = (6, "time_uniform") if case == "uniform6" else (10, "logSNR")
    kw, q_calls = {}, []
    if case == "uniform6":
        noises = [t.to(gpu) for t in tiny_inputs["q_noise"]]
        orig = tiny_model.q_sample

        def q_sample(x_start, t, noise=None):
            q_calls.append(int(t[0].item()))
            return orig(x_start, t, noise=noises[len(q_calls) - 1])
        object.__setattr__(tiny_model, "q_sample", q_sample)
        kw = dict(mask=tiny_inputs["mask"].to(gpu), x0=tiny_inputs["x0"].to(gpu))
    steps_seen, x0_seen = [], []
    try:
        lat, inter = DPMSolverSampler(tiny_model).sample(
            S=S, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=[10.0, 4.0],
            unconditional_conditioning=uc, x_T=tiny_inputs["x_T"].to(gpu), skip_type=skip, callback=steps_seen.append,
            img_callback=lambda p, i: x0_seen.append(p.data_ptr()), eta=0.0, **kw)
    finally:
        if case == "uniform6":
            object.__delattr__(tiny_model, "q_sample")
    err = np.abs(lat.cpu().numpy() - ref).max() / np.abs(ref).max()
    report(f"dropin DPMSolverSampler {case} ({n} steps) vs restatement on the oracle [f32]", err, float(np.abs(ref).max()), 1e-3)
    assert err < 1e-3, err
    assert steps_seen == list(range(n)) and len(inter["x_inter"]) >= 2 and len(inter["x_inter"]) == len(inter["pred_x0"])
    assert len(set(x0_seen)) == 2 and x0_seen[0] == x0_seen[2] != x0_seen[1]      # two history buffers, ping-ponged
    if case == "uniform6":
        assert n == 7 and q_calls == ref_calls == [997, 831, 665, 499, 333, 167, 1]


def test_order1_equals_ddim_sampler(gpu, report, tiny_model, tiny_inputs):
    """order = 1 against DDIMSampler (eta 0, same x_T, contexts and guidance) in f32 mode: 1e-3 of max|ref|, and the UNet sees
    the same timesteps in the same order."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    x_T = tiny_inputs["x_T"].to(gpu)
    seen = []
    twin, plain = tiny_model.apply_model_cfg_twin, tiny_model.apply_model

    def rec_twin(x, t, cond):
        seen.append(("twin", t.tolist()))
        return twin(x, t, cond)

    def rec_plain(x, t, cond):
        seen.append(("plain", t.tolist()))
        return plain(x, t, cond)
    object.__setattr__(tiny_model, "apply_model_cfg_twin", rec_twin)
    object.__setattr__(tiny_model, "apply_model", rec_plain)
    try:
        kw = dict(S=6, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=[4.0, 1.0],
                  unconditional_conditioning=uc, x_T=x_T, eta=0.0)
        a, _ = DDIMSampler(tiny_model).sample(**kw)
        calls_ddim, seen = seen, []
        b, _ = DPMSolverSampler(tiny_model).sample(order=1, **kw)
        calls_dpm = seen
    finally:
        object.__delattr__(tiny_model, "apply_model_cfg_twin")
        object.__delattr__(tiny_model, "apply_model")
    assert calls_dpm == calls_ddim and len(calls_ddim) == 7
    assert [k for k, _ in calls_ddim] == ["twin"] * 6 + ["plain"]          # 4 - 6 * 0.5 = 1 exactly at the last step: no twin forward
    assert [t for _, t in calls_ddim] == [[t] for t in (997, 831, 665, 499, 333, 167, 1)]
    err = (a - b).abs().max().item() / a.abs().max().item()
    report("dropin DPMSolverSampler order 1 vs DDIMSampler S=6 [f32]", err, a.abs().max().item(), 1e-3)
    assert err < 1e-3, err
    # the PLMS / CompVis spelling of a scalar guidance is the same run
    kw.pop("guidance_scale")
    s1, _ = DPMSolverSampler(tiny_model).sample(unconditional_guidance_scale=3.0, **kw)
    s2, _ = DPMSolverSampler(tiny_model).sample(guidance_scale=[3.0, 3.0], **kw)
    s3, _ = DPMSolverSampler(tiny_model).sample(guidance_scale=3.0, timesteps=np.asarray([1, 167, 333, 499, 665, 831, 997]),
                                                **{**kw, "S": 50})
    assert torch.equal(s1, s2) and torch.equal(s1, s3)


# rms(difference to the f32 mode) / rms(f32 result) of the final latent, S = 10 on the logSNR grid, B = 2, guidance [10, 4]:
# bar = 1.5 x the value measured on an MI355X, rounded up to one digit (a different device of the pool, a different rounding
# draw: the rms moves by a few per cent between them).  DDIM at S = 10 in the same run: bf16 3.33e-2, fp16 4.28e-3 (max-abs / max:
# DPM-Solver++ 4.17e-2 / 3.98e-3, DDIM 3.87e-2 / 4.85e-3; reported, not asserted).
MODE_RMS_MEASURED = {"bf16": 3.591e-2, "fp16": 4.350e-3}
MODE_RMS_BAR = {"bf16": 6e-2, "fp16": 7e-3}


@pytest.fixture(scope="module")
def mode_runs(gpu):
    """S = 10 logSNR DPM-Solver++ and S = 10 DDIM on the tiny model in the f32, bf16 and fp16 modes, and each f32 / bf16 run
    twice: {(sampler, mode): [latents]}."""
    from adaface_amd.configs import tiny_config
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.util import instantiate_from_config
    model = instantiate_from_config(tiny_config()["model"]).eval()
    missing, unexpected = model.load_state_dict(O.synth_state_dict(O.unet_param_shapes(O.TINY_UNET), seed=11), strict=False)
    assert not unexpected
    model = model.to(gpu)
    g = torch.Generator().manual_seed(5)
    B = 2
    x_T = torch.randn(B, 4, 16, 16, generator=g).to(gpu)
    c_emb, uc_emb = (torch.randn(B * 16, 77, 64, generator=g).to(gpu) for _ in range(2))
    out = {}
    for mode in ("f32", "bf16", "fp16"):
        model.set_compute_dtype(mode)
        c, uc = model.get_learned_conditioning(c_emb), model.get_learned_conditioning(uc_emb)
        kw = dict(S=10, batch_size=B, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=[10.0, 4.0],
                  unconditional_conditioning=uc, x_T=x_T, eta=0.0)
        out["dpm", mode] = [DPMSolverSampler(model).sample(skip_type="logSNR", **kw)[0].clone()
                            for _ in range(1 if mode == "fp16" else 2)]
        out["ddim", mode] = [DDIMSampler(model).sample(**kw)[0].clone()]
    torch.cuda.synchronize()
    return out


def _dev(a, ref):
    d = (a - ref).double()
    return (d.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item(), (d.abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_throughput_modes_against_f32_mode(gpu, report, mode_runs, mode):
    ref = mode_runs["dpm", "f32"][0]
    lat = mode_runs["dpm", mode][0]
    assert torch.isfinite(lat).all() and torch.isfinite(ref).all()
    rms, mx = _dev(lat, ref)
    rms_ddim, mx_ddim = _dev(mode_runs["ddim", mode][0], mode_runs["ddim", "f32"][0])
    print(f"DPM-Solver++ S=10 logSNR {mode} vs f32 mode: rms {rms:.3e} max-abs {mx:.3e}; DDIM S=10: rms {rms_ddim:.3e} max-abs {mx_ddim:.3e}")
    report(f"tiny DPMSolverSampler S=10 logSNR {mode} vs f32 mode: rms", rms, ref.double().pow(2).mean().sqrt().item(), MODE_RMS_BAR[mode])
    report(f"tiny DPMSolverSampler S=10 logSNR {mode} vs f32 mode: max-abs (not asserted)", mx, ref.abs().max().item())
    report(f"tiny DDIMSampler S=10 {mode} vs f32 mode: rms (beside it)", rms_ddim)
    report(f"tiny DDIMSampler S=10 {mode} vs f32 mode: max-abs (beside it)", mx_ddim)
    assert 0 < rms <= MODE_RMS_BAR[mode], (rms, MODE_RMS_BAR[mode])       # (0 would mean the mode never switched)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_sampler_is_deterministic(gpu, mode_runs, mode):
    a, b = mode_runs["dpm", mode]
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
