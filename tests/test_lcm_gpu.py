"""GPU tests of LCM / TCD few-step sampling: af_lcm_step element by element against float64 with a counted rounding bound
(tests/lcm_ref.py), its Philox contract and batch-split invariance, LCMSampler on the tiny model against the restatement driving
the CPU oracle, against DPMSolverSampler at order 1 for TCD gamma = 0, its call count, determinism, inpainting and strength, and
the guidance-scale embedding folded into time_embed.0's bias against the oracle that adds it in front of that layer."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import dpmpp_ref as R  # noqa: E402
import lcm_ref as LR  # noqa: E402
import philox_ref as P  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ROOT / "tests" / "golden"
SENTINEL = -12345.5
PAD = 8                                    # guard floats in front of and behind every output (32 bytes: keeps 16-byte alignment)
f32 = lambda v: float(np.float32(v))
SEED = 42
# |z_dev - z_ref| / max(rho_ref, 2^-10) of the in-kernel normals: the bar tests/test_philox_gpu.py holds af_philox_randn to (4 x the
# 1.662e-7 measured there on an MI355X); the step kernel generates the same bits
NORMAL_BAR = 4 * 1.662e-7
VEC = 4 * 128                              # elements one block covers on the four-element path
SIZES = [(1, 1), (3, 1), (4, 1), (5, 1), (VEC - 1, 1), (VEC, 1), (VEC + 3, 1), (2 * VEC + 6, 2)]      # (n, B)
FWD_TOL_F32 = 2e-4                         # tests/test_model_gpu.py: TOL["f32"], max-abs error / max |ref| of one forward
SAMPLER_TOL = 1e-3                         # tests/test_dpm_solver_gpu.py: the drop-in sampler bar, of max |ref|, f32 mode


# ======================================================================================================================
# kernel
# ======================================================================================================================
@pytest.fixture(scope="module")
def coef_sets():
    """Real steps' coefficients (alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n), rounded to fp32 as the sampler hands them over:
    the first, a middle and the final row of the S = 4 LCM table and a middle row of the TCD gamma = 0.3 table."""
    from adaface_amd.ldm.models.diffusion import lcm as L
    acp = R.sd_acp()
    lcm = L.lcm_schedule(acp, L.lcm_timesteps(4))
    tcd = L.lcm_schedule(acp, L.lcm_timesteps(4), gamma=0.3)
    out = [tuple(f32(v) for v in row[L.COL_ALPHA:L.COL_S]) for row in (lcm[0], lcm[1], lcm[3], tcd[1])]
    assert out[2][6] == 0.0 and all(c[6] > 0.0 for c in (out[0], out[1], out[3])) and out[3][3] == 0.0 < out[0][3]
    return out


def _guarded(n, gpu, offset=0):
    """an n-element fp32 view with PAD sentinel floats on either side, `offset` floats off 16-byte alignment"""
    buf = torch.full((n + 2 * PAD + offset,), SENTINEL, device=gpu, dtype=torch.float32)
    return buf, buf[PAD + offset: PAD + offset + n]


def _inputs(n, seed, gpu, offset=0):
    g = torch.Generator().manual_seed(seed)
    host = [torch.randn(n + offset, generator=g) for _ in range(4)]       # x, e_c, e_u, z
    dev = [h.to(gpu)[offset:] for h in host]
    for d in dev:
        assert d.data_ptr() % 16 == (4 * offset) % 16
    return [h[offset:].numpy() for h in host], dev


def _run_case(gpu, n, B, coef, cfg, noise, offset=0, alias=False, seed=0, ids=None, by_array=False, step=3):
    """One launch against lcm_ref.step_f64.  noise: "given" (z handed in), "philox" (z in registers; then also the run with
    ops.philox_randn's tensor handed in, which must give the same bits) or "none" (c_n = 0: nothing read or generated).
    Returns worst err / bound."""
    from adaface_amd import ops
    (x, ec, eu, z), (dx, dec, deu, dz) = _inputs(n, seed, gpu, offset)
    per = n // B
    g = 7.5
    alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n = coef
    if noise == "none":
        c_n = 0.0
    ids = list(range(5, 5 + B)) if ids is None else ids
    ids_dev, first = (torch.tensor(ids, dtype=torch.int64, device=gpu), 0) if by_array else (None, ids[0])
    rho, bar = None, 0.0
    if noise == "philox":
        zz, rr = P.normals(SEED, ids, P.STREAM_STEP, step, per)
        z, rho, bar = zz.reshape(-1), rr.reshape(-1), NORMAL_BAR
    ref_xn, ref_d, b_xn, b_d = LR.step_f64(x, ec, eu if cfg else None, z, rho, g, alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n,
                                           normal_bar=bar)
    if alias:
        xbuf, dx_view = _guarded(n, gpu, offset)
        dx_view.copy_(dx)
        dx, nbuf, nview = dx_view, xbuf, dx_view
    else:
        nbuf, nview = _guarded(n, gpu, offset)
    dbuf, dview = _guarded(n, gpu, offset)
    x_keep = dx.clone()
    # with c_n = 0 the noise pointer is a poisoned tensor: a kernel that read it would leave NaN behind
    z_arg = dz if noise == "given" else torch.full_like(dz, float("nan")) if noise == "none" else None
    got_xn, got_d = ops.lcm_step(dx.view(B, per), dec, deu if cfg else None, g, alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n,
                                 noise=z_arg, seed=SEED, step=step, sample_ids=ids_dev, first_id=first, x_next=nview, d_out=dview)
    torch.cuda.synchronize()
    assert got_xn.data_ptr() == nview.data_ptr() and got_d.data_ptr() == dview.data_ptr()
    tag = (n, B, cfg, noise, offset, alias)
    worst = 0.0
    for buf, ref, bound in ((nbuf, ref_xn, b_xn), (dbuf, ref_d, b_d)):
        host = buf.cpu().numpy().astype(np.float64)
        lo = PAD + offset
        assert (host[:lo] == SENTINEL).all() and (host[lo + n:] == SENTINEL).all(), ("wrote outside [0, n)", tag)
        err = np.abs(host[lo: lo + n] - ref)
        assert (err <= bound).all(), (tag, float((err / bound).max()), int(np.argmax(err / bound)))
        worst = max(worst, float((err / bound).max()))
    if noise == "philox":
        # THE CONTRACT: the in-register z is bit for bit what af_philox_randn writes for that element
        zt = ops.philox_randn(B, per, SEED, P.STREAM_STEP, step, sample_ids=ids_dev, first_id=first, device=gpu)
        xn2, d2 = ops.lcm_step(x_keep.view(B, per), dec, deu if cfg else None, g, alpha_t, sigma_t, k_out, k_skip, c_x, c_0, c_n,
                               noise=zt, seed=SEED + 9, step=step + 1)
        assert torch.equal(xn2.view(-1), nview) and torch.equal(d2.view(-1), dview), tag
    return worst


@pytest.mark.parametrize("n,B", SIZES)
def test_step_kernel_against_float64(gpu, report, coef_sets, n, B):
    """Every element of x_next and d_out within k 2^-24 (sum of |terms|) (+ c_n NORMAL_BAR max(rho, 2^-10) with in-kernel noise),
    k counted from the kernel's header (lcm_ref.step_f64: 9 / 6 for x_next with / without guidance, 8 / 5 with c_n = 0 and for
    d_out); nothing outside [0, n) written.  {guidance} x {z given, Philox z, c_n = 0}, the four coefficient sets in turn; the
    Philox runs equal the runs with af_philox_randn's tensor handed in, for first_id-based ids and for an id array."""
    worst, k = 0.0, 0
    for cfg in (True, False):
        for noise in ("given", "philox", "none"):
            coef = coef_sets[(0, 1, 3)[k % 3]] if noise != "none" else coef_sets[k % 4]    # (the final row has c_n = 0 itself)
            worst = max(worst, _run_case(gpu, n, B, coef, cfg, noise, seed=n + k))
            k += 1
    big = [7, 2 ** 40 + 3][:B]
    worst = max(worst, _run_case(gpu, n, B, coef_sets[3], True, "philox", seed=n + 20, ids=big, by_array=True, step=9))
    worst = max(worst, _run_case(gpu, n, B, coef_sets[2], True, "given", seed=n + 21))     # the final row as it is: c_n = 0
    report(f"af_lcm_step n={n} B={B}: worst |err| / bound over 8 argument forms", worst, 1.0, 1.0)


@pytest.mark.parametrize("n,B", [(5, 1), (VEC + 3, 1), (2 * VEC + 8, 2)])
def test_step_kernel_unaligned_views_and_in_place(gpu, report, coef_sets, n, B):
    """Every pointer one float off 16-byte alignment (the scalar path), and x_next aliasing x (aligned: the 16-byte path, where
    a lane's four loads precede its stores), each with z given, Philox z and c_n = 0."""
    w = 0.0
    for i, noise in enumerate(("given", "philox", "none")):
        w = max(w, _run_case(gpu, n, B, coef_sets[i], True, noise, offset=1, seed=50 + i))
        w = max(w, _run_case(gpu, n, B, coef_sets[(i + 1) % 4], i != 1, noise, alias=True, seed=60 + i))
    w = max(w, _run_case(gpu, n, B, coef_sets[3], True, "philox", offset=1, alias=True, seed=70))
    report(f"af_lcm_step n={n} B={B}: unaligned views / in place, worst |err| / bound", w, 1.0, 1.0)


def test_step_refuses_an_aliased_d_out_on_the_device(gpu):
    """d_out that is x or x_next is refused on the host with a message; so is an input of another size."""
    from adaface_amd import _lib, ops
    x, e, out = (torch.randn(2, 32, device=gpu) for _ in range(3))
    step = lambda **kw: ops.lcm_step(x, kw.pop("e", e), None, 1.0, 0.8, 0.6, 1.0, 0.0, 0.5, 0.4, 0.3, **kw)
    for kw in (dict(d_out=x), dict(x_next=out, d_out=out), dict(x_next=x, d_out=x)):
        with pytest.raises(_lib.AfError, match="alias"):
            step(**kw)
    with pytest.raises(ValueError, match="e_cond"):
        step(e=e[:1])
    with pytest.raises(ValueError, match="noise"):
        step(noise=e[:1])
    before = ops.lcm_step_launches()
    xn, d = step(x_next=x, seed=3)                     # in place is fine, and is one launch
    torch.cuda.synchronize()
    assert xn.data_ptr() == x.data_ptr() and ops.lcm_step_launches() == before + 1


@pytest.mark.parametrize("per", [VEC, VEC + 3])
@pytest.mark.parametrize("by_array", [False, True])
def test_step_batch_split_invariance(gpu, coef_sets, per, by_array):
    """A B = 4 batch gives, bit for bit, what two B = 2 halves with first_id 0 and 2 (or the matching id arrays) give; another
    step index gives other noise."""
    from adaface_amd import ops
    g = torch.Generator().manual_seed(per)
    x, ec, eu = (torch.randn(4, per, generator=g).to(gpu) for _ in range(3))
    coef = coef_sets[3]
    ids = [0, 1, 2, 3] if not by_array else [11, 2 ** 33 + 1, 5, 0]

    def run(lo, hi, step=4):
        ids_dev, first = (torch.tensor(ids[lo:hi], dtype=torch.int64, device=gpu), 0) if by_array else (None, ids[lo])
        return ops.lcm_step(x[lo:hi], ec[lo:hi], eu[lo:hi], 3.0, *coef, seed=SEED, step=step, sample_ids=ids_dev, first_id=first)
    whole, d_whole = run(0, 4)
    parts = [run(0, 2), run(2, 4)]
    assert torch.equal(torch.cat([p[0] for p in parts]), whole) and torch.equal(torch.cat([p[1] for p in parts]), d_whole)
    other, d_other = run(0, 4, step=5)
    assert not torch.equal(other, whole) and torch.equal(d_other, d_whole)       # (D carries no noise)


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
    return dict(x_T=torch.tensor(g["ddim_xT"]), c=torch.tensor(g["ddim_c"]), uc=torch.tensor(g["ddim_uc"]),
                mask=torch.tensor(g["inpaint_mask"]), x0=torch.tensor(g["inpaint_x0"]))


ORACLE_IDS = [6]          # the one sample of the oracle runs carries global index 6
ORACLE_GUIDANCE = (4.0, 2.0)


@pytest.fixture(scope="module")
def oracle_runs(tiny_inputs):
    """lcm_ref.sample_ref driving the CPU oracle's UNet, computed once: S = 4, annealed guidance [4, 2], LCM and TCD gamma = 0.3."""
    cfg = O.TINY_UNET
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=11)
    apply = lambda x, t, c: O.unet_forward(sd, cfg, x, t, c)
    acp = R.sd_acp()
    i = tiny_inputs
    gs = O.guidance_schedule(ORACLE_GUIDANCE, 4)
    out = {}
    for name, gamma in (("lcm", None), ("tcd0.3", 0.3)):
        with torch.no_grad():
            lat, dens, called = LR.sample_ref(apply, acp, LR.grid(4), i["x_T"], i["c"], i["uc"], gs, SEED, ORACLE_IDS, gamma=gamma)
        out[name] = (lat.numpy(), [d.numpy() for d in dens], called)
    return out


def _conds(model, inputs, gpu):
    return (model.get_learned_conditioning(inputs["c"].to(gpu)), model.get_learned_conditioning(inputs["uc"].to(gpu)))


@pytest.mark.parametrize("case", ["lcm", "tcd0.3"])
def test_sampler_matches_restatement_on_the_oracle(gpu, report, tiny_model, tiny_inputs, oracle_runs, case):
    """LCMSampler.sample at S = 4 in f32 mode (annealed guidance [4, 2], cond / uncond pair, fixed x_T, in-kernel step noise from
    stream 1) against lcm_ref.sample_ref in float64 on the CPU oracle with the reference normals: 1e-3 of max|ref|, the bar
    tests/test_dpm_solver_gpu.py applies to its sampler-vs-oracle comparison.  pred_x0 of every step is the restatement's
    denoised sample, to the same bar."""
    from adaface_amd.noise import PhiloxNoise
    from ldm.models.diffusion.lcm import LCMSampler
    ref, ref_dens, ref_calls = oracle_runs[case]
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    steps_seen, dens = [], []
    sampler = LCMSampler(tiny_model)
    lat, inter = sampler.sample(
        S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=list(ORACLE_GUIDANCE),
        unconditional_conditioning=uc, x_T=tiny_inputs["x_T"].to(gpu), callback=steps_seen.append,
        img_callback=lambda p, i: dens.append(p.cpu().numpy()), tcd_gamma=None if case == "lcm" else 0.3,
        noise_source=PhiloxNoise(SEED, sample_ids=ORACLE_IDS), log_every_t=1, eta=0.0, temperature=1.0)
    err = np.abs(lat.cpu().numpy() - ref).max() / np.abs(ref).max()
    err_d = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(dens, ref_dens))
    print(f"LCMSampler {case} S=4 vs float64 restatement: latent {err:.3e} of max|ref| {np.abs(ref).max():.3f}; denoised {err_d:.3e}")
    report(f"dropin LCMSampler {case} S=4 vs float64 restatement on the oracle [f32]", err, float(np.abs(ref).max()), SAMPLER_TOL)
    report(f"dropin LCMSampler {case} S=4 pred_x0 vs restatement [f32]", err_d, 1.0, SAMPLER_TOL)
    assert err < SAMPLER_TOL, err
    assert err_d < SAMPLER_TOL, err_d
    assert steps_seen == [0, 1, 2, 3] and ref_calls == [999, 759, 499, 259] == list(sampler.timesteps[::-1])
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 5
    assert np.abs(inter["x_inter"][-1].cpu().numpy() - dens[-1]).max() <= 1e-6 * np.abs(ref).max()   # the last step returns D


def test_tcd_gamma0_equals_dpm_solver_order1(gpu, report, tiny_model, tiny_inputs):
    """TCD at gamma = 0 draws no noise and every step but the last is DPMSolverSampler(order = 1)'s on the same explicit
    timesteps: the latent after each of them, and the data prediction of every step, agree to 1e-3 of max|ref| (that test's
    order-1-vs-DDIM tolerance).  The last step differs by design: TCD returns the data prediction, the DPM solver steps on to
    acp[0] -- so TCD's result is compared with the DPM solver's last data prediction."""
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.lcm import LCMSampler
    from adaface_amd.ldm.models.diffusion.lcm import lcm_timesteps
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    ts = lcm_timesteps(4)
    kw = dict(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=3.0,
              unconditional_conditioning=uc, x_T=tiny_inputs["x_T"].to(gpu), timesteps=ts, log_every_t=1)
    p_dpm, p_tcd = [], []
    a, ia = DPMSolverSampler(tiny_model).sample(order=1, img_callback=lambda p, i: p_dpm.append(p.clone()), **kw)
    b, ib = LCMSampler(tiny_model).sample(tcd_gamma=0.0, img_callback=lambda p, i: p_tcd.append(p.clone()), **kw)
    assert len(ia["x_inter"]) == len(ib["x_inter"]) == 5 and len(p_dpm) == len(p_tcd) == 4
    worst = 0.0
    for i in range(1, 4):                                 # the latent after steps 0, 1, 2
        worst = max(worst, (ia["x_inter"][i] - ib["x_inter"][i]).abs().max().item() / ia["x_inter"][i].abs().max().item())
    for pa, pb in zip(p_dpm, p_tcd):
        worst = max(worst, (pa - pb).abs().max().item() / pa.abs().max().item())
    end = (b - p_dpm[-1]).abs().max().item() / p_dpm[-1].abs().max().item()
    report("dropin LCMSampler TCD gamma=0 vs DPMSolverSampler order 1 S=4 [f32]", max(worst, end), 1.0, SAMPLER_TOL)
    assert worst < SAMPLER_TOL and end < SAMPLER_TOL, (worst, end)
    assert (a - b).abs().max().item() > 1e-3 * a.abs().max().item()       # (and the DPM solver's own last step is another one)
    # no noise: the same run again, with and without a noise source, is the same tensor
    from adaface_amd.noise import PhiloxNoise
    b2, _ = LCMSampler(tiny_model).sample(tcd_gamma=0.0, noise_source=PhiloxNoise(SEED), **kw)
    assert torch.equal(b, b2)


def test_guidance_one_makes_s_single_leg_calls(gpu, tiny_model, tiny_inputs):
    from ldm.models.diffusion.lcm import LCMSampler
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    seen = []
    twin, plain = tiny_model.apply_model_cfg_twin, tiny_model.apply_model

    def rec_twin(x, t, cond):
        seen.append(("twin", t.tolist()))
        return twin(x, t, cond)

    def rec_plain(x, t, cond):
        seen.append(("plain", t.tolist(), tuple(x.shape)))
        return plain(x, t, cond)
    object.__setattr__(tiny_model, "apply_model_cfg_twin", rec_twin)
    object.__setattr__(tiny_model, "apply_model", rec_plain)
    try:
        kw = dict(batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, unconditional_conditioning=uc,
                  x_T=tiny_inputs["x_T"].to(gpu))
        for S in (1, 2, 4, 8):
            seen.clear()
            LCMSampler(tiny_model).sample(S=S, guidance_scale=1.0, **kw)
            assert seen == [("plain", [t], (1, 4, 16, 16)) for t in LR.grid(S)], (S, seen)
        seen.clear()
        LCMSampler(tiny_model).sample(S=4, guidance_scale=[2.5, 1.0], **kw)
        assert [k[0] for k in seen] == ["twin"] * 3 + ["plain"]          # 2.5 - 3 * 0.5 = 1 exactly at the last step
        seen.clear()
        LCMSampler(tiny_model).sample(S=4, guidance_scale=1.5, **{**kw, "unconditional_conditioning": None})
        assert [k[0] for k in seen] == ["plain"] * 4
    finally:
        object.__delattr__(tiny_model, "apply_model_cfg_twin")
        object.__delattr__(tiny_model, "apply_model")


class _Standin:
    """apply_model replaced by an element-wise function of (x, t) on the GPU, so that a sample's eps depends on that sample alone
    (tests/test_philox_gpu.py): eps = sigma_t x + 0.05 sin(3 x), and 0.05 sin(2 x) for the unconditional half."""

    def __init__(self, model):
        self.model = model

    def eps(self, x, t, k):
        return self.model.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1) * x + 0.05 * torch.sin(k * x)

    def __enter__(self):
        object.__setattr__(self.model, "apply_model", lambda x, t, c: self.eps(x, t, 3.0))
        object.__setattr__(self.model, "apply_model_cfg_twin", lambda x, t, twin: torch.cat([self.eps(x, t, 3.0), self.eps(x, t, 2.0)]))
        return self

    def __exit__(self, *exc):
        object.__delattr__(self.model, "apply_model")
        object.__delattr__(self.model, "apply_model_cfg_twin")


def _loop(model, b, noise_source, gpu, mask=None, x0=None, **extra):
    from ldm.models.diffusion.lcm import LCMSampler
    ctx = torch.zeros(b * 16, 77, 64, device=gpu)
    kw = dict(S=4, batch_size=b, shape=[4, 16, 16], conditioning=ctx, unconditional_conditioning=ctx + 1.0, verbose=False,
              guidance_scale=[3.0, 1.5], mask=mask, x0=x0, noise_source=noise_source, **extra)
    return LCMSampler(model).sample(**kw)[0]


@pytest.mark.parametrize("gamma", [None, 0.3])
@pytest.mark.parametrize("blend", [False, True])
def test_whole_loop_is_split_invariant(gpu, tiny_model, blend, gamma):
    """Batch 4 with ids 0..3 is bit-equal to two runs of batch 2 with first_id 0 and 2, x_T None (the start code from stream 0),
    with and without the inpainting blend (stream 2); the same seed again gives the same tensor, seed + 1 another.  With the
    blend, fused_blend gives the bits of the unfused lines."""
    from adaface_amd.noise import PhiloxNoise
    g = torch.Generator().manual_seed(8)
    mask = (torch.rand(4, 1, 16, 16, generator=g) > 0.5).float().to(gpu) if blend else None
    x0 = torch.randn(4, 4, 16, 16, generator=g).to(gpu) if blend else None
    half = lambda t, lo: None if t is None else t[lo:lo + 2]
    with _Standin(tiny_model):
        whole = _loop(tiny_model, 4, PhiloxNoise(SEED), gpu, mask=mask, x0=x0, tcd_gamma=gamma)
        parts = [_loop(tiny_model, 2, PhiloxNoise(SEED, first_id=lo), gpu, mask=half(mask, lo), x0=half(x0, lo), tcd_gamma=gamma)
                 for lo in (0, 2)]
        again = _loop(tiny_model, 4, PhiloxNoise(SEED), gpu, mask=mask, x0=x0, tcd_gamma=gamma)
        other = _loop(tiny_model, 4, PhiloxNoise(SEED + 1), gpu, mask=mask, x0=x0, tcd_gamma=gamma)
        fused = _loop(tiny_model, 4, PhiloxNoise(SEED), gpu, mask=mask, x0=x0, tcd_gamma=gamma, fused_blend=True) if blend else None
        cooler = _loop(tiny_model, 4, PhiloxNoise(SEED), gpu, mask=mask, x0=x0, tcd_gamma=gamma, temperature=0.5)
    assert torch.isfinite(whole).all() and whole.std().item() > 0.1
    assert torch.equal(torch.cat(parts), whole)
    assert torch.equal(again, whole) and again.data_ptr() != whole.data_ptr()
    assert not torch.equal(other, whole) and not torch.equal(whole[0], whole[1])
    assert not torch.equal(cooler, whole)                 # temperature scales the step noise
    if blend:
        assert torch.equal(fused, whole)


def test_same_seed_same_image_on_the_model(gpu, tiny_model, tiny_inputs):
    """LCMSampler on the tiny UNet itself: the same seed twice is the same tensor, seed + 1 is not; inpainting with fused_blend
    is the unfused blend bit for bit."""
    from adaface_amd.noise import PhiloxNoise
    from ldm.models.diffusion.lcm import LCMSampler
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    run = lambda seed, **kw: LCMSampler(tiny_model).sample(
        S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=2.0, unconditional_conditioning=uc,
        noise_source=PhiloxNoise(seed), **kw)[0].clone()
    a, b, d = run(SEED), run(SEED), run(SEED + 1)
    assert torch.equal(a, b) and not torch.equal(a, d)
    inp = dict(mask=tiny_inputs["mask"].to(gpu), x0=tiny_inputs["x0"].to(gpu))
    u, f = run(SEED, **inp), run(SEED, fused_blend=True, **inp)
    assert torch.equal(u, f) and not torch.equal(u, a)


def test_strength_runs_the_tail_of_the_grid(gpu, tiny_model, tiny_inputs):
    """strength = 0.5 at S = 4 executes the two smallest timesteps of the S-step grid, [499, 259], from x0 noised to 499."""
    from adaface_amd import ops
    from adaface_amd.noise import PhiloxNoise
    from ldm.models.diffusion.lcm import LCMSampler
    c, uc = _conds(tiny_model, tiny_inputs, gpu)
    seen = []
    plain = tiny_model.apply_model

    def rec_plain(x, t, cond):
        seen.append((t.tolist(), x.clone()))
        return plain(x, t, cond)
    object.__setattr__(tiny_model, "apply_model", rec_plain)
    try:
        x0 = tiny_inputs["x0"].to(gpu)
        s = LCMSampler(tiny_model)
        lat, _ = s.sample(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, guidance_scale=1.0, x0=x0, strength=0.5,
                          noise_source=PhiloxNoise(SEED))
    finally:
        object.__delattr__(tiny_model, "apply_model")
    assert [t for t, _ in seen] == [[499], [259]] and list(s.timesteps) == [259, 499] and s.schedule.shape[0] == 2
    z = ops.philox_randn(1, 4 * 16 * 16, SEED, 0, 0, device=gpu).view(1, 4, 16, 16)
    start = tiny_model.q_sample(x0, torch.tensor([499], device=gpu), noise=z)
    assert torch.equal(seen[0][1], start)                 # the start: x0 noised to the first executed timestep
    assert torch.isfinite(lat).all()


# ======================================================================================================================
# guidance-scale embedding
# ======================================================================================================================
COND_DIM = 8


@pytest.fixture(scope="module")
def lcm_model(gpu):
    """The tiny model with a guidance-scale embedding (time_cond_proj_dim = 8) and a seeded cond_proj; (model, its state dict)."""
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    cfg = tiny_config()
    cfg["model"]["params"]["unet_config"]["params"]["time_cond_proj_dim"] = COND_DIM
    model = instantiate_from_config(cfg["model"]).eval()
    sd = O.synth_state_dict(O.unet_param_shapes(O.TINY_UNET), seed=11)
    wc = torch.randn(O.TINY_UNET.model_channels, COND_DIM, generator=torch.Generator().manual_seed(31)) * 0.3
    full = dict(sd)
    full[O.UNET_PREFIX + "time_embed.cond_proj.weight"] = wc
    full.update(O.synth_state_dict(O.vae_param_shapes(O.TINY_VAE), seed=12))
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected and not any("cond_proj" in k for k in missing)
    return model.to(gpu).set_compute_dtype("f32"), sd, wc


def _oracle_with_embedding(sd, wc, w, x, t, ctx):
    """The oracle's forward with Wc wemb(w) added to the timestep embedding in front of time_embed.0 (w None: the plain one)."""
    if w is None:
        return O.unet_forward(sd, O.TINY_UNET, x, t, ctx)
    add = (wc.double() @ torch.from_numpy(LR.w_embedding(w, COND_DIM))).float()
    orig = O.timestep_embedding
    O.timestep_embedding = lambda ts, dim, *a, **k: orig(ts, dim, *a, **k) + add
    try:
        return O.unet_forward(sd, O.TINY_UNET, x, t, ctx)
    finally:
        O.timestep_embedding = orig


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max() / (np.abs(ref).max() + 1e-12))


def test_guidance_embedding_forward_matches_the_oracle(gpu, report, lcm_model, tiny_inputs):
    """apply_model after set_guidance_embedding(w) against the oracle that adds Wc wemb in front of time_embed.0: the forward
    tolerance of tests/test_model_gpu.py in f32 mode.  set_guidance_embedding(None) gives the earlier forward back bit for bit.
    With a LoRA on time_embed.0 the fold uses the merged weight (oracle: the merged weight in its state dict), whichever of
    set_lora / set_guidance_embedding comes first."""
    model, sd, wc = lcm_model
    x = tiny_inputs["x_T"]
    t = torch.tensor([759])
    ctx = tiny_inputs["c"]
    c = model.get_learned_conditioning(ctx.to(gpu))
    fwd = lambda: model.apply_model(x.to(gpu), t.to(gpu), c).clone()
    with torch.no_grad():
        base_ref = _oracle_with_embedding(sd, wc, None, x, t, ctx).numpy()
    before = fwd()
    assert _rel(before.cpu().numpy(), base_ref) < FWD_TOL_F32
    for w in (1.5, 8.0):
        with torch.no_grad():
            ref = _oracle_with_embedding(sd, wc, w, x, t, ctx).numpy()
        model.set_guidance_embedding(w)
        assert model.guidance_embedding == w
        got = fwd().cpu().numpy()
        err = _rel(got, ref)
        report(f"tiny_unet with guidance-scale embedding w={w} vs oracle [f32]", err, 1.0, FWD_TOL_F32)
        assert err < FWD_TOL_F32, (w, err)
        assert _rel(ref, base_ref) > 50 * FWD_TOL_F32, "the embedding must change the forward for the comparison to mean anything"
    model.set_guidance_embedding(None)
    assert model.guidance_embedding is None and torch.equal(fwd(), before)
    # LoRA on time_embed.0: the fold follows the merged weight
    g = torch.Generator().manual_seed(41)
    mc = O.TINY_UNET.model_channels
    up, down, alpha, scale = torch.randn(4 * mc, 4, generator=g) * 0.2, torch.randn(4, mc, generator=g) * 0.2, 4.0, 0.8
    merged = dict(sd)
    key = O.UNET_PREFIX + "time_embed.0.weight"
    merged[key] = sd[key] + float(np.float32(scale * alpha / 4)) * (up @ down)
    with torch.no_grad():
        ref = _oracle_with_embedding(merged, wc, 8.0, x, t, ctx).numpy()
        ref_unmerged = _oracle_with_embedding(sd, wc, 8.0, x, t, ctx).numpy()
    adapters = [({"unet": {"time_embed.0": (up, down, alpha)}}, scale)]
    try:
        for order in ("lora first", "embedding first"):
            if order == "lora first":
                model.set_lora(adapters)
                model.set_guidance_embedding(8.0)
            else:
                model.set_guidance_embedding(8.0)
                model.set_lora(adapters)
            err = _rel(fwd().cpu().numpy(), ref)
            report(f"tiny_unet guidance-scale embedding + LoRA on time_embed.0 ({order}) vs oracle [f32]", err, 1.0, FWD_TOL_F32)
            assert err < FWD_TOL_F32, (order, err)
            model.set_guidance_embedding(None)
            model.clear_lora()
        assert _rel(ref_unmerged, ref) > 50 * FWD_TOL_F32, "the adapter must matter to the fold"
    finally:
        model.set_guidance_embedding(None)
        model.clear_lora()
    assert torch.equal(fwd(), before)


def test_sampler_guidance_embedding_runs_one_leg_and_restores_the_bias(gpu, lcm_model, tiny_model, tiny_inputs):
    """sample(guidance_embedding=True) sets w = guidance_scale, makes S single-leg calls although an unconditional conditioning
    is given, and removes the embedding again -- also when the run raises.  A model without cond_proj is refused by name."""
    from ldm.models.diffusion.lcm import LCMSampler
    model, sd, wc = lcm_model
    c, uc = _conds(model, tiny_inputs, gpu)
    x_T = tiny_inputs["x_T"].to(gpu)
    probe = lambda: model.apply_model(x_T, torch.tensor([499], device=gpu), c).clone()
    before = probe()
    seen = []
    plain = model.apply_model

    def rec_plain(x, t, cond):
        seen.append((t.tolist(), model.guidance_embedding))
        return plain(x, t, cond)
    kw = dict(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, unconditional_conditioning=uc, x_T=x_T,
              guidance_embedding=True, guidance_scale=8.0)
    object.__setattr__(model, "apply_model", rec_plain)
    try:
        with_emb, _ = LCMSampler(model).sample(**kw)
        assert seen == [([t], 8.0) for t in LR.grid(4)]
        assert model.guidance_embedding is None

        class Boom(RuntimeError):
            pass

        def boom(i):
            if i == 1:
                raise Boom()
        with pytest.raises(Boom):
            LCMSampler(model).sample(callback=boom, **kw)
        assert model.guidance_embedding is None
    finally:
        object.__delattr__(model, "apply_model")
    assert torch.equal(probe(), before)                   # the engine's bias is the original one again
    without, _ = LCMSampler(model).sample(**{**kw, "guidance_embedding": False, "guidance_scale": 1.0})
    assert not torch.equal(with_emb, without)
    with pytest.raises(ValueError, match="guidance_embedding"):
        LCMSampler(tiny_model).sample(**{**kw, "conditioning": c})
