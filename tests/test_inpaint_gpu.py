"""GPU tests of img2img by strength and inpainting: af_noise_blend bit for bit against the torch composition it replaces
(LatentDiffusion.q_sample followed by the samplers' blend line, z from af_philox_randn), the samplers' fused_blend and strength
on the tiny model, and the hybrid (9-channel) U-Net."""
import dataclasses
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import inpaint_ref as IR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ROOT / "tests" / "golden"
SEED = 42
SHAPES = [(1, 1, 1), (1, 4, 3), (3, 3, 7), (2, 4, 5), (2, 4, 64), (2, 4, 256 + 1), (8, 4, 4096)]
SA, S1 = float(np.float32(0.8312)), float(np.float32(0.5559))     # two fp32 scalars with full mantissas


# ======================================================================================================================
# operator
# ======================================================================================================================
def _operands(shape, gpu, seed):
    n, c, hw = shape
    g = torch.Generator().manual_seed(seed)
    x, x0, z = (torch.randn(n, c, hw, generator=g).to(gpu) for _ in range(3))
    return x, x0, z


def _masks(shape, gpu, seed):
    """(name, keep) for keep_channels 1 and C, binary and soft with values strictly inside (0, 1)."""
    n, c, hw = shape
    g = torch.Generator().manual_seed(seed + 1000)
    out = []
    for kc in (1, c):
        u = torch.rand(n, kc, hw, generator=g)
        out.append((f"binary kc={kc}", (u > 0.5).float().to(gpu)))
        out.append((f"soft kc={kc}", (0.01 + 0.98 * u).to(gpu)))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise_blend_equals_the_torch_composition(gpu, shape):
    """torch.equal against q_sample + blend, both noise sources (explicit noise; in-kernel Philox against the same z written
    by af_philox_randn), keep_channels 1 and C, binary and soft masks; keep=None; s1 = 0; in place."""
    from adaface_amd import ops
    n, c, hw = shape
    x, x0, _ = _operands(shape, gpu, seed=sum(shape))
    z = ops.philox_randn(n, c * hw, SEED, ops.STREAM_QSAMPLE, 3, first_id=11, device=gpu).view(n, c, hw)
    before = ops._lib.noise_blend_launches()
    calls = 0
    for name, keep in _masks(shape, gpu, seed=sum(shape)):
        want = IR.blend_torch(x, x0, keep, SA, S1, z)
        got_noise = ops.noise_blend(x, x0, keep, SA, S1, noise=z)
        got_key = ops.noise_blend(x, x0, keep, SA, S1, seed=SEED, step=3, first_id=11)
        assert torch.equal(got_noise, want), (name, "noise tensor")
        assert torch.equal(got_key, want), (name, "in-kernel Philox")
        # s1 = 0: no noise is read (a NaN tensor stands where it would be)
        want0 = IR.blend_torch(x, x0, keep, SA, 0.0, None)
        assert torch.equal(ops.noise_blend(x, x0, keep, SA, 0.0, noise=torch.full_like(z, float("nan"))), want0), (name, "s1 = 0")
        # in place: out is x
        xi = x.clone()
        assert ops.noise_blend(xi, x0, keep, SA, S1, seed=SEED, step=3, first_id=11, out=xi) is xi and torch.equal(xi, want), name
        calls += 4
    # keep None: the stochastic encode, x not needed
    want = IR.blend_torch(None, x0, None, SA, S1, z)
    assert torch.equal(ops.noise_blend(None, x0, None, SA, S1, noise=z), want)
    assert torch.equal(ops.noise_blend(None, x0, None, SA, S1, seed=SEED, step=3, first_id=11), want)
    assert torch.equal(ops.noise_blend(x, x0, None, SA, S1, seed=SEED, step=3, first_id=11), want)
    assert ops._lib.noise_blend_launches() - before == calls + 3          # one launch per call
    assert not torch.equal(ops.noise_blend(None, x0, None, SA, S1, seed=SEED, step=4, first_id=11), want) or c * hw * n < 2
    torch.cuda.synchronize()


def test_keep_none_equals_model_q_sample(gpu, tiny_model):
    """keep=None against LatentDiffusion.q_sample itself, with the model's own fp32 tables at a timestep."""
    from adaface_amd import ops
    _, x0, z = _operands((2, 4, 256), gpu, seed=3)
    x0, z = x0.view(2, 4, 16, 16), z.view(2, 4, 16, 16)
    for t in (1, 499, 997):
        ts = torch.full((2,), t, device=gpu, dtype=torch.long)
        sa, s1 = float(tiny_model.sqrt_alphas_cumprod[t]), float(tiny_model.sqrt_one_minus_alphas_cumprod[t])
        assert torch.equal(ops.noise_blend(None, x0, None, sa, s1, noise=z), tiny_model.q_sample(x0, ts, noise=z)), t


@pytest.mark.parametrize("shape", [(3, 3, 7), (2, 4, 5), (2, 4, 64), (2, 4, 256 + 1)], ids=lambda s: "x".join(map(str, s)))
def test_offset_pointers_take_the_scalar_path_with_the_same_bits(gpu, shape):
    """Every pointer one float off 16-byte alignment against the aligned run of the same values; guard floats around the
    output stay untouched."""
    from adaface_amd import ops
    n, c, hw = shape
    x, x0, z = _operands(shape, gpu, seed=7)
    keep = _masks(shape, gpu, seed=7)[3][1]                  # soft, C channels
    aligned = [ops.noise_blend(x, x0, keep, SA, S1, noise=z), ops.noise_blend(x, x0, keep, SA, S1, seed=SEED, step=1, first_id=5)]

    def off(t):
        buf = torch.empty(t.numel() + 1, device=gpu)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    xo, x0o, zo, ko = off(x), off(x0), off(z), off(keep)
    pad = 8
    for k, kw in enumerate((dict(noise=zo), dict(seed=SEED, step=1, first_id=5))):
        buf = torch.full((x.numel() + 2 * pad + 1,), -12345.5, device=gpu)
        out = buf[pad + 1: pad + 1 + x.numel()].view(x.shape)
        assert out.data_ptr() % 16 == 4
        ops.noise_blend(xo, x0o, ko, SA, S1, out=out, **kw)
        assert torch.equal(out, aligned[k]), k
        assert (buf[:pad + 1] == -12345.5).all() and (buf[pad + 1 + x.numel():] == -12345.5).all(), "wrote outside the output"
    torch.cuda.synchronize()


def test_sample_ids_and_batch_split(gpu):
    """sample_ids=[5, 2] equals first_id launches of the single samples, and the two samples in one launch equal the two
    launched alone (the 16-byte and the scalar path)."""
    from adaface_amd import ops
    for shape in ((2, 4, 64), (2, 3, 7)):
        x, x0, _ = _operands(shape, gpu, seed=9)
        keep = _masks(shape, gpu, seed=9)[1][1]              # soft, one channel
        ids = torch.tensor([5, 2], dtype=torch.int64, device=gpu)
        both = ops.noise_blend(x, x0, keep, SA, S1, seed=SEED, step=6, sample_ids=ids)
        for i, sid in enumerate((5, 2)):
            one = ops.noise_blend(x[i:i + 1], x0[i:i + 1], keep[i:i + 1], SA, S1, seed=SEED, step=6, first_id=sid)
            assert torch.equal(one[0], both[i]), (shape, sid)
            one_ids = ops.noise_blend(x[i:i + 1], x0[i:i + 1], keep[i:i + 1], SA, S1, seed=SEED, step=6, sample_ids=ids[i:i + 1].clone())
            assert torch.equal(one_ids[0], both[i]), (shape, sid)
        z = torch.stack([ops.philox_randn(1, shape[1] * shape[2], SEED, ops.STREAM_QSAMPLE, 6, first_id=s, device=gpu)[0] for s in (5, 2)])
        assert torch.equal(both, IR.blend_torch(x, x0, keep, SA, S1, z.view(shape)))
        assert not torch.equal(both, ops.noise_blend(x, x0, keep, SA, S1, seed=SEED, step=6, first_id=5))


def test_in_kernel_normals_statistics(gpu):
    """sa = 0, s1 = 1 on x0 = 0 returns z itself: the bits of af_philox_randn, under the bars tests/test_philox_cpu.py sets for
    the generator (|mean| <= 5 / sqrt(N), |std - 1| <= 5 / sqrt(2 N))."""
    from adaface_amd import ops
    n, c, hw = 8, 4, 4096
    z = ops.noise_blend(None, torch.zeros(n, c, hw, device=gpu), None, 0.0, 1.0, seed=SEED, stream=ops.STREAM_QSAMPLE, step=0)
    assert torch.equal(z.view(n, c * hw), ops.philox_randn(n, c * hw, SEED, ops.STREAM_QSAMPLE, 0, device=gpu))
    N = n * c * hw
    zz = z.double()
    mean, std = float(zz.mean()), float(zz.std())
    print(f"in-kernel normals of (8, 4, 4096): mean {mean:.5f} std - 1 {std - 1:.5f} max |z| {float(zz.abs().max()):.2f}")
    assert abs(mean) <= 5.0 / np.sqrt(N) and abs(std - 1.0) <= 5.0 / np.sqrt(2 * N)
    assert float(zz.abs().max()) <= 5.78


def test_refusals_on_the_device(gpu):
    from adaface_amd import _lib, ops
    x, x0, keep = torch.randn(2, 4, 16, device=gpu), torch.randn(2, 4, 16, device=gpu), torch.rand(2, 1, 16, device=gpu)
    with pytest.raises(_lib.AfError, match="overlaps"):
        ops.noise_blend(x, x0, keep, SA, S1, out=x0)
    with pytest.raises(_lib.AfError, match="step"):
        ops.noise_blend(x, x0, keep, SA, S1, step=1 << 24)
    with pytest.raises(ValueError, match="keep"):
        ops.noise_blend(x, x0, torch.rand(2, 2, 16, device=gpu), SA, S1)
    with pytest.raises(ValueError, match="keep"):
        ops.noise_blend(None, x0, keep, SA, S1)
    with pytest.raises(ValueError, match="noise"):
        ops.noise_blend(x, x0, keep, SA, S1, noise=torch.randn(2, 4, 8, device=gpu))
    torch.cuda.synchronize()


# ======================================================================================================================
# samplers, tiny model (fixtures as tests/test_dpm_solver_gpu.py)
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
def conds(gpu, tiny_model, tiny_inputs):
    return (tiny_model.get_learned_conditioning(tiny_inputs["c"].to(gpu)),
            tiny_model.get_learned_conditioning(tiny_inputs["uc"].to(gpu)))


def _sampler(name, model):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    return {"ddim": DDIMSampler, "dpm": DPMSolverSampler, "plms": PLMSSampler}[name.split(":")[0]](model)


def _run(name, model, conds, gpu, **kw):
    """One S = 6 run (7 grid steps) of the sampler `name` on the tiny model; guidance annealed where the sampler takes it."""
    c, uc = conds
    base = dict(S=6, batch_size=1, shape=[4, 16, 16], conditioning=c, unconditional_conditioning=uc, verbose=False)
    if name.startswith("plms"):
        base.update(unconditional_guidance_scale=3.0)
    else:
        base.update(guidance_scale=[10.0, 4.0])
    if name == "ddim:eta":
        base.update(eta=0.5)
    if name == "dpm:sde":
        base.update(algorithm="sde-dpmsolver++")
    base.update(kw)
    s = _sampler(name, model)
    lat, _ = s.sample(**base)
    return lat, s


SAMPLERS = ["ddim", "ddim:eta", "dpm", "dpm:sde", "plms"]


@pytest.mark.parametrize("name", SAMPLERS)
def test_fused_blend_equals_the_composition(gpu, tiny_model, tiny_inputs, conds, name):
    """fused_blend=True equals fused_blend=False exactly, with a PhiloxNoise and a mask; the fused run makes one blend launch
    per step and never calls q_sample, the other one calls it every step."""
    from adaface_amd import _lib
    from adaface_amd.noise import PhiloxNoise
    mask, x0, x_T = (tiny_inputs[k].to(gpu) for k in ("mask", "x0", "x_T"))
    q_calls = []
    orig = tiny_model.q_sample

    def q_sample(x_start, t, noise=None):
        q_calls.append(int(t[0]))
        return orig(x_start, t, noise=noise)
    object.__setattr__(tiny_model, "q_sample", q_sample)
    try:
        kw = dict(mask=mask, x0=x0, x_T=x_T)
        plain, _ = _run(name, tiny_model, conds, gpu, noise_source=PhiloxNoise(SEED, sample_ids=[5]), **kw)
        assert q_calls == [997, 831, 665, 499, 333, 167, 1]
        before = _lib.noise_blend_launches()
        fused, _ = _run(name, tiny_model, conds, gpu, noise_source=PhiloxNoise(SEED, sample_ids=[5]), fused_blend=True, **kw)
        assert len(q_calls) == 7 and _lib.noise_blend_launches() - before == 7
    finally:
        object.__delattr__(tiny_model, "q_sample")
    assert torch.isfinite(fused).all() and torch.equal(fused, plain), name
    other, _ = _run(name, tiny_model, conds, gpu, noise_source=PhiloxNoise(SEED, sample_ids=[6]), fused_blend=True, **kw)
    assert not torch.equal(other, fused)                                   # the blend's noise follows the sample id


def test_fused_blend_without_a_noise_source_draws_what_q_sample_draws(gpu, tiny_model, tiny_inputs, conds):
    """No noise_source: the fused blend passes torch.randn_like(x0), the draw q_sample makes, so a seeded device generator
    gives the same run."""
    mask, x0, x_T = (tiny_inputs[k].to(gpu) for k in ("mask", "x0", "x_T"))
    outs = []
    for fused in (False, True):
        torch.manual_seed(1234)
        outs.append(_run("ddim", tiny_model, conds, gpu, mask=mask, x0=x0, x_T=x_T, fused_blend=fused)[0])
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("algorithm", ["dpmsolver++", "sde-dpmsolver++"])
def test_dpm_strength_equals_the_manual_run(gpu, tiny_model, tiny_inputs, conds, algorithm):
    """strength on DPM-Solver++ against torch q_sample at ts[n - 1] followed by sample(timesteps=ts[:n], x_T=...), exactly;
    x_T is read as the noise; with a PhiloxNoise and no x_T the noise is the start code of the same seed."""
    from adaface_amd.ldm.models.diffusion.dpm_solver import dpmpp_timesteps
    from adaface_amd.noise import STREAM_XT, PhiloxNoise
    x0, z = tiny_inputs["x0"].to(gpu), tiny_inputs["x_T"].to(gpu)
    acp = tiny_model.alphas_cumprod.double().cpu().numpy()
    ts = dpmpp_timesteps(acp, 6)
    for strength in (0.5, 1.0, 0.01):
        n = IR.strength_n(len(ts), strength)
        t = torch.full((1,), int(ts[n - 1]), device=gpu, dtype=torch.long)
        src = lambda: PhiloxNoise(SEED, sample_ids=[3])
        manual, _ = _run("dpm", tiny_model, conds, gpu, algorithm=algorithm, timesteps=ts[:n], x_T=tiny_model.q_sample(x0, t, noise=z),
                         noise_source=src())
        got, s = _run("dpm", tiny_model, conds, gpu, algorithm=algorithm, strength=strength, x0=x0, x_T=z, noise_source=src())
        assert torch.equal(got, manual), (algorithm, strength)
        assert [int(v) for v in s.timesteps[::-1]] == IR.executed(ts, strength) and s.schedule.shape[0] == n
    zk = PhiloxNoise(SEED, sample_ids=[3]).randn(x0.shape, STREAM_XT, 0, gpu)
    t = torch.full((1,), int(ts[2]), device=gpu, dtype=torch.long)
    manual, _ = _run("dpm", tiny_model, conds, gpu, algorithm=algorithm, timesteps=ts[:3], x_T=tiny_model.q_sample(x0, t, noise=zk),
                     noise_source=PhiloxNoise(SEED, sample_ids=[3]))
    got, _ = _run("dpm", tiny_model, conds, gpu, algorithm=algorithm, strength=0.5, x0=x0, noise_source=PhiloxNoise(SEED, sample_ids=[3]))
    assert torch.equal(got, manual)


@pytest.fixture(scope="module")
def oracle_apply():
    cfg = O.TINY_UNET
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=11)
    return lambda x, t, c: O.unet_forward(sd, cfg, x, t, c)


def test_ddim_strength_matches_the_oracle(gpu, report, tiny_model, tiny_inputs, conds, oracle_apply):
    """DDIMSampler with strength 0.5 at S = 6 (3 of 7 steps: 333, 167, 1), without and with the blend, against
    inpaint_ref.ddim_strength_ref on the CPU oracle: 1e-3 of max|ref|, the bar of the drop-in sampler tests
    (tests/test_dropin_gpu.py, tests/test_dpm_solver_gpu.py)."""
    i = tiny_inputs
    sched = O.register_schedule()
    seen = []
    orig = tiny_model.apply_model_cfg_twin

    def rec(x, t, cond, **kw):
        seen.append(int(t[0]))
        return orig(x, t, cond, **kw)
    for blend in (False, True):
        kw_ref = dict(mask=i["mask"], q_noise=i["q_noise"]) if blend else {}
        ref, sub = IR.ddim_strength_ref(oracle_apply, sched, 6, 0.5, i["x0"], i["x_T"], i["c"], i["uc"], **kw_ref)
        assert [int(t) for t in sub] == [1, 167, 333]
        kw = {}
        if blend:
            noises = [t.to(gpu) for t in i["q_noise"]]
            calls = []
            q_orig = tiny_model.q_sample

            def q_sample(x_start, t, noise=None):
                calls.append(int(t[0]))
                return q_orig(x_start, t, noise=noises[len(calls) - 1])
            object.__setattr__(tiny_model, "q_sample", q_sample)
            kw = dict(mask=i["mask"].to(gpu))
        object.__setattr__(tiny_model, "apply_model_cfg_twin", rec)
        try:
            seen.clear()
            lat, _ = _run("ddim", tiny_model, conds, gpu, strength=0.5, x0=i["x0"].to(gpu), x_T=i["x_T"].to(gpu), **kw)
        finally:
            object.__delattr__(tiny_model, "apply_model_cfg_twin")
            if blend:
                object.__delattr__(tiny_model, "q_sample")
        assert seen == [333, 167, 1] and (not blend or calls == [333, 167, 1])
        ref = ref.numpy()
        err = float(np.abs(lat.cpu().numpy() - ref).max() / np.abs(ref).max())
        report(f"dropin DDIMSampler strength 0.5 S=6{' + blend' if blend else ''} vs restatement on the oracle [f32]", err,
               float(np.abs(ref).max()), 1e-3)
        assert err < 1e-3, (blend, err)


def test_plms_strength_matches_the_oracle(gpu, report, tiny_model, tiny_inputs, conds, oracle_apply):
    """PLMSSampler with strength 0.5 at S = 6 against inpaint_ref.plms_strength_ref: the eps history starts with the run (its
    first executed step is the two-call one); the same 1e-3 of max|ref|."""
    i = tiny_inputs
    ref, sub = IR.plms_strength_ref(oracle_apply, O.register_schedule(), 6, 0.5, i["x0"], i["x_T"], i["c"], i["uc"], guidance=3.0)
    seen = []
    orig = tiny_model.apply_model_cfg_twin

    def rec(x, t, cond, **kw):
        seen.append(int(t[0]))
        return orig(x, t, cond, **kw)
    object.__setattr__(tiny_model, "apply_model_cfg_twin", rec)
    try:
        lat, _ = _run("plms", tiny_model, conds, gpu, strength=0.5, x0=i["x0"].to(gpu), x_T=i["x_T"].to(gpu))
    finally:
        object.__delattr__(tiny_model, "apply_model_cfg_twin")
    assert seen == [333, 167, 167, 1]
    ref = ref.numpy()
    err = float(np.abs(lat.cpu().numpy() - ref).max() / np.abs(ref).max())
    report("dropin PLMSSampler strength 0.5 S=6 vs restatement on the oracle [f32]", err, float(np.abs(ref).max()), 1e-3)
    assert err < 1e-3, err


@pytest.mark.parametrize("name", ["ddim", "dpm", "plms"])
def test_strength_edges(gpu, tiny_model, tiny_inputs, conds, name):
    """Keep mask all ones + finish returns x0 exactly; keep mask all zeros equals the maskless run exactly; strength 1
    executes every step of the grid."""
    from adaface_amd.img2img import finish
    from adaface_amd.noise import PhiloxNoise
    x0, z = tiny_inputs["x0"].to(gpu), tiny_inputs["x_T"].to(gpu)
    src = (lambda: None) if name == "plms" else (lambda: PhiloxNoise(SEED, sample_ids=[1]))
    kw = dict(strength=0.5, x0=x0, x_T=z)
    ones, zeros = torch.ones(1, 1, 16, 16, device=gpu), torch.zeros(1, 1, 16, 16, device=gpu)
    kept, _ = _run(name, tiny_model, conds, gpu, mask=ones, fused_blend=True, noise_source=src(), **kw)
    assert not torch.equal(kept, x0) and torch.equal(finish(kept, x0, ones), x0)
    maskless, _ = _run(name, tiny_model, conds, gpu, noise_source=src(), **kw)
    for fused in (True, False):
        free, _ = _run(name, tiny_model, conds, gpu, mask=zeros, fused_blend=fused, noise_source=src(), **kw)
        assert torch.equal(free, maskless), (name, fused)
    assert torch.equal(finish(maskless, x0, zeros), maskless)
    steps = []
    _run(name, tiny_model, conds, gpu, strength=1.0, x0=x0, x_T=z, callback=steps.append)
    assert steps == list(range(7))
    steps.clear()
    _run(name, tiny_model, conds, gpu, strength=0.01, x0=x0, x_T=z, callback=steps.append)
    assert steps == [0]


@pytest.mark.parametrize("name", ["ddim", "dpm"])
def test_logs_run_over_the_executed_steps(gpu, tiny_model, tiny_inputs, conds, name):
    """With deep_cache_interval=2 and with tgate_step the logs have n entries; a gate beyond n - 1 is refused."""
    x0, z = tiny_inputs["x0"].to(gpu), tiny_inputs["x_T"].to(gpu)
    kw = dict(strength=0.6, x0=x0, x_T=z)                       # n = int(7 * 0.6) = 4
    _, s = _run(name, tiny_model, conds, gpu, deep_cache_interval=2, **kw)
    assert s.deep_cache_log == ["refresh", "reuse", "refresh", "reuse"], s.deep_cache_log
    _, s = _run(name, tiny_model, conds, gpu, tgate_step=2, **kw)
    assert s.tgate_log == [None, "capture", "replay", "replay"]
    with pytest.raises(ValueError, match="tgate_step"):
        _run(name, tiny_model, conds, gpu, tgate_step=4, **kw)


# ======================================================================================================================
# hybrid: the 9-channel inpainting U-Net
# ======================================================================================================================
HYBRID_UNET = dataclasses.replace(O.TINY_UNET, in_channels=9)
FWD_TOL = {"f32": 2e-4, "bf16": 3e-2}        # tests/test_model_gpu.py TOL, tests/test_dropin_gpu.py: the tiny forward's bars


@pytest.fixture(scope="module")
def hybrid(gpu):
    from adaface_amd.configs import tiny_config
    from adaface_amd.img2img import select_hybrid
    from ldm.util import instantiate_from_config
    cfg = tiny_config()
    cfg["model"]["params"]["unet_config"]["params"]["in_channels"] = 9
    assert select_hybrid(cfg)
    model = instantiate_from_config(cfg["model"]).eval()
    sd = O.synth_state_dict(O.unet_param_shapes(HYBRID_UNET), seed=31)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith("model.diffusion_model.")]
    g = torch.Generator().manual_seed(32)
    B = 2
    inputs = dict(x=torch.randn(B, 4, 16, 16, generator=g), cc=torch.randn(B, 5, 16, 16, generator=g),
                  t=torch.tensor([997, 333]), c=torch.randn(B * 16, 77, 64, generator=g), uc=torch.randn(B * 16, 77, 64, generator=g))
    with torch.no_grad():
        ref = O.unet_forward(sd, HYBRID_UNET, torch.cat([inputs["x"], inputs["cc"]], 1), inputs["t"], inputs["c"])
    return model.to(gpu).set_compute_dtype("f32"), inputs, ref.numpy()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_hybrid_apply_model(gpu, report, hybrid, mode):
    """apply_model with set_concat_cond equals apply_model on the hand-concatenated dict form exactly; both against the
    oracle's forward on the concatenated input within the tiny forward's bar of the dtype."""
    model, i, ref = hybrid
    model.set_compute_dtype(mode)
    x, cc, t = i["x"].to(gpu), i["cc"].to(gpu), i["t"].to(gpu)
    cond = model.get_learned_conditioning(i["c"].to(gpu))
    try:
        model.set_concat_cond(cc)
        a = model.apply_model(x, t, cond)
        model.set_concat_cond(None)
        b = model.apply_model(x, t, {"c_concat": [cc], "c_crossattn": [cond]})
        with pytest.raises(ValueError, match="set_concat_cond"):
            model.apply_model(x, t, cond)
    finally:
        model.set_concat_cond(None)
        model.set_compute_dtype("f32")
    assert a.shape == (2, 4, 16, 16) and torch.equal(a, b)
    err = float(np.abs(a.cpu().numpy() - ref).max() / np.abs(ref).max())
    report(f"hybrid tiny_unet (9 -> 4 channels) apply_model vs oracle [{mode}]", err, float(np.abs(ref).max()), FWD_TOL[mode])
    assert err < FWD_TOL[mode], err


def test_hybrid_twin_equals_the_concatenated_batch(gpu, report, hybrid):
    """apply_model_cfg_twin (x and the concatenated condition of ONE leg) against apply_model on [x; x] with the condition
    repeated, f32 mode: tests/test_model_gpu.py's BATCH_TOL for the 4-channel twin, 1e-5 of max|full|; the halves differ."""
    model, i, _ = hybrid
    x, cc, t = i["x"].to(gpu), i["cc"].to(gpu), i["t"].to(gpu)
    twin_cond = model.get_learned_conditioning(torch.cat([i["c"], i["uc"]]).to(gpu))
    model.set_concat_cond(cc)
    try:
        twin = model.apply_model_cfg_twin(x, t, twin_cond)
        full = model.apply_model(torch.cat([x, x]), torch.cat([t, t]), twin_cond)
        one = model.set_concat_cond(cc[:1]).apply_model_cfg_twin(x[:1], t[:1], model.get_learned_conditioning(
            torch.cat([i["c"][:16], i["uc"][:16]]).to(gpu)))
    finally:
        model.set_concat_cond(None)
    scale = full.abs().max().item()
    err = (twin - full).abs().max().item() / scale
    report("hybrid tiny_unet apply_model_cfg_twin vs apply_model(cat) [f32]", err, scale, 1e-5)
    assert twin.shape == (4, 4, 16, 16) and err <= 1e-5, err
    assert (twin[:2] - twin[2:]).abs().max().item() > 1e-3 * scale
    assert (one[0] - twin[0]).abs().max().item() <= 1e-5 * scale


def test_hybrid_sampler_run_and_concat_cond(gpu, hybrid):
    """The samplers stay unaware of the hybrid condition: an inpainting run (strength, mask, fused blend, finish) on the
    9-channel model is finite, keeps x0 where the mask says so, and follows the concatenated condition."""
    from adaface_amd.img2img import finish
    from adaface_amd.noise import PhiloxNoise
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    model, i, _ = hybrid
    g = torch.Generator().manual_seed(33)
    x0 = torch.randn(2, 4, 16, 16, generator=g).to(gpu)
    keep = (torch.rand(2, 1, 16, 16, generator=g) > 0.5).float().to(gpu)
    c, uc = model.get_learned_conditioning(i["c"].to(gpu)), model.get_learned_conditioning(i["uc"].to(gpu))
    outs = []
    try:
        for cc in (i["cc"], -i["cc"]):
            model.set_concat_cond(cc.to(gpu))
            lat, _ = DPMSolverSampler(model).sample(S=6, batch_size=2, shape=[4, 16, 16], conditioning=c, unconditional_conditioning=uc,
                                                    guidance_scale=3.0, verbose=False, x0=x0, mask=keep, strength=0.5,
                                                    fused_blend=True, noise_source=PhiloxNoise(SEED))
            outs.append(finish(lat, x0, keep))
    finally:
        model.set_concat_cond(None)
    for o in outs:
        assert torch.isfinite(o).all() and torch.equal(o * keep, x0 * keep)
    assert not torch.equal(outs[0], outs[1])
