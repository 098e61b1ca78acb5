"""ControlNet without a GPU: the parameter inventory and the residual plan against the reference restatement
(tests/controlnet_ref.py), the restatement's own invariants, the sensitivity condition that keeps the GPU tests honest, and the
host-side logic (window, scales, checkpoint key prefixes, command-line refusals)."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))
from oracle import ldm_oracle as O  # noqa: E402
import controlnet_ref as R  # noqa: E402

BF16_BAR = 3e-2          # TOL["bf16"] of tests/test_model_gpu.py


def _kw(cfg):
    return dict(in_channels=cfg.in_channels, model_channels=cfg.model_channels, num_res_blocks=cfg.num_res_blocks,
                attention_resolutions=cfg.attention_resolutions, channel_mult=cfg.channel_mult, num_heads=cfg.num_heads,
                context_dim=cfg.context_dim, transformer_depth=cfg.transformer_depth)


# ------------------------------------------------------------------ shapes and plan ------------------------------------
@pytest.mark.parametrize("cfg", [O.TINY_UNET, O.SD15_UNET], ids=["tiny", "sd15"])
def test_param_shapes_equal_the_reference_inventory(cfg):
    from adaface_amd import layout
    kw = {k: v for k, v in _kw(cfg).items() if k != "num_heads"}
    lay = {R.CONTROL_PREFIX + k: tuple(v) for k, v in layout.controlnet_param_shapes(**kw).items()}
    ref = {k: tuple(v) for k, v in R.param_shapes(cfg).items()}
    assert lay == ref
    assert sum(1 for k in lay if ".zero_convs." in k) == 2 * (R.n_residuals(cfg) - 1)
    assert "control_model.input_hint_block.14.weight" in lay and lay["control_model.input_hint_block.0.weight"] == (16, 3, 3, 3)
    assert not any(k.startswith(("control_model.output_blocks.", "control_model.out.")) for k in lay)


def test_sd15_plan_64():
    from adaface_amd.engine import control_plan
    plan = control_plan(_kw(O.SD15_UNET), 64, 64)
    shapes = [(320, 64)] * 3 + [(320, 32)] + [(640, 32)] * 2 + [(640, 16)] + [(1280, 16)] * 2 + [(1280, 8)] * 3 + [(1280, 8)]
    assert len(plan) == 13
    assert [(c, h) for c, h, w, _ in plan] == shapes and all(h == w for _, h, w, _ in plan)
    off = 0
    for c, h, w, o in plan:
        assert o == off
        off += c * h * w
    assert plan == R.plan(O.SD15_UNET, 64, 64)


def test_plan_of_a_non_square_latent_and_refusals():
    from adaface_amd import _lib
    from adaface_amd.engine import control_plan
    for cfg in (O.SD15_UNET, O.TINY_UNET):
        assert control_plan(_kw(cfg), 32, 16) == R.plan(cfg, 32, 16)
    assert control_plan(_kw(O.TINY_UNET), 32, 16)[-1][:3] == (256, 4, 2)
    with pytest.raises(_lib.AfError):
        control_plan(_kw(O.TINY_UNET), 12, 16)           # (not a multiple of 8: the three downsamples)


# ------------------------------------------------------------------ the restatement's own invariants ---------------------
@pytest.fixture(scope="module")
def tiny_case():
    cfg = O.TINY_UNET
    sd, csd = R.weights(cfg)
    x, t, ctx, hint = R.case(cfg, 2, 16, 16)
    res = R.control_forward(csd, cfg, x, t, ctx, hint)
    plain = O.unet_forward(sd, cfg, x, t, ctx)
    return dict(cfg=cfg, sd=sd, csd=csd, x=x, t=t, ctx=ctx, hint=hint, res=res, plain=plain)


def test_reference_zero_scales_is_the_plain_forward(tiny_case):
    c = tiny_case
    eps = R.controlled_unet_forward(c["sd"], c["cfg"], c["x"], c["t"], c["ctx"], c["res"], [0.0] * len(c["res"]))
    assert torch.equal(eps, c["plain"])


def test_reference_truncated_control_is_a_prefix(tiny_case):
    c = tiny_case
    assert len(c["res"]) == 13
    for k in (1, 2, 5, 12):
        part = R.control_forward(c["csd"], c["cfg"], c["x"], c["t"], c["ctx"], c["hint"], n_blocks=k)
        assert len(part) == k and all(torch.equal(a, b) for a, b in zip(part, c["res"]))
    for (cc, h, w, _), r in zip(R.plan(c["cfg"], 16, 16), c["res"]):
        assert tuple(r.shape) == (2, cc, h, w)


def test_reference_cond_only_leaves_the_second_leg(tiny_case):
    c = tiny_case
    cfg, x, t = c["cfg"], c["x"], c["t"]
    uc = torch.randn(c["ctx"].shape, generator=torch.Generator().manual_seed(9))
    x2, t2, ctx2 = torch.cat([x, x]), torch.cat([t, t]), torch.cat([c["ctx"], uc])
    plain2 = O.unet_forward(c["sd"], cfg, x2, t2, ctx2)
    eps = R.controlled_unet_forward(c["sd"], cfg, x2, t2, ctx2, c["res"], R.case_scales(cfg), cond_only=True)
    assert torch.equal(eps[2:], plain2[2:])
    assert not torch.equal(eps[:2], plain2[:2])


def test_sensitivity_control_moves_eps_far_above_the_bf16_bar(tiny_case):
    """The GPU tests compare controlled forwards at the bf16 bar: control must move eps by at least 10 bars on these inputs, or a
    forward that ignored the residuals would pass."""
    c = tiny_case
    eps = R.controlled_unet_forward(c["sd"], c["cfg"], c["x"], c["t"], c["ctx"], c["res"], R.case_scales(c["cfg"]))
    moved = float((eps - c["plain"]).abs().max() / c["plain"].abs().max())
    print(f"control moves eps by {moved:.3f} of max|eps|")
    assert moved >= 10 * BF16_BAR, moved
    # ... and every single residual matters on its own
    for i in range(len(c["res"])):
        s = [0.0] * len(c["res"])
        s[i] = 1.0
        e = R.controlled_unet_forward(c["sd"], c["cfg"], c["x"], c["t"], c["ctx"], c["res"], s)
        assert float((e - c["plain"]).abs().max()) > 0.0, i


def test_synthetic_weights_have_live_zero_convs():
    from adaface_amd import layout
    from adaface_amd.synth import synth_controlnet_state_dict, synth_hint
    kw = {k: v for k, v in _kw(O.TINY_UNET).items() if k != "num_heads"}
    shapes = layout.controlnet_param_shapes(**kw)
    sd = synth_controlnet_state_dict(shapes, seed=3, prefix="control_model.")
    assert set(sd) == {"control_model." + k for k in shapes}
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(shapes[k[len("control_model."):]])
        if ".zero_convs." in k or ".middle_block_out." in k:
            assert float(v.abs().max()) > 0.0, k
    again = synth_controlnet_state_dict(shapes, seed=3, prefix="control_model.")
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    h = synth_hint(2, 7, 64, 32)
    assert tuple(h.shape) == (2, 3, 64, 32) and float(h.min()) >= 0.0 and float(h.max()) <= 1.0
    # the product's draws move the reference's eps as far as the oracle's do (same condition as above)
    cfg = O.TINY_UNET
    usd, _ = R.weights(cfg)
    x, t, ctx, hint = R.case(cfg, 2, 16, 16)
    res = R.control_forward(sd, cfg, x, t, ctx, hint)
    plain = O.unet_forward(usd, cfg, x, t, ctx)
    eps = R.controlled_unet_forward(usd, cfg, x, t, ctx, res, [1.0] * len(res))
    assert float((eps - plain).abs().max() / plain.abs().max()) >= 10 * BF16_BAR


# ------------------------------------------------------------------ window, scales, files, command line ------------------
def test_window_logic_and_fraction_mapping():
    from adaface_amd.engine import check_control_window, control_active, control_window_from_fractions
    assert check_control_window(None) == (0, 999)
    assert check_control_window((200, 800)) == (200, 800)
    for bad in ((5,), (800, 200), "ab", 3):
        with pytest.raises(ValueError):
            check_control_window(bad)
    w = (200, 800)
    assert control_active(torch.tensor([200, 800]), w) and control_active(torch.tensor([500]), w)
    assert not control_active(torch.tensor([500, 801]), w) and not control_active(torch.tensor([199]), w)
    assert control_window_from_fractions(0.0, 1.0) == (0, 999)
    assert control_window_from_fractions(0.0, 0.5) == (500, 999)       # t_lo = 999 (1 - end), t_hi = 999 (1 - start)
    assert control_window_from_fractions(0.25, 1.0) == (0, 749)
    for bad in ((-0.1, 1.0), (0.0, 1.5), (0.6, 0.4), (True, 1.0)):
        with pytest.raises(ValueError):
            control_window_from_fractions(*bad)


def test_scales_validation():
    from adaface_amd.engine import check_control_scales
    assert check_control_scales(0.5, None, 13) == (0.5,) * 13
    guess = [0.825 ** (12 - i) for i in range(13)]
    assert check_control_scales(1.0, guess, 13) == tuple(guess)
    for bad in ([1.0] * 12, [1.0] * 14, [1.0] * 12 + [float("nan")], [1.0] * 12 + [float("inf")], [1.0] * 12 + ["a"]):
        with pytest.raises(ValueError):
            check_control_scales(1.0, bad, 13)
    for bad in (float("nan"), float("inf"), None, True):
        with pytest.raises(ValueError):
            check_control_scales(bad, None, 13)


def _tiny_ctor():
    return dict(image_size=32, hint_channels=3, use_spatial_transformer=True, legacy=False, **_kw(O.TINY_UNET))


def test_from_file_key_prefixes(tmp_path):
    from ldm.modules.diffusionmodules.controlnet import ControlNet
    cfg = O.TINY_UNET
    _, csd = R.weights(cfg)
    bare = {k[len(R.CONTROL_PREFIX):]: v for k, v in csd.items()}
    full = dict(csd)
    full["model.diffusion_model.time_embed.0.weight"] = torch.zeros(3)     # (a cldm checkpoint holds the other networks too)
    torch.save(full, tmp_path / "with_prefix.pth")
    torch.save({"state_dict": bare}, tmp_path / "bare.ckpt")
    nets = [ControlNet.from_file(tmp_path / n, **_tiny_ctor()) for n in ("with_prefix.pth", "bare.ckpt")]
    for net in nets:
        own = net.state_dict()
        assert set(own) == set(bare) and all(torch.equal(own[k], bare[k]) for k in bare)
        assert net._weights_dirty
    broken = {k: v for k, v in bare.items() if not k.startswith("zero_convs.3.")}
    torch.save(broken, tmp_path / "broken.pth")
    with pytest.raises(KeyError, match="zero_convs.3"):
        ControlNet.from_file(tmp_path / "broken.pth", **_tiny_ctor())
    with pytest.raises(NotImplementedError):
        ControlNet(**{**_tiny_ctor(), "use_scale_shift_norm": True})
    with pytest.raises(ValueError):
        nets[0].set_compute_dtype("fp8")


def test_unet_set_control_host_checks():
    from ldm.modules.diffusionmodules.controlnet import ControlNet
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    kw = dict(image_size=32, out_channels=4, use_spatial_transformer=True, **_kw(O.TINY_UNET))
    unet, net = UNetModel(**kw), ControlNet(**_tiny_ctor())
    hint = torch.rand(1, 3, 128, 128)
    unet.set_control(net, hint, scale=0.7, t_range=(100, 900), cond_only=True)
    assert unet.control["scales"] == (0.7,) * 13 and unet.control["window"] == (100, 900) and unet.control["cond_only"]
    unet.set_control(None)
    assert unet.control is None
    with pytest.raises(ValueError):
        unet.set_control(net, hint, scales=[1.0] * 12)
    with pytest.raises(ValueError):
        unet.set_control(net, torch.rand(1, 3, 100, 128))
    with pytest.raises(ValueError):
        unet.set_control(net, None)
    with pytest.raises(TypeError):
        unet.set_control(unet, hint)
    other = ControlNet(**{**_tiny_ctor(), "model_channels": 128})
    with pytest.raises(ValueError, match="model_channels"):
        unet.set_control(other, hint)


def test_cli_refusals_and_mapping(capsys):
    import stable_txt2img as cli
    opt = cli.parse_args(["--synthetic", "--controlnet", "synthetic:0.8", "--control_start", "0.2", "--control_end", "0.9"])
    assert opt.controlnet == ("synthetic", 0.8) and opt.control_t_range == (100, 799)
    opt = cli.parse_args(["--synthetic", "--controlnet", "cn.pth", "--control_image", "a.png", "--n_samples", "4"])
    assert opt.controlnet == ("cn.pth", 1.0) and opt.control_t_range == (0, 999) and not opt.control_cond_only
    for bad in (["--controlnet", "synthetic", "--pag_scale", "3"], ["--controlnet", "synthetic", "--tgate", "5"],
                ["--controlnet", "cn.pth"], ["--control_image", "a.png"], ["--control_cond_only"],
                ["--controlnet", "synthetic", "--control_start", "0.8", "--control_end", "0.2"],
                ["--controlnet", "synthetic", "--control_image", "a.png", "b.png", "--n_samples", "3"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["--synthetic"] + bad)
    capsys.readouterr()


def test_abi_is_documented():
    text = (ROOT / "INTEGRATION.md").read_text()
    for sym in ("af_control_set_hint", "af_control_forward", "af_unet_set_control", "af_control_plan_query", "af_control_stats",
                "af_op_control_add"):
        assert sym in text, sym
