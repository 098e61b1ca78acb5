"""CPU tests of regional prompts (adaface_amd/regions.py, af_region_attn.hip's host side): parsing, box -> area-fraction masks,
build_weights / pyramid / active_pairs on hand cases, the plan query, the refusals that need no device, the ABI surface, the
CLI's exclusions, and the reference restatement itself on the oracle (tests/region_ref.py)."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import region_cases as RC  # noqa: E402
import region_ref as RR  # noqa: E402
from adaface_amd import regions as RG  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402


# ---- parsing and masks --------------------------------------------------------------------------------------------------
def test_parse_box():
    assert RG.parse_box("0,0,0.5,1") == (0.0, 0.0, 0.5, 1.0, 1.0)
    assert RG.parse_box("0.25,0.5,1,0.75:0.3") == (0.25, 0.5, 1.0, 0.75, 0.3)
    for bad in ("0,0,1", "0,0,1,1,1", "a,0,1,1", "0.5,0,0.5,1", "0,0,1.5,1", "-0.1,0,1,1", "0,0,1,1:-1", "0,0,1,1:nan",
                "0,0,1,1:x", "0,0.6,1,0.4"):
        with pytest.raises(ValueError):
            RG.parse_box(bad)


def test_boxes_become_area_fractions():
    """Boxes on cell edges give 0 / 1 exactly; a box edge in the middle of a cell gives that cell one half (one quarter in a
    corner); the weight scales the mask."""
    m = RG.masks_from_boxes(["0,0,0.5,1", "0.25,0.25,0.75,0.75:0.5"], 8, 8)
    assert m.dtype == torch.float64 and tuple(m.shape) == (2, 8, 8)
    want0 = torch.zeros(8, 8, dtype=torch.float64)
    want0[:, :4] = 1.0
    assert torch.equal(m[0], want0)
    want1 = torch.zeros(8, 8, dtype=torch.float64)
    want1[2:6, 2:6] = 0.5
    assert torch.equal(m[1], want1)
    # half cells: x from 1.5 to 2.5 cells of 4, y the first 0.5 cell
    h = RG.masks_from_boxes([(0.375, 0.0, 0.625, 0.125, 1.0)], 4, 4)[0]
    want = torch.zeros(4, 4, dtype=torch.float64)
    want[0, 1] = want[0, 2] = 0.25
    assert torch.equal(h, want)
    assert float(RG.masks_from_boxes(["0,0,1,1:0.7"], 8, 16).min()) == 0.7


def test_mask_from_image_area_averages():
    img = torch.zeros(32, 64)
    img[:, :24] = 1.0
    m = RG.mask_from_image(img, 8, 8)      # 8 image columns per latent column: columns 0-2 full, the rest empty
    want = torch.zeros(8, 8, dtype=torch.float64)
    want[:, :3] = 1.0
    assert torch.allclose(m, want, atol=1e-15)
    img2 = torch.zeros(16, 16, dtype=torch.uint8)
    img2[:, :4] = 255
    m2 = RG.mask_from_image(img2, 8, 8)    # 2 image columns per latent column
    assert torch.allclose(m2[:, :2], torch.ones(8, 2, dtype=torch.float64)) and float(m2[:, 2:].abs().max()) == 0.0
    m3 = RG.mask_from_image(torch.ones(12, 12), 8, 8)      # no whole ratio: a constant image stays constant
    assert torch.allclose(m3, torch.ones(8, 8, dtype=torch.float64), atol=1e-15)
    with pytest.raises(ValueError):
        RG.mask_from_image(-torch.ones(8, 8), 8, 8)


def test_build_weights_and_concat_contexts():
    masks = RG.masks_from_boxes(["0,0,0.5,1", "0.5,0,1,1"], 8, 16)
    w = RG.build_weights(masks, 0.2, B=2, legs=2)
    assert w.dtype == torch.float32 and tuple(w.shape) == (4, 3, 8, 16)
    assert torch.equal(w[0], w[1]) and float(w[0, 0].min()) == float(w[0, 0].max()) == pytest.approx(0.2)
    assert torch.equal(w[0, 1], masks[0].float()) and torch.equal(w[1, 2], masks[1].float())
    unc = torch.zeros(3, 8, 16)
    unc[0] = 1.0
    assert torch.equal(w[2], unc) and torch.equal(w[3], unc)
    assert tuple(RG.build_weights(masks, 0.0, B=1, legs=1).shape) == (1, 3, 8, 16)
    per = RG.build_weights(torch.stack([masks, masks.flip(0)]), 0.5, B=2)
    assert torch.equal(per[1, 1], masks[1].float())
    for bad in (dict(region_masks=-masks), dict(region_masks=masks * float("nan")), dict(region_masks=masks, base_weight=-0.1),
                dict(region_masks=masks, base_weight=float("inf")), dict(region_masks=masks[:, :7]), dict(region_masks=masks, legs=3),
                dict(region_masks=torch.zeros(8, 8, 16))):
        with pytest.raises(ValueError):
            RG.build_weights(**bad)
    g = torch.Generator().manual_seed(1)
    c = [torch.randn(32, 77, 64, generator=g) for _ in range(3)]
    uc = torch.randn(32, 77, 64, generator=g)
    cat = RG.concat_contexts(c, uc)
    assert tuple(cat.shape) == (64, 231, 64)
    assert torch.equal(cat[:32, 77:154], c[1]) and torch.equal(cat[32:, 154:], uc) and torch.equal(cat[32:, :77], uc)
    assert torch.equal(RG.concat_contexts(c), cat[:32])
    with pytest.raises(ValueError):
        RG.concat_contexts([c[0], c[1][:, :76]])
    with pytest.raises(ValueError):
        RG.concat_contexts(c, uc[:16])


def test_pyramid_and_active_pairs_on_hand_cases():
    m = torch.zeros(1, 2, 8, 8)
    m[0, 0] = 1.0
    m[0, 1, :, :4] = 3.0                  # left half: (1/4, 3/4); right half: (1, 0)
    m[0, :, 0, 7] = 0.0                   # one pixel with no weight at all -> (1, 0) at level 0
    m[0, 1, 4:, 4] = 1.0                  # one column of the right half in the lower rows
    pyr = RG.pyramid(m)
    assert [tuple(p.shape) for p in pyr] == [(1, 2, 8, 8), (1, 2, 4, 4), (1, 2, 2, 2), (1, 2, 1, 1)]
    assert torch.equal(pyr[0][0, :, 3, 1], torch.tensor([0.25, 0.75], dtype=torch.float64))
    assert torch.equal(pyr[0][0, :, 0, 7], torch.tensor([1.0, 0.0], dtype=torch.float64))
    assert torch.equal(pyr[0][0, :, 5, 4], torch.tensor([0.5, 0.5], dtype=torch.float64))
    # level 1, cell (0, 3): region 0's box holds 3 of 4 ones (mean 3/4), region 1's none
    assert torch.equal(pyr[1][0, :, 0, 3], torch.tensor([1.0, 0.0], dtype=torch.float64))
    # level 1, cell (2, 2) = rows 4-5, columns 4-5: a_0 = 1, a_1 = 2/4
    assert torch.equal(pyr[1][0, :, 2, 2], torch.tensor([1.0 / 1.5, 0.5 / 1.5], dtype=torch.float64))
    # level 3: a_0 = 63/64, a_1 = (32 * 3 + 4) / 64
    a0, a1 = 63.0 / 64.0, 100.0 / 64.0
    assert torch.allclose(pyr[3][0, :, 0, 0], torch.tensor([a0 / (a0 + a1), a1 / (a0 + a1)], dtype=torch.float64), rtol=1e-15)
    for p in pyr:
        assert torch.allclose(p.sum(dim=1), torch.ones_like(p[:, 0]), rtol=1e-15)
    # all-zero map: the base region everywhere
    z = RG.pyramid(torch.zeros(2, 3, 8, 8))
    assert all(bool((p[:, 0] == 1).all()) and bool((p[:, 1:] == 0).all()) for p in z)
    # active bits, row-major pixels: level 0 has 64 queries = 2 blocks (rows 0-3, rows 4-7), both see both regions
    assert RG.active_pairs(pyr[0]).tolist() == [[3, 3]]
    m2 = torch.zeros(1, 3, 8, 8)
    m2[0, 0, :4] = 1.0                    # block 0: region 0 only
    m2[0, 2, 4:] = 1.0                    # block 1: region 2 only
    p2 = RG.pyramid(m2)
    assert RG.active_pairs(p2[0]).tolist() == [[1, 4]]
    assert RG.active_pairs(p2[1]).tolist() == [[5]]           # 16 queries, one block
    assert RG.active_pairs(p2[0].reshape(1, 3, 64)[:, :, :33]).tolist() == [[1, 4]]
    for bad in (torch.ones(1, 9, 8, 8), torch.ones(1, 2, 8, 12), -torch.ones(1, 2, 8, 8), torch.full((1, 2, 8, 8), float("inf")),
                torch.ones(2, 8, 8)):
        with pytest.raises(ValueError):
            RG.pyramid(bad)


def test_level_offsets():
    w_off, b_off, n_w, n_b = RG.level_offsets(3, 2, 16, 24)
    assert w_off == [0, 3 * 2 * 384, 3 * 2 * (384 + 96), 3 * 2 * (384 + 96 + 24)] and n_w == 3 * 2 * (384 + 96 + 24 + 6)
    assert b_off == [0, 3 * 12, 3 * 15, 3 * 16] and n_b == 3 * 17


# ---- the library's host side --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from adaface_amd import _lib, build
    if not _lib.lib_path().exists():
        build.build(verbose=False)
    return _lib.load()


def test_abi_surface():
    from adaface_amd import _lib, build
    text = (ROOT / "include" / "adaface_hip.h").read_text()
    for s in ("af_set_regions", "af_region_state", "af_region_plan_query", "af_region_attn_launches", "af_op_region_weights",
              "af_op_region_attention"):
        assert re.search(rf"\b{s}\s*\(", text) and s in _lib.EXPORTED_SYMBOLS, s
    assert "af_region_attn.hip" in build.SOURCES
    assert (ROOT / "adaface_amd" / "csrc" / "af_region_attn.hip").exists()


def test_plan_query(lib):
    """dtype x dh x T x R: fused for the 16-bit types, the kernel's head dims and T <= 96; the composition for f32, longer
    segments and the attention kernels' other head dims; refused for R outside 1 .. 8, no key, a head dim no kernel takes."""
    from adaface_amd import _lib
    fused_dh = (32, 40, 64, 80, 128, 160)
    try:
        for dtype in ("bf16", "f16", "f32"):
            for dh in (8, 16, 24, 32, 40, 48, 64, 80, 128, 160, 256):
                for T in (0, 1, 77, 96, 97, 154):
                    for R in (0, 1, 3, 8, 9):
                        got = RG.plan_query(dtype, dh, T, R)
                        if R < 1 or R > 8 or T < 1 or dh not in (8, 16) + fused_dh:
                            want = "refused"
                        elif dtype != "f32" and T <= 96 and dh in fused_dh:
                            want = "fused"
                        else:
                            want = "composition"
                        assert got == want, (dtype, dh, T, R, got)
        _lib.set_knob("region_fused", 0)
        assert RG.plan_query("bf16", 40, 77, 3) == "composition" and RG.plan_query("bf16", 40, 77, 9) == "refused"
    finally:
        _lib.reset_knobs()
    assert RG.plan_query("bf16", 40, 77, 3) == "fused"
    v = C.c_int(-1)
    assert lib.af_knob_get(b"region_fused", C.byref(v)) == 0 and v.value == 1
    assert lib.af_region_plan_query(7, 40, 77, 3, C.byref(C.c_int64())) != 0
    assert lib.af_region_plan_query(0, 40, 77, 3, None) != 0


def test_host_refusals(lib):
    """Null handles and null arguments are refused before any device is touched; the launch counter reads."""
    assert lib.af_set_regions(None, None, 1, 1, 8, 8, None) != 0
    assert b"null handle" in lib.af_last_error()
    assert lib.af_region_state(None, (C.c_int * 4)()) != 0
    assert lib.af_op_region_weights(None, 1, 1, 8, 8, None, None, None) != 0
    assert lib.af_op_region_attention(0, None, None, None, None, None, 1, 32, 1, 77, 8, 40, 0.1, 0, 0, None) != 0
    assert lib.af_region_attn_launches() >= 0


def test_engine_and_module_argument_checks():
    """UNetModel.set_regions validates on the host: shape, sign, finiteness, map sides, region count."""
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    cfg = O.TINY_UNET
    net = instantiate_from_config(tiny_config()["model"]["params"]["unet_config"])
    assert net.regions is None
    for bad in (torch.ones(3, 8, 8), -torch.ones(1, 2, 8, 8), torch.full((1, 2, 8, 8), float("nan")), torch.ones(1, 2, 8, 12),
                torch.ones(1, 9, 8, 8)):
        with pytest.raises(ValueError):
            net.set_regions(bad)
    w = torch.ones(2, 3, 16, 16)
    assert net.set_regions(w) is net and tuple(net.regions.shape) == (2, 3, 16, 16)
    x, t, ctx = torch.zeros(1, 4, 16, 16), torch.zeros(1, dtype=torch.long), torch.zeros(32, 231, cfg.context_dim)
    with pytest.raises(NotImplementedError):
        net(x, t, ctx, cfg_pag=True)
    with pytest.raises(NotImplementedError):
        net(x, t, ctx, tgate="capture")
    assert net.set_regions(None).regions is None


# ---- the CLI ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", [["--pag_scale", "3.0"], ["--tgate", "5"], ["--controlnet", "synthetic"]])
def test_cli_exclusions(other):
    """--regions with PAG, T-GATE or a ControlNet: one error that names both options, before any model is built."""
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "stable_txt2img.py"), "--regions", "synthetic:2", *other],
                       capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode != 0
    assert "--regions" in r.stderr and other[0] in r.stderr, r.stderr[-400:]


# ---- the reference on the oracle ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_case():
    cfg = O.TINY_UNET
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=11)
    g = torch.Generator().manual_seed(5)
    x, t = torch.randn(2, 4, 16, 16, generator=g), torch.tensor([981, 500])
    ctx = torch.randn(2 * 16, 3 * 77, cfg.context_dim, generator=g)
    return cfg, sd, x, t, ctx


def test_reference_on_the_oracle(oracle_case):
    """TINY_UNET, a 2 x 16 x 16 latent, R = 3, T = 77.  All weight on region 1 is the plain oracle on segment 1, exactly; the
    regional result (base 0.2 + a hard and a soft region, tests/region_cases.py) is far from the joint softmax over all 231
    keys and from segment 0 alone, so a build that ignores regions fails every model test by an order of magnitude."""
    cfg, sd, x, t, ctx = oracle_case
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    with torch.no_grad():
        one = torch.zeros(2, 3, 16, 16)
        one[:, 1] = 2.5
        with RR.patched(one, 3, (16, 16)):
            got = O.unet_forward(sd, cfg, x, t, ctx)
        seg1 = O.unet_forward(sd, cfg, x, t, ctx[:, 77:154].contiguous())
        assert torch.equal(got, seg1)
        m = RC.model_maps(2, 16, 16, 1)
        with RR.patched(m, 3, (16, 16)):
            ref = O.unet_forward(sd, cfg, x, t, ctx)
        joint = O.unet_forward(sd, cfg, x, t, ctx)
        seg0 = O.unet_forward(sd, cfg, x, t, ctx[:, :77].contiguous())
    d_joint, d_seg0 = rel(joint, ref), rel(seg0, ref)
    print(f"regional vs joint softmax {d_joint:.3f}, vs segment 0 alone {d_seg0:.3f} (of max|ref|)")
    assert d_joint > 0.1 and d_seg0 > 0.1, (d_joint, d_seg0)


def test_operator_reference_reduces_to_plain_attention():
    """R = 1 and weight 1 is softmax(q k^T) v; a region with weight 0 and NaN rows leaves the result untouched."""
    q, k, v, w = RC.op_inputs((40, 77, 3, 64, 2, 1, 0))
    one = torch.ones(1, 1, 64)
    ref = RR.region_attention(q, k[:, :77], v[:, :77], one, 2, 1)
    qh, kh, vh = (t.double().reshape(1, -1, 2, 40).permute(0, 2, 1, 3) for t in (q, k[:, :77], v[:, :77]))
    plain = (torch.einsum("bhid,bhjd->bhij", qh, kh) * 40 ** -0.5).softmax(-1) @ vh
    assert torch.equal(ref, plain.permute(0, 2, 1, 3).reshape(1, 64, 80))
    w0 = torch.zeros(1, 3, 64)
    w0[:, 0] = 1.0
    kn = k.clone()
    kn[:, 77:] = float("nan")
    assert torch.equal(RR.region_attention(q, kn, v, w0, 2, 3), ref)
