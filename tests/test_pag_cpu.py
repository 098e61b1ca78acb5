"""CPU tests of perturbed-attention guidance and guidance rescale: the restatement of tests/pag_ref.py against the oracle's own
attention and a direct torch.std formula, the site names for the tiny and the SD-1.5 layout, the adaptive scale, the host-only plan
queries, the refusals that need no device, the new C symbols in header, binding and library, the samplers' refusals on a stub
model and the CLI flags."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import pag_ref as PR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

SYMS = ("af_set_pag", "af_pag_num_sites", "af_pag_site", "af_pag_plan_query", "af_unet_forward_pag", "af_guidance",
        "af_guidance_plan_query")
NAMES = {"mid": (6,), "down.blocks.0": (0, 1), "down.blocks.1": (2, 3), "down.blocks.2": (4, 5), "up.blocks.1": (7, 8, 9),
         "up.blocks.2": (10, 11, 12), "up.blocks.3": (13, 14, 15)}


# ------------------------------------------------------------------ the reference itself ----------------------------
def test_identity_attention_is_attention_with_a_diagonal_mask():
    """to_out(to_v(n)) equals the oracle's attention with -inf off the diagonal of the scores, in fp64"""
    g = torch.Generator().manual_seed(3)
    C, heads, N, B = 32, 2, 24, 3
    p = "blk.attn1"
    sd = {f"{p}.to_q.weight": torch.randn(C, C, generator=g, dtype=torch.float64),
          f"{p}.to_k.weight": torch.randn(C, C, generator=g, dtype=torch.float64),
          f"{p}.to_v.weight": torch.randn(C, C, generator=g, dtype=torch.float64),
          f"{p}.to_out.0.weight": torch.randn(C, C, generator=g, dtype=torch.float64),
          f"{p}.to_out.0.bias": torch.randn(C, generator=g, dtype=torch.float64)}
    n = torch.randn(B, N, C, generator=g, dtype=torch.float64)
    got = PR.identity_attention(sd, p, n)
    # the oracle's cross_attention with an additive mask: restated here around its own linears and softmax
    q, k, v = O._lin(sd, p + ".to_q", n), O._lin(sd, p + ".to_k", n), O._lin(sd, p + ".to_v", n)
    dh = C // heads
    split = lambda t: t.reshape(B, N, heads, dh).permute(0, 2, 1, 3)
    sim = torch.einsum("bhid,bhjd->bhij", split(q), split(k)) * dh ** -0.5
    mask = torch.full((N, N), float("-inf"), dtype=torch.float64)
    mask.fill_diagonal_(0.0)
    out = torch.einsum("bhij,bhjd->bhid", (sim + mask).softmax(dim=-1), split(v)).permute(0, 2, 1, 3).reshape(B, N, C)
    ref = O._lin(sd, p + ".to_out.0", out)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # and the unmasked oracle attention is something else
    assert float((O.cross_attention(sd, p, n, None, None, heads) - ref).abs().max()) > 1e-3


def test_patched_oracle_perturbs_only_the_given_legs():
    cfg = O.TINY_UNET
    sd = O.synth_state_dict(O.unet_param_shapes(cfg), seed=11)
    g = torch.Generator().manual_seed(400)
    c, uc = (torch.randn(16, 77, cfg.context_dim, generator=g) for _ in range(2))
    x = torch.randn(1, 4, 16, 16, generator=g)
    x3, t3, ctx3 = torch.cat([x] * 3), torch.tensor([500] * 3), torch.cat([c, uc, c])
    with torch.no_grad():
        plain = O.unet_forward(sd, cfg, x3, t3, ctx3)
        with PR.patched(PR.sites_of(cfg, ("mid",)), slice(2, 3)):
            mid = O.unet_forward(sd, cfg, x3, t3, ctx3)
        with PR.patched((), slice(2, 3)):
            none = O.unet_forward(sd, cfg, x3, t3, ctx3)
    assert torch.equal(none, plain)
    assert float((plain[2] - plain[0]).abs().max() / plain[0].abs().max()) < 1e-5      # (leg 2 unperturbed is leg 0, up to torch's batching)
    assert torch.equal(mid[:2], plain[:2])
    dev = float((mid[2] - mid[0]).abs().max() / mid[0].abs().max())
    assert dev > 5 * 2e-4, dev                       # f32's bar, five times: the middle block alone is visible to the f32 test


def test_rescale_restatement_against_torch_std():
    g = torch.Generator().manual_seed(5)
    ec, eu, ep = (torch.randn(3, 4, 8, 8, generator=g) * (i + 1) + 0.3 * i for i in range(3))
    w, s, phi = 7.5, 3.0, 0.7
    got, f = PR.guidance(ec, eu, ep, w, s, phi)
    e = eu.double() + w * (ec.double() - eu.double()) + s * (ec.double() - ep.double())
    for b in range(3):
        fb = torch.std(ec[b].double()) / torch.std(e[b])
        assert abs(float(f[b] - fb)) <= 1e-13 * float(fb)
        ref = e[b] * (phi * fb + 1 - phi)
        assert float((got[b] - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    # phi = 1 gives the conditional prediction's deviation; phi = 0 leaves e alone and computes no factor
    full, _ = PR.guidance(ec, eu, ep, w, s, 1.0)
    assert torch.allclose(full.reshape(3, -1).std(dim=1), ec.double().reshape(3, -1).std(dim=1), rtol=1e-12, atol=0)
    off, f0 = PR.guidance(ec, eu, ep, w, s, 0.0)
    assert f0 is None and torch.equal(off, e)
    # absent legs drop their term
    assert torch.equal(PR.guidance(ec, eu, None, w, s, 0.0)[0], eu.double() + w * (ec.double() - eu.double()))
    assert torch.equal(PR.guidance(ec, None, ep, w, s, 0.0)[0], ec.double() + s * (ec.double() - ep.double()))


@pytest.mark.parametrize("cfg", [O.SD15_UNET, O.TINY_UNET], ids=["sd15", "tiny"])
def test_names_and_sites(cfg):
    from adaface_amd.engine import pag_layout, pag_sites_of
    lay = pag_layout(cfg)
    assert lay["n_sites"] == 16 and lay["n_input_blocks"] == 12 and lay["names"] == NAMES
    assert [b for b, _ in PR.site_blocks(cfg)] == list(lay["blocks"])
    assert lay["blocks"] == (1, 2, 4, 5, 7, 8, 12, 16, 17, 18, 19, 20, 21, 22, 23, 24)
    for name, sites in NAMES.items():
        assert pag_sites_of(cfg, (name,)) == sites == PR.sites_of(cfg, (name,))
    assert pag_sites_of(cfg, None) == () and pag_sites_of(cfg, ()) == ()
    assert pag_sites_of(cfg, "mid") == (6,) and pag_sites_of(cfg, 3) == (3,)
    assert pag_sites_of(cfg, ("mid", "up.blocks.1", 7, 0)) == (0, 6, 7, 8, 9) == PR.sites_of(cfg, ("mid", "up.blocks.1", 7, 0))
    for bad in (("middle",), ("up.blocks.0",), (16,), (-1,), (True,), (1.5,), (None,)):
        with pytest.raises(ValueError, match="PAG"):
            pag_sites_of(cfg, bad)


def test_names_follow_the_block_structure():
    """Not hard-coded to 16: another depth, other attention resolutions, two levels."""
    from adaface_amd.engine import pag_layout
    lay = pag_layout(dict(channel_mult=(1, 2, 4, 4), num_res_blocks=2, attention_resolutions=(4, 2, 1), transformer_depth=2))
    assert lay["n_sites"] == 32 and lay["names"]["mid"] == (12, 13) and lay["names"]["down.blocks.0"] == (0, 1, 2, 3)
    lay = pag_layout(dict(channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(2,)))
    assert lay["names"] == {"down.blocks.1": (0,), "mid": (1,), "up.blocks.0": (2, 3)} and lay["n_input_blocks"] == 4
    assert lay["blocks"] == (3, 4, 5, 6) and lay["ds"] == (2, 2, 2, 2)


def test_adaptive_scale():
    from adaface_amd.engine import pag_scale_at
    for f in (PR.pag_scale_at, pag_scale_at):
        assert f(999, 3.0, 0.0) == 3.0 and f(1, 3.0, 0.0) == 3.0
        assert f(1000, 3.0, 0.01) == 3.0
        assert abs(f(900, 3.0, 0.01) - 2.0) < 1e-12 and abs(f(701, 3.0, 0.01) - 0.01) < 1e-12
        assert f(700, 3.0, 0.01) == 0.0 and f(1, 3.0, 0.01) == 0.0        # the clamp
    assert all(PR.pag_scale_at(t, 2.5, 0.004) == pag_scale_at(t, 2.5, 0.004) for t in range(1, 1000, 37))


def test_plan_of_the_forward():
    """The first block with a set site and the input blocks that run on two legs, from the constructor arguments alone (the
    handle's own query is compared with this on the GPU)."""
    from adaface_amd.engine import pag_plan
    for cfg in (O.SD15_UNET, O.TINY_UNET):
        assert pag_plan(cfg, ("mid",)) == {"first_block": 12, "two_leg_blocks": 12, "two_leg_blocks_reuse": 0}
        assert pag_plan(cfg, ("mid",), depth=3) == {"first_block": 12, "two_leg_blocks": 12, "two_leg_blocks_reuse": 3}
        assert pag_plan(cfg, ("down.blocks.2",)) == {"first_block": 7, "two_leg_blocks": 7, "two_leg_blocks_reuse": 0}
        assert pag_plan(cfg, ("down.blocks.2",), depth=9)["two_leg_blocks_reuse"] == 7
        assert pag_plan(cfg, ("mid", "up.blocks.1"))["two_leg_blocks"] == 12
        assert pag_plan(cfg, ("up.blocks.3",)) == {"first_block": 22, "two_leg_blocks": 12, "two_leg_blocks_reuse": 0}
        assert pag_plan(cfg, (0,)) == {"first_block": 1, "two_leg_blocks": 1, "two_leg_blocks_reuse": 0}
        assert pag_plan(cfg, ("mid",), share_prefix=False)["two_leg_blocks"] == 0
        assert pag_plan(cfg, ()) == {"first_block": -1, "two_leg_blocks": 0, "two_leg_blocks_reuse": 0}


# ------------------------------------------------------------------ the library, host only --------------------------
def test_header_binding_and_library_have_the_symbols():
    from adaface_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "adaface_hip.h").read_text(), flags=re.S)
    if not _lib.lib_path().exists():
        build.build(verbose=False)
    exported = subprocess.run(["nm", "-D", "--defined-only", os.fspath(_lib.lib_path())], check=True, capture_output=True,
                              text=True).stdout
    for s in SYMS:
        assert re.search(rf"\bint\s+{s}\s*\(", text), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert re.search(rf"\sT\s+{s}$", exported, flags=re.M), s
    assert "af_guidance.hip" in build.SOURCES
    assert re.search(r"AF_UNET_FORM_PLAIN\s*=\s*0,\s*AF_UNET_FORM_TWIN\s*=\s*1,\s*AF_UNET_FORM_PAG\s*=\s*2", text)
    lib = _lib.load()
    assert lib.af_version() >= 2
    # null handles and null outputs are refused on the host, with a message and without a device
    assert lib.af_set_pag(None, None, 0) == -1 and b"af_set_pag" in lib.af_last_error()
    assert lib.af_pag_site(None, 0, None) == -1 and b"af_pag_site" in lib.af_last_error()
    assert lib.af_pag_plan_query(None, 0, None) == -1 and b"af_pag_plan_query" in lib.af_last_error()
    assert lib.af_pag_num_sites(None) == 0
    assert lib.af_unet_forward_pag(None, None, None, None, 3, 16, 16, None) == -1
    assert lib.af_guidance_plan_query(1, 16, 0, None) == -1
    assert lib.af_guidance(None, None, None, 1, 16, 1.0, 0.0, 0.0, None, None, None) == -1
    # the knob of the shared prefix: on by default
    import ctypes as C
    v = C.c_int(-1)
    assert lib.af_knob_get(b"pag_share_prefix", C.byref(v)) == 0 and v.value == 1


def test_guidance_plan_query():
    from adaface_amd import _lib
    q = _lib.guidance_plan_query
    for n in (1, 3):
        for per in (2, 5, 255, 256, 257, 1024, 1027, 16384, 16385):
            chunks = -(-per // 256)
            assert q(n, per, False) == {"kernel": "combine", "launches": 1, "chunks": chunks, "partial_bytes": 0}, (n, per)
            if per <= 1024:
                assert q(n, per, True) == {"kernel": "single", "launches": 1, "chunks": chunks, "partial_bytes": 0}, (n, per)
            else:
                assert q(n, per, True) == {"kernel": "chunked", "launches": 2, "chunks": chunks, "partial_bytes": chunks * 16}, (n, per)
    assert q(8, 16384, True)["chunks"] == 64
    for bad in ((0, 16), (-1, 16), (1, 1), (1, 0), (1, 2 ** 31 + 1), (2 ** 31, 4096)):
        for on in (False, True):
            with pytest.raises(_lib.AfError, match="guidance"):
                q(*bad, on)


# ------------------------------------------------------------------ the modules and the samplers --------------------
def test_set_pag_on_the_modules():
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    unet = instantiate_from_config(tiny_config()["model"]["params"]["unet_config"])
    assert unet.pag == ()
    with pytest.raises(ValueError, match="PAG"):
        unet.set_pag(("middle",))
    with pytest.raises(ValueError, match="PAG"):
        unet.set_pag((16,))
    assert unet.pag == ()
    assert unet.set_pag(("mid",)) is unet and unet.pag == (6,)
    assert unet.set_pag(("mid", "up.blocks.1", 0)).pag == (0, 6, 7, 8, 9)
    for dt in ("f16", "fp8", "f32", "bf16"):                            # every compute dtype keeps it
        assert unet.set_compute_dtype(dt).pag == (0, 6, 7, 8, 9)
    assert unet.set_freeu(1, 1.2, 1.4, 0.9, 0.2).pag == (0, 6, 7, 8, 9) and unet.set_token_merging(0.5).pag == (0, 6, 7, 8, 9)
    assert unet.set_pag(None).pag == () and unet.set_pag(()).pag == ()
    # no layer set: the three-leg forward is refused before it needs a device
    with pytest.raises(ValueError, match="set_pag"):
        unet.forward(torch.zeros(1, 4, 16, 16), torch.tensor([1]), torch.zeros(32, 77, 64), cfg_pag=True)
    with pytest.raises(ValueError, match="cfg_pag and cfg_twin"):
        unet.set_pag(("mid",)).forward(torch.zeros(1, 4, 16, 16), torch.tensor([1]), torch.zeros(32, 77, 64), cfg_pag=True, cfg_twin=True)


class _Stub:
    """A model that must never be called: the samplers refuse before their first step."""
    num_timesteps = 1000
    parameterization = "eps"

    def __init__(self, pag=(), with_entry=True):
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
        self.betas = betas.float()
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0).float()
        self.alphas_cumprod_prev = torch.cat([torch.ones(1), self.alphas_cumprod[:-1]])
        self.sqrt_one_minus_alphas_cumprod = torch.sqrt(1.0 - self.alphas_cumprod)
        self.device = torch.device("cpu")
        self.pag = pag
        if with_entry:
            self.apply_model_cfg_pag = self._never

    def _never(self, *a, **k):
        raise AssertionError("the model was called")

    apply_model = apply_model_cfg_twin = _never


def _samplers():
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    return {"ddim": (DDIMSampler, "guidance_scale"), "plms": (PLMSSampler, "unconditional_guidance_scale"),
            "dpm": (DPMSolverSampler, "guidance_scale")}


@pytest.mark.parametrize("name", ["ddim", "plms", "dpm"])
def test_samplers_refuse_as_specified(name):
    cls, gkey = _samplers()[name]
    c, uc = torch.zeros(16, 77, 64), torch.zeros(16, 77, 64)
    kw = dict(S=4, batch_size=1, shape=[4, 16, 16], conditioning=c, verbose=False, x_T=torch.zeros(1, 4, 16, 16), **{gkey: 5.0})
    with pytest.raises(ValueError, match="unconditional_conditioning"):           # PAG without an unconditional leg
        cls(_Stub(pag=(6,))).sample(pag_scale=3.0, **kw)
    with pytest.raises(ValueError, match="set_pag"):                              # a model without set sites
        cls(_Stub(pag=())).sample(pag_scale=3.0, unconditional_conditioning=uc, **kw)
    with pytest.raises(ValueError, match="apply_model_cfg_pag"):                  # a model without the entry point
        cls(_Stub(pag=(6,), with_entry=False)).sample(pag_scale=3.0, unconditional_conditioning=uc, **kw)
    for bad in (dict(pag_scale=-1.0), dict(guidance_rescale=1.5), dict(guidance_rescale=-0.1), dict(pag_adaptive_scale=-0.01),
                dict(pag_scale="3")):
        with pytest.raises(ValueError):
            cls(_Stub(pag=(6,))).sample(unconditional_conditioning=uc, **bad, **kw)
    if name == "ddim":
        with pytest.raises(ValueError, match="unconditional_conditioning"):
            s = cls(_Stub(pag=(6,)))
            s.make_schedule(4, verbose=False)
            s.decode(torch.zeros(1, 4, 16, 16), c, 2, guidance_scale=5.0, pag_scale=3.0)


def test_helper_is_not_entered_when_off(monkeypatch):
    """pag_scale = 0 and guidance_rescale = 0: the samplers make the calls they make without the feature."""
    from adaface_amd.ldm.models.diffusion import guidance as G
    assert not G.is_on(0.0, 0.0) and G.is_on(3.0, 0.0) and G.is_on(0.0, 0.7)
    assert G.check_args() == (0.0, 0.0, 0.0) and G.check_args(3, 0.01, 1) == (3.0, 0.01, 1.0)

    def boom(*a, **k):
        raise AssertionError("guided_eps was entered")
    monkeypatch.setattr(G, "guided_eps", boom)
    calls = []

    class Model(_Stub):
        def apply_model(self, x, t, c, **k):
            calls.append("single")
            raise RuntimeError("stop here")
        apply_model_cfg_twin = apply_model

    for name, (cls, gkey) in _samplers().items():
        with pytest.raises(RuntimeError, match="stop here"):
            cls(Model()).sample(S=4, batch_size=1, shape=[4, 16, 16], conditioning=torch.zeros(16, 77, 64), verbose=False,
                                x_T=torch.zeros(1, 4, 16, 16), **{gkey: 5.0})
    assert calls == ["single"] * 3


def test_cli_flags_parse(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("stable_txt2img_cli_pag", ROOT / "scripts" / "stable_txt2img.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    opt = cli.parse_args(["--synthetic"])
    assert opt.pag_scale == 0.0 and opt.pag_layers is None and opt.pag_adaptive_scale == 0.0 and opt.guidance_rescale == 0.0
    opt = cli.parse_args(["--synthetic", "--pag_scale", "3"])
    assert opt.pag_scale == 3.0 and opt.pag_layers == ["mid"]
    opt = cli.parse_args(["--synthetic", "--pag_scale", "3", "--pag_layers", "mid", "up.blocks.1", "7", "--pag_adaptive_scale", "0.01",
                          "--guidance_rescale", "0.7", "--deep_cache", "3", "--dpm_solver", "--freeu", "1.2", "1.4", "0.9", "0.2",
                          "--gpus", "2", "--tome", "0.5"])
    assert opt.pag_layers == ["mid", "up.blocks.1", 7] and opt.pag_adaptive_scale == 0.01 and opt.guidance_rescale == 0.7
    for dt in ("bf16", "f32", "fp16", "fp8"):
        assert cli.parse_args(["--synthetic", "--dtype", dt, "--pag_scale", "2.5", "--guidance_rescale", "1"]).pag_scale == 2.5
    assert cli.parse_args(["--synthetic", "--plms", "--pag_scale", "3"]).plms
    assert cli.parse_args(["--synthetic", "--guidance_rescale", "0.5"]).guidance_rescale == 0.5          # rescale alone
    assert cli.parse_args(["--synthetic", "--pag_scale", "3", "--pag_layers", "down.blocks.1", "--tome", "0.5"]).tome == 0.5
    for bad in (["--pag_layers", "mid"], ["--pag_adaptive_scale", "0.1"], ["--pag_scale", "-1"], ["--guidance_rescale", "1.5"],
                ["--pag_scale", "3", "--pag_layers", "middle"], ["--pag_scale", "3", "--pag_layers", "16"],
                ["--pag_scale", "3", "--pag_layers", "down.blocks.0", "--tome", "0.5"],
                ["--pag_scale", "3", "--pag_layers", "up.blocks.2", "--tome", "0.5", "--tome_max_downsample", "2"],
                ["--pag_scale", "x"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["--synthetic"] + bad)
        assert e.value.code == 2, bad
    assert "--pag_layers" in capsys.readouterr().err
