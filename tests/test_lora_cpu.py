"""CPU tests of the LoRA adapters: key-name mapping, file reading, the overlay's bookkeeping on a module without an engine, the
command line, and the restated layout formula of tests/lora_ref.py against a hand-written example.  No GPU is needed."""
import re
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import lora_ref as LR  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402


def _cfg_dict(cfg):
    return dict(in_channels=cfg.in_channels, model_channels=cfg.model_channels, out_channels=cfg.out_channels,
                num_res_blocks=cfg.num_res_blocks, attention_resolutions=list(cfg.attention_resolutions),
                channel_mult=list(cfg.channel_mult), context_dim=cfg.context_dim, transformer_depth=cfg.transformer_depth)


def _tiny_unet():
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    c = O.TINY_UNET
    return UNetModel(image_size=16, use_spatial_transformer=True, num_heads=c.num_heads, **_cfg_dict(c))


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_abi_and_build_list():
    from adaface_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "adaface_hip.h").read_text(), flags=re.S)
    for s in ("af_load_tensor_lora", "af_op_lora_repack"):
        assert re.search(rf"\b{s}\s*\(", text) and s in _lib.EXPORTED_SYMBOLS, s
    assert "af_lora.hip" in build.SOURCES
    assert (_lib.LORA_MAX_ADAPTERS, _lib.LORA_MAX_RANK) == (8, 256)
    assert "AF_LORA_MAX_ADAPTERS = 8, AF_LORA_MAX_RANK = 256" in text
    assert "af_load_tensor_lora" in (ROOT / "INTEGRATION.md").read_text()


# ------------------------------------------------------------------------------------------------------------ names
@pytest.mark.parametrize("which", ["sd15", "tiny"])
def test_every_kohya_unet_name_maps_onto_a_parameter(which):
    from adaface_amd import layout
    from adaface_amd.lora import kohya_unet_map, split_lora
    cfg = O.SD15_UNET if which == "sd15" else O.TINY_UNET
    shapes = layout.unet_param_shapes(**_cfg_dict(cfg))          # (the drop-in UNetModel's parameters: tests/test_host_cpu.py)
    names = LR.kohya_unet_names(cfg)
    kmap = kohya_unet_map(_cfg_dict(cfg))
    seen = set()
    for kohya, want in names:
        got = kmap.get(kohya)
        assert got == want, (kohya, got, want)
        assert len(shapes[got + ".weight"]) >= 2, got
        assert got not in seen, got                               # injective
        seen.add(got)
    assert len(seen) == len(names) == len(kmap)
    # every conv / linear weight of the U-Net is reachable
    assert seen == {k[:-len(".weight")] for k, s in shapes.items() if k.endswith(".weight") and len(s) >= 2}
    # ... and through split_lora (shapes do not matter to the mapping)
    raw = {}
    for kohya, _ in names[:40]:
        raw[f"lora_unet_{kohya}.lora_up.weight"] = torch.zeros(1, 1)
        raw[f"lora_unet_{kohya}.lora_down.weight"] = torch.zeros(1, 1)
    out = split_lora(raw, _cfg_dict(cfg), strict=True)
    assert sorted(out["unet"]) == sorted(w for _, w in names[:40]) and not out["text"] and not out["unused"]


def test_pinned_names():
    from adaface_amd.lora import kohya_text_name, kohya_unet_map
    kmap = kohya_unet_map(_cfg_dict(O.SD15_UNET))
    assert kmap["down_blocks_1_attentions_0_transformer_blocks_0_attn2_to_k"] == "input_blocks.4.1.transformer_blocks.0.attn2.to_k"
    assert kmap["up_blocks_1_upsamplers_0_conv"] == "output_blocks.5.2.conv"
    assert kmap["up_blocks_0_upsamplers_0_conv"] == "output_blocks.2.1.conv"
    assert kmap["mid_block_resnets_1_conv2"] == "middle_block.2.out_layers.3"
    assert kmap["down_blocks_0_downsamplers_0_conv"] == "input_blocks.3.0.op"
    assert kmap["down_blocks_2_resnets_0_conv_shortcut"] == "input_blocks.7.0.skip_connection"
    assert "down_blocks_2_resnets_1_conv_shortcut" not in kmap and "down_blocks_3_attentions_0_proj_in" not in kmap
    assert kmap["up_blocks_3_attentions_2_transformer_blocks_0_ff_net_0_proj"] == "output_blocks.11.1.transformer_blocks.0.ff.net.0.proj"
    assert kohya_text_name("text_model_encoder_layers_11_mlp_fc1") == "transformer.text_model.encoder.layers.11.mlp.fc1"
    assert kohya_text_name("text_model_encoder_layers_0_self_attn_out_proj") == "transformer.text_model.encoder.layers.0.self_attn.out_proj"
    assert kohya_text_name("text_model_embeddings_token_embedding") is None


def test_every_kohya_text_name_maps_onto_a_parameter():
    from adaface_amd import layout
    from adaface_amd.ldm.modules.encoders.modules import CLIP_VIT_L14_TEXT
    from adaface_amd.lora import kohya_text_name
    shapes = {"transformer.text_model." + k: v for k, v in layout.clip_text_param_shapes(**CLIP_VIT_L14_TEXT).items()}
    names = LR.kohya_text_names(CLIP_VIT_L14_TEXT["layers"])
    got = [kohya_text_name(k) for k, _ in names]
    assert got == [w for _, w in names] and len(set(got)) == len(got)
    assert all(len(shapes[g + ".weight"]) == 2 for g in got)
    assert set(got) == {k[:-len(".weight")] for k, s in shapes.items() if ".encoder.layers." in k and k.endswith(".weight") and len(s) == 2}


# ------------------------------------------------------------------------------------------------------------ files
def _kohya_file(tmp_path, with_alpha=True):
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(5)
    raw = {"lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn2_to_k.lora_up.weight": torch.randn(64, 4, generator=g),
           "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn2_to_k.lora_down.weight": torch.randn(4, 64, generator=g),
           "lora_unet_down_blocks_0_resnets_0_conv1.lora_up.weight": torch.randn(64, 2, 1, 1, generator=g),
           "lora_unet_down_blocks_0_resnets_0_conv1.lora_down.weight": torch.randn(2, 64, 3, 3, generator=g),
           "lora_te_text_model_encoder_layers_1_mlp_fc1.lora_up.weight": torch.randn(128, 3, generator=g),
           "lora_te_text_model_encoder_layers_1_mlp_fc1.lora_down.weight": torch.randn(3, 32, generator=g)}
    if with_alpha:
        raw["lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn2_to_k.alpha"] = torch.tensor(2.0)
    path = tmp_path / "a.safetensors"
    save_file(raw, str(path))
    return path, raw


def test_file_round_trip_and_missing_alpha(tmp_path):
    from adaface_amd.lora import load_lora_file, split_lora
    path, raw = _kohya_file(tmp_path)
    back = load_lora_file(path)
    assert sorted(back) == sorted(raw) and all(torch.equal(back[k], raw[k]) for k in raw)
    out = split_lora(back, _cfg_dict(O.TINY_UNET), strict=True)
    k = "input_blocks.1.1.transformer_blocks.0.attn2.to_k"
    assert sorted(out["unet"]) == ["input_blocks.1.0.in_layers.2", k] and out["unused"] == []
    assert sorted(out["text"]) == ["transformer.text_model.encoder.layers.1.mlp.fc1"]
    up, down, alpha = out["unet"][k]
    assert alpha == 2.0 and torch.equal(up, raw["lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn2_to_k.lora_up.weight"])
    assert out["unet"]["input_blocks.1.0.in_layers.2"][2] == 2.0          # missing alpha: the rank
    assert out["text"]["transformer.text_model.encoder.layers.1.mlp.fc1"][2] == 3.0
    # the same through a .pt holding a plain tensor dict, and native names with and without the checkpoint prefix
    torch.save(raw, tmp_path / "a.pt")
    assert sorted(load_lora_file(tmp_path / "a.pt")) == sorted(raw)
    native = {"model.diffusion_model." + k + ".lora_up.weight": up, "model.diffusion_model." + k + ".lora_down.weight": down,
              "middle_block.1.proj_in.lora_up.weight": torch.zeros(256, 1, 1, 1), "middle_block.1.proj_in.lora_down.weight": torch.zeros(1, 256, 1, 1),
              "cond_stage_model.transformer.text_model.encoder.layers.0.self_attn.q_proj.lora_up.weight": torch.zeros(32, 1),
              "cond_stage_model.transformer.text_model.encoder.layers.0.self_attn.q_proj.lora_down.weight": torch.zeros(1, 32)}
    out = split_lora(native, _cfg_dict(O.TINY_UNET), strict=True)
    assert sorted(out["unet"]) == [k, "middle_block.1.proj_in"] and out["unet"][k][2] == 4.0
    assert sorted(out["text"]) == ["transformer.text_model.encoder.layers.0.self_attn.q_proj"]
    with pytest.raises(ValueError, match="plain dict"):
        torch.save([1, 2], tmp_path / "b.pt")
        load_lora_file(tmp_path / "b.pt")


@pytest.mark.parametrize("key,kind", [("lora_unet_mid_block_attentions_0_proj_in.dora_scale", "DoRA"),
                                      ("lora_unet_mid_block_attentions_0_proj_in.hada_w1_a", "LoHa"),
                                      ("lora_unet_mid_block_attentions_0_proj_in.lokr_w1", "LoKr"),
                                      ("lora_unet_mid_block_resnets_0_conv1.lora_mid.weight", "lora_mid")])
def test_other_adapter_kinds_are_refused_by_name(key, kind):
    from adaface_amd.lora import split_lora
    with pytest.raises(NotImplementedError, match=kind):
        split_lora({key: torch.zeros(1)}, _cfg_dict(O.TINY_UNET))


def test_unknown_keys_strict_and_not():
    from adaface_amd.lora import split_lora
    raw = {"lora_unet_down_blocks_9_attentions_0_proj_in.lora_up.weight": torch.zeros(4, 1),
           "lora_unet_down_blocks_9_attentions_0_proj_in.lora_down.weight": torch.zeros(1, 4),
           "lora_te2_text_model_encoder_layers_0_mlp_fc1.alpha": torch.tensor(1.0), "something_else": torch.zeros(1),
           "input_blocks.1.0.in_layers.0.lora_up.weight": torch.zeros(4, 1), "input_blocks.1.0.in_layers.0.lora_down.weight": torch.zeros(1, 4)}
    out = split_lora(raw, _cfg_dict(O.TINY_UNET))
    assert out["unet"] == {} and out["text"] == {} and out["unused"] == sorted(raw)      # (a GroupNorm weight is no target)
    with pytest.raises(KeyError, match="down_blocks_9"):
        split_lora(raw, _cfg_dict(O.TINY_UNET), strict=True)
    with pytest.raises(ValueError, match="mid_block_attentions_0_proj_in"):              # half a pair
        split_lora({"lora_unet_mid_block_attentions_0_proj_in.lora_up.weight": torch.zeros(4, 1)}, _cfg_dict(O.TINY_UNET))


# ------------------------------------------------------------------------------------------------------------ overlay
def test_overlay_bookkeeping_without_an_engine():
    m = _tiny_unet()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    shapes = {k[:-len(".weight")]: tuple(v.shape) for k, v in before.items() if k.endswith(".weight")}
    a = LR.exact_adapter(shapes, ["input_blocks.1.1.proj_in", "input_blocks.1.0.in_layers.2"], 4, seed=1)
    b = LR.exact_adapter(shapes, ["input_blocks.1.1.proj_in", "middle_block.1.transformer_blocks.0.ff.net.0.proj"], 2, seed=2)
    assert m.lora_targets() == []
    assert m.set_lora([(a, 1.0), (b, 0.5)]) is m
    assert m.lora_targets() == sorted(set(a) | set(b))
    after = m.state_dict()
    assert sorted(after) == sorted(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert m._engine is None
    s = m._lora_of("input_blocks.1.1.proj_in")
    assert [x[2] for x in s] == [1.0 * (4 * 2.0 ** -8) / 4, 0.5 * (2 * 2.0 ** -8) / 2]      # scale * alpha / r, list order
    m.clear_lora()
    assert m.lora_targets() == [] and m._lora == []
    # refusals name the key and leave the set as it was
    m.set_lora([(a, 1.0)])
    with pytest.raises(KeyError, match="no.such.layer"):
        m.set_lora([({"no.such.layer": a["input_blocks.1.1.proj_in"]}, 1.0)])
    with pytest.raises(KeyError, match="in_layers.0"):                                        # a norm is no target
        m.set_lora([({"input_blocks.1.0.in_layers.0": a["input_blocks.1.1.proj_in"]}, 1.0)])
    up, down, alpha = a["input_blocks.1.1.proj_in"]
    with pytest.raises(ValueError, match="input_blocks.1.1.proj_in"):
        m.set_lora([({"input_blocks.1.1.proj_in": (up[:-1], down, alpha)}, 1.0)])
    with pytest.raises(ValueError, match="input_blocks.1.0.in_layers.2"):                     # a 1x1 down for a 3x3 weight
        m.set_lora([({"input_blocks.1.0.in_layers.2": (up, down, alpha)}, 1.0)])
    with pytest.raises(ValueError, match="rank"):
        m.set_lora([({"input_blocks.1.1.proj_in": (torch.zeros(64, 257), torch.zeros(257, 64), 1.0)}, 1.0)])
    with pytest.raises(ValueError, match="at most 8"):
        m.set_lora([(a, 1.0)] * 9)
    with pytest.raises(ValueError, match="scale"):
        m.set_lora([(a, float("nan"))])
    assert m.lora_targets() == sorted(a)
    m.set_lora([(a, 1.0)] * 8)                                                                # eight are accepted


def test_set_lora_drops_fp8_shifts_and_reaches_every_module_class():
    from adaface_amd.ldm.models.autoencoder import AutoencoderKL
    from adaface_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    m = _tiny_unet()
    object.__setattr__(m, "_fp8_shifts", {"x": 1})
    m.set_lora([])                                     # nothing before, nothing after: no change
    assert m._fp8_shifts == {"x": 1}
    shapes = {k[:-len(".weight")]: tuple(v.shape) for k, v in m.state_dict().items() if k.endswith(".weight")}
    m.set_lora([(LR.exact_adapter(shapes, ["middle_block.1.proj_out"], 1, seed=3), 1.0)])
    assert m._fp8_shifts is None and m._ctx_key is None
    for cls in (FrozenCLIPEmbedder, AutoencoderKL):
        assert cls.set_lora is type(m).set_lora and cls.clear_lora is type(m).clear_lora and cls.lora_targets is type(m).lora_targets


# ------------------------------------------------------------------------------------------------------------ CLI
def test_cli_parses_path_and_scale():
    import importlib.util
    from adaface_amd.lora import parse_lora_arg
    assert parse_lora_arg("a.safetensors") == ("a.safetensors", 1.0)
    assert parse_lora_arg("a.safetensors:0.5") == ("a.safetensors", 0.5)
    assert parse_lora_arg("C:/loras/a.safetensors") == ("C:/loras/a.safetensors", 1.0)
    assert parse_lora_arg("C:/loras/a.safetensors:-1e-1") == ("C:/loras/a.safetensors", -0.1)
    assert parse_lora_arg("dir:with:colons/a.pt:2") == ("dir:with:colons/a.pt", 2.0)
    spec = importlib.util.spec_from_file_location("stable_txt2img", ROOT / "scripts" / "stable_txt2img.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opt = mod.parse_args(["--synthetic", "--lora", "x:y/a.safetensors:0.25", "--lora", "b.pt", "--lora_strict"])
    assert opt.lora == [("x:y/a.safetensors", 0.25), ("b.pt", 1.0)] and opt.lora_strict
    assert mod.parse_args(["--synthetic"]).lora is None
    with pytest.raises(SystemExit):
        mod.parse_args(["--synthetic"] + ["--lora", "a.pt"] * 9)
    with pytest.raises(SystemExit):
        mod.parse_args(["--synthetic", "--lora_strict"])


# ------------------------------------------------------------------------------------------------------------ the restated layout
def test_layout_formula_on_a_hand_written_example():
    """rows 4, cin 3, one tap, cin_pad 4, ldw 6, row_off 1 of 6 rows: written out by hand."""
    flat = torch.arange(1.0, 13.0).reshape(4, 3)
    got = LR.pack(flat, cin=3, kk=1, cin_pad=4, ldw=6, row_off=1, rows_total=6, fill=-1.0)
    want = torch.tensor([[-1, -1, -1, -1, -1, -1],
                         [1, 2, 3, 0, -1, -1],
                         [4, 5, 6, 0, -1, -1],
                         [7, 8, 9, 0, -1, -1],
                         [10, 11, 12, 0, -1, -1],
                         [-1, -1, -1, -1, -1, -1]], dtype=torch.float32)
    assert torch.equal(got, want)
    # two taps: the weight's own order is (c, tap), the packed one (tap, c padded)
    flat = torch.tensor([[1.0, 2.0, 3.0, 4.0]])                       # c0t0 c0t1 c1t0 c1t1
    assert LR.pack(flat, cin=2, kk=2, cin_pad=3).tolist() == [[1.0, 3.0, 0.0, 2.0, 4.0, 0.0]]
    assert LR.packed_index(0, 1, 1, rows=1, cin_pad=3, ldw=6) == 4
    # the GEGLU row order: value / gate groups of 16 interleaved (rows 64: value 0..31, gate 32..63)
    assert [LR.geglu_perm(n, 32) for n in (0, 15, 16, 31, 32, 47, 48, 63)] == [0, 15, 32, 47, 16, 31, 48, 63]
    p = LR.pack(torch.arange(64.0)[:, None], cin=1, kk=1, perm=True)[:, 0].tolist()
    assert p[:16] == list(range(16)) and p[16:32] == list(range(32, 48)) and p[32:48] == list(range(16, 32)) and p[48:] == list(range(48, 64))
    assert sorted(LR.geglu_perm(n, 32) for n in range(64)) == list(range(64))
    # the merge and its bound on a case small enough to do by hand: W = 1, up = [2], down = [3], s = 0.5 -> 4
    base, ad = torch.ones(1, 1), [(torch.tensor([[2.0]]), torch.tensor([[3.0]]), 0.5)]
    assert LR.merge64(base, ad).item() == 4.0 and LR.merge32(base, ad).item() == 4.0 and LR.magnitude(base, ad).item() == 4.0
    ref, b = LR.bound(base, ad, "bf16")
    assert ref.item() == 4.0 and b.item() == 4 * 2.0 ** -24 * 4.0 + 2.0 ** (2 - 7)
