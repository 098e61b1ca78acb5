"""Subject-token conv attention (attention.py:208-216, ldm/util.py:701-879) on the GPU: the one-pass kernels
(conv_attn_map_kernel + xs::xattn_short_conv_kernel) and the flash + subj_scores + merge path at SD-1.5's head dims,
at the operator level against the fp64 reference of tests/conv_attn_cases.py, and through the whole SD-1.5 UNet.
tests/test_conv_attn_cpu.py shows that the reference of every case differs from plain attention and from the mis-shifted
replacements by >= 10 bars."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import ldm_oracle as O  # noqa: E402  (the checker, never the thing measured)
from tests import conv_attn_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(gpu, case, path, dtype="bf16"):
    from adaface_amd import ops
    B, Hh, Ww, S, heads, dh, ks, groups = case
    q, k, v, token_idx = CC.inputs(case)
    out = ops.conv_attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, (Hh, Ww), ks, [list(g) for g in token_idx],
                             dtype=dtype, path=path)
    return out.double().cpu()


def _err(a, ref):
    return (a - ref).abs().max().item() / ref.abs().max().item()


@pytest.mark.parametrize("case", CC.ONE_PASS_CASES, ids=CC.case_id)
def test_conv_attention_one_pass(gpu, report, case):
    """path 2 (conv map + one-pass short-key kernel) and path 1 (flash + subj_scores + merge) against the fp64 reference at
    the project's bf16 operator bar, and against each other at twice that bar (as
    test_attention_short_keys_register_resident holds the short-key kernel against the flash kernel); the launch counter
    proves which kernel ran; the f32 mode has no one-pass kernel."""
    from adaface_amd import _lib
    ref = CC.reference(case)
    _lib.plan_counts(reset=True)
    one = _run(gpu, case, "one_pass")
    assert _lib.plan_counts(reset=True)["conv_attn_short"] == 1
    merge = _run(gpu, case, "merge")
    assert _lib.plan_counts(reset=True)["conv_attn_short"] == 0
    e_one, e_merge, d = _err(one, ref), _err(merge, ref), _err(one, merge)
    name = "conv_attention " + CC.case_id(case)
    report(name + " one-pass vs fp64 reference [bf16]", e_one, ref.abs().max().item(), CC.BF16_BAR)
    report(name + " flash + merge vs fp64 reference [bf16]", e_merge, ref.abs().max().item(), CC.BF16_BAR)
    report(name + " one-pass vs flash + merge [bf16]", d, ref.abs().max().item(), 2 * CC.BF16_BAR)
    print(f"{name}: one-pass {e_one:.3e}, merge {e_merge:.3e}, one-pass vs merge {d:.3e}")
    assert torch.isfinite(one).all() and torch.isfinite(merge).all()
    assert e_one <= CC.BF16_BAR, e_one
    assert e_merge <= CC.BF16_BAR, e_merge
    assert d <= 2 * CC.BF16_BAR, d
    from adaface_amd._lib import AfError
    with pytest.raises(AfError):
        _run(gpu, case, "one_pass", dtype="f32")


def test_conv_attention_auto_takes_the_one_pass_kernel(gpu, knobs):
    """path "auto" is the planner's choice: the one-pass kernel by default, the merge path with knob conv_attn_short = 0;
    the same numbers as the explicit paths."""
    from adaface_amd import _lib
    case = CC.ONE_PASS_CASES[0]
    _lib.plan_counts(reset=True)
    auto = _run(gpu, case, "auto")
    assert _lib.plan_counts(reset=True)["conv_attn_short"] == 1
    assert torch.equal(auto, _run(gpu, case, "one_pass"))
    knobs("conv_attn_short", 0)
    _lib.plan_counts(reset=True)
    auto0 = _run(gpu, case, "auto")
    assert _lib.plan_counts(reset=True)["conv_attn_short"] == 0
    assert torch.equal(auto0, _run(gpu, case, "merge"))


@pytest.mark.parametrize("case,dtype,bar", [(CC.MERGE_ONLY_CASE_DH160, "bf16", CC.BF16_BAR),
                                            (CC.MERGE_ONLY_CASE_F32, "f32", CC.F32_BAR)],
                         ids=["dh160_bf16", "dh40_f32"])
def test_conv_attention_merge_path_only(gpu, report, case, dtype, bar):
    """Where no one-pass kernel exists (dh 160, the f32 mode): flash + subj_scores + merge against the fp64 reference, and
    "auto" takes that path."""
    from adaface_amd import _lib
    ref = CC.reference(case)
    _lib.plan_counts(reset=True)
    out = _run(gpu, case, "merge", dtype=dtype)
    e = _err(out, ref)
    report(f"conv_attention {CC.case_id(case)} flash + merge vs fp64 reference [{dtype}]", e, ref.abs().max().item(), bar)
    print(f"conv_attention {CC.case_id(case)} [{dtype}] merge: {e:.3e}")
    assert e <= bar, e
    assert torch.equal(_run(gpu, case, "auto", dtype=dtype), out)
    assert _lib.plan_counts(reset=True)["conv_attn_short"] == 0


def test_sd15_unet_conv_attention_paths_ab(gpu, report, knobs):
    """The SD-1.5 UNet with 3 x 3 conv attention on samples 0 and 1 of a Bf = 4 batch (32 x 32 latent): the default forward
    (A: conv map + one-pass kernel on the samples with the subject, plain short-key kernel on the others) against knob
    conv_attn_short = 0 (B: flash + subj_scores + merge / flash), both against the f32-mode forward with the same
    set_conv_attn, judged by _assert_bf16_ab with its bars unchanged.  Conv attention covers CA layers 0-5 and 11-15
    (openaimodel.py:922-932): layers 0, 1, 13, 14, 15 at dh 40 and 2, 3, 11, 12 at dh 80 have one run with the subject each
    -> 9 launches of the one-pass kernel; layers 4 and 5 are dh 160 (merge path).  No level measured slower than the merge
    path, so no level rule removes one.  The one-launch layer stays off in conv-attention layers.  A is bit-identical run
    to run.  After set_conv_attn(0) the forward launches what it launched before this kernel existed: at this size (4096
    rows at the 320-wide level, below the row-panel GEMMs whose LayerNorm partial sums the one-launch layer needs) that is
    no xattn_fused launch and ten short-key launches, five per level -- counted with the library of the commit before this
    kernel on the same inputs (profiles/conv_attn_short_vs_3abc2a4.txt; the request for this test expected 2 and 5 here without
    having run it)."""
    from adaface_amd import _lib
    from adaface_amd.engine import Engine
    from adaface_amd.synth import synth_weights_into
    from tests.test_model_gpu import _assert_bf16_ab, _unet_kwargs
    cfg = O.SD15_UNET
    Bf = 4
    g = torch.Generator().manual_seed(81)
    x = torch.randn(Bf, 4, 32, 32, generator=g).to(gpu)
    t = torch.randint(0, 1000, (Bf,), generator=g).to(gpu)
    ctx = torch.randn(Bf * 16, 77, cfg.context_dim, generator=g).to(gpu)
    toks = torch.randperm(77, generator=g)[:9].tolist()
    conv = dict(ks=3, batch_idx=[0, 1], token_idx=[toks, toks])

    eng = Engine(dtype="bf16", unet=_unet_kwargs(cfg))
    synth_weights_into(eng, O.unet_param_shapes(cfg), seed=82, device=gpu)
    eng.set_conv_attn(**conv)
    eng.set_context(ctx, Bf, layerwise=True)
    _lib.plan_counts(reset=True)
    a = eng.unet_forward(x, t)
    pc_a = _lib.plan_counts(reset=True)
    a2 = eng.unet_forward(x, t)
    _lib.plan_counts(reset=True)
    knobs("conv_attn_short", 0)
    b = eng.unet_forward(x, t)
    pc_b = _lib.plan_counts(reset=True)
    knobs("conv_attn_short", 1)
    eng.set_conv_attn(0)
    eng.set_context(ctx, Bf, layerwise=True)
    eng.unet_forward(x, t)
    pc_off = _lib.plan_counts(reset=True)
    eng.close()
    print("plan counts A", pc_a, "\nB", pc_b, "\noff", pc_off)
    assert pc_a["conv_attn_short"] == 9 and pc_a["xattn_fused"] == 0, pc_a
    assert pc_b["conv_attn_short"] == 0 and pc_b["xattn_fused"] == 0, pc_b
    assert pc_off["xattn_fused"] == 0 and pc_off["attn_short"] == 10 and pc_off["conv_attn_short"] == 0, pc_off
    assert torch.equal(a, a2)

    ref_eng = Engine(dtype="f32", unet=_unet_kwargs(cfg))
    synth_weights_into(ref_eng, O.unet_param_shapes(cfg), seed=82, device=gpu)
    ref_eng.set_conv_attn(**conv)
    ref_eng.set_context(ctx, Bf, layerwise=True)
    ref = ref_eng.unet_forward(x, t)
    ref_eng.close()
    _assert_bf16_ab(report, "sd15_unet Bf=4 32x32 conv attention one-pass (A) vs flash + merge (B)", a, b, ref)
