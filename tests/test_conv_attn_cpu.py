"""Conv attention in one pass (af_op_conv_attention, xs::xattn_short_conv_kernel): what can be checked without a GPU.
The symbols exist everywhere they must, the wrapper's key permutation is the one af_set_context makes, and the inputs of
tests/test_conv_attn_gpu.py are able to tell a right kernel from a wrong one."""
import ctypes
import re
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from adaface_amd import _lib  # noqa: E402
from tests import conv_attn_cases as CC  # noqa: E402

NEW_SYMBOLS = ("af_op_conv_attention", "af_conv_attn_short_launches")
ALL_CASES = CC.ONE_PASS_CASES + [CC.MERGE_ONLY_CASE_DH160]


def test_new_symbols():
    """Header, ctypes table and the built library all carry the operator and the counter; the counter answers without a
    device (it is a host-side count of launches)."""
    header = (ROOT / "include" / "adaface_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    cdll = ctypes.CDLL(str(_lib.lib_path()))
    for name in NEW_SYMBOLS:
        assert hasattr(cdll, name), name
    cdll.af_conv_attn_short_launches.restype = ctypes.c_int64
    assert cdll.af_conv_attn_short_launches() == 0
    # the knob is in the name table
    val = ctypes.c_int(-1)
    assert cdll.af_knob_get(b"conv_attn_short", ctypes.byref(val)) == 0 and val.value == 1


def test_key_order_moves_subject_tokens_to_the_tail():
    from adaface_amd.ops import conv_attn_key_order
    order = conv_attn_key_order(12, [[7, 2, 9, 0], [5, 11, 1, 3]], 2)
    assert order == [4, 6, 8, 10, 7, 2, 9, 0, 5, 11, 1, 3]      # others in order, then string by string in tap order
    assert sorted(order) == list(range(12))
    order = conv_attn_key_order(10, [list(range(9))], 3)
    assert order == [9, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    # group g's tokens sit at rows n - (G - g) * ks^2 + t, the layout af_op_conv_attention documents
    toks = [[3, 1, 4, 15], [9, 2, 6, 5], [8, 7, 14, 0]]
    order = conv_attn_key_order(20, toks, 2)
    for g, grp in enumerate(toks):
        assert order[20 - (3 - g) * 4: 20 - (2 - g) * 4] == grp


@pytest.mark.parametrize("n,toks,ks", [
    (12, [[1, 2, 3, 3]], 2),                 # duplicate inside a string
    (12, [[1, 2, 3, 4], [4, 5, 6, 7]], 2),   # duplicate across strings
    (12, [[1, 2, 3, 12]], 2),                # out of range
    (12, [[-1, 2, 3, 4]], 2),
    (12, [[1, 2, 3]], 2),                    # not ks^2 positions
    (9, [list(range(9))], 3),                # no ordinary key left
    (12, [], 2),
    (40, [list(range(25))], 5),              # kernel size the reference does not have
])
def test_key_order_refuses_bad_positions(n, toks, ks):
    from adaface_amd.ops import conv_attn_key_order
    with pytest.raises(ValueError):
        conv_attn_key_order(n, toks, ks)


@pytest.mark.parametrize("case", ALL_CASES, ids=CC.case_id)
def test_reference_tells_right_from_wrong(case):
    """Preconditions of the GPU test, on the reference alone.  The index-level restatement equals the oracle's
    conv_attn_rows; plain attention (subject columns ignored), the y / x transposed replacement and the replacement with
    the shift sign flipped each differ from the reference by >= 10 bars (bar = BF16_BAR * max|ref|), so none of them could
    pass the operator test."""
    ref = CC.reference(case)
    scale = ref.abs().max().item()
    bar = CC.BF16_BAR * scale
    assert (CC.variant(case, "exact") - ref).abs().max().item() <= 1e-12 * scale
    for kind in ("plain", "transposed", "flipped"):
        d = (CC.variant(case, kind) - ref).abs().max().item()
        print(f"{CC.case_id(case)} {kind}: {d / bar:.1f} bars")
        assert d >= 10 * bar, (kind, d / bar)


def test_inputs_follow_the_stated_recipe():
    """Seed, draw order, subject rows doubled, everything bf16-representable."""
    case = CC.ONE_PASS_CASES[0]
    B, Hh, Ww, S, heads, dh, ks, groups = case
    q, k, v, token_idx = CC.inputs(case)
    g = torch.Generator().manual_seed(1000 * ks + S + dh + Hh)
    q0 = torch.randn(B, Hh * Ww, heads * dh, generator=g)
    k0 = torch.randn(B, S, heads * dh, generator=g)
    assert torch.equal(q, q0.to(torch.bfloat16).float())
    pos = [t for grp in token_idx for t in grp]
    assert len(set(pos)) == groups * ks * ks and all(0 <= t < S for t in pos)
    other = [t for t in range(S) if t not in pos]
    assert torch.equal(k[:, other], k0[:, other].to(torch.bfloat16).float())
    assert torch.equal(k[:, pos], (2 * k0[:, pos]).to(torch.bfloat16).float())
    for t in (q, k, v):
        assert torch.equal(t, t.to(torch.bfloat16).float())
