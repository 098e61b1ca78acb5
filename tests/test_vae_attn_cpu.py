"""The references of tests/test_vae_attn_gpu.py, proven on the CPU before anyone trusts them (tests/vae_attn_ref.py; as
tests/test_exact_operands_cpu.py does for the conv / GEMM cases): for every exact case the GPU test uses, the conditions of a
bit-exact comparison hold, the three references agree bit for bit, and every plausible mistake of the four launches changes the
reference in a large share of the rows.  The Gaussian model-vs-exact table of DESIGN.md is reproduced here."""
import functools

import pytest
import torch

import exact_operands as X
import vae_attn_ref as R

_onehot = functools.lru_cache(maxsize=None)(lambda shape: R.onehot_case(*shape, seed=R.onehot_seed(*shape)))
_ids = lambda shapes: ["x".join(str(v) for v in s) for s in shapes]


@pytest.mark.parametrize("shape", R.ONEHOT_SHAPES, ids=_ids(R.ONEHOT_SHAPES))
def test_onehot_case_is_exact_in_every_storage_type(shape):
    """Operands, P and the output are representable in bf16, fp16 and f32, >= 90 % of the outputs are non-zero with >= 40 distinct
    values, and the construction's P and output ARE what the oracle's formula and the storage model return: fp32 and fp64
    softmax agree bit for bit, exact_attention == storage_model == the construction."""
    c = _onehot(shape)
    st = R.check_onehot_case(c)
    assert st["classes"] <= shape[2] and set(c["sizes"]) <= {1, 2, 4, 8, 16} and sum(c["sizes"]) == shape[1]
    q, k, v = c["q"], c["k"], c["v"]
    a = R.alpha_f32(shape[2])
    s64 = torch.bmm(q.double(), k.double().transpose(1, 2)) * a
    assert float(s64[s64 != 0].min()) >= 1024.0 and set(torch.unique(s64).tolist()) == {0.0, a * R.Q_ONEHOT}
    p64 = torch.softmax(s64, dim=2)
    p32 = torch.softmax(s64.float(), dim=2)
    assert torch.equal(p64, c["ref_probs"]) and torch.equal(p32.double(), p64)
    ex = R.exact_attention(q, k, v)
    assert torch.equal(ex, c["ref_out"])
    for storage in R.STORAGES:
        refs = R.stage_refs(q, k, v, storage)
        assert torch.equal(refs["probs"], c["ref_probs"]), storage
        assert torch.equal(refs["out"], ex), storage
        assert torch.equal(R.storage_model(q, k, v, storage), ex), storage


@pytest.mark.parametrize("shape", R.ONEHOT_SHAPES, ids=_ids(R.ONEHOT_SHAPES))
def test_onehot_case_sees_the_mistakes(shape):
    """Dropping the last 64 keys (the last K tile of the P v GEMM) or the last 32 (the f32 K tile), reading the next sample's
    K / V, and transposing P each change at least 25 % of the query rows of every sample.  Where counting caps a dropped tile
    near or below that (R.drop_floor: N = 4096, and 32 keys of N = 1920) half the cap is asserted.  Measured, the worst sample
    of each case: 64 keys 40 - 100 % up to N = 1920 and 18 % at N = 4096; 32 keys 32 - 98 % up to N = 1024, 21 % at N = 1920,
    11 % at N = 4096; 100 % for the other two mistakes."""
    c = _onehot(shape)
    B, N, _ = shape
    for T in sorted(set(R.BK.values())):
        m = R.mistaken_outputs(c, T)
        assert ("next_sample" in m) == (B > 1)
        for name, out in m.items():
            share = R.changed_row_share(out, c["ref_out"])
            floor = R.drop_floor(T, N) if name == "drop_tail" else 0.25
            assert float(share.min()) >= floor, (name, T, share.tolist(), floor)


def test_alpha_is_invisible_to_the_onehot_case_but_not_to_the_others():
    """Without alpha the one-hot scores are 32768 and 0 instead of alpha * 32768 and 0: the same P, the same output -- that case
    cannot see a missing or wrong alpha.  The integer scores case and the Gaussian case each move under it."""
    c = _onehot((3, 576, 128))
    s = torch.bmm(c["q"].double(), c["k"].double().transpose(1, 2))
    assert torch.equal(torch.bmm(torch.softmax(s, dim=2), c["v"].double()), c["ref_out"])
    for shape in R.INT_SCORES_SHAPES:
        i = R.int_scores_case(*shape, seed=sum(shape))
        no_alpha = X.roundtrip(i["exact_scores"] / R.alpha_f32(shape[2]), "bf16")
        assert float((no_alpha != i["ref_scores"]).double().mean()) >= 0.9
    B, N, C = R.GAUSS_SHAPES[0]
    q, k, v = R.gaussian_case(B, N, C, 1, R.GAUSS_SEED)
    _, _, model, exact = R.model_vs_exact(q, k, v, "f32")
    no_alpha = R.exact_attention(q * (C ** 0.5), k, v)
    assert float((no_alpha - exact).abs().max() / exact.abs().max()) > 0.5


@pytest.mark.parametrize("shape", R.INT_SCORES_SHAPES, ids=_ids(R.INT_SCORES_SHAPES))
def test_int_scores_case_is_one_rounding_of_an_exact_product(shape):
    """(int_scores_case asserts: integer sums, sum |q||k| < 2^24, alpha a power of two.)  The reference is well spread -- >= 90 %
    non-zero, >= 40 distinct values -- the wide values are in play (the stored q differs from q), a share of the scores is NOT
    representable, so the store's rounding is tested, and ties occur, so round-to-nearest-EVEN is."""
    i = R.int_scores_case(*shape, seed=sum(shape))
    ref, ex = i["ref_scores"], i["exact_scores"]
    assert float((ref != 0).double().mean()) >= X.MIN_NONZERO_OUTPUTS and torch.unique(ref).numel() >= X.MIN_DISTINCT_OUTPUTS
    assert not torch.equal(X.roundtrip(i["q"], "bf16"), i["q"].double())
    rounded = ref != ex
    assert float(rounded.double().mean()) >= 0.01, float(rounded.double().mean())
    tie = rounded & ((ref - ex).abs() * 2 == R.spacing(ex, "bf16"))
    assert int(tie.sum()) >= 100, int(tie.sum())
    assert torch.equal(R.stage_refs(i["q"], i["k"], i["v"], "bf16")["scores"], ref)


@pytest.mark.parametrize("key", sorted(R.GAUSS_TABLE), ids=["-".join(str(v) for v in k) for k in sorted(R.GAUSS_TABLE)])
def test_gaussian_model_vs_exact_table(key):
    """The figures DESIGN.md quotes for what bf16 / fp16 scores cost, reproduced to +-30 % (max |score| to +-15 %): this notices
    when someone changes the storage model.  f32 storage: below 1e-6."""
    B, N, C, qscale = key
    smax, bf, f16 = R.GAUSS_TABLE[key]
    q, k, v = R.gaussian_case(B, N, C, qscale, R.GAUSS_SEED)
    for storage, quoted in (("bf16", bf), ("f16", f16)):
        err, s, _, _ = R.model_vs_exact(q, k, v, storage)
        assert 0.7 * quoted <= err <= 1.3 * quoted, (key, storage, err, quoted)
        assert 0.85 * smax <= s <= 1.15 * smax, (key, storage, s, smax)
    assert R.model_vs_exact(q, k, v, "f32")[0] < 1e-6


def test_spacing_is_one_step_of_the_storage_type():
    for storage, dt in (("bf16", torch.bfloat16), ("f16", torch.float16), ("f32", torch.float32)):
        x = torch.tensor([1.0, 1.5, 2.0, 3.0, 0.0625, 40.0, 1e-3], dtype=dt)
        up = torch.nextafter(x, torch.full_like(x, float("inf"))) if dt != torch.bfloat16 else None
        if up is not None:
            assert torch.equal(R.spacing(x.double(), storage), (up.double() - x.double()))
    assert float(R.spacing(torch.tensor([1.0, 40.0]).double(), "bf16")[0]) == 2.0 ** -7
    assert float(R.spacing(torch.tensor([40.0]).double(), "bf16")[0]) == 0.25
    assert float(R.spacing(torch.tensor([0.0]).double(), "f16")[0]) == 2.0 ** -24
