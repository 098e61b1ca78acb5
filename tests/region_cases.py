"""The cases the regional-prompt tests share (tests/test_region_cpu.py, tests/test_region_gpu.py): shapes and seeded inputs.
The shapes are the smallest at which a kernel can still go wrong: tails in the query blocks (Nq % 32), in the key blocks
(T % 32), one key, the full 96, one region and eight, heads that do not fill a workgroup (1, 2, 5) and that do (8)."""
import torch

# ---- weights kernel ----
W_BATCHES = (1, 3)
W_REGIONS = (1, 3, 8)
W_MAPS = ((8, 8), (16, 24), (64, 64))
W_REL_BOUND = 160 * 2.0 ** -24      # 63 + 63 additions of the two box sums, 7 of the region sum, the scale and the division

# ---- operator: (dh, T, R, Nq, heads, B, ld_slack); every value of every list of the issue appears ----
OP_CASES = [
    (32, 77, 3, 64, 2, 1, 0),
    (40, 77, 3, 257, 8, 3, 8),
    (64, 33, 2, 33, 1, 1, 0),
    (80, 96, 8, 192, 5, 1, 0),
    (128, 16, 2, 31, 2, 3, 8),
    (160, 77, 3, 64, 8, 1, 0),
    (40, 1, 8, 1, 1, 1, 0),
    (80, 77, 1, 33, 8, 1, 0),
    (160, 96, 2, 257, 2, 1, 8),
    (64, 16, 8, 192, 5, 3, 0),
]
# the composition alone: f32 storage, and more keys per segment than the fused kernel holds
COMPOSE_ONLY_CASES = [
    ("f32", (40, 77, 3, 64, 2, 1, 0)),
    ("f32", (64, 33, 2, 33, 1, 3, 8)),
    ("bf16", (40, 154, 2, 64, 8, 1, 0)),
    ("f16", (80, 154, 2, 33, 2, 1, 8)),
]
OP_TOL = {"bf16": 1.5e-2, "f16": 1.5e-2 / 8, "f32": 2e-4}       # the attention operator's bars, of max|ref|
MODEL_TOL = {"f32": 2e-4, "bf16": 3e-2, "f16": 3.75e-3}         # the model bars
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def normalise(a):
    """a [B, R, N] >= 0 (float64) -> w = a / s, (1, 0, ..) where s = 0; fp32, as a level of the pyramid"""
    s = a.sum(dim=1, keepdim=True)
    w = torch.where(s > 0, a / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(a))
    w[:, 0] = torch.where(s[:, 0] > 0, w[:, 0], torch.ones_like(w[:, 0]))
    return w.float()


def op_inputs(case, seed=0):
    """q, k, v (fp32) and normalised weights w [B, R, Nq]: random weights, 40 % of the entries zero, one region switched off
    over a whole 32-query block where there is one, some queries with no weight at all (-> the base region)."""
    dh, T, R, Nq, heads, B, _ = case
    g = torch.Generator().manual_seed(1000 + seed)
    C = heads * dh
    q = torch.randn(B, Nq, C, generator=g)
    k = torch.randn(B, R * T, C, generator=g)
    v = torch.randn(B, R * T, C, generator=g)
    a = torch.rand(B, R, Nq, generator=g, dtype=torch.float64)
    a = a * (torch.rand(B, R, Nq, generator=g) > 0.4)
    if Nq >= 32 and R > 1:
        a[:, R - 1, :32] = 0.0
    if Nq > 4:
        a[:, :, 3] = 0.0
    return q, k, v, normalise(a)


def storage_round(t, dtype):
    return t.to(TORCH_DT[dtype]).double()


def weight_maps(Bf, R, H, W, kind, seed=0):
    """kind "binary": 0 / 1 masks (box sums are exact); "random": uniform [0, 1) with 30 % zeros.  Both with one 8 x 8 cell of
    no weight at all in every sample (s = 0 at every level)."""
    g = torch.Generator().manual_seed(2000 + seed)
    if kind == "binary":
        m = (torch.rand(Bf, R, H, W, generator=g) > 0.5).float()
    else:
        m = torch.rand(Bf, R, H, W, generator=g) * (torch.rand(Bf, R, H, W, generator=g) > 0.3)
    m[:, :, :8, :8] = 0.0
    return m.float()


def model_maps(B, H, W, legs):
    """R = 3 for the model tests: the base at 0.2 everywhere; a hard region (the left half); a soft region overlapping it (a
    horizontal ramp over the middle columns, full rows); in the LAST sample a gap -- rows H/2 .. of the right quarter carry no
    weight at all, the base included, so s = 0 there.  legs = 2 appends B unconditional legs (1, 0, 0).  -> fp32 [B legs, 3, H, W]"""
    from adaface_amd import regions as RG
    hard = torch.zeros(H, W, dtype=torch.float64)
    hard[:, : W // 2] = 1.0
    soft = torch.zeros(H, W, dtype=torch.float64)
    ramp = torch.linspace(0.1, 0.9, W // 2, dtype=torch.float64)
    soft[:, W // 4: W // 4 + W // 2] = ramp
    w = RG.build_weights(torch.stack([hard, soft]), 0.2, B, legs).double()
    w[B - 1, :, H // 2:, 3 * W // 4:] = 0.0
    return w.float()
