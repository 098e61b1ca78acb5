"""GPU test of the samplers' host loops on the tiny model (f32): the final latent of every run of
tests/golden/gen_sampler_traces.py --gpu -- DDIM, PLMS, DPM-Solver++ (deterministic and SDE with a PhiloxNoise) and LCM at S = 4,
each with plain CFG, PAG + rescale, SAG and the fused inpainting blend -- has the bits the commit named in
tests/golden/sampler_latents_tiny.npz gave.  The same device, library and launches in the same order: equality, no tolerance.
Every recorded run gave the same bits twice on that commit."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import gen_sampler_traces as GT  # noqa: E402

pytestmark = pytest.mark.gpu


def test_latents_have_the_recorded_bits(gpu):
    gold = dict(np.load(GT.LATENTS))
    assert len(str(gold.pop("commit"))) == 40 and sorted(gold) == sorted(GT.gpu_names())
    model = GT.tiny_model(gpu)
    differ = []
    for name in GT.gpu_names():
        lat = GT.gpu_latent(model, gpu, name).cpu()
        assert torch.isfinite(lat).all(), name
        if not torch.equal(lat, torch.tensor(gold[name])):
            differ.append((name, float((lat - torch.tensor(gold[name])).abs().max())))
    assert not differ, differ
