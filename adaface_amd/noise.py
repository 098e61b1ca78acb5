"""Seed-stable noise for the stochastic sampling paths: a counter-based generator (Philox4x32-10, csrc/af_philox.h).

A sample's noise is a pure function of (seed, the sample's GLOBAL index, stream, step, element) -- not of the rank that
draws it, its position in the batch, or the order of the launches.  So `--seed` names an image under any batch split and any
number of GPUs, which the device's default generator (torch.randn(..., device=...)) cannot give: every rank would draw the
same stream for different samples.
"""
from __future__ import annotations

import math

import torch

from . import ops

# the streams of the keying contract (csrc/af_philox.h)
STREAM_XT = 0         # start code x_T
STREAM_STEP = 1       # sampler step noise (DDIM eta > 0, DPM-Solver++ SDE); af_dpmpp_sde_step draws from it in-kernel
STREAM_QSAMPLE = 2    # q_sample noise of the inpainting blend


# the per-tag constants of PhiloxNoise.derive; a new tag takes a new constant, an existing one never changes
DERIVE_TAGS = {"hires": 0x68697265735F3031}    # ASCII "hires_01"
_M64 = 0xFFFFFFFFFFFFFFFF


def splitmix64(x: int) -> int:
    """One output of splitmix64 (Steele, Lea, Flood, "Fast Splittable Pseudorandom Number Generators", OOPSLA 2014) from state x:
    z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31,
    all mod 2^64."""
    z = (int(x) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class PhiloxNoise:
    """The noise of the samples `sample_ids` (global indices; None: first_id, first_id + 1, ...) under `seed`.

    randn(shape, stream, step, device): fp32 normals of shape [n_samples, ...]; row i belongs to sample id i of this source,
    whatever else the tensor holds.  Two sources with the same seed agree on every sample id they share."""

    def __init__(self, seed, sample_ids=None, first_id=0):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.first_id = int(first_id)
        if self.first_id < 0:
            raise ValueError("PhiloxNoise: first_id must be >= 0")
        self.sample_ids = None if sample_ids is None else [int(i) for i in sample_ids]
        if self.sample_ids is not None and any(i < 0 for i in self.sample_ids):
            raise ValueError("PhiloxNoise: sample ids must be >= 0")
        self._ids_dev = {}

    def ids(self, n):
        """The global indices of the first n samples of this source (host list)."""
        if self.sample_ids is None:
            return list(range(self.first_id, self.first_id + n))
        if n > len(self.sample_ids):
            raise ValueError(f"PhiloxNoise: {n} samples asked for, {len(self.sample_ids)} sample ids given")
        return self.sample_ids[:n]

    def ids_device(self, n, device):
        """(int64 device tensor of n ids or None, first_id): the id arguments of af_philox_randn / af_dpmpp_sde_step."""
        if self.sample_ids is None:
            return None, self.first_id
        key = (n, str(device))
        if key not in self._ids_dev:
            self._ids_dev[key] = torch.tensor(self.ids(n), dtype=torch.int64, device=device)
        return self._ids_dev[key], 0

    def repeated(self, n):
        """A source whose n samples all carry this source's first id (the samplers' repeat_noise)."""
        return PhiloxNoise(self.seed, sample_ids=[self.ids(1)[0]] * n)

    def derive(self, tag: str):
        """A source for the same sample ids whose seed is splitmix64(seed + DERIVE_TAGS[tag]) mod 2^64: a second run of the same
        samples (the hires fix's pass two) draws noise uncorrelated with this source's, still a pure function of (seed, global
        sample index)."""
        if tag not in DERIVE_TAGS:
            raise ValueError(f"PhiloxNoise.derive: tag {tag!r} (one of {', '.join(DERIVE_TAGS)})")
        return PhiloxNoise(splitmix64(self.seed + DERIVE_TAGS[tag]), sample_ids=self.sample_ids, first_id=self.first_id)

    def randn(self, shape, stream, step, device):
        shape = tuple(int(s) for s in shape)
        n = shape[0]
        ids_dev, first = self.ids_device(n, device)
        return ops.philox_randn(n, math.prod(shape[1:]), self.seed, stream, step, sample_ids=ids_dev, first_id=first,
                                device=device).view(shape)
