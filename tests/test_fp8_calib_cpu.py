"""Calibrated fp8 activation scales, the host side (no GPU): the amax -> shift rule of the library against its definition,
and the scale file's round trip and refusals.  The GPU side is tests/test_fp8_calib_gpu.py."""
import json
import math
import random

import pytest

S_MIN, S_MAX, S_DEFAULT = -16, 8, 3


def _shift_ref(amax, headroom):
    """Largest s in [-16, 8] with amax * 2^(s + headroom) <= 448, from math.frexp (exact: no logarithm is rounded)."""
    if not (amax > 0.0) or math.isinf(amax):
        return S_DEFAULT
    m, e = math.frexp(amax)                 # amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    s = 9 - e - (1 if m > 0.875 else 0) - headroom
    return max(S_MIN, min(S_MAX, s))


def _f32(v):
    import struct
    return struct.unpack("f", struct.pack("f", v))[0]


def test_shift_for_amax_matches_its_definition():
    from adaface_amd import _lib
    from adaface_amd.fp8_calib import shift_for_amax, shift_reference
    lib = _lib.load()
    rng = random.Random(20240607)
    values = [56.0, 56.0001, 447.9, 448.0, 1.0, 0.1, 3.5, 7.0, 112.0, 1e4, 1e-9, 0.0, math.inf, math.nan]
    values += [10.0 ** rng.uniform(-6.0, 6.0) for _ in range(1000)]
    n_bracketed = 0
    for v in values:
        a = _f32(v)                          # the library takes a float: hold the reference to the same number
        for headroom in (0, 1, 2):
            got = lib.af_fp8_shift_for_amax(a, headroom)
            assert got == _shift_ref(a, headroom) == shift_reference(a, headroom) == shift_for_amax(a, headroom), (v, headroom, got)
            assert S_MIN <= got <= S_MAX
            if a > 0.0 and math.isfinite(a) and S_MIN < got < S_MAX:
                assert a * 2.0 ** (got + headroom) <= 448.0 < a * 2.0 ** (got + headroom + 1), (v, headroom, got)
                n_bracketed += 1
    assert n_bracketed > 1000          # (amax below 1.75 sits at the upper clamp: about half of the log-uniform draws)
    # the two the issue names: 56 fills the range exactly at shift 3, the next float above it does not
    assert lib.af_fp8_shift_for_amax(56.0, 0) == 3
    assert lib.af_fp8_shift_for_amax(_f32(56.0001), 0) == 2
    assert lib.af_fp8_shift_for_amax(448.0, 0) == 0 and lib.af_fp8_shift_for_amax(_f32(447.9), 0) == 0
    # defaults and clamps
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan):
        assert lib.af_fp8_shift_for_amax(bad, 1) == S_DEFAULT
    assert lib.af_fp8_shift_for_amax(1e-9, 0) == S_MAX and lib.af_fp8_shift_for_amax(1e30, 0) == S_MIN
    # the heavy-tailed tensor of the saturation test (max|y| = 86.8): 2 with no headroom, 1 with one binade
    assert lib.af_fp8_shift_for_amax(_f32(86.8), 0) == 2 and lib.af_fp8_shift_for_amax(_f32(86.8), 1) == 1


def test_scale_file_round_trip_and_refusals(tmp_path):
    from adaface_amd.fp8_calib import check_shifts, load_scales, save_scales
    names = [f"model.diffusion_model.input_blocks.{i}.0.in_layers.2.weight" for i in range(1, 6)]
    names.append("model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight")
    shifts = {n: s for n, s in zip(names, (3, -16, 8, 0, -3, 5))}
    path = tmp_path / "scales.json"
    save_scales(path, shifts, amax={n: 1.5 * (i + 1) for i, n in enumerate(names)}, headroom=1)
    assert load_scales(path, names) == shifts
    assert load_scales(path, reversed(names)) == shifts            # keyed by name, not by position
    doc = json.loads(path.read_text())
    assert doc["shifts"] == shifts and doc["headroom"] == 1
    # a wrong site name: one unknown and one missing
    wrong = dict(shifts)
    wrong["model.diffusion_model.input_blocks.9.0.in_layers.2.weight"] = wrong.pop(names[0])
    save_scales(path, wrong)
    with pytest.raises(KeyError):
        load_scales(path, names)
    # a missing site, an extra site
    save_scales(path, {n: shifts[n] for n in names[1:]})
    with pytest.raises(KeyError):
        load_scales(path, names)
    save_scales(path, dict(shifts, extra=3))
    with pytest.raises(KeyError):
        load_scales(path, names)
    # shifts outside the range or not integers
    for bad in (9, -17, 2.5, "3", True, None):
        with pytest.raises(ValueError):
            check_shifts(dict(shifts, **{names[2]: bad}), names)
    # not a scale file
    path.write_text(json.dumps({"shifts": shifts}))
    with pytest.raises(ValueError):
        load_scales(path, names)
    path.write_text(json.dumps([1, 2, 3]))
    with pytest.raises(ValueError):
        load_scales(path, names)


def test_dropin_module_keeps_and_clears_shifts_without_an_engine():
    """The UNet drop-in holds the shifts itself (the engine is rebuilt on dtype / device changes): set, read back, cleared
    by load_state_dict, kept across set_compute_dtype.  No engine exists on a machine without a GPU; none is needed."""
    from adaface_amd.configs import tiny_config
    from ldm.util import instantiate_from_config
    unet = instantiate_from_config(tiny_config()["model"]["params"]["unet_config"]).eval()
    assert unet.fp8_shifts() is None
    unet.set_fp8_shifts({"a": 1, "b": -2})
    assert unet.fp8_shifts() == {"a": 1, "b": -2}
    for bad in (2.5, 9, "3"):                     # values are checked at once (names only an engine can check)
        with pytest.raises(ValueError):
            unet.set_fp8_shifts({"a": bad})
    assert unet.fp8_shifts() == {"a": 1, "b": -2}
    unet.set_compute_dtype("fp8").set_compute_dtype("bf16")
    assert unet.fp8_shifts() == {"a": 1, "b": -2}
    unet.load_state_dict(unet.state_dict())
    assert unet.fp8_shifts() is None
    with pytest.raises(RuntimeError):
        unet.save_fp8_scales("/nonexistent/never-written.json")
