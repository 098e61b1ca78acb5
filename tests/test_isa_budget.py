"""Instruction budget of the K loop of conv3x3_halo8_kernel, read from the built gfx950 code object (CPU only).

The loop is a loop over channel chunks whose body is the nine tap steps unrolled at compile time: every
step between two s_barriers issues its 40 MFMAs with a fixed skeleton of fragment reads, LDS-DMA pieces and waits around
them.  The bookkeeping this replaced (per-step divisions, a switch over the halo piece, per-lane selects, runtime tests of
the wave group) cost ~190 SALU and ~40 branches per step, and the loop was bound by instruction issue, not by the MFMAs.
This guards against it coming back.
"""
import importlib.util
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
KERNEL = "conv3x3_halo8_kernelILi0E"     # the library's instantiation (LABL = 0)
BRANCH = ("s_cbranch", "s_branch", "s_setpc")
NOT_SALU = BRANCH + ("s_waitcnt", "s_nop", "s_barrier", "s_setprio")


def _load_scanner():
    spec = importlib.util.spec_from_file_location("check_isa_hazards", ROOT / "scripts" / "check_isa_hazards.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _kernel_code():
    from adaface_amd import _lib, build
    obj = ROOT / "adaface_amd" / "_build" / "af_conv_gemm.hip.o"
    if not _lib.lib_path().exists() or not obj.exists():
        build.build(verbose=False)        # (a fresh tree only, as the ISA-hazard test does)
    mod = _load_scanner()
    with tempfile.TemporaryDirectory() as td:
        funcs = mod.disassemble(obj, Path(td))
    code = [ins for name, ins in funcs or [] if KERNEL in name]
    assert len(code) == 1, [name for name, _ in funcs or []]
    return code[0]


def _steps(ins):
    """K steps: from each s_barrier to the next s_barrier or the first branch (the loop's back-edge closes the last step of
    a chunk; what follows it is the loop exit), keeping the pieces that issue MFMAs."""
    steps, cur = [], None
    for t in ins:
        if t.startswith("s_barrier"):
            if cur:
                steps.append(cur)
            cur = []
        elif cur is not None:
            cur.append(t)
            if t.startswith(BRANCH):
                steps.append(cur)
                cur = None
    if cur:
        steps.append(cur)
    return [s for s in steps if any(t.startswith("v_mfma") for t in s)]


def test_halo8_k_loop_instruction_budget():
    steps = _steps(_kernel_code())
    # two bodies (one per wave group) of nine tap steps each
    assert len(steps) == 18, len(steps)
    for k, s in enumerate(steps):
        mfma = sum(t.startswith("v_mfma") for t in s)
        salu = sum(t.startswith("s_") and not t.startswith(NOT_SALU) for t in s)
        cond = sum(t.startswith("s_cbranch") for t in s)
        what = f"step {k}: {len(s)} instructions, {mfma} MFMA, {salu} SALU, {cond} conditional branches"
        # a step is one straight run: a branch inside it would leave fewer than its 40 MFMAs before the cut
        assert mfma == 40, what
        assert len(s) <= 120, what
        assert salu <= 30, what
        assert cond <= 1, what                      # the back-edge, on the last tap only
        assert not any(t.startswith("v_cndmask") for t in s), what
    # the back-edges: the last tap of each body ends in the one conditional branch
    assert [k for k, s in enumerate(steps) if s[-1].startswith("s_cbranch")] == [8, 17]
