"""What the built gfx950 code object of af_conv_gemm.hip holds, read from it on the CPU.

Instruction budget of the K loop of conv3x3_halo8_kernel: the loop is a loop over channel chunks whose body is the nine tap
steps unrolled at compile time: every step between two s_barriers issues its 40 MFMAs with a fixed
skeleton of fragment reads, LDS-DMA pieces and waits around them.  The bookkeeping this replaced (per-step divisions, a
switch over the halo piece, per-lane selects, runtime tests of the wave group) cost ~190 SALU and ~40 branches per step,
and the loop was bound by instruction issue, not by the MFMAs.  This guards against it coming back.

The instantiations of conv_gemm_pp_kernel: exactly the ones launch_pp / launch_pp8 / launch_up_phase4 can reach, so that
unused schedule or epilogue variants do not quietly come back.
"""
import importlib.util
import re
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


def _functions():
    from adaface_amd import _lib, build
    obj = ROOT / "adaface_amd" / "_build" / "af_conv_gemm.hip.o"
    if not _lib.lib_path().exists() or not obj.exists():
        build.build(verbose=False)        # (a fresh tree only, as the ISA-hazard test does)
    mod = _load_scanner()
    with tempfile.TemporaryDirectory() as td:
        funcs = mod.disassemble(obj, Path(td))
    assert funcs, obj
    return funcs


def _kernel_code():
    funcs = _functions()
    code = [ins for name, ins in funcs if KERNEL in name]
    assert len(code) == 1, [name for name, _ in funcs]
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


# <BN, GATHER, LNMODE, FP8, SCHED>: SCHED 2 = merged, 0 = phased (GEGLU, which is BN 128 only and never a LayerNorm-statistics
# producer, and the gathers without tap masks, LNMODE 0 only); fp8 is merged-only with the plain epilogue
PP_EXPECTED = (
    {(bn, False, ln, False, 2) for bn in (128, 160) for ln in (0, 1, 2)}
    | {(bn, True, 0, False, 2) for bn in (128, 160)}
    | {(bn, gather, 0, True, 2) for bn in (128, 160) for gather in (False, True)}
    | {(128, False, ln, False, 0) for ln in (0, 1)}
    | {(bn, True, 0, False, 0) for bn in (128, 160)}
)
PP_MANGLED = re.compile(r"conv_gemm_pp_kernelILi(\d+)ELb([01])ELi(\d+)ELb([01])ELi(\d+)E")


def test_conv_gemm_pp_instantiations():
    found = set()
    for name, _ in _functions():
        m = PP_MANGLED.search(name)
        if m:
            found.add((int(m[1]), m[2] == "1", int(m[3]), m[4] == "1", int(m[5])))
    assert len(PP_EXPECTED) == 16
    assert found == PP_EXPECTED, (sorted(found - PP_EXPECTED), sorted(PP_EXPECTED - found))
