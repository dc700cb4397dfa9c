"""The structure csrc/sgo_playout.hip promises, held on its compiled code (no GPU needed), with the tool and the checks
tests/test_engine_isa.py uses on csrc/sgo_engine.hip: k_playout keeps a whole game and four accumulator tables in registers, a board
row per lane, so every device function it reaches must be inlined -- no call instruction, no function emitted besides the kernels --
and no kernel may use scratch.  One k_playout per board size and the one zeroing kernel.  Register counts are not pinned: they move
with the compiler."""
import pytest

from tests.test_engine_isa import SIZES, _tool, kernel_descriptors, structure_problems


def test_playout_kernels_are_call_free_and_scratch_free():
    asm = _tool().device_asm(source="sgo_playout.hip")
    if asm is None:
        pytest.skip("no hipcc")
    kern = kernel_descriptors(asm)
    for s in SIZES:
        assert sum(k.startswith("_ZN3sgo9k_playoutILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
    assert sum(k.startswith("_ZN3sgo14k_playout_zero") for k in kern) == 1, sorted(kern)
    assert len(kern) == len(SIZES) + 1
    assert structure_problems(asm) == []
