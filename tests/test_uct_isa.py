"""The structure csrc/sgo_uct.hip promises, held on its compiled code (no GPU needed), with the tool and the checks
tests/test_engine_isa.py uses on csrc/sgo_engine.hip: k_uct keeps the game of the running simulation and the ownership counts of its
tree in registers, a board row per lane, so every device function it reaches must be inlined -- no call instruction, no function
emitted besides the kernels -- and no kernel may use scratch.  One k_uct per board size and the two small kernels (zeroing, best).
Register counts are not pinned: they move with the compiler."""
import pytest

from tests.test_engine_isa import SIZES, _tool, kernel_descriptors, structure_problems


def test_uct_kernels_are_call_free_and_scratch_free():
    asm = _tool().device_asm(source="sgo_uct.hip")
    if asm is None:
        pytest.skip("no hipcc")
    kern = kernel_descriptors(asm)
    for s in SIZES:
        assert sum(k.startswith("_ZN3sgo5k_uctILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
    assert sum(k.startswith("_ZN3sgo10k_uct_zero") for k in kern) == 1, sorted(kern)
    assert sum(k.startswith("_ZN3sgo10k_uct_best") for k in kern) == 1, sorted(kern)
    assert len(kern) == len(SIZES) + 2
    assert structure_problems(asm) == []
