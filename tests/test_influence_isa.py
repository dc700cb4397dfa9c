"""The structure csrc/sgo_influence.hip promises, held on its compiled code (no GPU needed), with the tool and the checks
tests/test_engine_isa.py uses on csrc/sgo_engine.hip: k_influence<S> keeps the S values of a board row in registers, so every
device function it reaches must be inlined -- no call instruction, no function emitted besides the kernels -- and no kernel may use
scratch (a dynamically indexed value array would go there).  One kernel per board size.  Register counts are not pinned: they move
with the compiler."""
import pytest

from tests.test_engine_isa import SIZES, _tool, kernel_descriptors, structure_problems


def test_influence_kernels_are_call_free_and_scratch_free():
    asm = _tool().device_asm(source="sgo_influence.hip")
    if asm is None:
        pytest.skip("no hipcc")
    kern = kernel_descriptors(asm)
    for s in SIZES:
        assert sum(k.startswith("_ZN3sgo11k_influenceILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
    assert len(kern) == len(SIZES)
    assert structure_problems(asm) == []
