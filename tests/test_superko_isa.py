"""The structure csrc/sgo_superko.hip promises, held on its compiled code (no GPU needed), with the tool and the checks
tests/test_engine_isa.py uses on csrc/sgo_engine.hip: the two stages keep a board row per lane in registers, so every device
function they reach must be inlined -- no call instruction, no function emitted besides the kernels -- and no kernel may use
scratch.  One kernel per stage and board size.  Register counts are not pinned: they move with the compiler."""
import pytest

from tests.test_engine_isa import SIZES, _tool, kernel_descriptors, structure_problems


def test_superko_kernels_are_call_free_and_scratch_free():
    asm = _tool().device_asm(source="sgo_superko.hip")
    if asm is None:
        pytest.skip("no hipcc")
    kern = kernel_descriptors(asm)
    for s in SIZES:
        assert sum(k.startswith("_ZN3sgo9k_superkoILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
        assert sum(k.startswith("_ZN3sgo14k_superko_keysILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
    assert len(kern) == 2 * len(SIZES)
    assert structure_problems(asm) == []
