"""The structure csrc/sgo_race.hip promises, held on its compiled code (no GPU needed), with the tool and the checks
tests/test_solve_isa.py uses on csrc/sgo_solve.hip: k_race_pairs<S> and k_race_read<S> keep their row bitboards in registers (the
reader's frames in LDS), so every device function they reach (the ply, the legal set, the floods) must be inlined -- no call
instruction, no function emitted besides the kernels -- and no kernel may use scratch.  One kernel of each per board size.
Register counts are not pinned: they move with the compiler."""
import pytest

from tests.test_engine_isa import SIZES, _tool, kernel_descriptors, structure_problems


def test_race_kernels_are_call_free_and_scratch_free():
    asm = _tool().device_asm(source="sgo_race.hip")
    if asm is None:
        pytest.skip("no hipcc")
    kern = kernel_descriptors(asm)
    for s in SIZES:
        assert sum(k.startswith("_ZN3sgo12k_race_pairsILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
        assert sum(k.startswith("_ZN3sgo11k_race_readILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
    assert len(kern) == 2 * len(SIZES)
    assert structure_problems(asm) == []
