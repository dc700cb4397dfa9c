"""The structure csrc/sgo_solve.hip promises, held on its compiled code (no GPU needed), with the tool and the checks
tests/test_secure_isa.py uses on csrc/sgo_secure.hip: k_solve_targets<S> and k_solve_read<S> keep their row bitboards in registers
(the reader's frames in LDS), so every device function they reach (the ply, the legal set, life_core) must be inlined -- no call
instruction, no function emitted besides the kernels -- and no kernel may use scratch.  One kernel of each per board size.
Register counts are not pinned: they move with the compiler."""
import pytest

from tests.test_engine_isa import SIZES, _tool, kernel_descriptors, structure_problems


def test_solve_kernels_are_call_free_and_scratch_free():
    asm = _tool().device_asm(source="sgo_solve.hip")
    if asm is None:
        pytest.skip("no hipcc")
    kern = kernel_descriptors(asm)
    for s in SIZES:
        assert sum(k.startswith("_ZN3sgo15k_solve_targetsILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
        assert sum(k.startswith("_ZN3sgo12k_solve_readILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
    assert len(kern) == 2 * len(SIZES)
    assert structure_problems(asm) == []
