"""The structure csrc/sgo_connect.hip promises, held on its compiled code (no GPU needed), with the tool and the checks
tests/test_solve_isa.py uses on csrc/sgo_solve.hip: k_connect_pairs<S>, k_connect_read<S> and k_connect_groups<S> keep their row
bitboards in registers (the reader's frames and the group labels in LDS), so every device function they reach (the ply, the legal set,
the floods) must be inlined -- no call instruction, no function emitted besides the kernels -- and no kernel may use scratch.  One
kernel of each per board size.  Register counts are not pinned: they move with the compiler."""
import pytest

from tests.test_engine_isa import SIZES, _tool, kernel_descriptors, structure_problems


def test_connect_kernels_are_call_free_and_scratch_free():
    asm = _tool().device_asm(source="sgo_connect.hip")
    if asm is None:
        pytest.skip("no hipcc")
    kern = kernel_descriptors(asm)
    for s in SIZES:
        assert sum(k.startswith("_ZN3sgo15k_connect_pairsILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
        assert sum(k.startswith("_ZN3sgo14k_connect_readILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
        assert sum(k.startswith("_ZN3sgo16k_connect_groupsILi%dEE" % s) for k in kern) == 1, (s, sorted(kern))
    assert len(kern) == 3 * len(SIZES)
    assert structure_problems(asm) == []
