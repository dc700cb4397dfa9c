"""CPU: the model of the position keys (tests/keys_model.py) has the properties include/sgo.h states, and the case set the GPU
test runs (tests/test_gpu_keys.py) notices every fault switch of the model -- a green GPU run means something."""
import numpy as np
import pytest

from tests import keys_model as K


def _stones(S, rec):
    NW = (S * S + 31) // 32
    rec = np.asarray(rec, np.uint32).reshape(16, NW)
    black, white = np.flatnonzero(K._bits(rec[0])[:S * S]), np.flatnonzero(K._bits(rec[1])[:S * S])
    return [int(a) for a in black], [int(a) for a in white], bool(rec[0, NW - 1] >> 31)


@pytest.mark.parametrize("S", K.SIZES)
def test_canon_and_action_are_invariant_under_all_eight(S):
    """the record of the position moved by g with the target moved by g has the same (canon, canon_action), for every g"""
    N = S * S
    names, recs = K.case_records(S)
    L = K.luts(S)
    pick = range(len(recs)) if S <= 9 else range(0, len(recs), 5)
    for r in pick:
        b, w, wtp = _stones(S, recs[r])
        targets = [N, (7 * r) % N, (13 * r + 5) % N, N - 1, 0]
        base = [K.outputs(S, K.record_keys(S, recs[r]), t) for t in targets]
        for g in range(1, 8):
            key = K.record_keys(S, K.build_record(S, K.moved(S, g, b), K.moved(S, g, w), wtp))
            for t, want in zip(targets, base):
                got = K.outputs(S, key, int(L[g, t]))
                assert (got[1], got[3]) == (want[1], want[3]), (names[r], g, t)
                assert bin(got[2]).count("1") == bin(want[2]).count("1")


@pytest.mark.parametrize("S", K.SIZES)
def test_masks_have_the_size_of_the_symmetry_group(S):
    for name, b, w, order in K.case_positions(S):
        for wtp in (False, True):
            _, canon, mask, _ = K.outputs(S, K.record_keys(S, K.build_record(S, b, w, wtp)), None)
            assert bin(mask).count("1") == order and mask != 0, (name, mask)
            if name == "empty":
                assert mask == 255 and canon == (K.z(S, 2, 0) if wtp else 0)
    m = S - 1
    mid = K.outputs(S, K.record_keys(S, K.build_record(S, [(m // 2) * S + 0], [], False)), None)      # a stone on a mid-line
    assert bin(mid[2]).count("1") == 2


def test_constants_and_tables():
    """sm on a known value of the generator it is (splitmix64 from state 0), the tables against the package's integer form, the
    inverse tables differ for k = 4 and 6 only"""
    from sejonggo_amd import records as R
    assert K.sm(0) == 0xE220A8397B1DCDAF
    assert int(R.sm64(np.array([0, 5], np.uint64))[0]) == K.sm(0) and int(R.sm64(np.array([0, 5], np.uint64))[1]) == K.sm(5)
    for S in K.SIZES:
        assert np.array_equal(R.sym_luts(S), K.luts(S))
        differ = [k for k in range(8) if not np.array_equal(K.luts(S)[k], K.luts(S, True)[k])]
        assert differ == [4, 6]


@pytest.mark.parametrize("S", K.SIZES)
@pytest.mark.parametrize("fault", K.FAULTS)
def test_every_fault_is_noticed_by_the_gpu_case_set(S, fault):
    names, recs = K.case_records(S)
    if S > 9:                                         # the model is slow on the large boards: the constructed half and four goldens
        keep = [i for i, n in enumerate(names) if not n.startswith("golden")][::3] + [i for i, n in enumerate(names) if n.startswith("golden")][:4]
        names, recs = [names[i] for i in keep], recs[keep]
    index, target = K.case_rows(S, names, len(recs))
    good, bad = K.keys(S, recs, index, target), K.keys(S, recs, index, target, fault=fault)
    assert any(not np.array_equal(good[k], bad[k]) for k in good), fault
