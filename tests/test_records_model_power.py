"""CPU: every fault switch of tests/records_model.py changes a value the GPU tests compare, on a case those tests run."""
import numpy as np
import pytest

from tests import records_model as M
from tests.test_gpu_records import _score_case

S = 5
REPLAY_CASES = {"write_after_refusal": ("refuse_middle", "written"), "in_turn_only": ("white_setup", "records")}


@pytest.fixture(scope="module")
def legal():
    return M.replay(S, _score_case(S, 0, 1, 1)[0])["legal"]


@pytest.mark.parametrize("fault", [f for f in M.FAULTS if f in REPLAY_CASES])
def test_replay_faults_show(fault):
    name, key = REPLAY_CASES[fault]
    game = M.constructed_games(S)[name]
    good, bad = M.replay(S, [game]), M.replay(S, [game], fault)
    assert not np.array_equal(good[key], bad[key])
    if fault == "in_turn_only":
        assert not np.array_equal(M.replay(S, [M.constructed_games(S)["handicap"]])["records"],
                                  M.replay(S, [M.constructed_games(S)["handicap"]], fault)["records"])


@pytest.mark.parametrize("fault", [f for f in M.FAULTS if f not in REPLAY_CASES])
def test_score_faults_show(fault, legal):
    """the 300-row case of test_score_rows_bit_for_bit under symmetry 4"""
    n, k, NB = 300, 4, 7
    _, index, target, z, bucket, policy, value = _score_case(S, 100 + n + k, n, NB)
    good = M.score(S, legal, index, target, z, bucket, NB, policy, value, k)
    bad = M.score(S, legal, index, target, z, bucket, NB, policy, value, k, fault)
    changed = [key for key in ("rank", "best", "flags", "counters") if not np.array_equal(good[key], bad[key])]
    changed += ["p_target"] if not np.array_equal(good["p_target"].view(np.uint32), bad["p_target"].view(np.uint32)) else []
    assert changed, fault


def test_model_agrees_with_the_golden_records():
    """the model's own replay against the reference: hashes and masks of the first 40 plies of golden game 1"""
    from tests.helpers import load, sha8, unpack_mask
    z = load("sgf_S19.npz")
    mv = z["g01_moves"][:40]
    acts = [361 if y >= 19 else int(y) * 19 + int(x) for x, y, _ in mv]
    w = M.replay(19, [(acts, [int(c) for _, _, c in mv])])
    bits = np.unpackbits(w["legal"].view(np.uint8), axis=1, bitorder="little")[:, :362]
    for k in range(41):
        assert np.array_equal(sha8(w["boards"][k]), z["g01_hashes"][k])
        assert np.array_equal(bits[k], 1 - unpack_mask(z["g01_masks"][k], 362))
