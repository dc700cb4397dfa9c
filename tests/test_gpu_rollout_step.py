"""GPU: k_rollout_step (csrc/sgo_rollout.hip) ply by ply on the constructed cases of tests/rollout_cases.py, bit for bit against
the oracle-based model tests/rollout_model.py.  The test builds every policy tensor itself and drives sgo_rollout_start_dev,
sgo_rollout_list, sgo_rollout_step and sgo_rollout_result through ctypes; after EVERY step it compares

 * records: the record each listed rollout wrote, word for word with rollout_model.expected_records;
 * bytes:   the whole array of 2 * max_rollouts records -- every word outside those records is as it was before the step;
 * list:    n_live / n_done and the new list, a duplicate-free permutation of the survivors' new record indices;

and at the end black_own, white_own and sums.  tests/test_rollout_step_power.py shows (no GPU) what these cases can catch."""
import ctypes as C

import numpy as np
import pytest

from tests import rollout_cases as RC
from tests import rollout_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


def _view(torch, address, shape):
    """int32 device memory of the rollout object as a tensor (RolloutEngine.source_records reads the records the same way)"""
    class _Mem(object):
        pass
    m = _Mem()
    m.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<i4", "data": (int(address), False), "version": 2}
    return torch.as_tensor(m, device="cuda")


def _drive(L, key):
    """One case from its start to its result; returns the number of steps."""
    import torch
    lib = L.load()
    c, e = RC.case(key), RC.expected(key)
    RW, NW, mr, n = 16 * c.NW, c.NW, c.max_rollouts, c.n_total
    h = C.c_void_p(lib.sgo_rollout_create(c.S, mr, c.n_src, 0))
    assert h, lib.sgo_last_error().decode()
    try:
        table = torch.from_numpy(c.records.view(np.int32)).cuda()
        index = torch.from_numpy(c.index).cuda()
        st = L.RolloutStatus()
        L.check(lib.sgo_rollout_start_dev(h, c.n_src, L.ptr(table), L.ptr(index), c.per_src, c.seed, c.max_plies, L.stream_ptr()),
                "sgo_rollout_start_dev")
        rec_p, idx_p = C.c_void_p(), C.c_void_p()
        assert lib.sgo_rollout_list(h, C.byref(rec_p), C.byref(idx_p)) == mr
        rec = _view(torch, rec_p.value, (2 * mr, RW))
        torch.cuda.synchronize()
        before = rec.cpu().numpy().view(np.uint32)
        lst = _view(torch, idx_p.value, (n,)).cpu().numpy()
        assert np.array_equal(lst, np.arange(n))                                  # list[0] is the identity after a start
        assert np.array_equal(before[:n], c.records[np.repeat(c.index, c.per_src)])
        live, t = n, 0
        while live:
            assert t < c.max_plies
            rid = np.where(lst >= mr, lst - mr, lst)
            out = np.where(lst >= mr, rid, rid + mr)
            assert np.array_equal(np.sort(rid), np.flatnonzero(e.action[t] >= 0)), (c.name, t)
            policy = torch.from_numpy(np.ascontiguousarray(e.rows[t][rid])).cuda()
            assert tuple(policy.shape) == (live, c.A)
            L.check(lib.sgo_rollout_step(h, L.ptr(policy), c.sym[t % len(c.sym)], L.stream_ptr(), C.byref(st)), "sgo_rollout_step")
            torch.cuda.synchronize()
            after = rec.cpu().numpy().view(np.uint32)
            want = before.copy()
            want[out] = M.expected_records(before[lst], e.pair[t][rid])
            if not np.array_equal(after, want):
                bad = np.flatnonzero((after != want).any(axis=1))
                listed = np.isin(bad, out)
                first = int(bad[0])
                g = int(first - mr if first >= mr else first)
                raise AssertionError("%s ply %d: %d records differ (%d of them not written by a listed rollout); first: record %d, "
                                     "rollout %d, model action %d, words %s" % (c.name, t, len(bad), int((~listed).sum()), first, g,
                                                                                 int(e.action[t][g]), np.flatnonzero(after[first] != want[first])[:8]))
            survivors = np.sort(out[e.live_after[t][rid]])
            assert (st.n_live, st.n_done, st.steps, st.error) == (len(survivors), n - len(survivors), t + 1, 0), (c.name, t)
            live = st.n_live
            assert lib.sgo_rollout_list(h, C.byref(rec_p), C.byref(idx_p)) == mr and rec_p.value == rec.data_ptr()
            lst = _view(torch, idx_p.value, (live,)).cpu().numpy() if live else np.zeros(0, np.int32)
            assert np.array_equal(np.sort(lst), survivors), (c.name, t)         # survivors is duplicate-free: so is the list
            before = after
            t += 1
        assert t == int(e.plies.max())
        black, white = np.zeros((c.n_src, c.N), np.int32), np.zeros((c.n_src, c.N), np.int32)
        sums = np.zeros((c.n_src, 8), np.int64)
        L.check(lib.sgo_rollout_result(h, c.n_src, L.ptr(black), L.ptr(white), L.ptr(sums)), "sgo_rollout_result")
        for name, got, want in (("black_own", black, e.black_own), ("white_own", white, e.white_own), ("sums", sums, e.sums)):
            if not np.array_equal(got, want):
                s = int(np.flatnonzero((got != want).any(axis=1))[0])
                raise AssertionError("%s %s: source %d of %d differs: %s, model %s" % (c.name, name, s, c.n_src, got[s], want[s]))
        print("%s: %d rollouts of %d sources, %d steps, records, bytes, lists and results equal the model's" % (c.name, n, c.n_src, t))
        return t
    finally:
        lib.sgo_rollout_destroy(h)


@pytest.mark.parametrize("S", RC.SIZES)
def test_shape_probes(L, S):
    """Every position of rule_shapes_S<S>.npz, one rollout per empty point (and two occupied ones) with a one-hot row: the
    legality of every point, make_play on every legal one, the scoring fill on every position that results.  Positions whose
    side to move has no legal board point pass; their second ply ends them."""
    assert _drive(L, ("probes", S, False)) == 1
    assert _drive(L, ("probes", S, True)) == 2


@pytest.mark.parametrize("S", RC.SIZES)
def test_chains(L, S):
    """One probe in eight continued to three plies with HashNet rows under sym_k 0, 3, 6: the ping-pong back into the first
    record and three plies of history."""
    assert _drive(L, ("chains", S)) == 3


@pytest.mark.parametrize("S", RC.BOUNDARY_SIZES)
def test_pick_boundaries(L, S):
    """Weights built so that t sits on or just below a prefix sum at the first and last two legal points, across a row end,
    across a row without a legal point, at t = 0 and t = T - 1; on the empty board, a dense position and a ko position."""
    for where in ("empty", "dense", "ko"):
        _drive(L, ("boundaries", S, where))


def test_largest_total(L):
    """361 weights of 2^20 + 1: prefix sums beyond 2^28 in the uint32 scan."""
    _drive(L, ("max_total",))


@pytest.mark.parametrize("S", RC.BOUNDARY_SIZES)
def test_special_values(L, S):
    """NaN, +-0, negatives, infinities, 1.0 and its neighbours, 2.0, 2^-20 and the float below, denormals on every legal point
    in turn; NaN and +inf in the pass entry."""
    for where in ("empty", "dense"):
        _drive(L, ("specials", S, where))


@pytest.mark.parametrize("S", (13, 19))
def test_symmetry(L, S):
    """The pick-boundary rows of the dense (asymmetric) position handed over under each sym_k."""
    for k in range(8):
        _drive(L, ("boundaries", S, "dense", k))


@pytest.mark.parametrize("S", RC.SIZES)
def test_wave_neighbours(L, S):
    """The deepest scoring fill beside one that ends at once, in both orders in one wave, beside an idle half, and alone."""
    for order in RC.NEIGHBOUR_ORDERS:
        _drive(L, ("neighbours", S, order))


def test_contention(L):
    """4 096 rollouts of one source all end on step 2 and add to the same counters: the exact counts, black winning and (the
    colour mirror) white winning; and 8 sources x 512."""
    R = 4096
    cols = np.arange(25) % 5
    for first, sign in ((0, 1), (1, -1)):
        key = ("contention", 1, R, first)
        e = RC.expected(key)
        left, right = np.where(cols < 3, R, 0), np.where(cols >= 3, R, 0)
        assert np.array_equal(e.black_own[0], left if sign > 0 else right) and np.array_equal(e.white_own[0], right if sign > 0 else left)
        assert e.sums[0].tolist() == [R if sign > 0 else 0, R if sign < 0 else 0, 0, sign * 5 * R, 25 * R, 2 * R, 0, R]
        assert _drive(L, key) == 2
    assert _drive(L, ("contention", 8, 512)) == 2
