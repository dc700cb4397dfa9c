"""GPU: the device PUCT selector on its own.  sgo_debug_top_one writes a child table into a slot's root block and runs
Eng<S>::top_one on it -- the function every descent step of k_search calls -- so its score arithmetic is compared with the
reference's outputs bit for bit: on tests/golden/puct_ties.npz (two children equal or one ulp apart, for the three device
geometries; tests/test_selector_power.py shows that a reassociated, widened or wrong-regime score fails it) and on the 600
random tables of puct.npz.  Whole games observe only the argmax and cannot see a last-bit error of a score."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import selector_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


def _context(L, S, n_games):
    cfg = L.Config(size=S, n_games=n_games, sims=16, energy=8, stop_exploration=0, num_moves=4, blocks_per_game=0, self_play=1,
                   komi=5.5, dirichlet_epsilon=0.25, device_id=0, two_model=0, shared_blocks=0)
    ctx = C.c_void_p(L.load().sgo_ctx_create(C.byref(cfg)))
    assert ctx, L.load().sgo_last_error().decode()
    return ctx


def _device_top_one(L, ctx, z, rows, root64):
    """The device selector's answers for cases `rows` (all of one regime) of table set z, in that order."""
    import torch
    lib = L.load()
    A = z["P"].shape[1]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[rows], dtype=dt)).cuda()
    P64, P32 = dev(z["P"], np.float64), dev(z["P"].astype(np.float32), np.float32)
    N, Q, V, EX = dev(z["N"], np.int32), dev(z["Q"], np.float32), dev(z["V"], np.int8), dev(z["EX"], np.uint8)
    out = torch.full((len(rows),), -7, dtype=torch.int32, device="cuda")
    for t in (P64, P32, N, Q, V, EX):
        assert t.is_contiguous() and t.shape == (len(rows), A)
    L.check(lib.sgo_debug_top_one(ctx, len(rows), L.ptr(P32), L.ptr(P64) if root64 else None, L.ptr(N), L.ptr(Q), L.ptr(V),
                                  L.ptr(EX), int(root64), L.ptr(out), L.stream_ptr()), "sgo_debug_top_one")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _describe(z, names, rows, got):
    bad = []
    for c, g in zip(rows, got):
        if g != z["out_vl"][c]:
            bad.append("case %d (%s, %s, pair %s): device %d, reference %d" % (
                c, "float64 root" if z["F64"][c] else "float32", names[z["cls"][c]] if names else "random table",
                (int(z["I"][c]), int(z["J"][c])) if names else "-", g, z["out_vl"][c]))
    return bad


@pytest.mark.parametrize("S", [5, 9, 19])
def test_device_selector_equals_the_reference(L, S):
    A = S * S + 1
    sets = [(z, names) for a, z, names in selector_tables("puct_ties.npz") if a == A]
    assert len(sets) == 1
    if S == 9:
        sets += [(z, names) for a, z, names in selector_tables("puct.npz") if a == A]
        assert len(sets) == 2
    ctx = _context(L, S, 37)                # 37 slots: the cases run in several chunks, the last one partial
    try:
        n_run = 0
        for z, names in sets:
            assert z["P"].shape[1] == A
            for root64 in (0, 1):
                rows = np.flatnonzero(z["F64"] == root64)
                assert len(rows) > 90
                got = _device_top_one(L, ctx, z, rows, root64)
                bad = _describe(z, names, rows, got)
                assert not bad, "%d of %d cases differ:\n%s" % (len(bad), len(rows), "\n".join(bad[:40]))
                # another order puts every case behind another one in another slot's block: nothing of the block's previous
                # contents (busy flags, float64 priors, legal words) may leak into the next answer
                perm = np.random.RandomState(S + root64).permutation(len(rows))
                got2 = _device_top_one(L, ctx, z, rows[perm], root64)
                bad = _describe(z, names, rows[perm], got2)
                assert not bad, "shuffled order: %d of %d cases differ:\n%s" % (len(bad), len(rows), "\n".join(bad[:40]))
                n_run += len(rows)
        assert n_run == sum(len(z["F64"]) for z, _ in sets)
    finally:
        L.load().sgo_ctx_destroy(ctx)


def test_selector_hook_refuses_a_context_with_games_in_flight(L):
    import torch
    from sejonggo_amd.engine import SelfPlayEngine
    from sejonggo_amd.stub_nets import make_stub
    S, A = 5, 26
    eng = SelfPlayEngine(make_stub("hash", S), size=S, n_games=2, sims=16, energy=8, stop_exploration=0, num_moves=2,
                         symmetry="identity")
    z = selector_tables("puct_ties.npz")[0][1]
    rows = np.flatnonzero(z["F64"] == 0)[:2]
    assert (_device_top_one(L, eng.ctx, z, rows, 0) == z["out_vl"][rows]).all()           # idle context: served
    eng.start_games([0])
    torch.cuda.synchronize()
    with pytest.raises(L.SgoError, match="in flight"):
        _device_top_one(L, eng.ctx, z, rows, 0)
    games = eng.run()                                                                      # the game was not disturbed
    assert len(games) == 1 and len(games[0]["moves"]) == 2
    eng.close()
