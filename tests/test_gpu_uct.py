"""GPU: the playout tree search (include/sgo.h "playout tree search", csrc/sgo_uct.hip) against the model (tests/uct_model.py) word for
word -- visits, wins2, rave, own, sums, info and the trace of every simulation -- at every board size and under both rule sets, on the
runs tests/test_uct_model_power.py shows to notice the model's fault switches (tests/uct_cases.py).  The model's rows are computed
once per process and shared.  Whole games are played at 5x5, 7x7 and 9x9 only; the model takes a few seconds per size."""
import functools

import numpy as np
import pytest

from tests import uct_cases as UC
from tests import uct_model as UM

pytestmark = pytest.mark.gpu

SGO_ERR_ARG = -1
FILL32, FILL64 = 0x3C3C3C3C, 0x5A5A5A5A5A5A5A5A
GRID_UNITS = 2 * (1 << 15)                                           # csrc/sgo_uct.hip: two trees per workgroup, UCT_MAX_BLOCKS
KEYS = ("visits", "wins2", "rave", "own", "sums", "info", "trace")
OPTIONAL = ("rave", "own", "trace")


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _args(p):
    """the ints of a run between d_index and the outputs"""
    max_nodes = p["sims"] + 1 if p["max_nodes"] is None else p["max_nodes"]
    return (p["trees"], p["sims"], p["seed"], p["rules"], p["max_plies"], p["komi2"], p["expand_at"], p["rave_equiv"], p["prior"], max_nodes)


def _buffers(S, n, trees, sims, pad, make):
    N = S * S
    return {"visits": make((n + pad, N + 1), FILL32, "int32"), "wins2": make((n + pad, N + 1), FILL32, "int32"),
            "rave": make((n + pad, 2, N + 1), FILL32, "int32"), "own": make((n + pad, 2, N), FILL32, "int32"),
            "sums": make((n + pad, 8), FILL64, "int64"), "info": make((n + pad, 4), FILL32, "int32"),
            "trace": make(((n + pad) * trees, sims), FILL32, "int32")}


def _run(S, records, p, n=None, pad=2, without=()):
    """sgo_uct_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    index = p["index"]
    R = len(records)
    n = (R if index is None else len(index)) if n is None else n
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev) if index is not None else None
    out = _buffers(S, n, p["trees"], p["sims"], pad, lambda shape, fill, dt: torch.full(shape, fill, dtype=getattr(torch, dt), device=dev))
    a = _args(p)
    wb = lib.sgo_uct_workspace(S, n, a[0], a[-1])
    assert wb >= 0
    work = torch.empty(max(wb, 4) // 4, dtype=torch.int32, device=dev)
    rc = lib.sgo_uct_dev(S, n, L.ptr(d_rec), R, L.ptr(d_idx), *a, *[None if k in without else L.ptr(out[k]) for k in KEYS], L.ptr(work), wb,
                         L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, n, trees, what, without=()):
    """every word of the seven outputs; the rows behind n (and a table the call was not given) are as they were filled"""
    for k in KEYS:
        rows_ = n * trees if k == "trace" else n
        fill = FILL64 if k == "sums" else FILL32
        if k in without:
            assert (got[k] == fill).all(), (what, k, "a table that was not to be written")
            continue
        assert (got[k][rows_:] == fill).all(), (what, k, "rows behind n")
        if not n:
            continue
        g, w = got[k][:rows_].reshape(rows_, -1), want[k][:rows_].reshape(rows_, -1)
        assert g.dtype == w.dtype, (what, k, g.dtype, w.dtype)
        bad = np.flatnonzero((g != w).any(axis=1))
        if len(bad):
            i = int(bad[0])
            at = np.flatnonzero(g[i] != w[i])[:8]
            raise AssertionError((what, k, "rows", bad[:8].tolist(), "row", i, "at", at.tolist(), g[i][at].tolist(), w[i][at].tolist()))


def _check(S, got, want, n, trees, what, without=()):
    _same(got, want, n, trees, what, without)


@pytest.mark.parametrize("S", UM.SIZES)
def test_runs_word_for_word(S):
    """every run of the case set: both rule sets, trees of 1, 2 and 3, expand_at of 0 and 2, a pool too small, komi2 = 0 with draws and
    an odd komi2, games that end inside the tree, depth 64 reached and held"""
    recs = UC.case_records(S)[1]
    for name, p in UC.runs(S).items():
        want = UC.run_model(S, name)
        _check(S, _run(S, recs, p), want, len(want["sums"]), p["trees"], (S, name))


@functools.lru_cache(maxsize=None)
def _listed(S, rules):
    names, recs = UC.case_records(S)
    R = len(recs)
    rng = np.random.RandomState(S)
    index = tuple(np.concatenate([rng.permutation(R)[:10], [0, 0, R, R - 1, -1, 1, 1 << 30]]).astype(int).tolist())
    p = dict(UC.DEFAULTS, index=index, trees=2, sims=12, seed=21, rules=rules, max_plies=6, komi2=-1, expand_at=1)
    return p, UM.search(S, recs, **p)


@pytest.mark.parametrize("S", UM.SIZES)
def test_index_list_null_tables_and_host_twin(S):
    """a list that permutes the records, repeats some and holds entries out of range (their rows are zero, best = -1; g counts the list
    position); the same without rave, own and trace; the host entry on the same list, with and without the tables"""
    L, lib = _lib()
    recs = UC.case_records(S)[1]
    R = len(recs)
    for rules in (0, 1):
        p, want = _listed(S, rules)
        n = len(p["index"])
        assert not want["sums"][[12, 14, 16]].any() and want["sums"][:10, 7].all() and want["info"][[12, 14, 16], 3].tolist() == [-1] * 3
        _check(S, _run(S, recs, p), want, n, 2, (S, "listed", rules))
        _check(S, _run(S, recs, p, without=OPTIONAL), want, n, 2, (S, "no tables", rules), without=OPTIONAL)
        index = np.asarray(p["index"], np.int32)
        for without in ((), OPTIONAL):
            out = _buffers(S, n, 2, p["sims"], 1, lambda shape, fill, dt: np.full(shape, fill, getattr(np, dt)))
            rc = lib.sgo_uct(S, R, L.ptr(np.ascontiguousarray(recs)), n, L.ptr(index), *_args(p),
                             *[None if k in without else L.ptr(out[k]) for k in KEYS])
            assert rc == 0, lib.sgo_last_error()
            _check(S, out, want, n, 2, (S, "host twin", rules, without), without=without)


def test_n_of_0_1_2_3_and_the_refusals():
    import torch
    L, lib = _lib()
    S = 7
    recs = UC.case_records(S)[1]
    R = len(recs)
    p = dict(UC.runs(S)["short"], index=None)
    want = UC.run_model(S, "short")                                  # its list is every record in order
    for n in (0, 1, 2, 3):
        _check(S, _run(S, recs, p, n=n), want, n, 1, ("n", n))
    dev = torch.device("cuda", 0)
    d_rec = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32)).to(dev)
    out = _buffers(S, 2, 2, 8, 0, lambda shape, fill, dt: torch.full(shape, fill, dtype=getattr(torch, dt), device=dev))
    wb = lib.sgo_uct_workspace(S, 2, 2, 9)
    work = torch.empty(wb // 4, dtype=torch.int32, device=dev)
    ok = dict(S=S, n=2, rec=L.ptr(d_rec), R=R, trees=2, sims=8, rules=1, max_plies=0, komi2=0, expand_at=2, rave_equiv=64, prior=4, max_nodes=9,
              visits=L.ptr(out["visits"]), wins2=L.ptr(out["wins2"]), sums=L.ptr(out["sums"]), info=L.ptr(out["info"]), work=L.ptr(work), wb=wb)
    N = S * S
    bad = [dict(S=6), dict(n=-1), dict(R=-1), dict(trees=0), dict(trees=UM.MAX_TREES + 1), dict(sims=0), dict(sims=UM.MAX_SIMS + 1), dict(rules=2),
           dict(rules=-1), dict(max_plies=4 * N + 1), dict(komi2=4 * N + 1), dict(komi2=-4 * N - 1), dict(expand_at=-1), dict(expand_at=9),
           dict(rave_equiv=-1), dict(rave_equiv=(1 << 20) + 1), dict(prior=-1), dict(prior=1025), dict(max_nodes=0), dict(max_nodes=10),
           dict(rec=None), dict(visits=None), dict(wins2=None), dict(sums=None), dict(info=None), dict(work=None), dict(wb=wb - 1),
           dict(n=1 << 12, trees=1 << 10, sims=1 << 10, max_nodes=1)]

    def call(a):
        return lib.sgo_uct_dev(a["S"], a["n"], a["rec"], a["R"], None, a["trees"], a["sims"], 1, a["rules"], a["max_plies"], a["komi2"], a["expand_at"],
                               a["rave_equiv"], a["prior"], a["max_nodes"], a["visits"], a["wins2"], L.ptr(out["rave"]), L.ptr(out["own"]), a["sums"],
                               a["info"], L.ptr(out["trace"]), a["work"], a["wb"], L.stream_ptr())
    for change in bad:
        assert call(dict(ok, **change)) == SGO_ERR_ARG, change
    assert lib.sgo_uct_workspace(6, 1, 1, 1) < 0 and lib.sgo_uct_workspace(S, -1, 1, 1) < 0 and lib.sgo_uct_workspace(S, 1, 0, 1) < 0
    assert lib.sgo_uct_workspace(S, 1, 1, 0) < 0 and lib.sgo_uct_workspace(S, 0, 1, 1) == 0 and lib.sgo_uct_workspace(S, 3, 2, 5) == 3 * lib.sgo_uct_workspace(S, 1, 2, 5)
    h = _buffers(S, 2, 2, 8, 0, lambda shape, fill, dt: np.full(shape, fill, getattr(np, dt)))
    hrec = L.ptr(np.ascontiguousarray(recs))
    tail = [L.ptr(h[k]) for k in KEYS]
    assert lib.sgo_uct(S, R, hrec, 2, None, 2, 8, 1, 3, 0, 0, 2, 64, 4, 9, *tail) == SGO_ERR_ARG
    assert lib.sgo_uct(S, R, None, 2, None, 2, 8, 1, 1, 0, 0, 2, 64, 4, 9, *tail) == SGO_ERR_ARG
    assert lib.sgo_uct(S, R, hrec, 2, None, 2, 8, 1, 1, 0, 0, 2, 64, 4, 10, *tail) == SGO_ERR_ARG
    torch.cuda.synchronize()
    for k in KEYS:
        assert (out[k].cpu().numpy() == (FILL64 if k == "sums" else FILL32)).all() and (h[k] == (FILL64 if k == "sums" else FILL32)).all(), k
    assert call(ok) == 0, lib.sgo_last_error()                       # and the accepted call writes
    torch.cuda.synchronize()
    assert out["sums"].cpu().numpy()[:, 7].tolist() == [16, 16]


def test_short_beside_long():
    """a row that ends after two passes beside a row that runs to the cap, in one wavefront (trees 2k, 2k + 1) and in neighbouring ones,
    both ways round"""
    S = 9
    names, recs = UC.case_records(S)
    short, long_ = names.index("none"), names.index("empty")
    index = (short, long_, long_, short, short, short, long_, long_, long_)
    for rules in (0, 1):
        p = dict(UC.DEFAULTS, index=index, sims=6, seed=31, rules=rules, max_plies=30, expand_at=0, komi2=1)
        want = UM.search(S, recs, **p)
        assert want["sums"][:, 5].tolist() == [6 * (30 if r == long_ else 2) for r in index]
        assert want["sums"][:, 6].tolist() == [6 * int(r == long_) for r in index]
        _check(S, _run(S, recs, p), want, len(index), 1, ("short beside long", rules))


def test_trees_behind_the_first_grid_trip():
    """more trees than the capped grid holds in one trip, at 5x5 under max_plies = 4.  The records are those whose movers never have
    more than one candidate, so a simulation does not depend on its g (the model says so below) and the expected rows are the model's
    rows of the records, re-listed; every 4 099th entry counted from the last row is out of range."""
    S = 5
    names, recs = UC.case_records(S)
    pick = [i for i, nm in enumerate(names) if nm.split("_x")[0] in ("none", "ko_ban", "ko_free", "connect", "full")]
    sub = recs[pick]
    R = len(sub)
    p = dict(UC.DEFAULTS, sims=3, seed=41, max_plies=4, expand_at=0, max_nodes=3)
    table = UM.search(S, sub, **p)
    shifted = UM.search(S, sub, **dict(p, index=tuple([R] * 7 + list(range(R)))))      # the same records with other g
    assert all(np.array_equal(table[k], shifted[k][7:]) for k in KEYS)
    n = GRID_UNITS + 37
    i = np.arange(n)
    index = ((i + i // GRID_UNITS) % R).astype(np.int32)
    index[(n - 1 - i) % 4099 == 0] = R
    nil = {k: np.zeros_like(v[:1]) for k, v in table.items()}
    nil["info"][0, 3] = -1
    want = {k: np.concatenate([v, nil[k]])[index] for k, v in table.items()}
    assert (want["sums"][GRID_UNITS:, 7] == 3).sum() >= 30 and len(set(map(tuple, want["visits"][GRID_UNITS:].tolist()))) > 2
    _check(S, _run(S, sub, dict(p, index=index)), want, n, 1, "past the grid cap")


def test_python_surface_on_the_device():
    """uct.search on host records gives the model's words and knows its side to move"""
    from sejonggo_amd import uct
    S = 7
    recs = UC.case_records(S)[1]
    p, want = _listed(S, 1)
    v = uct.search(S, recs, p["index"], trees=2, sims=12, seed=21, rules=1, komi=-0.5, max_plies=6, expand_at=1, trace=True)
    for k in KEYS:
        assert np.array_equal(getattr(v, k), want[k]), k
    assert v.best(0) == int(want["info"][0, 3]) and v.best(12) is None
    rows_ = recs[np.clip(np.asarray(p["index"]), 0, len(recs) - 1)]
    assert v.white_to_play.tolist() == [bool(r.reshape(16, -1)[0, -1] >> 31) for r in rows_]
