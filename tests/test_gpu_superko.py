"""GPU: the superko kernels (include/sgo.h "superko", csrc/sgo_superko.hip) against the model (tests/superko_model.py) word for word
at every board size and under both rules, on the case set tests/test_superko_model_power.py shows to notice the model's fault
switches (tests/superko_cases.py)."""
import numpy as np
import pytest

from tests import superko_cases as SC
from tests import superko_model as SM

pytestmark = pytest.mark.gpu

SGO_ERR_ARG = -1
FILL16, FILL32 = 0x5A5A, 0x3C3C3C3C


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _run(S, records, index, first, rule, n=None, n_records=None, pad=2):
    """sgo_superko_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    n = len(first) if n is None else n
    NW = (S * S + 31) // 32
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev) if index is not None else None
    d_first = torch.from_numpy(np.ascontiguousarray(first, np.int32)).to(dev)
    R = len(records) if n_records is None else n_records
    keys = torch.zeros(max(R, 1), dtype=torch.int64, device=dev)
    sets = torch.full((n + pad, 3, NW), FILL32, dtype=torch.int32, device=dev)
    back = torch.full((n + pad, S * S), FILL16, dtype=torch.int16, device=dev)
    counts = torch.full((n + pad, 8), FILL32, dtype=torch.int32, device=dev)
    rc = lib.sgo_superko_dev(S, n, L.ptr(d_rec), R, L.ptr(d_idx), L.ptr(d_first), rule, L.ptr(keys), L.ptr(sets), L.ptr(back), L.ptr(counts),
                             L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return {"sets": sets.cpu().numpy().view(np.uint32), "back": back.cpu().numpy(), "counts": counts.cpu().numpy()}


def _same(got, want, n, what, refuted=True):
    """every word of the three outputs (refuted=False: all but counts[6]); the rows behind n are as they were filled"""
    for k in ("sets", "back", "counts") if n else ():
        g, w = got[k][:n].reshape(n, -1).copy(), want[k][:n].reshape(n, -1).copy()
        if k == "counts" and not refuted:
            g[:, 6] = w[:, 6] = 0
        bad = np.flatnonzero((g != w).any(axis=1))
        if len(bad):
            i = int(bad[0])
            at = np.flatnonzero(g[i] != w[i])[:8]
            raise AssertionError((what, k, "rows", bad[:8].tolist(), "row", i, "at", at.tolist(), g[i][at].tolist(), w[i][at].tolist()))
    assert (got["sets"][n:] == FILL32).all() and (got["back"][n:] == FILL16).all() and (got["counts"][n:] == FILL32).all(), (what, "rows behind n")


def _pick(want, sel):
    return {k: v[np.asarray(sel, np.int64)] for k, v in want.items()}


def _in_order_rows(S):
    """one row per record of the case set, in order: the record with the history from the first record of its game"""
    recs, _, _, bases = SC.case_set(S)
    starts = np.array(sorted(bases.values()))
    return [(r, int(starts[np.searchsorted(starts, r, "right") - 1])) for r in range(len(recs))]


@pytest.mark.parametrize("S", SM.SIZES)
def test_case_set_word_for_word(S):
    """both rules: in order without an index list (every record against its game), then the rows of the case set through a list
    that permutes them, repeats some and holds the zero rows; the host twin on the same list"""
    L, lib = _lib()
    recs, rows, names, _ = SC.case_set(S)
    R, NW = len(recs), (S * S + 31) // 32
    order = _in_order_rows(S)
    rng = np.random.RandomState(S)
    perm = np.concatenate([rng.permutation(len(rows)), [0, 0, len(rows) - 1, 1]])
    for rule in (0, 1):
        _same(_run(S, recs, None, [f for _, f in order], rule), SM.superko(S, recs, order, rule), R, ("in order", rule))
        want = _pick(SC.case_model(S, rule), perm)
        _same(_run(S, recs, rows[perm, 0], rows[perm, 1], rule), want, len(perm), ("indexed", rule))
        n = len(perm)
        sets, back, counts = np.full((n, 3, NW), FILL32, np.uint32), np.full((n, S * S), FILL16, np.int16), np.full((n, 8), FILL32, np.int32)
        idx, first = np.ascontiguousarray(rows[perm, 0], np.int32), np.ascontiguousarray(rows[perm, 1], np.int32)
        assert lib.sgo_superko(S, R, L.ptr(np.ascontiguousarray(recs)), n, L.ptr(idx), L.ptr(first), rule, L.ptr(sets), L.ptr(back), L.ptr(counts)) == 0
        got = {"sets": np.concatenate([sets, np.full((1, 3, NW), FILL32, np.uint32)]), "back": np.concatenate([back, np.full((1, S * S), FILL16, np.int16)]),
               "counts": np.concatenate([counts, np.full((1, 8), FILL32, np.int32)])}
        _same(got, want, n, ("host twin", rule))


def test_long_history_and_both_halves_of_a_wave():
    """the 19x19 history of SGO_SUPERKO_MAX_HISTORY(19) records and one longer, against the model; rows 2k and 2k + 1 share a
    wavefront and its loop counts: an odd n, and the longest history beside the empty board with f = r, both ways round"""
    S = SC.LONG_S
    recs, rows, names, _ = SC.long_history()
    long_, empty = names.index("one_too_long"), names.index("empty_alone")
    for rule in (0, 1):
        want = SC.long_model(rule)
        assert want["counts"][long_, 5] == SM.max_history(S) and want["counts"][long_, 7] == 1 and want["counts"][empty].tolist() == [0, 0, 0, -1, 0, 1, 0, 0]
        _same(_run(S, recs, rows[:, 0], rows[:, 1], rule), want, len(rows), ("long", rule))
        for pick in ([long_, empty, empty, long_, long_], [empty, long_, empty], [long_]):
            _same(_run(S, recs, rows[pick, 0], rows[pick, 1], rule), _pick(want, pick), len(pick), ("halves", rule, pick))


def test_six_bit_keys_take_the_confirmation_path():
    """sgo_superko_mode(1) compares six bits of a key: every output but counts[6] stays, counts[6] becomes positive on the long
    history and is 0 with whole keys"""
    L, lib = _lib()
    S = SC.LONG_S
    recs, rows, names, _ = SC.long_history()
    crecs, crows, _, _ = SC.case_set(7)
    assert lib.sgo_superko_mode(-1) == 0
    try:
        for rule in (0, 1):
            whole = _run(S, recs, rows[:, 0], rows[:, 1], rule)
            assert (whole["counts"][:len(rows), 6] == 0).all()
            assert lib.sgo_superko_mode(1) == 0 and lib.sgo_superko_mode(7) == 1
            six = _run(S, recs, rows[:, 0], rows[:, 1], rule)
            _same(six, SC.long_model(rule), len(rows), ("six bits", rule), refuted=False)
            assert six["counts"][names.index("one_too_long"), 6] > 0 and six["counts"][names.index("exactly_max"), 6] > 0
            _same(_run(7, crecs, crows[:, 0], crows[:, 1], rule), SC.case_model(7, rule), len(crows), ("six bits, cases", rule), refuted=False)
            assert lib.sgo_superko_mode(0) == 1
    finally:
        lib.sgo_superko_mode(0)


def _golden_record_set():
    from sejonggo_amd.records import Record, RecordSet
    games = SC.golden_games()
    return RecordSet([Record("g%d" % gi, 19, e, [False] * len(e), list(range(1, len(e) + 1)), None) for gi, e in enumerate(games)], size=19)


def test_golden_games_replayed_on_the_device():
    """the five golden 19x19 games replayed on the device, RecordSet.superko over all their records in one chunk: the rows of the
    fixed sample (the last six records of each game and every 40th) are the model's, under both rules"""
    grecs, grows = SC.golden_sample()
    rs = _golden_record_set()
    try:
        for rule in (0, 1):
            chunks = list(rs.superko(rule))
            assert len(chunks) == 1
            v = chunks[0].superko
            assert len(v) == len(grecs)
            want = SC.golden_model(rule)
            got = {"sets": v.sets[grows[:, 0]], "back": v.back[grows[:, 0]], "counts": v.counts[grows[:, 0]]}
            for k in got:
                assert np.array_equal(got[k], want[k]), (rule, k, np.flatnonzero((got[k] != want[k]).reshape(len(grows), -1).any(axis=1))[:8].tolist())
            assert (v.counts[:, 5] == np.concatenate([np.arange(len(g) + 1) + 1 for g in SC.golden_games()])).all()
    finally:
        rs.close()


def test_row_counts_and_bad_arguments():
    """n of 0, 1, 2, 3; n_records bounds the index; the refusals leave the outputs as they were"""
    import torch
    L, lib = _lib()
    S = 9
    recs, rows, names, _ = SC.case_set(S)
    want = SC.case_model(S, 0)
    sel = (np.arange(7) * 5) % len(rows)
    for n in (0, 1, 2, 3, 7):
        _same(_run(S, recs, rows[sel[:max(n, 1)], 0], rows[sel[:max(n, 1)], 1], 0, n=n), _pick(want, sel[:n]), n, n)
    k = names.index("ko_b_1_0")
    r, f = int(rows[k, 0]), int(rows[k, 1])
    zero = names.index("zero_below")
    _same(_run(S, recs, [r, r], [f, f], 0, n_records=r), _pick(want, [zero, zero]), 2, "n_records")
    _same(_run(S, recs, [r, r - 1], [f, f], 0, n_records=r + 1), _pick(want, [k, names.index("ko_b_0_0")]), 2, "n_records + 1")
    dev = torch.device("cuda", 0)
    NW = (S * S + 31) // 32
    d = torch.zeros(1024, dtype=torch.int32, device=dev)
    keys = torch.zeros(4, dtype=torch.int64, device=dev)
    sets = torch.full((2, 3, NW), FILL32, dtype=torch.int32, device=dev)
    back = torch.full((2, S * S), FILL16, dtype=torch.int16, device=dev)
    counts = torch.full((2, 8), FILL32, dtype=torch.int32, device=dev)
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), kw.get("R", 1), None, kw.get("first", P(d)), kw.get("rule", 0),   # noqa: E731
                         kw.get("keys", P(keys)), kw.get("sets", P(sets)), kw.get("back", P(back)), kw.get("counts", P(counts)), L.stream_ptr()]
    for bad in (dict(S=8), dict(S=0), dict(n=-1), dict(R=-1), dict(rule=2), dict(rule=-1), dict(rec=None), dict(first=None), dict(keys=None),
                dict(sets=None), dict(back=None), dict(counts=None)):
        assert lib.sgo_superko_dev(*args(**bad)) == SGO_ERR_ARG, bad
    torch.cuda.synchronize()
    assert (sets == FILL32).all() and (back == FILL16).all() and (counts == FILL32).all()
    assert lib.sgo_superko_dev(*args()) == 0
    torch.cuda.synchronize()
    assert not sets[0, :2].any() and (back[0] == -1).all() and (back[1] == FILL16).all() and counts[0].tolist() == [0, 0, 0, -1, 0, 1, 0, 0]
    h, hf = np.zeros(1024, np.uint32), np.zeros(1, np.int32)
    hs, hb, hc = np.full((1, 3, NW), FILL32, np.uint32), np.full((1, S * S), FILL16, np.int16), np.full((1, 8), FILL32, np.int32)
    host = lambda **kw: [kw.get("S", S), kw.get("R", 1), kw.get("rec", P(h)), kw.get("n", 1), None, kw.get("first", P(hf)), kw.get("rule", 0),   # noqa: E731
                         kw.get("sets", P(hs)), kw.get("back", P(hb)), kw.get("counts", P(hc))]
    for bad in (dict(S=8), dict(n=-1), dict(R=-1), dict(rule=2), dict(rec=None), dict(first=None), dict(sets=None), dict(back=None), dict(counts=None)):
        assert lib.sgo_superko(*host(**bad)) == SGO_ERR_ARG, bad
    assert lib.sgo_superko(*host(n=0)) == 0
    assert (hs == FILL32).all() and (hb == FILL16).all() and (hc == FILL32).all()


def test_capturable_in_a_graph():
    """the call (both launches) alone in a captured graph, replayed twice over re-filled outputs: the eager result"""
    import torch
    L, lib = _lib()
    S = 13
    recs, rows, _, _ = SC.case_set(S)
    want = SC.case_model(S, 1)
    n, NW = len(rows), (S * S + 31) // 32
    dev = torch.device("cuda", 0)
    eager = _run(S, recs, rows[:, 0], rows[:, 1], 1, pad=1)          # first, so that the capture is not the kernels' first launch
    d_rec = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(rows[:, 0], np.int32)).to(dev)
    d_first = torch.from_numpy(np.ascontiguousarray(rows[:, 1], np.int32)).to(dev)
    keys = torch.zeros(len(recs), dtype=torch.int64, device=dev)
    sets = torch.full((n + 1, 3, NW), FILL32, dtype=torch.int32, device=dev)
    back = torch.full((n + 1, S * S), FILL16, dtype=torch.int16, device=dev)
    counts = torch.full((n + 1, 8), FILL32, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.sgo_superko_dev(S, n, L.ptr(d_rec), len(recs), L.ptr(d_idx), L.ptr(d_first), 1, L.ptr(keys), L.ptr(sets), L.ptr(back),
                                 L.ptr(counts), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    for _ in range(2):
        for t, v in ((sets, FILL32), (back, FILL16), (counts, FILL32)):
            t.fill_(v)
        keys.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = {"sets": sets.cpu().numpy().view(np.uint32), "back": back.cpu().numpy(), "counts": counts.cpu().numpy()}
        _same(got, want, n, "graph replay")
    assert all(np.array_equal(eager[k], got[k]) for k in got)


def test_python_surface():
    """superko.superko on host records: the result object's views of the sending-two-returning-one row"""
    from sejonggo_amd.superko import superko
    S = 5
    recs, rows, names, _ = SC.case_set(S)
    k = names.index("send_two_b_2_0")
    sel = [k, names.index("zero_above"), names.index("ko_b_1_0")]
    v0, v1 = (superko(S, recs, rows[sel, 0], rows[sel, 1], rule) for rule in ("positional", "situational"))
    for v, rule in ((v0, 0), (v1, 1)):
        want = _pick(SC.case_model(S, rule), sel)
        assert np.array_equal(v.sets, want["sets"]) and np.array_equal(v.back, want["back"]) and np.array_equal(v.counts, want["counts"])
    assert v0.extra(0) == [(1, 2)] and v1.extra(0) == [] and v0.repeat(2) == [(2, 1)] and v0.extra(2) == [] and len(v0) == 3
    assert not v0.legal(0)[1] and v1.legal(0)[1] and v0.legal(0)[S * S] and v0.played(0, 1) == (True, True, 2) and v0.played(0, S * S) == (False, False, -1)
    assert v0.count(0, "history") == 3 and v0.count(1, "history") == 0 and not v0.legal(1).any()


@pytest.fixture()
def env():
    from sejonggo_amd import _lib
    from sejonggo_amd.conf import conf
    _lib.require_gpu()
    keep = dict(conf)
    yield conf
    conf.clear()
    conf.update(keep)


def test_gtp_on_the_device(env):
    """the 7x7 triple ko played into ONE device session stone by stone: `sgo-superko` names the move that would close the cycle, five
    plies back; with --superko `play` on it is refused and the game is as it was, and genmove answers another legal vertex"""
    from sejonggo_amd import gtp
    from sejonggo_amd.stub_nets import make_stub
    S = 7
    m = S - 1
    P = lambda x, y: y * S + x                                                           # noqa: E731
    env.update({'SIZE': S, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    walls_b = [P(0, 0), P(1, 1), P(0, m), P(1, m - 1), P(m, 1), P(m - 1, 2)]
    walls_w = [P(3, 0), P(2, 1), P(3, m), P(2, m - 1), P(m, 4), P(m - 1, 3)]
    L, Rt = [P(1, 0), P(1, m), P(m, 2)], [P(2, 0), P(2, m), P(m, 3)]
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", S), size=S, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev, superko="positional")
        for c, pts in (("B", walls_b + [Rt[0]]), ("W", walls_w + [L[1], L[2]])):          # white's stones last: black is to move
            for a in pts:
                assert e.parse_command("play %s %s" % (c, e._vertex(a))) == "=\n\n"
        assert e.parse_command("sgo-superko") == "=\n\n"
        for c, a in (("B", Rt[1]), ("W", L[0]), ("B", Rt[2]), ("W", L[1]), ("B", Rt[0])):
            assert e.parse_command("play %s %s" % (c, e._vertex(a))) == "=\n\n", (c, a)
        closing = e._vertex(L[2])
        for words in ("", " situational"):
            # the plain ko first: black has just taken at the top, the retake is one ply back and the inherited rule forbids it
            assert e.parse_command("sgo-superko" + words) == "= %s 1\n%s 5 forbidden\n\n" % (e._vertex(L[0]), closing)
        v = dev.superko("situational")
        assert v.extra(0) == [(L[2], 5)] and v.count(0, "history") == len(dev.moves) + 1 and v.count(0, "seen") == 0
        board, n = np.array(dev.board), len(dev.moves)
        legal = dev.legal()
        assert legal[L[2]] and not legal[L[0]]                       # the inherited rule allows it: black's last capture was elsewhere
        assert e.parse_command("play W " + closing) == "? illegal move\n\n"
        assert np.array_equal(np.array(dev.board), board) and len(dev.moves) == n
        answer = e.parse_command("genmove w")
        assert answer.startswith("= ") and answer != "= %s\n\n" % closing and len(dev.moves) == n + 1
        a = dev.moves[-1][0]
        assert a != L[2] and legal[a] and answer == "= %s\n\n" % e._vertex(a)
    finally:
        dev.close()
