"""GPU: the chains-and-ladders kernels (include/sgo.h "chains and ladders", csrc/sgo_tactics.hip) against the model
(tests/tactics_model.py) word for word at every board size, on the case set tests/test_tactics_model_power.py shows to notice the
model's fault switches (tests/tactics_cases.py)."""
import numpy as np
import pytest

from tests import tactics_cases as TC
from tests import tactics_model as T

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL8, FILL32 = 0xA5, 0x3C3C3C3C


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _run(S, records, index, max_chains=128, n=None, n_records=None, pad=2):
    """sgo_tactics_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    n = (len(index) if index is not None else len(records)) if n is None else n
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev) if index is not None else None
    libs = torch.full((n + pad, S * S), FILL8, dtype=torch.uint8, device=dev)
    n_chains = torch.full((n + pad,), FILL32, dtype=torch.int32, device=dev)
    chains = torch.full((n + pad, max_chains, 8), FILL32, dtype=torch.int32, device=dev)
    rc = lib.sgo_tactics_dev(S, n, L.ptr(d_rec), len(records) if n_records is None else n_records, L.ptr(d_idx), max_chains, L.ptr(libs),
                             L.ptr(n_chains), L.ptr(chains), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return {"libs": libs.cpu().numpy(), "n_chains": n_chains.cpu().numpy(), "chains": chains.cpu().numpy()}


def _same(got, want, n, what):
    """libs, n_chains and every word of every stored chain row; the rows behind them and the rows behind n are as they were filled"""
    assert np.array_equal(got["n_chains"][:n], want["n_chains"][:n]), (what, np.flatnonzero(got["n_chains"][:n] != want["n_chains"][:n])[:8])
    bad = np.flatnonzero((got["libs"][:n] != want["libs"][:n]).any(axis=1))
    assert len(bad) == 0, (what, "libs", bad[:8])
    for i in range(n):
        rows = want["rows"][i]
        k = len(rows)
        assert np.array_equal(got["chains"][i, :k], rows), (what, i, got["chains"][i, :k][(got["chains"][i, :k] != rows).any(axis=1)][:4],
                                                            rows[(got["chains"][i, :k] != rows).any(axis=1)][:4])
        assert (got["chains"][i, k:] == FILL32).all(), (what, i, "rows behind the stored ones")
    assert (got["libs"][n:] == FILL8).all() and (got["n_chains"][n:] == FILL32).all() and (got["chains"][n:] == FILL32).all(), what


def _indexed(want, index, R, max_chains=128):
    """the model's outputs of records 0 .. R - 1 re-listed through an index (out of range: the zero row)"""
    N = want["libs"].shape[1]
    out = {"libs": np.zeros((len(index), N), np.uint8), "n_chains": np.zeros(len(index), np.int32), "rows": []}
    for i, r in enumerate(index):
        if 0 <= r < R:
            out["libs"][i], out["n_chains"][i] = want["libs"][r], want["n_chains"][r]
            out["rows"].append(want["rows"][r][:max_chains])
        else:
            out["rows"].append(np.zeros((0, 8), np.int32))
    return out


@pytest.mark.parametrize("S", T.SIZES)
def test_case_set_word_for_word(S):
    """every constructed position for both sides to move and the rule shapes: in order without an index list, then through a
    list that permutes them, repeats some and holds entries out of range; the host twin"""
    L, lib = _lib()
    names, recs = TC.case_records(S)
    want = TC.case_model(S)
    R = len(recs)
    _same(_run(S, recs, None), want, R, "in order")
    rng = np.random.RandomState(S)
    index = np.concatenate([rng.permutation(R), [-1, R, 0, 0, 2 ** 31 - 1, -2 ** 31, R - 1, 1, R + 7]]).astype(np.int64)
    _same(_run(S, recs, index.astype(np.int32)), _indexed(want, index, R), len(index), "indexed")
    # the host twin: same words, rows behind the stored ones as the caller filled them
    libs, nc = np.full((R, S * S), FILL8, np.uint8), np.full(R, FILL32, np.int32)
    chains = np.full((R, 128, 8), FILL32, np.int32)
    assert lib.sgo_tactics(S, R, L.ptr(np.ascontiguousarray(recs)), 128, L.ptr(libs), L.ptr(nc), L.ptr(chains)) == 0
    _same({"libs": libs, "n_chains": nc, "chains": chains}, want, R, "host twin")


@pytest.mark.parametrize("max_chains", [1, 2, 128])
def test_more_chains_than_rows(max_chains):
    """the lattice holds 272 listed chains: n_chains is the true number, the first max_chains rows are written and read out, the
    rest of the buffer stays; beside it a record with fewer chains than rows and an empty one"""
    S = 19
    names, recs = TC.case_records(S)
    want = TC.case_model(S)
    pick = [names.index("lattice_w"), names.index("ladder_beside_b"), names.index("empty_b"), names.index("lattice_b")]
    assert want["n_chains"][pick[0]] > 128 and 1 < want["n_chains"][pick[1]] < 128
    _same(_run(S, recs, np.array(pick, np.int32), max_chains=max_chains), _indexed(want, pick, len(recs), max_chains), len(pick),
          max_chains)


def test_both_halves_of_a_wave():
    """chain slots 2k and 2k + 1 of a row share a wavefront: the 19x19 ladder (75 nodes, 59 plies deep) beside an idle half
    (`ladder`: one chain), beside a short query (`ladder_beside`), and the ladder that runs into the depth cap"""
    S = 19
    names, recs = TC.case_records(S)
    want = TC.case_model(S)
    a, b = names.index("ladder_b"), names.index("ladder_beside_w")
    assert want["n_chains"][a] == 1 and want["n_chains"][b] == 4
    rows = want["rows"][b]
    assert rows[3, 0] == 60 and rows[3, 7] >= 70 and rows[2, 7] != rows[3, 7]
    pick = np.array([a, b, names.index("ladder_deep_b"), a], np.int32)
    _same(_run(S, recs, pick), _indexed(want, pick, len(recs)), len(pick), "halves")


def test_golden_positions():
    """every fourth position of the five golden 19x19 games (the records model replays them): one call; queries that end at the
    node cap and one that is 80 plies deep are among them"""
    recs = TC.golden_records()
    want = TC.golden_model()
    _same(_run(19, recs, None), want, len(recs), "golden")


def test_row_counts_and_bad_arguments():
    """n of 0, 1, 2, 3 (a lone half-wave); n_records bounds the index; the refusals"""
    import torch
    L, lib = _lib()
    S = 9
    names, recs = TC.case_records(S)
    want = TC.case_model(S)
    idx = (np.arange(7) * 5 % len(recs)).astype(np.int32)
    for n in (0, 1, 2, 3, 7):
        _same(_run(S, recs, idx[:max(n, 1)], n=n), _indexed(want, idx[:n], len(recs)), n, n)
    k = names.index("ladder_b")
    got = _run(S, recs, np.array([k, k + 1], np.int32), n_records=k + 1)
    _same(got, _indexed(want, [k, -1], len(recs)), 2, "n_records")
    dev = torch.device("cuda", 0)
    d, d1, d2, d3 = (torch.zeros(1024, dtype=torch.int32, device=dev) for _ in range(4))
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), 1, None, kw.get("mc", 4), kw.get("libs", P(d1)),   # noqa: E731
                         kw.get("nc", P(d2)), kw.get("ch", P(d3)), L.stream_ptr()]
    assert lib.sgo_tactics_dev(*args()) == 0
    for bad in (dict(S=8), dict(n=-1), dict(rec=None), dict(libs=None), dict(nc=None), dict(ch=None), dict(mc=0), dict(mc=129)):
        assert lib.sgo_tactics_dev(*args(**bad)) == SGO_ERR_ARG, bad
    h, h1, h2, h3 = (np.zeros(1024, np.uint32) for _ in range(4))
    assert lib.sgo_tactics(8, 1, P(h), 4, P(h1), P(h2), P(h3)) == SGO_ERR_ARG
    assert lib.sgo_tactics(S, 1, P(h), 0, P(h1), P(h2), P(h3)) == SGO_ERR_ARG
    assert lib.sgo_tactics(S, 1, P(h), 4, None, P(h2), P(h3)) == SGO_ERR_ARG
    assert lib.sgo_tactics(S, 0, P(h), 4, P(h1), P(h2), P(h3)) == 0
    torch.cuda.synchronize()


def test_python_surface_and_record_set():
    """tactics.tactics on host records, and RecordSet.tactics over the golden collection in one chunk: row ch.index[e] is the
    position before entry e (every fourth compared with the model's golden rows)"""
    from sejonggo_amd.records import RecordSet
    from sejonggo_amd.records import Record
    from sejonggo_amd.tactics import tactics
    from tests.helpers import load
    S = 9
    names, recs = TC.case_records(S)
    want = TC.case_model(S)
    t = tactics(S, recs, index=[names.index("ladder_b"), -1], max_chains=8)
    c = t.chains_of(0)[0]
    assert tuple(c) == tuple(int(v) for v in want["rows"][names.index("ladder_b")][0]) and c.capturable and not c.dead and not c.unknown
    assert t.n_chains[1] == 0 and not t.libs[1].any() and t.chains_of(1) == []
    z = load("sgf_S19.npz")
    games = []
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        entries = [(19 * 19 if y >= 19 else int(y) * 19 + int(x), int(c)) for x, y, c in mv]
        games.append(Record("g%d" % gi, 19, entries, [False] * len(entries), list(range(1, len(entries) + 1)), None))
    rs = RecordSet(games, size=19)
    try:
        chunks = list(rs.tactics())
        assert len(chunks) == 1
        tt = chunks[0].tactics
        gold = TC.golden_model()
        for j in range(0, len(gold["n_chains"]), 7):
            r = 4 * j
            assert tt.n_chains[r] == gold["n_chains"][j] and np.array_equal(tt.libs[r], gold["libs"][j])
            assert np.array_equal(tt.chains[r, :len(gold["rows"][j])], gold["rows"][j])
    finally:
        rs.close()


def test_session_tactics():
    """slots set up from prefixes of a golden game against the model on the records of the same plies; a slot that is no session
    is refused and its rows stay as they were filled; a slot may be listed twice"""
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    from tests.helpers import load
    S = 19
    z = load("sgf_S19.npz")
    mv = z["g02_moves"]
    acts, cols = [S * S if y >= S else int(y) * S + int(x) for x, y, _ in mv], [int(c) for _, _, c in mv]
    gold = TC.golden_model()
    n_before = sum(len(z["g%02d_moves" % g]) + 1 for g in range(2))        # records of games 0 and 1 in the replay
    plies = [p for p in range(len(acts) + 1) if (n_before + p) % 4 == 0][10::12][:4]
    rows = [(n_before + p) // 4 for p in plies]
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=6, sims=8, energy=4, symmetry="identity")
    try:
        lib = L.require_gpu()
        slots = [4, 0, 3, 1]
        eng.open(slots)
        st, _ = eng.setup(slots, [acts[:p] for p in plies], [cols[:p] for p in plies])
        assert not st.any()
        t = eng.tactics(slots)
        assert not t.status.any()
        for i, r in enumerate(rows):
            assert t.n_chains[i] == gold["n_chains"][r] and np.array_equal(t.libs[i], gold["libs"][r])
            assert np.array_equal(t.chains[i, :len(gold["rows"][r])], gold["rows"][r]) and not t.chains[i, len(gold["rows"][r]):].any()
        ask = np.array([2, 3, 5, 3, 4], np.int32)
        mc = 16
        out = {"status": np.full(5, 77, np.int32), "libs": np.full((5, S * S), FILL8, np.uint8), "n_chains": np.full(5, FILL32, np.int32),
               "chains": np.full((5, mc, 8), FILL32, np.int32)}
        rc = lib.sgo_session_tactics(eng.ctx, 5, L.ptr(ask), mc, L.ptr(out["status"]), L.ptr(out["libs"]), L.ptr(out["n_chains"]),
                                     L.ptr(out["chains"]), L.stream_ptr())
        assert rc == 0 and out["status"].tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for i in (0, 2):
            assert (out["libs"][i] == FILL8).all() and out["n_chains"][i] == FILL32 and (out["chains"][i] == FILL32).all()
        for i, r in ((1, rows[2]), (3, rows[2]), (4, rows[0])):
            k = min(mc, len(gold["rows"][r]))
            assert out["n_chains"][i] == gold["n_chains"][r] and np.array_equal(out["libs"][i], gold["libs"][r])
            assert np.array_equal(out["chains"][i, :k], gold["rows"][r][:k]) and (out["chains"][i, k:] == FILL32).all()
        assert lib.sgo_session_tactics(eng.ctx, 1, L.ptr(np.array([6], np.int32)), mc, L.ptr(out["status"]), L.ptr(out["libs"]),
                                       L.ptr(out["n_chains"]), L.ptr(out["chains"]), L.stream_ptr()) == SGO_ERR_ARG
    finally:
        eng.close()


@pytest.fixture()
def env():
    from sejonggo_amd import _lib
    from sejonggo_amd.conf import conf
    _lib.require_gpu()
    keep = dict(conf)
    yield conf
    conf.clear()
    conf.update(keep)


def test_gtp_and_review_on_the_device(env, tmp_path):
    """the 9x9 ladder in atari played into a device session: `sgo-ladders` before and after the run-out; the same moves as a
    record through review.main --tactics: the flags tests/test_tactics_host.py derives from the model, and without --tactics
    the lines are the same text without them"""
    import io
    from sejonggo_amd import gtp, review
    from sejonggo_amd.stub_nets import make_stub
    from tests.test_tactics_host import PLAY, SHAPE
    S = 9
    env.update({'SIZE': S, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", S), size=S, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev)
        for a, c in SHAPE:
            assert e.parse_command("play %s %s" % ("B" if c > 0 else "W", e._vertex(a))) == "=\n\n"
        board = dev.board
        assert e.parse_command("sgo-ladders") == "= D6 black size 1 liberties 1 dead attack E6 defend none\n\n"
        assert e.parse_command("play B E6") == "=\n\n"
        assert e.parse_command("sgo-ladders") == "= D6 black size 2 liberties 2 capturable attack F6 defend F6\n\n"
        assert e.parse_command("undo") == "=\n\n" and np.array_equal(dev.board, board)      # the slot was only read
    finally:
        dev.close()
    L = "abcdefghi"
    text = "(;FF[4]SZ[9]KM[5.5]AB[%s]AW%s" % (L[3] + L[3], "".join("[%s]" % (L[a % S] + L[a // S]) for a, c in SHAPE if c < 0)) + \
        "".join(";%s[%s]" % ("B" if c > 0 else "W", L[a % S] + L[a // S]) for a, c in PLAY) + ")"
    sgf = tmp_path / "g.sgf"
    sgf.write_text(text)
    args = [str(sgf), "--net", "hash", "--symmetry", "identity", "--sims", "8", "--energy", "4"]
    plain, flagged = io.StringIO(), io.StringIO()
    assert review.main(args, out=plain) == 0 and review.main(args + ["--tactics"], out=flagged) == 0
    a, b = plain.getvalue().rstrip("\n").split("\n"), flagged.getvalue().rstrip("\n").split("\n")
    assert len(a) == len(b) == 5 and "|" not in plain.getvalue()
    assert b == [a[0] + "  | ladder", a[1], a[2] + "  | ladder", a[3] + "  | missed", a[4]]
