"""GPU: the move-outcome kernel (include/sgo.h "move outcomes", csrc/sgo_moves.hip) against the model (tests/moves_model.py) word
for word at every board size and for both sides, on the case set tests/test_moves_model_power.py shows to notice the model's fault
switches (tests/moves_cases.py)."""
import numpy as np
import pytest

from tests import moves_cases as MC
from tests import moves_model as M

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL16, FILL32 = 0x5A5A, 0x3C3C3C3C


def _lib():
    from sejonggo_amd import _lib as L
    return L, L.require_gpu()


def _run(S, records, index, side, n=None, n_records=None, pad=2):
    """sgo_moves_dev on device copies; outputs are pre-filled and `pad` rows longer than n: returns them whole, as numpy"""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda", 0)
    n = (len(index) if index is not None else len(records)) if n is None else n
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.int32)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev) if index is not None else None
    rows = torch.full((n + pad, S * S, 8), FILL16, dtype=torch.int16, device=dev)
    counts = torch.full((n + pad, 8), FILL32, dtype=torch.int32, device=dev)
    rc = lib.sgo_moves_dev(S, n, L.ptr(d_rec), len(records) if n_records is None else n_records, L.ptr(d_idx), side, L.ptr(rows),
                           L.ptr(counts), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    torch.cuda.synchronize()
    return {"rows": rows.cpu().numpy(), "counts": counts.cpu().numpy()}


def _same(got, want, n, what):
    """every word of rows and counts; the rows behind n are as they were filled"""
    bad = np.flatnonzero((got["rows"][:n] != want["rows"][:n]).any(axis=(1, 2)))
    if len(bad):
        i = int(bad[0])
        a = int(np.flatnonzero((got["rows"][i] != want["rows"][i]).any(axis=1))[0])
        raise AssertionError((what, "rows", bad[:8].tolist(), "record", i, "point", a, got["rows"][i, a].tolist(), want["rows"][i, a].tolist()))
    bad = np.flatnonzero((got["counts"][:n] != want["counts"][:n]).any(axis=1))
    assert len(bad) == 0, (what, "counts", bad[:8].tolist(), got["counts"][bad[0]].tolist(), want["counts"][bad[0]].tolist())
    assert (got["rows"][n:] == FILL16).all() and (got["counts"][n:] == FILL32).all(), (what, "rows behind n")


def _indexed(want, index, R):
    """the model's outputs of records 0 .. R - 1 re-listed through an index (out of range: the zero row)"""
    out = {"rows": np.zeros((len(index),) + want["rows"].shape[1:], np.int16), "counts": np.zeros((len(index), 8), np.int32)}
    for i, r in enumerate(index):
        if 0 <= r < R:
            out["rows"][i], out["counts"][i] = want["rows"][r], want["counts"][r]
    return out


@pytest.mark.parametrize("S", M.SIZES)
def test_case_set_word_for_word(S):
    """every constructed position for both colours to move and the rule shapes, for side 0 and side 1: in order without an index
    list, then through a list that permutes them, repeats some and holds entries out of range; the host twin"""
    L, lib = _lib()
    names, recs = MC.case_records(S)
    R = len(recs)
    rng = np.random.RandomState(S)
    index = np.concatenate([rng.permutation(R), [-1, R, 0, 0, 2 ** 31 - 1, -2 ** 31, R - 1, 1, R + 7]]).astype(np.int64)
    for side in (0, 1):
        want = MC.case_model(S, side)
        _same(_run(S, recs, None, side), want, R, ("in order", side))
        _same(_run(S, recs, index.astype(np.int32), side), _indexed(want, index, R), len(index), ("indexed", side))
        rows, counts = np.full((R, S * S, 8), FILL16, np.int16), np.full((R, 8), FILL32, np.int32)
        assert lib.sgo_moves(S, R, L.ptr(np.ascontiguousarray(recs)), side, L.ptr(rows), L.ptr(counts)) == 0
        _same({"rows": rows, "counts": counts}, want, R, ("host twin", side))


def test_both_halves_of_a_wave():
    """rows 2k and 2k + 1 share a wavefront and its loop counts: an odd n (the last half idle), the empty board (no contact point)
    beside the case with the most, and the same pair the other way round"""
    S = 19
    names, recs = MC.case_records(S)
    e = names.index("empty_b")
    for side in (0, 1):
        want = MC.case_model(S, side)
        contact = [MC.contact_points(S, r) for r in recs]
        f = int(np.argmax(contact))
        assert contact[e] == 0 and contact[f] > 60 and want["counts"][e].tolist() == [S * S, 0, 0, -1, 0, 0, 0, 0]
        for pick in ([e, f, f, e, f], [f, e, e], [f]):
            pick = np.array(pick, np.int32)
            _same(_run(S, recs, pick, side), _indexed(want, pick, len(recs)), len(pick), ("halves", side, pick.tolist()))


def test_golden_positions():
    """every 32nd record of the five golden 19x19 games and each game's last (moves_cases.GOLDEN_STRIDE, 57 positions: the model
    takes about a second for both sides); one call per side"""
    recs, want0, want1 = MC.golden_sample()
    assert MC.GOLDEN_STRIDE == 32 and len(recs) >= 40
    _same(_run(19, recs, None, 0), want0, len(recs), "golden side 0")
    _same(_run(19, recs, None, 1), want1, len(recs), "golden side 1")


def test_row_counts_and_bad_arguments():
    """n of 0, 1, 2, 3 (a lone half-wave); n_records bounds the index; the refusals leave the outputs as they were"""
    import torch
    L, lib = _lib()
    S = 9
    names, recs = MC.case_records(S)
    want = MC.case_model(S, 0)
    idx = (np.arange(7) * 5 % len(recs)).astype(np.int32)
    for n in (0, 1, 2, 3, 7):
        _same(_run(S, recs, idx[:max(n, 1)], 0, n=n), _indexed(want, idx[:n], len(recs)), n, n)
    k = names.index("join4_b")
    _same(_run(S, recs, np.array([k, k + 1], np.int32), 0, n_records=k + 1), _indexed(want, [k, -1], len(recs)), 2, "n_records")
    dev = torch.device("cuda", 0)
    d = torch.zeros(1024, dtype=torch.int32, device=dev)
    rows = torch.full((2, S * S, 8), FILL16, dtype=torch.int16, device=dev)
    counts = torch.full((2, 8), FILL32, dtype=torch.int32, device=dev)
    P = L.ptr
    args = lambda **kw: [kw.get("S", S), kw.get("n", 1), kw.get("rec", P(d)), kw.get("R", 1), None, kw.get("side", 0),   # noqa: E731
                         kw.get("rows", P(rows)), kw.get("counts", P(counts)), L.stream_ptr()]
    for bad in (dict(S=8), dict(S=0), dict(n=-1), dict(R=-1), dict(side=2), dict(side=-1), dict(rec=None), dict(rows=None), dict(counts=None),
                dict(rows=rows.data_ptr() + 2)):
        assert lib.sgo_moves_dev(*args(**bad)) == SGO_ERR_ARG, bad
    torch.cuda.synchronize()
    assert (rows == FILL16).all() and (counts == FILL32).all()
    assert lib.sgo_moves_dev(*args()) == 0
    torch.cuda.synchronize()
    assert (rows[0, :, 0] == M.ALLOWED).all() and (rows[1] == FILL16).all() and counts[0].tolist() == [S * S, 0, 0, -1, 0, 0, 0, 0]
    h = np.zeros(1024, np.uint32)
    hr, hc = np.full((1, S * S, 8), FILL16, np.int16), np.full((1, 8), FILL32, np.int32)
    assert lib.sgo_moves(8, 1, P(h), 0, P(hr), P(hc)) == SGO_ERR_ARG and lib.sgo_moves(S, -1, P(h), 0, P(hr), P(hc)) == SGO_ERR_ARG
    assert lib.sgo_moves(S, 1, P(h), 2, P(hr), P(hc)) == SGO_ERR_ARG and lib.sgo_moves(S, 1, None, 0, P(hr), P(hc)) == SGO_ERR_ARG
    assert lib.sgo_moves(S, 1, P(h), 0, None, P(hc)) == SGO_ERR_ARG and lib.sgo_moves(S, 1, P(h), 0, P(hr), None) == SGO_ERR_ARG
    assert lib.sgo_moves(S, 0, P(h), 0, P(hr), P(hc)) == 0
    assert (hr == FILL16).all() and (hc == FILL32).all()


def test_capturable_in_a_graph():
    """the call alone in a captured graph, replayed twice over re-filled outputs: the eager result"""
    import torch
    L, lib = _lib()
    S = 13
    names, recs = MC.case_records(S)
    want = MC.case_model(S, 0)
    R = len(recs)
    dev = torch.device("cuda", 0)
    eager = _run(S, recs, None, 0, pad=1)                            # first, so that the capture is not the kernel's first launch
    d_rec = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32)).to(dev)
    rows = torch.full((R + 1, S * S, 8), FILL16, dtype=torch.int16, device=dev)
    counts = torch.full((R + 1, 8), FILL32, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.sgo_moves_dev(S, R, L.ptr(d_rec), R, None, 0, L.ptr(rows), L.ptr(counts), L.stream_ptr())
    assert rc == 0, lib.sgo_last_error()
    for _ in range(2):
        rows.fill_(FILL16)
        counts.fill_(FILL32)
        g.replay()
        torch.cuda.synchronize()
        _same({"rows": rows.cpu().numpy(), "counts": counts.cpu().numpy()}, want, R, "graph replay")
    assert np.array_equal(eager["rows"], rows.cpu().numpy()) and np.array_equal(eager["counts"], counts.cpu().numpy())


def _golden_games():
    from tests.helpers import load
    z = load("sgf_S19.npz")
    games = []
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        games.append([(19 * 19 if y >= 19 else int(y) * 19 + int(x), int(c)) for x, y, c in mv])
    return games


def test_python_surface_and_record_set():
    """moves.moves on host records, and RecordSet.moves over the golden collection in one chunk: the played row of entry e is the
    model's row of the entry's action in the record before it (compared on the positions of the golden sample)"""
    from sejonggo_amd.moves import moves
    from sejonggo_amd.records import Record, RecordSet
    S = 9
    names, recs = MC.case_records(S)
    k = names.index("join4_b")
    for side in (0, 1):
        want = MC.case_model(S, side)
        v = moves(S, recs, index=[k, -1, 0], side=side)
        assert np.array_equal(v.rows[0], want["rows"][k]) and np.array_equal(v.counts[0], want["counts"][k]) and len(v) == 3
        assert not v.rows[1].any() and not v.counts[1].any() and v.count(2, "allowed") == S * S
    m = moves(S, recs).move(k, 2 * S + 2)
    assert (m.joined, m.weakest, m.size) == (4, 1, 6) and m.forbidden_sound and not m.allowed and not m.escapes
    games = _golden_games()
    rs = RecordSet([Record("g%d" % gi, 19, e, [False] * len(e), list(range(1, len(e) + 1)), None) for gi, e in enumerate(games)], size=19)
    try:
        chunks = list(rs.moves())
        assert len(chunks) == 1
        ch = chunks[0]
        total = sum(len(e) for e in games)
        assert ch.played.shape == (total, 8) and ch.move_counts.shape == (total, 8)
        # in_turn: the entry's colour is the side to move of the record before it (each golden game ends with a pass out of turn)
        white_to_play = (MC.golden_records(1)[ch.index][:, 11] >> 31).astype(bool)
        assert np.array_equal(ch.in_turn, np.where(white_to_play, -1, 1) == ch.colour) and (~ch.in_turn).sum() == 5
        _, want0, _ = MC.golden_sample()
        at = {int(r): e for e, r in enumerate(ch.index)}             # record -> the entry played from it
        seen = 0
        for j, r in enumerate(MC.golden_sample_index()):
            if r not in at:                                          # a game's last record: nothing is played from it
                continue
            e, a = at[r], int(ch.action[at[r]])
            assert np.array_equal(ch.move_counts[e], want0["counts"][j]), r
            assert ch.played[e].tolist() == (want0["rows"][j][a].tolist() if a < 361 else [0] * 8), (r, a)
            seen += 1
        assert seen >= 40
    finally:
        rs.close()


def test_session_moves():
    """slots set up from prefixes of a golden game against the model on the records of the same plies, for both sides; a slot that
    is no session is refused and its rows stay as they were filled; a slot may be listed twice"""
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    S = 19
    games = _golden_games()
    acts, cols = [a for a, _ in games[2]], [c for _, c in games[2]]
    n_before = sum(len(g) + 1 for g in games[:2])                    # records of games 0 and 1 in the replay
    plies = [37, 120, len(acts) // 2, len(acts) - 3]
    recs = MC.golden_records(1)[[n_before + p for p in plies]]
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=6, sims=8, energy=4, symmetry="identity")
    try:
        lib = L.require_gpu()
        slots = [4, 0, 3, 1]
        eng.open(slots)
        st, _ = eng.setup(slots, [acts[:p] for p in plies], [cols[:p] for p in plies])
        assert not st.any()
        want = [M.moves(S, recs, side=side) for side in (0, 1)]
        for side in (0, 1):
            v = eng.moves(slots, side)
            assert not v.status.any() and np.array_equal(v.rows, want[side]["rows"]) and np.array_equal(v.counts, want[side]["counts"])
        ask = np.array([2, 3, 5, 3, 4], np.int32)
        status, rows, counts = np.full(5, 77, np.int32), np.full((5, S * S, 8), FILL16, np.int16), np.full((5, 8), FILL32, np.int32)
        rc = lib.sgo_session_moves(eng.ctx, 5, L.ptr(ask), 1, L.ptr(status), L.ptr(rows), L.ptr(counts), L.stream_ptr())
        assert rc == 0 and status.tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for i in (0, 2):
            assert (rows[i] == FILL16).all() and (counts[i] == FILL32).all()
        for i, k in ((1, 2), (3, 2), (4, 0)):
            assert np.array_equal(rows[i], want[1]["rows"][k]) and np.array_equal(counts[i], want[1]["counts"][k])
        one = np.array([6], np.int32)
        assert lib.sgo_session_moves(eng.ctx, 1, L.ptr(one), 0, L.ptr(status), L.ptr(rows), L.ptr(counts), L.stream_ptr()) == SGO_ERR_ARG
        assert lib.sgo_session_moves(eng.ctx, 1, L.ptr(ask), 2, L.ptr(status), L.ptr(rows), L.ptr(counts), L.stream_ptr()) == SGO_ERR_ARG
        assert lib.sgo_session_moves(eng.ctx, 1, L.ptr(ask), 0, L.ptr(status), None, L.ptr(counts), L.stream_ptr()) == SGO_ERR_ARG
        assert lib.sgo_session_moves(eng.ctx, 0, None, 0, None, None, None, L.stream_ptr()) == 0
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
    """the 9x9 `two_chains` position played into a device session stone by stone: `sgo-moves capture` and `sgo-moves opponent
    capture` are the model's lines; then the committed 19x19 record through review.main --moves and records.main --moves: the
    flags and the table the model gives on the positions the records model replays"""
    import io
    import json
    import os
    from sejonggo_amd import gtp, moves as mv, records, review, sgfload
    from sejonggo_amd.stub_nets import make_stub
    from tests import records_model
    S = 9
    env.update({'SIZE': S, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    names, recs = MC.case_records(S)
    black, white = [(n, b, w) for n, b, w, _, _ in MC.positions(S) if n == "two_chains"][0][1:]
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", S), size=S, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev)
        for c, pts in (("B", black), ("W", white)):                  # white's stones last: black is to move
            for a in pts:
                assert e.parse_command("play %s %s" % (c, e._vertex(a))) == "=\n\n"
        k = names.index("two_chains_b")
        for words, side, kind in (("capture", 0, "capture"), ("opponent capture", 1, "capture"), ("atari", 0, "atari"), ("", 0, "all")):
            m = M.moves(S, recs[k:k + 1], side=side)
            text = mv.format_kind(mv.Moves(S, m["rows"], m["counts"]), 0, kind, e._vertex)
            assert e.parse_command(("sgo-moves " + words).strip()) == ("= " + text).rstrip(" ") + "\n\n", words
        assert e.parse_command("sgo-moves capture").startswith("= B9 captures 2 ") and "sgo-moves" in e.parse_command("list_commands").split()
    finally:
        dev.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    record = os.path.join(root, "tests", "golden", "review_S19.sgf")
    game = sgfload.load_file(record)
    assert game.size == 19 and not any(game.setup)
    replay = records_model.replay(19, [([a for a, _ in game.moves], [c for _, c in game.moves])])
    assert replay["status"][0] == 0
    model = M.moves(19, replay["records"][:len(game.moves)], side=0)                     # the position before every move
    every = 40
    args = [record, "--net", "hash", "--symmetry", "identity", "--sims", "8", "--energy", "4", "--every", str(every)]
    plain, flagged = io.StringIO(), io.StringIO()
    assert review.main(args, out=plain) == 0 and review.main(args + ["--moves"], out=flagged) == 0
    a, b = plain.getvalue().rstrip("\n").split("\n"), flagged.getvalue().rstrip("\n").split("\n")
    numbers = list(range(1, len(game.moves) + 1, every))
    assert len(a) == len(b) == len(numbers) and "|" not in plain.getvalue()
    for line, with_flags, m in zip(a, b, numbers):
        action = game.moves[m - 1][0]
        flags = mv.review_flags(19, action, model["rows"][m - 1][min(action, 360)], model["counts"][m - 1], lambda p: review.vertex(p, 19))
        assert with_flags == line + ("  | " + " ".join(flags) if flags else ""), m
    # every move of the record, without the search: the flag lists of the whole game
    found = review.add_moves([{"move_number": m} for m in range(1, len(game.moves) + 1)], game)
    for m, row in enumerate(found, 1):
        action = game.moves[m - 1][0]
        assert row["moves_flags"] == mv.review_flags(19, action, model["rows"][m - 1][min(action, 360)], model["counts"][m - 1],
                                                     lambda p: review.vertex(p, 19)), m
    assert any(f.startswith("captures") for r in found for f in r["moves_flags"]) and any("atari" in r["moves_flags"] for r in found)
    # records --moves: the table of the model's played rows and counts
    out, doc = io.StringIO(), tmp_path / "moves.json"
    env.update({'SIZE': 19})
    assert records.main([record, "--size", "19", "--moves", "--json", str(doc)], out=out) == 0
    actions = np.array([a for a, _ in game.moves])
    played = np.array([model["rows"][i][a] if a < 361 else np.zeros(8, np.int16) for i, a in enumerate(actions)])
    want = mv.bucket_table(np.arange(len(actions)), actions, played, model["counts"], 19, 20)
    assert json.load(open(str(doc)))["moves"] == json.loads(json.dumps(want))
    assert mv.format_bucket_table(want) in out.getvalue()
