"""GPU: sgo_session_influence (include/sgo.h "influence") on 9x9 session slots set up with sgo_session_setup: the outputs equal the
model (tests/influence_model.py) on what sgo_game_board shows; a slot that is no holding session is refused and its rows stay as
they were filled; a slot may be listed twice; the context is left byte for byte as it was.  Then the Python surface on the device:
RecordSet.influence(dead="life"), GTP and `review --influence` against the model on the first moves of
tests/golden/review_S19.sgf (61 positions: no call lists more than 64 rows)."""
import io
import os

import numpy as np
import pytest

from tests import influence_cases as IC
from tests import influence_model as M
from tests import life_model

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_STATE = -1, -203
FILL, FILL16 = 0x3C3C3C3C, 0x3C3C
S = 9
CASES = ("corners", "walls", "dead_inside", "last_lines", "contact", "half_split")
RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "review_S19.sgf")
PLIES = 60


def _points(board17):
    from sejonggo_amd.rollout import real_board
    stones = real_board(board17).reshape(-1)
    return [int(a) for a in np.flatnonzero(stones == 1)], [int(a) for a in np.flatnonzero(stones == -1)]


def _model(size, black, white, dead, triple):
    NW = (size * size + 31) // 32
    m = M.bouzy(size, black, white, dead, *triple)
    return (np.array(m["values"], np.int16), np.stack([M.words_of(s, NW) for s in m["sets"]]), np.array(m["counts"], np.int32))


def _proved_dead(size, black, white):
    """the stones unconditional life proves dead: white stones in terr_black, black stones in terr_white"""
    m = life_model.point_life(size, black, white)
    return sorted((m["terr"][0] & set(white)) | (m["terr"][1] & set(black)))


def test_session_influence():
    import torch
    from sejonggo_amd import _lib as L
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    pos = dict((n, (b, w, d)) for n, b, w, d in IC.positions(S))
    N, NW = S * S, (S * S + 31) // 32
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=8, sims=8, energy=4, symmetry="identity")
    try:
        lib = L.require_gpu()
        slots = [4, 0, 3, 1, 6, 2]
        eng.open(slots)
        moves, cols, dead = [], [], np.zeros((len(slots), NW), np.uint32)
        for k, name in enumerate(CASES):
            b, w, d = pos[name]
            if k % 2:                                            # every other case with the colours swapped
                b, w = w, b
            moves.append(list(b) + list(w))
            cols.append([1] * len(b) + [-1] * len(w))
            dead[k] = M.words_of(d or [], NW)
        st, _ = eng.setup(slots, moves, cols)
        assert not st.any()
        stones = [_points(eng.board(s)) for s in slots]
        assert [sorted(m) for m in moves] == [sorted(b + w) for b, w in stones]          # nothing was captured on the way
        boards = [np.array(eng.board(s), copy=True) for s in range(8) if s in slots]
        for triple in (M.TERRITORY, M.AREA, (8, 31, 31)):
            want = [_model(S, b, w, M.points_of(dead[i], 32 * NW), triple) for i, (b, w) in enumerate(stones)]
            v = eng.influence(slots, dead=dead, **dict(zip(("dilate", "erode_moyo", "erode_terr"), triple)))
            assert not v.status.any()
            for i in range(len(slots)):
                assert np.array_equal(v.values[i], want[i][0]) and np.array_equal(v.sets[i], want[i][1]), (CASES[i], triple)
                assert np.array_equal(v.counts[i], want[i][2]), (CASES[i], triple)
        # dead=None, and dead="life": what the life model proves dead (nothing in these open positions but what it says)
        plain = [_model(S, b, w, (), M.TERRITORY) for b, w in stones]
        v = eng.influence(slots, dead=None)
        assert all(np.array_equal(v.values[i], plain[i][0]) and np.array_equal(v.counts[i], plain[i][2]) for i in range(len(slots)))
        proved = [_model(S, b, w, _proved_dead(S, b, w), M.TERRITORY) for b, w in stones]
        v = eng.influence(slots)
        assert all(np.array_equal(v.values[i], proved[i][0]) and np.array_equal(v.counts[i], proved[i][2]) for i in range(len(slots)))
        # slots 5 and 7 are no sessions; slot 3 is listed twice, with two different dead rows
        want = [_model(S, b, w, M.points_of(dead[i], 32 * NW), M.TERRITORY) for i, (b, w) in enumerate(stones)]
        ask = np.array([5, 3, 7, 3, 4], np.int32)
        rows = np.stack([dead[2], dead[2], dead[2], np.zeros(NW, np.uint32), dead[0]])
        status, values = np.full(5, 77, np.int32), np.full((5, N), FILL16, np.int16)
        sets, counts = np.full((5, 4, NW), FILL, np.uint32), np.full((5, 8), FILL, np.int32)
        call = lambda n=5, slots_=ask, d=rows, t=(5, 10, 21), st_=status, va=values, se=sets, co=counts: lib.sgo_session_influence(   # noqa: E731
            eng.ctx, n, L.ptr(slots_), L.ptr(d), t[0], t[1], t[2], L.ptr(st_), L.ptr(va), L.ptr(se), L.ptr(co), L.stream_ptr())
        assert call() == 0 and status.tolist() == [SGO_ERR_STATE, 0, SGO_ERR_STATE, 0, 0]
        for i in (0, 2):
            assert (values[i] == FILL16).all() and (sets[i] == FILL).all() and (counts[i] == FILL).all()
        for i, w in ((1, want[2]), (3, plain[2]), (4, want[0])):
            assert np.array_equal(values[i], w[0]) and np.array_equal(sets[i], w[1]) and np.array_equal(counts[i], w[2]), i
        assert not np.array_equal(want[2][2], plain[2][2])                               # the dead row made a difference
        # the context is only read: every board as it was
        torch.cuda.synchronize()
        assert all(np.array_equal(a, eng.board(s)) for a, s in zip(boards, [s for s in range(8) if s in slots]))
        # the refusals: a slot outside the context, NULL outputs, parameters out of range; n == 0 is a no-op
        assert call(n=1, slots_=np.array([8], np.int32)) == SGO_ERR_ARG
        assert call(va=None) == SGO_ERR_ARG and call(se=None) == SGO_ERR_ARG and call(co=None) == SGO_ERR_ARG and call(st_=None) == SGO_ERR_ARG
        assert call(t=(9, 0, 0)) == SGO_ERR_ARG and call(t=(5, 11, 10)) == SGO_ERR_ARG and call(t=(5, 10, 32)) == SGO_ERR_ARG
        assert lib.sgo_session_influence(eng.ctx, 0, None, None, 5, 10, 21, None, None, None, None, L.stream_ptr()) == 0
        assert call(d=None) == 0 and np.array_equal(counts[1], plain[2][2])
        with pytest.raises(ValueError):
            eng.influence(slots, dilate=9)
    finally:
        eng.close()


def test_session_context_is_byte_for_byte_unchanged():
    """sgo_session_influence between two tree serialisations and two board reads of every slot"""
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=4, sims=8, energy=4, symmetry="identity")
    try:
        eng.open([0, 1, 2])
        b, w, _ = dict((n, (b, w, d)) for n, b, w, d in IC.positions(S))["corners"]
        st, _ = eng.setup([0, 2], [list(b) + list(w), list(w)], [[1] * len(b) + [-1] * len(w), [1] * len(w)])
        assert not st.any()
        eng.analyze([0], 8)                                          # a tree behind slot 0
        state = lambda: [(eng.board(s).tobytes(), eng.tree_serialize(s)[0].tobytes()) for s in range(3)]   # noqa: E731
        before = state()
        v = eng.influence([0, 1, 2, 3])
        assert v.status.tolist() == [0, 0, 0, SGO_ERR_STATE] and not v.counts[3].any() and v.counts[1].tolist() == [0] * 6 + [81, 0]
        assert state() == before
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


def _opening():
    """the first PLIES moves of the golden record as a game, and the packed records of its PLIES + 1 positions"""
    from sejonggo_amd import sgfload
    from tests import records_model
    game = sgfload.load_file(RECORD)
    assert game.size == 19 and not any(game.setup) and len(game.moves) >= PLIES
    game = sgfload.SgfGame(19, game.komi, list(game.moves[:PLIES]), [False] * PLIES)
    replay = records_model.replay(19, [([a for a, _ in game.moves], [c for _, c in game.moves])])
    assert replay["status"][0] == 0
    return game, replay["records"][:PLIES + 1]


def _sgf(game):
    L = "abcdefghijklmnopqrs"
    pt = lambda a: "[%s]" % (L[a % 19] + L[a // 19] if a < 361 else "")                 # noqa: E731
    return "(;FF[4]SZ[19]" + ("KM[%s]" % game.komi if game.komi is not None else "") + "".join(";%s%s" % ("B" if c > 0 else "W", pt(a)) for a, c in game.moves) + ")"


def test_record_set_review_and_records_on_the_device(env, tmp_path):
    """RecordSet.influence(dead="life") over the opening of the golden record equals the model row for row (the dead sets from the
    life model); `review --influence` prints the model's estimate and gain per move without a net; `records --influence` the
    model's buckets"""
    import json
    from sejonggo_amd import influence as inf, records, review
    game, recs = _opening()
    komi = game.komi if game.komi is not None else 0.0
    NW = 12
    dead = np.zeros((len(recs), NW), np.uint32)
    for i, rec in enumerate(recs):
        b, w, _ = M.record_stones(19, rec)
        dead[i] = M.words_of(_proved_dead(19, b, w), NW)
    want = M.influence(19, recs, None, dead, *M.TERRITORY)
    rs = records.RecordSet([records.Record("g", 19, list(game.moves), list(game.setup), list(range(1, PLIES + 1)), None)], size=19)
    try:
        chunks = list(rs.influence(stones=True))
        assert len(chunks) == 1
        v = chunks[0].influence
        assert np.array_equal(v.values, want["values"]) and np.array_equal(v.sets, want["sets"]) and np.array_equal(v.counts, want["counts"])
        area = next(rs.influence(dead=None, **inf.PRESETS["area"])).influence
        assert np.array_equal(area.counts, M.influence(19, recs, None, None, *M.AREA)["counts"])
    finally:
        rs.close()
    path = tmp_path / "opening.sgf"
    path.write_text(_sgf(game))
    out, doc = io.StringIO(), tmp_path / "review.json"
    assert review.main([str(path), "--influence", "--json", str(doc)], out=out) == 0
    lines = out.getvalue().rstrip("\n").split("\n")
    margins = want["counts"][:, 7].astype(int)
    gains = [int(c) * int(margins[m] - margins[m - 1]) for m, (_, c) in enumerate(game.moves, 1)]
    assert len(lines) == PLIES + 1
    for m, ((a, c), line) in enumerate(zip(game.moves, lines), 1):
        assert line == "%4d %s %-4s  | estimate %s gain %+d" % (m, "B" if c > 0 else "W", review.vertex(a, 19),
                                                               inf.score_text(margins[m - 1] - komi), gains[m - 1]), m
    best, worst = inf.review_summary(list(enumerate(gains, 1)))
    part = lambda ms: " ".join("%d (%+d)" % (m, gains[m - 1]) for m in ms)               # noqa: E731
    assert lines[-1] == "influence: highest gain %s; lowest gain %s" % (part(best), part(worst))
    assert [p["gain"] for p in json.load(open(str(doc)))["positions"]] == gains
    env.update({'SIZE': 19})
    out, doc = io.StringIO(), tmp_path / "records.json"
    assert records.main([str(path), "--size", "19", "--influence", "--json", str(doc)], out=out) == 0
    got = json.load(open(str(doc)))["influence"]
    c = want["counts"].astype(np.int64)
    assert [b["positions"] for b in got["buckets"]] == [20, 20, 20, 1] and got["games"] == [{"name": "opening", "plies": PLIES, "margin": int(c[-1, 7])}]
    for k, b in enumerate(got["buckets"]):
        rows = c[20 * k:20 * k + 20]
        assert b["abs_margin"] == float(np.abs(rows[:, 7]).mean()) and b["neutral"] == float(rows[:, 6].mean())
        assert b["moyo_beyond_black"] == float((rows[:, 2] - rows[:, 0]).mean()) and b["moyo_beyond_white"] == float((rows[:, 3] - rows[:, 1]).mean())
    assert "influence opening plies %d estimate %s\n" % (PLIES, inf.score_text(int(c[-1, 7]))) in out.getvalue()


def test_record_set_lifts_a_proved_dead_stone_on_the_device():
    """a 5x5 record that ends with a white stone on the corner point of a living black group: dead="life" lifts it on the device
    (sgo_life_dev, two mask operations, sgo_influence_dev), dead=None leaves it standing; every row against the model"""
    from sejonggo_amd import records
    from tests.life_cases import diagram
    size = 5
    black, white = diagram(size, ["O.XXX", ".XX.X", "XXXXX"])
    entries = [(a, 1) for a in black] + [(a, -1) for a in white]
    stones = [([a for a, c in entries[:k] if c > 0], [a for a, c in entries[:k] if c < 0]) for k in range(len(entries) + 1)]
    rs = records.RecordSet([records.Record("g", size, entries, [False] * len(entries), list(range(1, len(entries) + 1)), None)], size=size)
    try:
        for dead in ("life", None):
            v = next(rs.influence(dead=dead)).influence
            assert len(v) == len(stones)
            for k, (b, w) in enumerate(stones):
                vals, sets, counts = _model(size, b, w, _proved_dead(size, b, w) if dead else (), M.TERRITORY)
                assert np.array_equal(v.values[k], vals) and np.array_equal(v.sets[k], sets) and np.array_equal(v.counts[k], counts), (dead, k)
            assert v.live(len(entries), -1) == (0 if dead else 1) and v.margin(len(entries)) == (25 if dead else 21)
    finally:
        rs.close()


def test_gtp_on_the_device(env):
    """the 5x5 board of tests/test_life_host.py played into a device session: white's stone inside black's living group is lifted by
    `sgo-influence` and stands with `nodead`; the text is the model's"""
    from sejonggo_amd import gtp, influence as inf
    from sejonggo_amd.stub_nets import make_stub
    from tests.life_cases import diagram
    size = 5
    env.update({'SIZE': size, 'MCTS_SIMULATIONS': 8, 'ENERGY': 4})
    black, white = diagram(size, ["O.XXX", ".XX.X", "XXXXX"])
    stones = np.zeros(size * size, np.int8)
    stones[black], stones[white] = 1, -1
    dev = gtp.DeviceSejongGoEngine(8, net=make_stub("hash", size), size=size, energy=4, symmetry="identity", n_games=1)
    try:
        e = gtp.GTPEngine(engine=dev)
        for c, pts in (("B", black), ("W", white)):
            for a in pts:
                assert e.parse_command("play %s %s" % (c, e._vertex(a))) == "=\n\n"
        e.parse_command("komi 6.5")
        assert _proved_dead(size, black, white) == [0]
        for words, dead, preset in (("", [0], "territory"), ("nodead", [], "territory"), ("area", [0], "area"), ("area nodead", [], "area")):
            p = inf.PRESETS[preset]
            vals, sets, counts = _model(size, black, white, dead, (p["dilate"], p["erode_moyo"], p["erode_terr"]))
            v = inf.Influence(size, vals[None], sets[None], counts[None])
            assert e.parse_command(("sgo-influence " + words).strip()) == "= " + inf.format_board(v, stones, 0, 6.5) + "\n\n", words
            assert e.parse_command(("sgo-estimate " + words).strip()) == "= " + inf.score_text(v.estimate(0, 6.5)) + "\n\n", words
        assert e.parse_command("sgo-influence").split("\n")[0] == "= bbXXX" and e.parse_command("sgo-estimate") == "= B+18.5\n\n"
        assert e.parse_command("sgo-influence nodead").split("\n")[0].startswith("= O")
    finally:
        dev.close()
