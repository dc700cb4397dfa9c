"""CPU: the host side of the position keys -- records.RecordSet.keys / book / duplicates, records.Book and its .npz, the command
line, and GTP's sgo-book and book genmove -- on the fake replay object (tests/fake_records.py) extended with a `keys` method from
the model (tests/keys_model.py) and on scripted engines; no GPU, no library."""
import io
import json

import numpy as np
import pytest

from sejonggo_amd import gtp
from sejonggo_amd import records as R
from tests import keys_model as K
from tests.fake_records import FakeRecords

S = 7
N = S * S
# a line of play without symmetry after its first move, with a pass and a capture-free finish; black wins
BASE = [(1, 2), (4, 4), (2, 5), None, (5, 1), (3, 3), (0, 6), (6, 0)]
LETTERS = "abcdefghijklmnopqrs"


class KeyedRecords(FakeRecords):
    """FakeRecords with the keys surface of records.DeviceRecords: the model on the records of the last replay, numpy out"""

    def keys(self, index, target=None):
        self.calls.append(("keys", len(index), target is not None))
        out = K.keys(self.S, self.last["records"], index, target)
        return out["key0"], out["canon"], out["mask"], (out["canon_action"] if target is not None else None)


def line_of(points, g, size=S):
    """[(action, colour)] of the line moved by table g; colours alternate from black"""
    L = K.luts(size)
    acts = [size * size if p is None else int(L[g, p[1] * size + p[0]]) for p in points]
    return [(a, 1 if i % 2 == 0 else -1) for i, a in enumerate(acts)]


def record_of(name, entries, winner=1, size=S, setup=None):
    setup = setup or [False] * len(entries)
    return R.Record(name, size, list(entries), list(setup), list(range(1, len(entries) + 1)), winner)


def eight_copies(size=S, points=BASE, winner=1):
    return [record_of("copy%d" % g, line_of(points, g, size), winner, size) for g in range(8)]


def make_set(recs, size=S, **kw):
    return R.RecordSet(recs, size, backend=KeyedRecords(size, kw.get("max_games", 16), kw.get("max_entries", 256)), **kw)


def test_keys_rows_beside_the_chunk_fields():
    recs = eight_copies()[:2] + [record_of("cut", [(0, 1), (0, -1), (5, 1)])]
    ch = next(make_set(recs).keys())
    assert ch.key0.dtype == ch.canon.dtype == np.uint64 and ch.mask.dtype == ch.canon_action.dtype == np.int32
    assert len(ch.canon) == len(ch.index) == 19
    assert ch.mask[0] == 255 and ch.canon[0] == 0 and ch.key0[0] == 0                      # the empty board, black to play
    assert np.array_equal(ch.canon[:8], ch.canon[8:16]) and np.array_equal(ch.canon_action[:8], ch.canon_action[8:16])
    assert not np.array_equal(ch.key0[1:8], ch.key0[9:16])
    assert ch.canon_action[3] == N                                                        # a pass stays a pass
    # the move onto a stone and what follows it were not played: they key nothing
    assert ch.valid.tolist()[16:] == [True, False, False]
    assert ch.canon[17:].tolist() == [0, 0] and ch.mask[17:].tolist() == [0, 0] and ch.canon_action[17:].tolist() == [-1, -1]


def test_eight_copies_are_one_line_of_play():
    book = make_set(eight_copies()).book()
    assert len(book) == len(BASE) and book.size == S
    assert book.count.tolist() == [8] * len(BASE)
    assert sorted(zip(book.wins.tolist(), book.losses.tolist())) == [(0, 8)] * 4 + [(8, 0)] * 4      # black won: its moves win
    assert len(np.unique(book.key)) == len(BASE)
    assert np.all(book.key[1:] > book.key[:-1])                                           # sorted, unsigned
    # unknown results count in count only; white winning swaps the columns
    open_book = make_set(eight_copies(winner=None)).book()
    assert open_book.count.tolist() == [8] * len(BASE) and not open_book.wins.any() and not open_book.losses.any()
    white = make_set(eight_copies(winner=-1)).book()
    assert np.array_equal(white.wins, book.losses) and np.array_equal(white.losses, book.wins) and np.array_equal(white.key, book.key)
    # the compat label of unknown results is a sample's, not a result
    compat = make_set(eight_copies(winner=None), compat_unknown_result=True).book()
    assert compat == open_book


def test_book_moves_come_back_in_the_board_frame():
    recs = eight_copies()
    rs = make_set(recs)
    book = rs.book()
    L = K.luts(S)
    for ch in rs.keys():
        for row in range(len(ch.index)):
            got = book.moves(ch.canon[row], ch.mask[row])
            assert len(got) == 1 and got[0][1] == 8
            a, played = got[0][0], int(ch.action[row])
            if bin(int(ch.mask[row])).count("1") == 1:
                assert a == played, row
            else:                               # a symmetric position (the empty board): the move up to the position's own symmetries
                assert a in {int(L[k, played]) for k in range(8)}
    assert book.moves(12345, 1) == [] and book.moves(int(book.key[0]), 0) == []
    # two moves in one position: ordered by count descending, then by the point
    other = [record_of("other%d" % i, line_of(BASE[:2] + [(6, 6)], 0)) for i in range(2)]
    third = [record_of("third", line_of(BASE[:2] + [(0, 0)], 0)), record_of("fourth", line_of(BASE[:2] + [(3, 0)], 0))]
    rs = make_set(recs[:1] + other + third)
    book = rs.book()
    ch = next(rs.keys())
    got = book.moves(ch.canon[2], ch.mask[2])
    assert [(a, c) for a, c, _, _ in got] == [(6 * S + 6, 2), (0, 1), (3, 1), (5 * S + 2, 1)]


def test_plies_min_count_and_chunking():
    recs = eight_copies() + [record_of("short", line_of(BASE[:3], 3), winner=-1)]
    full = make_set(recs).book()
    assert full.count.tolist().count(9) == 3 and full.count.tolist().count(8) == len(BASE) - 3
    cut = make_set(recs).book(plies=3)                       # nodes 1 and 2: the first two moves
    assert len(cut) == 2 and cut.count.tolist() == [9, 9]
    assert len(make_set(recs).book(plies=1)) == 0 and len(make_set(recs).book(plies=0)) == 0
    assert make_set(recs).book(min_count=9).count.tolist() == [9, 9, 9] and len(make_set(recs).book(min_count=10)) == 0
    # one game per replay call, and a split by entries: the same book
    one = make_set(recs, max_games=1)
    assert one.book() == full and [c[:2] for c in one.backend.calls if c[0] == "replay"] == [("replay", 1)] * 9
    assert make_set(recs, max_entries=20).book() == full
    assert make_set([]).book() == R.Book(S, [], [], [], [], [])


def test_set_up_stones_are_no_book_rows_but_count_for_duplicates():
    entries = [(8, 1), (40, -1)] + line_of(BASE[:4], 0)
    a = record_of("a", entries, setup=[True, True] + [False] * 4)
    b = record_of("b", [(int(K.luts(S)[5, x]), c) for x, c in entries], setup=[True, True] + [False] * 4)
    c = record_of("c", entries[2:])                                                        # the same moves without the stones
    rs = make_set([a, b, c])
    assert rs.book().count.sum() == 12 and rs.duplicates() == [["a", "b"]]


def test_duplicates():
    recs = eight_copies()
    changed = record_of("changed", line_of(BASE[:-1] + [(6, 1)], 2))
    shorter = record_of("shorter", line_of(BASE[:-1], 6))
    refused = record_of("refused", line_of(BASE, 1) + [(0, 1), (0, -1), (3, 1)])          # cut at the move onto a stone
    refused2 = record_of("refused2", line_of(BASE, 7) + [(int(K.luts(S)[7, 0]), 1), (int(K.luts(S)[7, 0]), -1)])
    twin = [record_of("t1", line_of([(3, 3), (0, 1)], 0)), record_of("t2", line_of([(3, 3), (0, 1)], 4))]
    rs = make_set(recs[:3] + [changed, twin[0]] + recs[3:] + [shorter, refused, twin[1], refused2])
    assert rs.duplicates() == [["copy%d" % g for g in range(8)], ["t1", "t2"], ["refused", "refused2"]]
    assert make_set(recs[:1] + [changed]).duplicates() == []
    assert make_set(recs, max_games=1).duplicates() == [["copy%d" % g for g in range(8)]]
    assert make_set([record_of("e1", []), record_of("e2", [])]).duplicates() == [["e1", "e2"]]


def test_a_signature_collision_is_not_a_duplicate(monkeypatch):
    monkeypatch.setattr(R, "sm64", lambda x: np.zeros_like(np.asarray(x, np.uint64)))       # every signature collides
    recs = eight_copies()[:2] + [record_of("changed", line_of(BASE[:-1] + [(6, 1)], 2))]
    assert make_set(recs).duplicates() == [["copy0", "copy1"]]


def test_npz_round_trip(tmp_path):
    book = make_set(eight_copies() + [record_of("short", line_of(BASE[:3], 3), winner=-1)]).book()
    path = str(tmp_path / "book.npz")
    book.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["action", "count", "key", "losses", "size", "wins"] and int(z["size"]) == S
        assert z["key"].dtype == np.uint64 and z["action"].dtype == np.int32
        assert z["count"].dtype == z["wins"].dtype == z["losses"].dtype == np.int64
        order = np.lexsort((z["action"], z["key"]))
        assert np.array_equal(order, np.arange(len(order)))
    assert R.Book.load(path) == book
    # keys above 2^63 sort as unsigned
    b = R.Book(S, [1 << 63, 5, (1 << 64) - 1], [3, 2, 1], [1, 2, 3], [0, 0, 0], [0, 0, 0])
    assert b.key.tolist() == [5, 1 << 63, (1 << 64) - 1] and b.count.tolist() == [2, 1, 3]
    assert b.moves((1 << 64) - 1, 1) == [(1, 3, 0, 0)] and b.moves(-1, 1) == [(1, 3, 0, 0)]       # the int64 of the same bits


def _sgf(entries, size=S, result="B+R"):
    vertex = lambda a: "" if a == size * size else LETTERS[a % size] + LETTERS[a // size]          # noqa: E731
    return "(;FF[4]SZ[%d]RE[%s]%s)" % (size, result, "".join(";%s[%s]" % ("B" if c == 1 else "W", vertex(a)) for a, c in entries))


def test_command_line(tmp_path, monkeypatch):
    monkeypatch.setattr(R, "DeviceRecords", lambda size, max_games, max_entries, device=0: KeyedRecords(size, max_games, max_entries))
    d = tmp_path / "games"
    d.mkdir()
    for g in range(8):
        (d / ("copy%d.sgf" % g)).write_text(_sgf(line_of(BASE, g)))
    (d / "changed.sgf").write_text(_sgf(line_of(BASE[:-1] + [(6, 1)], 2)))
    out, bookfile, doc = io.StringIO(), str(tmp_path / "b.npz"), str(tmp_path / "doc.json")
    assert R.main([str(d), "--size", str(S), "--book", bookfile, "--book-plies", "4", "--duplicates", "--json", doc], out=out) == 0
    book = R.Book.load(bookfile)
    assert len(book) == 3 and book.count.tolist() == [9, 9, 9]                            # nodes 1..3
    text = out.getvalue()
    assert "book 3 entries in 3 positions from 27 moves (plies < 4)" in text
    assert "duplicates: " + " ".join("copy%d" % g for g in range(8)) in text and "duplicate groups 1" in text
    with open(doc) as f:
        j = json.load(f)
    assert j["book"] == {"file": bookfile, "plies": 4, "entries": 3, "positions": 3, "moves": 27}
    assert j["duplicates"] == [["copy%d" % g for g in range(8)]]
    # neither option: neither entry, and no keys call
    out = io.StringIO()
    assert R.main([str(d), "--size", str(S), "--json", doc], out=out) == 0
    with open(doc) as f:
        j = json.load(f)
    assert "book" not in j and "duplicates" not in j


# ---------------------------------------------------------------------------------------------- GTP on a scripted engine
class _Net(object):
    name = "scripted"


class BookEngine(object):
    """The surface GTPEngine drives on gtp.DeviceSejongGoEngine, without a device: stones never die, the position keys are the
    model's, genmove answers from a script and says so in the trace."""

    def __init__(self, size, answers=()):
        self.size, self.model, self.trace = size, _Net(), []
        self.answers, self.illegal = list(answers), set()
        self.stones, self.to_play, self.move, self.mcts_tree = {}, 1, 1, None

    @property
    def board(self):
        b = np.zeros((1, self.size, self.size, 17), np.int32)
        for a, c in self.stones.items():
            b[0, a // self.size, a % self.size, 0 if c == self.to_play else 1] = 1
        b[..., 16] = self.to_play
        return b

    @board.setter
    def board(self, board):
        self.stones, self.to_play = {}, 1
        self.trace.append(("clear",))

    def _put(self, a, colour):
        if a < self.size * self.size:
            self.stones[a] = colour
        self.to_play = -colour

    def play(self, color, x, y, update_tree=True):
        a = y * self.size + x if y < self.size else self.size * self.size
        self.trace.append(("play", color, a))
        self._put(a, color)
        return self.board, color

    def genmove(self, color):
        a = self.answers.pop(0)
        self.trace.append(("genmove", color, a))
        self._put(a, color)
        x, y = (a % self.size, a // self.size) if a < self.size * self.size else (0, self.size)
        return x, y, None, 0.0, self.board, color

    def load(self, moves, colors=None, n_setup=0):
        raise AssertionError("not reached")

    def keys(self):
        rec = K.build_record(self.size, [a for a, c in self.stones.items() if c == 1], [a for a, c in self.stones.items() if c == -1],
                             self.to_play == -1)
        _, canon, mask, _ = K.outputs(self.size, K.record_keys(self.size, rec), None)
        self.trace.append(("keys",))
        return canon, mask

    def legal(self):
        ok = np.ones(self.size * self.size + 1, bool)
        ok[list(self.stones) + list(self.illegal)] = False
        return ok


@pytest.fixture()
def conf7(monkeypatch):
    from sejonggo_amd.conf import conf
    monkeypatch.setitem(conf, 'SIZE', S)
    empty = np.zeros((1, S, S, 17), np.int32)
    empty[..., 16] = 1
    monkeypatch.setattr(gtp, "game_init", lambda size=None: (empty.copy(), 1))
    return conf


def _vertex(e, a):
    return e.print_move(a % S, a // S) if a < N else "pass"


def test_gtp_sgo_book_and_book_genmove(conf7):
    # the book holds the line rotated by table 4; the game on the board is the line as written: the moves come back in ITS frame
    book = make_set([record_of("r%d" % i, line_of(BASE, 4)) for i in range(3)] + [record_of("alt", line_of(BASE[:2] + [(6, 6)], 4), -1)]).book()
    line = [a for a, _ in line_of(BASE, 0)]
    eng = BookEngine(S, answers=[11, 12])
    e = gtp.GTPEngine(engine=eng, book=book)
    assert e.parse_command("known_command sgo-book") == "= true\n\n" and "sgo-book" in e.parse_command("list_commands").split()
    first = e.parse_command("sgo-book")
    assert first.startswith("= ") and first.endswith(" 4 3 1\n\n") and first.count("\n") == 2       # one move, some image of the first
    assert e.parse_command("play B %s" % _vertex(e, line[0])) == "=\n\n"
    assert e.parse_command("sgo-book") == "= %s 4 1 3\n\n" % _vertex(e, line[1])
    assert e.parse_command("genmove W") == "= %s\n\n" % _vertex(e, line[1])
    assert eng.trace[-1] == ("play", -1, line[1])                                           # through play, not through the search
    assert e.parse_command("sgo_book") == "= %s 3 3 0\n%s 1 0 1\n\n" % (_vertex(e, line[2]), _vertex(e, 6 * S + 6))
    assert e.parse_command("genmove B") == "= %s\n\n" % _vertex(e, line[2])
    assert e.parse_command("genmove W") == "= pass\n\n" and eng.trace[-1] == ("play", -1, N)  # the book's pass is a move like any other
    # the book move is not legal: the search answers
    eng.illegal = {line[4]}
    assert e.parse_command("genmove B") == "= %s\n\n" % _vertex(e, 11) and eng.trace[-1] == ("genmove", 1, 11)
    # a position the book does not know: an empty answer, and the search
    assert e.parse_command("sgo-book") == "=\n\n"
    assert e.parse_command("genmove W") == "= %s\n\n" % _vertex(e, 12) and eng.trace[-1] == ("genmove", -1, 12)
    assert eng.answers == []


def test_gtp_book_min_and_out_of_turn(conf7):
    book = make_set([record_of("r%d" % i, line_of(BASE, 0)) for i in range(3)] + [record_of("alt", line_of(BASE[:1] + [(6, 6)], 0))]).book()
    line = [a for a, _ in line_of(BASE, 0)]
    eng = BookEngine(S, answers=[20, 21, 22])
    e = gtp.GTPEngine(engine=eng, book=book, book_min=4)
    orbit = {"= %s\n\n" % _vertex(e, int(K.luts(S)[k, line[0]])) for k in range(8)}
    assert e.parse_command("genmove B") in orbit and eng.trace[-1][0] == "play"             # played 4 times; the empty board is symmetric
    assert e.parse_command("clear_board") == "=\n\n" and e.parse_command("play B %s" % _vertex(e, line[0])) == "=\n\n"
    assert e.parse_command("sgo-book").count("\n") == 3                                     # both moves are listed ...
    assert e.parse_command("genmove W") == "= %s\n\n" % _vertex(e, 20)                      # ... 3 and 1 times: below the minimum
    assert eng.trace[-1] == ("genmove", -1, 20)
    e3 = gtp.GTPEngine(engine=BookEngine(S), book=book, book_min=3)
    assert e3.parse_command("play B %s" % _vertex(e, line[0])) == "=\n\n"
    assert e3.parse_command("genmove W") == "= %s\n\n" % _vertex(e, line[1])
    # the side that is not to move: the engine's own answer (the device engine refuses it), the book is not asked
    n_keys = eng.trace.count(("keys",))
    assert e.parse_command("genmove W") == "= %s\n\n" % _vertex(e, 21) and eng.trace.count(("keys",)) == n_keys


def test_gtp_without_a_book_is_unchanged(conf7, monkeypatch):
    """the reference's recorded session (tests/golden/gtp_S9.npz) through GTPEngine on an engine that answers genmove with the
    recorded moves: the transcript is the golden's, the engine is never asked for keys, and an EMPTY book changes nothing either"""
    from sejonggo_amd.conf import conf
    from tests.helpers import load, name_of
    z = load("gtp_S9.npz")
    size = int(z["size"])
    monkeypatch.setitem(conf, 'SIZE', size)
    script, replies = name_of(z, "script").split("\n"), name_of(z, "replies").split("\x1e")
    text = gtp.GTPEngine(engine=object())
    answers = []
    for cmd, rep in zip(script, replies):
        if cmd.startswith("genmove"):
            x, y = text.parse_move(rep[2:].strip())
            answers.append(y * size + x if y < size else size * size)
    for kw in ({}, {"book": R.Book(size, [], [], [], [], [])}):
        eng = BookEngine(size, answers=list(answers))
        e = gtp.GTPEngine(engine=eng, **kw)
        assert [e.parse_command(c) for c in script] == replies
        assert (("keys",) in eng.trace) == bool(kw)
        assert [t[0] for t in eng.trace if t[0] != "keys"] == ["clear"] + ["play" if c.startswith("play") else "genmove"
                                                                          for c in script if c.startswith(("play", "genmove"))]
    assert e.parse_command("sgo-book") == "=\n\n"
    assert gtp.GTPEngine(engine=BookEngine(size)).parse_command("sgo-book") == "=\n\n"     # no book at all: nothing to list


def test_the_host_engine_refuses_a_book(conf7, capsys):
    class Host(object):
        model = _Net()
    with pytest.raises(ValueError, match="device engine"):
        gtp.GTPEngine(engine=Host(), book=R.Book(S, [], [], [], [], []))
    assert gtp.GTPEngine(engine=Host()).parse_command("sgo-book") == "? not supported\n\n"
    with pytest.raises(ValueError, match="the book is 5x5"):
        gtp.GTPEngine(engine=BookEngine(S), book=R.Book(5, [], [], [], [], []))
    assert gtp.main(io.StringIO("quit\n"), io.StringIO(), device=False, book="book.npz") == 2
    assert "--book needs the device engine" in capsys.readouterr().err
