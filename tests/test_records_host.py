"""CPU: the host side of records.py -- reading records (RE, node indices, skipped files), value targets, chunking, the sample
layout -- on a fake replay object (tests/fake_records.py); no GPU, no library."""
import os

import numpy as np

from sejonggo_amd import records as R
from sejonggo_amd import sgfload
from tests.fake_records import FakeRecords
from tests.helpers import read_sample


def _winner(text):
    return sgfload.result_winner(sgfload.root_properties(text))


def test_result_parsing():
    assert _winner("(;SZ[5]RE[B+R];B[aa])") == 1
    assert _winner("(;SZ[5]RE[W+2.5];B[aa])") == -1
    assert _winner("(;SZ[5]RE[b+Resign];B[aa])") == 1
    assert _winner("(;SZ[5]RE[0];B[aa])") is None
    assert _winner("(;SZ[5]RE[Void];B[aa])") is None
    assert _winner("(;SZ[5];B[aa])") is None
    assert sgfload.root_properties("(;SZ[5]PB[x]RE[B+1];B[aa]RE[W+1])") == {"SZ": ["5"], "PB": ["x"], "RE": ["B+1"]}


def test_node_indices():
    # a root without a move: the first move is node 1, as enumerate(get_main_sequence()) numbers it
    assert sgfload.node_indices("(;SZ[5];B[aa];W[bb];B[])") == [1, 2, 3]
    # a root that carries a move is node 0
    assert sgfload.node_indices("(;B[aa];W[bb])") == [0, 1]
    # set-up stones carry their node's index; a compressed rectangle counts every point; an empty node still counts
    text = "(;SZ[5]AB[aa:bb][dd]AW[ee];;B[cc](;W[ca])(;W[cb];B[da]))"
    game = sgfload.loads(text)
    assert sgfload.node_indices(text) == [0] * 6 + [2, 3] and len(game.moves) == 8
    assert game.setup == [True] * 6 + [False, False]
    rec = R.parse_record(text, "g")
    assert rec.nodes == [0] * 6 + [2, 3] and rec.winner is None and rec.size == 5


def test_value_targets_default_and_compat():
    z, has = R.value_targets(1, [1, -1, 1])
    assert z.tolist() == [1, -1, 1] and has.all()
    z, has = R.value_targets(-1, [1, -1, 1])
    assert z.tolist() == [-1, 1, -1] and has.all()
    z, has = R.value_targets(None, [1, -1])
    assert z.tolist() == [0, 0] and not has.any()
    z, has = R.value_targets(None, [1, -1], compat_unknown=True)
    assert z.tolist() == [-1, -1] and has.all()


TEXTS = {"won": "(;SZ[5]RE[B+R]AB[bb]AW[dd];B[cc];W[];B[ab])",
         "open": "(;SZ[5];B[aa];W[bb])",
         "refused": "(;SZ[5]RE[W+1];B[aa];W[aa];B[cc])"}


def _set(names, **kw):
    recs = [R.parse_record(TEXTS[n], n) for n in names]
    return R.RecordSet(recs, 5, backend=FakeRecords(5, kw.get("max_games", 8), kw.get("max_entries", 64)), **kw)


def test_replay_rows_and_chunks():
    rs = _set(["won", "open", "refused"])
    chunks = list(rs.replay())
    assert len(chunks) == 1
    ch = chunks[0]
    assert ch.index.tolist() == [0, 1, 2, 3, 4, 6, 7, 9, 10, 11]          # base_g + j with base_g = off[g] + g
    assert ch.game.tolist() == [0] * 5 + [1] * 2 + [2] * 3
    assert ch.node.tolist() == [0, 0, 1, 2, 3, 1, 2, 1, 2, 3]
    assert ch.setup.tolist() == [True, True] + [False] * 8
    assert ch.z.tolist() == [1, -1, 1, -1, 1, 0, 0, -1, 1, -1]
    assert ch.valid.tolist() == [True] * 8 + [False, False]               # the move onto a stone and what follows it
    assert ch.sample.tolist() == [False, False, True, True, True, False, False, True, False, False]
    assert rs.refused == [("refused", -101, 1)]
    # one game per call: three chunks with indices of their own
    rs = _set(["won", "open", "refused"], max_games=1)
    chunks = list(rs.replay())
    assert [c.games for c in chunks] == [[0], [1], [2]] and chunks[1].index.tolist() == [0, 1]
    assert [c[:2] for c in rs.backend.calls] == [("replay", 1)] * 3
    # by entries: 5 + 2 fit 7, the third game starts a new call
    rs = _set(["won", "open", "refused"], max_entries=7)
    assert [c.games for c in rs.replay()] == [[0, 1], [2]]
    rs = _set(["open"], compat_unknown_result=True)
    ch = next(rs.replay())
    assert ch.z.tolist() == [-1, -1] and ch.sample.all()


def test_sample_layout_and_existing_directory(tmp_path):
    from oracle import oracle
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "KGS", "refused"))
    rs = _set(["won", "open", "refused"])
    out = rs.write_samples(root)
    assert out == {"games": 1, "samples": 3, "existing": ["refused"], "empty": ["open"]}
    assert sorted(os.listdir(os.path.join(root, "KGS"))) == ["refused", "won"]
    assert os.listdir(os.path.join(root, "KGS", "refused")) == []         # left alone
    assert sorted(os.listdir(os.path.join(root, "KGS", "won"))) == ["move_001", "move_002", "move_003"]
    board, _ = oracle.game_init(5)
    oracle.make_play(1, 1, board, 1)
    oracle.make_play(3, 3, board, -1)
    for node, a, colour in ((1, 12, 1), (2, 25, -1), (3, 5, 1)):
        b, p, v = read_sample(os.path.join(root, "KGS", "won", "move_%03d" % node, "sample.h5"))
        assert b.shape == (1, 5, 5, 17) and b.dtype == np.float32 and np.array_equal(b, board.astype(np.float32))
        assert p.shape == (26,) and p.dtype == np.float32 and p[a] == 1.0 and p.sum() == 1.0
        assert np.shape(v) == () and float(v) == float(colour)            # black won
        oracle.make_play(a % 5 if a < 25 else 0, a // 5 if a < 25 else 5, board, colour)
    # the reference's label for a record without a decided result
    rs = _set(["open"], compat_unknown_result=True)
    out = rs.write_samples(root)
    assert out["samples"] == 2
    for node in (1, 2):
        assert float(read_sample(os.path.join(root, "KGS", "open", "move_%03d" % node, "sample.h5"))[2]) == -1.0


def test_skipped_files(tmp_path):
    d = tmp_path / "sgf"
    d.mkdir()
    (d / "a_good.sgf").write_text(TEXTS["won"])
    (d / "b_broken.sgf").write_text("(;SZ[5];B[aa")
    (d / "c_size9.sgf").write_text("(;SZ[9];B[aa])")
    (d / "d_binary.sgf").write_bytes(b"\xff\xfe\x00(")
    (d / "e_long.sgf").write_text("(;SZ[5]" + ";B[]" * 101 + ")")
    (d / "notes.txt").write_text("no record")
    recs, skipped = R.read_path(str(d), 5)
    assert [r.name for r in recs] == ["a_good"]
    assert skipped == {"unreadable": ["b_broken", "d_binary"], "wrong_size": ["c_size9"], "too_long": ["e_long"]}
    recs, skipped = R.read_path(str(d / "a_good.sgf"), 5)
    assert len(recs) == 1 and recs[0].winner == 1


def test_float_sums_and_tables():
    p = np.array([0.5, 0.0, np.nan, 2.0, 0.25], np.float32)
    v = np.array([0.5, -1.0, 0.0, 1.0, -0.5], np.float32)
    z = np.array([1, -1, 0, 1, 1], np.int32)
    b = np.array([0, 1, 1, 0, 0], np.int32)
    ce, se = R.float_sums(p, v, z, b, 2)
    assert ce[0] == (0.0 + -np.log(0.5)) + 0.0 + -np.log(0.25) and ce[1] == 2 * -np.log(2.0 ** -149)
    assert se.tolist() == [0.25 + 0.0 + 2.25, 0.0]
    counters = np.array([[3, 1, 3, 0, 3, 2, 0, 0], [2, 0, 1, 1, 1, 1, 0, 0]], np.int64)
    buckets, total = R.tables(counters, ce, se, 20)
    assert buckets[1]["first_move"] == 20 and buckets[0]["value_mse"] == 2.5 / 3 and total["rows"] == 5
    assert total["ce_sum"] == ce[0] + ce[1] and total["value_agree"] == 3
