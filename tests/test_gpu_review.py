"""GPU: `python -m sejonggo_amd.review` on the committed game record with the rounding-free stub net, in a fresh child process,
against an engine.SessionEngine driven by hand."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "review_S19.sgf")
EVERY, SIMS, E, TOP, DEPTH = 40, 16, 8, 3, 6


def test_review_of_the_committed_record(tmp_path):
    from sejonggo_amd import _lib, review, sgfload
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.stub_nets import make_stub
    _lib.require_gpu()
    out = tmp_path / "review.json"
    cmd = [sys.executable, "-m", "sejonggo_amd.review", RECORD, "--net", "hash", "--symmetry", "identity", "--every", str(EVERY),
           "--sims", str(SIMS), "--energy", str(E), "--top", str(TOP), "--depth", str(DEPTH), "--json", str(out)]
    res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.rstrip("\n").split("\n")
    doc = json.load(open(str(out)))
    game = sgfload.load_file(RECORD)
    moves = list(range(1, game.n_moves + 1, EVERY))
    assert len(lines) == len(moves) == len(doc["positions"]) == 8
    assert [int(l.split()[0]) for l in lines] == moves
    assert lines == [review.format_row(r) for r in doc["positions"]]
    assert (doc["size"], doc["komi"], doc["sims"], doc["energy"], doc["moves"]) == (19, 6.5, SIMS, E, game.n_moves)

    # the same positions by hand: one slot each, setup / analyze / report
    eng = SessionEngine(make_stub("hash", 19), size=19, n_games=len(moves), sims=SIMS, energy=E, komi=6.5, symmetry="identity")
    try:
        slots = np.arange(len(moves))
        eng.open(slots)
        lists = [game.moves[:m - 1] for m in moves]
        status, _ = eng.setup(slots, [[a for a, _ in l] for l in lists], [[c for _, c in l] for l in lists])
        assert not status.any()
        eng.analyze(slots, SIMS)
        r = eng.report(slots, top=TOP, depth=DEPTH)
    finally:
        eng.close()
    for i, (m, row) in enumerate(zip(moves, doc["positions"])):
        played, colour = game.moves[m - 1]
        N, Q, P = r["N"][i], r["Q"][i], r["P"][i]
        assert row["move_number"] == m and row["colour"] == ("B" if colour > 0 else "W") and row["played"] == review.vertex(played, 19)
        assert row["visits"] == int(N[N > 0].sum()) == SIMS and row["root_value"] == float(r["root_value"][i])
        assert row["played_visits"] == max(0, int(N[played])) and row["played_mean"] == float(Q[played])
        assert row["played_share"] == max(0, int(N[played])) / float(SIMS)
        best = int(r["top_action"][i][0])
        assert row["best"] == review.vertex(best, 19) and row["best_mean"] == float(Q[best]) and row["best_visits"] == int(N[best])
        assert [t["move"] for t in row["top"]] == [review.vertex(int(a), 19) for a in r["top_action"][i]]
        assert [t["visits"] for t in row["top"]] == [int(N[a]) for a in r["top_action"][i]]
        assert [t["prior"] for t in row["top"]] == [float(P[a]) for a in r["top_action"][i]]
        assert [t["pv"] for t in row["top"]] == [[review.vertex(int(v), 19) for v in line if v >= 0] for line in r["pv"][i]]
