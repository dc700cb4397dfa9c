"""Wall-clock time per call of the host paths around the six position analyses, through the public surface only (so the same
file times any commit): on a 19x19 SessionEngine with --sessions slots set to prefixes of tests/golden/review_S19.sgf, each of
SessionEngine.keys / tactics / life / influence / shapes / moves for one slot and for all slots; and one full RecordSet pass each
of tactics, life, influence, shapes, moves and keys over the five records of tests/golden/sgf_S19.npz times --copies.

Every arm is timed with time.perf_counter around the call (the calls wait for their own results), the arms interleaved repetition
by repetition after a warm-up.  One JSON line: per arm the median, p10, p90 and min in microseconds.

    python tools/bench_analysis_plumbing.py [--reps 30] [--pass-reps 5] [--sessions 4] [--copies 8] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S = 19
SHAPE = ".XO/*X."


def summary(seconds):
    s = sorted(seconds)
    q = lambda f: 1e6 * s[min(len(s) - 1, int(f * len(s)))]          # noqa: E731
    return {"median_us": q(0.5), "p10_us": q(0.1), "p90_us": q(0.9), "min_us": 1e6 * s[0], "reps": len(s)}


def run(arms, reps, warmup):
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    took = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            took[k].append(time.perf_counter() - t0)
    return {k: summary(v) for k, v in took.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--sessions", type=int, default=4)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from sejonggo_amd import sgfload
    from sejonggo_amd.engine import SessionEngine
    from sejonggo_amd.records import Record, RecordSet
    from sejonggo_amd.shapes import Shape
    from sejonggo_amd.stub_nets import make_stub
    shape = Shape.parse(SHAPE)
    out = {"board": S, "sessions": a.sessions, "copies": a.copies, "arms": {}}

    game = sgfload.load_file(os.path.join(ROOT, "tests", "golden", "review_S19.sgf"))
    eng = SessionEngine(make_stub("hash", S), size=S, n_games=a.sessions, sims=8, energy=4, symmetry="identity")
    try:
        slots = list(range(a.sessions))
        plies = [game.n_moves * (i + 1) // a.sessions for i in slots]
        eng.open(slots)
        status, _ = eng.setup(slots, [[m for m, _ in game.prefix(p)] for p in plies], [[c for _, c in game.prefix(p)] for p in plies])
        assert not status.any()
        arms = {}
        for label, who in (("one", slots[-1:]), ("all", slots)):
            arms["session_keys_" + label] = lambda who=who: eng.keys(who)
            arms["session_tactics_" + label] = lambda who=who: eng.tactics(who)
            arms["session_life_" + label] = lambda who=who: eng.life(who)
            arms["session_influence_" + label] = lambda who=who: eng.influence(who)
            arms["session_shapes_" + label] = lambda who=who: eng.shapes(who, shape)
            arms["session_moves_" + label] = lambda who=who: eng.moves(who)
        out["arms"].update(run(arms, a.reps, 3))
    finally:
        eng.close()

    z = np.load(os.path.join(ROOT, "tests", "golden", "sgf_S19.npz"))
    records = []
    for copy in range(a.copies):
        for gi in range(5):
            entries = [(S * S if y >= S else int(y) * S + int(x), int(c)) for x, y, c in z["g%02d_moves" % gi]]
            records.append(Record("g%02d_%d" % (gi, copy), S, entries, [False] * len(entries), list(range(1, len(entries) + 1)), None))
    rs = RecordSet(records, S)
    try:
        def whole(gen):
            n = sum(len(ch.action) for ch in gen)
            torch.cuda.synchronize()
            return n
        passes = {"records_tactics": lambda: whole(rs.tactics()), "records_life": lambda: whole(rs.life()),
                  "records_influence": lambda: whole(rs.influence()), "records_shapes": lambda: whole(rs.shapes(shape)),
                  "records_moves": lambda: whole(rs.moves()), "records_keys": lambda: whole(rs.keys())}
        out["entries"] = passes["records_keys"]()
        out["arms"].update(run(passes, a.pass_reps, 1))
    finally:
        rs.close()
    text = json.dumps(out, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
