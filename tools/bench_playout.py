"""The light playouts beside their neighbours in the records pipeline, on one 19x19 chunk: the five records of
tests/golden/sgf_S19.npz repeated --copies times, replayed by sgo_records_replay, then played out by sgo_playout_dev under both rule
sets with a small per_row (every record of the chunk), and read by sgo_moves_dev (side 0) and sgo_life_dev on the same rows; one
sgo_playout_dev call on ONE position with a large per_row, from the empty board at 19x19 and at 9x9.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, playouts/s and plies/s (plies from the sums the call returns), the capped share under both rule
sets, and the compiler's resource figures of k_playout per board size.

    python tools/bench_playout.py [--reps 7] [--copies 8] [--per-row 4] [--single 16384] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_chunk import S, load_games, resources, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--per-row", type=int, default=4)
    ap.add_argument("--single", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from sejonggo_amd import _lib as L
    from sejonggo_amd.records import DeviceRecords
    lib = L.require_gpu()
    n_entries, off, acts, cols, _ = load_games(a.copies)
    total = int(n_entries.sum())
    R = total + len(n_entries)
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    n, N, NW = R, S * S, be.NW
    index = torch.arange(n, dtype=torch.int32, device=dev)
    own = torch.zeros((n, 2, N), dtype=torch.int32, device=dev)
    amaf = torch.zeros((n, 2, N), dtype=torch.int32, device=dev)
    sums = torch.zeros((2, n, 8), dtype=torch.int64, device=dev)
    rows = torch.zeros((n, N, 8), dtype=torch.int16, device=dev)
    mcounts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    lsets, lcounts = torch.zeros((n, 4, NW), dtype=torch.int32, device=dev), torch.zeros((n, 8), dtype=torch.int32, device=dev)
    single = {}
    for s in (19, 9):
        single[s] = {"rec": torch.zeros((1, 16 * ((s * s + 31) // 32)), dtype=torch.int32, device=dev),
                     "own": torch.zeros((1, 2, s * s), dtype=torch.int32, device=dev), "amaf": torch.zeros((1, 2, s * s), dtype=torch.int32, device=dev),
                     "sums": torch.zeros((2, 1, 8), dtype=torch.int64, device=dev)}
    P = L.ptr

    def chunk(rules):
        def call():
            L.check(lib.sgo_playout_dev(S, n, be.rec_ptr, be.cap, P(index), a.per_row, 1, rules, 0, P(own), P(amaf), P(sums[rules]),
                                        L.stream_ptr()), "sgo_playout_dev")
        return call

    def one(s, rules):
        d = single[s]

        def call():
            L.check(lib.sgo_playout_dev(s, 1, P(d["rec"]), 1, None, a.single, 2, rules, 0, P(d["own"]), P(d["amaf"]), P(d["sums"][rules]),
                                        L.stream_ptr()), "sgo_playout_dev")
        return call

    def moves():
        L.check(lib.sgo_moves_dev(S, n, be.rec_ptr, be.cap, P(index), 0, P(rows), P(mcounts), L.stream_ptr()), "sgo_moves_dev")

    def life():
        L.check(lib.sgo_life_dev(S, n, be.rec_ptr, be.cap, P(index), P(lsets), P(lcounts), L.stream_ptr()), "sgo_life_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    arms = {"replay": replay, "moves": moves, "life": life, "playout_chunk_sound": chunk(1), "playout_chunk_inherited": chunk(0),
            "playout_one_19_sound": one(19, 1), "playout_one_19_inherited": one(19, 0), "playout_one_9_sound": one(9, 1),
            "playout_one_9_inherited": one(9, 0)}
    for fn in arms.values():                                   # warm-up: code objects, the pinned staging block
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    torch.cuda.synchronize()
    got = {"playout_chunk_sound": sums[1].cpu().numpy().sum(axis=0), "playout_chunk_inherited": sums[0].cpu().numpy().sum(axis=0)}
    for s in (19, 9):
        for rules, name in ((1, "sound"), (0, "inherited")):
            got["playout_one_%d_%s" % (s, name)] = single[s]["sums"][rules].cpu().numpy().sum(axis=0)
    assert int(got["playout_chunk_sound"][7]) == n * a.per_row and int(got["playout_one_9_sound"][7]) == a.single
    out = {"what": "sgo_playout_dev (k_playout_zero + k_playout) under both rule sets beside sgo_records_replay, sgo_moves_dev and sgo_life_dev on "
                   "one 19x19 chunk with a small per_row; one call on the empty board with a large per_row at 19x19 and 9x9; one MI355X; HIP "
                   "events around every call, arms interleaved",
           "board": S, "games": len(n_entries), "rows": n, "per_row": a.per_row, "single_per_row": a.single, "unit": 16,
           "not_measured": "the mean number of active halves per wave-ply (the kernel carries no counter) and the time of "
                           "rollout.RolloutEngine for the same number of games (it needs a resident net)",
           "resources_gfx950": {"k_playout": resources("sgo_playout.hip", "k_playout")}, "arms": {}}
    for k, v in ms.items():
        st = stats(v)
        if k in got:
            g = got[k]
            st["playouts"], st["plies"], st["capped_share"] = int(g[7]), int(g[5]), float(g[6]) / float(g[7])
            st["playouts_per_s"] = int(g[7]) / (st["median_us"] * 1e-6)
            st["plies_per_s"] = int(g[5]) / (st["median_us"] * 1e-6)
            st["mean_score"] = float(g[3]) / float(g[7])
        else:
            st["rows_per_s"] = n / (st["median_us"] * 1e-6)
        out["arms"][k] = st
    for k in ("moves", "life", "replay"):
        out["playout_chunk_sound_over_" + k] = out["arms"]["playout_chunk_sound"]["median_us"] / out["arms"][k]["median_us"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
