"""The playout tree search beside the light playouts it stands on, at equal playout counts in one session: sgo_uct_dev from the empty
board at 19x19 and at 9x9 with many shallow trees (--wide: trees x sims) and with few deep ones (--deep), and on one 19x19 chunk -- the
five records of tests/golden/sgf_S19.npz repeated --copies times, replayed by sgo_records_replay -- with one tree of a few simulations
per record; each time sgo_playout_dev on the same rows with per_row = trees * sims as the yardstick.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, simulations/s and plies/s (from the sums the call returns), the nodes created and the largest
depth, the ratio to the playouts' rate, and the compiler's resource figures of k_uct per board size.  The settings are uct.py's
untuned defaults (expand_at, rave_equiv, prior), max_nodes = sims + 1, rules = 1, komi 7.5.

    python tools/bench_uct.py [--reps 5] [--copies 8] [--wide 1024 64] [--deep 64 1024] [--chunk-sims 4] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--wide", type=int, nargs=2, default=(1024, 64), metavar=("TREES", "SIMS"))
    ap.add_argument("--deep", type=int, nargs=2, default=(64, 1024), metavar=("TREES", "SIMS"))
    ap.add_argument("--chunk-sims", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sejonggo_amd import _lib as L
    from sejonggo_amd import uct as U
    from sejonggo_amd.records import DeviceRecords
    lib = L.require_gpu()
    n_entries, off, acts, cols, _ = load_games(a.copies)
    total = int(n_entries.sum())
    R = total + len(n_entries)
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    P = L.ptr
    komi2 = 15
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)                # noqa: E731
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)                # noqa: E731
    arms, keep = {}, {}

    def add(name, s, n, rec_ptr, cap, index, trees, sims):
        N = s * s
        max_nodes = sims + 1
        wb = L.check(lib.sgo_uct_workspace(s, n, trees, max_nodes), "sgo_uct_workspace")
        d = {"visits": i32(n, N + 1), "wins2": i32(n, N + 1), "rave": i32(n, 2, N + 1), "own": i32(n, 2, N), "sums": i64(n, 8), "info": i32(n, 4),
             "work": i32(wb // 4), "p_own": i32(n, 2, N), "p_amaf": i32(n, 2, N), "p_sums": i64(n, 8)}
        keep[name] = (d, trees, sims, wb)

        def uct():
            L.check(lib.sgo_uct_dev(s, n, rec_ptr, cap, P(index), trees, sims, 2, 1, 0, komi2, min(U.EXPAND_AT, sims), U.RAVE_EQUIV, U.PRIOR, max_nodes,
                                    P(d["visits"]), P(d["wins2"]), P(d["rave"]), P(d["own"]), P(d["sums"]), P(d["info"]), None, P(d["work"]), wb,
                                    L.stream_ptr()), "sgo_uct_dev")

        def playout():
            L.check(lib.sgo_playout_dev(s, n, rec_ptr, cap, P(index), trees * sims, 2, 1, 0, P(d["p_own"]), P(d["p_amaf"]), P(d["p_sums"]),
                                        L.stream_ptr()), "sgo_playout_dev")
        arms["uct_" + name], arms["playout_" + name] = uct, playout

    empty = {s: torch.zeros((1, 16 * ((s * s + 31) // 32)), dtype=torch.int32, device=dev) for s in (19, 9)}
    for s in (19, 9):
        for kind, (trees, sims) in (("wide", a.wide), ("deep", a.deep)):
            add("one_%d_%s" % (s, kind), s, 1, P(empty[s]), 1, None, trees, sims)

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()
    replay()
    add("chunk", S, R, be.rec_ptr, be.cap, torch.arange(R, dtype=torch.int32, device=dev), 1, a.chunk_sims)

    for fn in arms.values():                                   # warm-up: code objects
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    torch.cuda.synchronize()
    out = {"what": "sgo_uct_dev (k_uct_zero + k_uct + k_uct_best) beside sgo_playout_dev on the same rows with per_row = trees * sims: one call "
                   "from the empty board at 19x19 and 9x9 with many shallow trees (wide) and few deep ones (deep), and one 19x19 chunk of replayed "
                   "golden records with one small tree each; rules = 1, komi 7.5, the untuned defaults of uct.py, max_nodes = sims + 1; one MI355X; "
                   "HIP events around every call, arms interleaved",
           "board": S, "games": len(n_entries), "chunk_rows": R, "wide": list(a.wide), "deep": list(a.deep), "chunk_sims": a.chunk_sims,
           "settings": {"expand_at": U.EXPAND_AT, "rave_equiv": U.RAVE_EQUIV, "prior": U.PRIOR, "komi2": komi2, "rules": 1},
           "not_measured": "the share of a simulation's time spent on tree plies (the kernel carries no counter) and playing strength",
           "resources_gfx950": {"k_uct": resources("sgo_uct.hip", "k_uct")}, "arms": {}}
    for name, (d, trees, sims, wb) in keep.items():
        g, p = d["sums"].cpu().numpy().sum(axis=0), d["p_sums"].cpu().numpy().sum(axis=0)
        info = d["info"].cpu().numpy()
        assert int(g[7]) == int(p[7]) == len(info) * trees * sims
        u, q = stats(ms["uct_" + name]), stats(ms["playout_" + name])
        for st, v in ((u, g), (q, p)):
            st["playouts"], st["plies"], st["capped_share"] = int(v[7]), int(v[5]), float(v[6]) / float(v[7])
            st["playouts_per_s"] = int(v[7]) / (st["median_us"] * 1e-6)
            st["plies_per_s"] = int(v[5]) / (st["median_us"] * 1e-6)
        u.update({"trees": trees, "sims": sims, "workspace_bytes": int(wb), "nodes_created": int(info[:, 0].sum()),
                  "nodes_per_tree": float(info[:, 0].sum()) / (len(info) * trees), "largest_depth": int(info[:, 1].max()),
                  "trees_refused": int(info[:, 2].sum())})
        out["arms"]["uct_" + name], out["arms"]["playout_" + name] = u, q
        out["uct_over_playout_rate_" + name] = u["playouts_per_s"] / q["playouts_per_s"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
