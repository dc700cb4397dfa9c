"""The life-and-death reader on one 19x19 chunk and on single worst-case queries: the five records of tests/golden/sgf_S19.npz
repeated --copies times, replayed by sgo_records_replay, then every enclosed chain of every record enumerated and read by
sgo_solve_dev at the Python defaults (rules 1, max_region 12, max_nodes 4096, max_targets 64), beside sgo_life_dev and
sgo_tactics_dev on the same rows; and ONE asked query on a constructed position (a chain around a 2 x 6 block of empty points in the
corner, far beyond any budget without a transposition table) that spends the full node budget, at 19x19 and at 9x9, with max_nodes
4096 and SGO_SOLVE_MAX_NODES: the time of one node of one query, and the longest launch a single `sgo-solve` can cause.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, the listed rows, the nodes read, the share of rows per verdict (the unknown share among them),
and the compiler's resource figures of k_solve_targets<S> and k_solve_read<S> per board size.

    python tools/bench_solve.py [--reps 5] [--copies 8] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_chunk import S, load_games, resources, stats, timed  # noqa: E402

BLOCK = ["......XO", "......XO", "XXXXXXXO", "OOOOOOOO"]        # the asked chain is the X wall; its anchor is (6, 0)


def block_record(size):
    """uint32 [1, 16 * NW]: the worst-case position at `size`, white (the attacker) to play"""
    import numpy as np
    NW = (size * size + 31) // 32
    rec = np.zeros((16, NW), np.uint32)
    for y, line in enumerate(BLOCK):
        for x, ch in enumerate(line):
            if ch in "XO":
                a = y * size + x
                for plane in ((0, 2) if ch == "X" else (1, 3)):
                    rec[plane, a >> 5] |= np.uint32(1 << (a & 31))
    rec[0, NW - 1] |= np.uint32(0x80000000)
    return rec.reshape(1, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from sejonggo_amd import _lib as L
    from sejonggo_amd import solve as sv
    from sejonggo_amd.records import DeviceRecords
    lib = L.require_gpu()
    n_entries, off, acts, cols, first = load_games(a.copies)
    total = int(n_entries.sum())
    n = total + len(n_entries)                                 # rows: every record of the chunk
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    T, N = sv.MAX_TARGETS, S * S
    index = torch.arange(n, dtype=torch.int32, device=dev)
    n_targets = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = torch.zeros((n, T, 8), dtype=torch.int32, device=dev)
    regions = torch.zeros((n, T, be.NW), dtype=torch.int32, device=dev)
    lsets = torch.zeros((n, 4, be.NW), dtype=torch.int32, device=dev)
    lcounts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    libs = torch.zeros((n, N), dtype=torch.uint8, device=dev)
    n_chains = torch.zeros(n, dtype=torch.int32, device=dev)
    chains = torch.zeros((n, 128, 8), dtype=torch.int32, device=dev)
    P = L.ptr

    def solve():
        L.check(lib.sgo_solve_dev(S, n, be.rec_ptr, be.cap, P(index), None, None, 1, 12, 4096, T, P(n_targets), P(rows), P(regions), L.stream_ptr()),
                "sgo_solve_dev")

    def life():
        L.check(lib.sgo_life_dev(S, n, be.rec_ptr, be.cap, P(index), P(lsets), P(lcounts), L.stream_ptr()), "sgo_life_dev")

    def tactics():
        L.check(lib.sgo_tactics_dev(S, n, be.rec_ptr, be.cap, P(index), 128, P(libs), P(n_chains), P(chains), L.stream_ptr()), "sgo_tactics_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    # one asked query that spends its whole budget: (size, max_nodes) -> buffers
    single, single_out = {}, {}
    for size in (19, 9):
        rec = torch.from_numpy(block_record(size).view(np.int32)).to(dev)
        ask = torch.tensor([6], dtype=torch.int32, device=dev)
        for budget in (4096, sv.MAX_NODES):
            out = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((1, 1, 8), dtype=torch.int32, device=dev),
                   torch.zeros((1, 1, (size * size + 31) // 32), dtype=torch.int32, device=dev))
            single_out[(size, budget)] = out

            def one(size=size, rec=rec, ask=ask, budget=budget, out=out):
                L.check(lib.sgo_solve_dev(size, 1, P(rec), 1, None, P(ask), None, 1, 12, budget, 1, P(out[0]), P(out[1]), P(out[2]), L.stream_ptr()),
                        "sgo_solve_dev")
            single["one_query_S%d_nodes%d" % (size, budget)] = one

    arms = {"replay": replay, "life": life, "tactics": tactics, "solve": solve}
    arms.update(single)
    for fn in arms.values():                                   # warm-up: code objects, the pinned staging block
        fn()
        torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    nt, rw = n_targets.cpu().numpy(), rows.cpu().numpy()
    listed = np.arange(T)[None, :] < np.minimum(nt, T)[:, None]
    st = rw[:, :, 3][listed]
    verdicts = [sv.verdict_of(s) for s in st.tolist()]
    nodes = int(rw[:, :, 6][listed].sum() + rw[:, :, 7][listed].sum())
    out = {"what": "sgo_solve_dev (k_solve_targets + k_solve_read; rules 1, max_region 12, max_nodes 4096, max_targets 64, every enclosed "
                   "chain enumerated) beside sgo_records_replay, sgo_life_dev and sgo_tactics_dev on one 19x19 chunk, and one asked query "
                   "that spends its whole node budget (a chain around a 2 x 6 block of empty points) at 19x19 and 9x9, one MI355X; HIP "
                   "events around every call, arms interleaved",
           "board": S, "games": len(n_entries), "rows": n, "positions_with_targets": int((nt > 0).sum()), "targets_true": int(nt.sum()),
           "targets_listed": int(listed.sum()), "targets_cut_by_max_targets": int((nt - np.minimum(nt, T)).sum()), "targets_max": int(nt.max()),
           "nodes": nodes, "verdict_share": {v: verdicts.count(v) / float(max(1, len(verdicts))) for v in sv.VERDICTS},
           "resources_gfx950": {"k_solve_targets": resources("sgo_solve.hip", "k_solve_targets"), "k_solve_read": resources("sgo_solve.hip", "k_solve_read")},
           "arms": {}, "one_query": {}}
    for k, v in ms.items():
        out["arms"][k] = stats(v)
    med = out["arms"]["solve"]["median_us"]
    out["solve_us_per_listed_target"] = med / max(1, int(listed.sum()))
    out["solve_nodes_per_us_whole_chip"] = nodes / med
    out["solve_over_life"] = med / out["arms"]["life"]["median_us"]
    out["solve_over_tactics"] = med / out["arms"]["tactics"]["median_us"]
    for (size, budget), o in single_out.items():
        row = o[1].cpu().numpy()[0, 0]
        q = int(row[6]) + int(row[7])
        t = out["arms"]["one_query_S%d_nodes%d" % (size, budget)]["median_us"]
        out["one_query"]["S%d_nodes%d" % (size, budget)] = {"row": row.tolist(), "nodes": q, "median_us": t, "us_per_node": t / max(1, q)}
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
