"""The capturing-race reader on one 19x19 chunk and on single worst-case queries: the five records of tests/golden/sgf_S19.npz
repeated --copies times, replayed by sgo_records_replay, then every pair in contact of every record enumerated and read by
sgo_race_dev at the Python defaults (rules 1, max_libs 4, max_region 8, max_nodes 1024, max_pairs 64), beside sgo_solve_dev and
sgo_tactics_dev on the same rows; and ONE asked pair on a constructed position (two one-eyed racers and a walled block of empty points,
far beyond any budget without a transposition table) whose longer racer spends the full node budget, at 19x19 and at 9x9, with
max_nodes 4096 and SGO_RACE_MAX_NODES: the time of one node of one query, and the longest launch a single `sgo-race` can cause.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, the listed pairs, the nodes read, the share of racers per verdict (the unknown share among them),
and the compiler's resource figures of k_race_pairs<S> and k_race_read<S> per board size.

    python tools/bench_race.py [--reps 5] [--copies 8] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_chunk import S, load_games, resources, stats, timed  # noqa: E402

RACERS = ["OOOXXXXXX", "XXXOOOOOX", ".XXOOO.OX"]                  # bottom-left: black and white with one one-point eye each


def block_case(size):
    """(record uint32 [1, 16 * NW], asked pair, region uint32 [1, NW]) at `size`, white to play: the racers in the bottom rows, the
    region their two eyes and a block of empty points, 5 wide, in the top-left corner behind a black wall"""
    import numpy as np
    NW = (size * size + 31) // 32
    h = 6 if size >= 13 else 4
    pic = [".....X"] * h + ["XXXXXX"] + [""] * (size - h - 4) + RACERS
    rec = np.zeros((16, NW), np.uint32)
    for y, line in enumerate(pic):
        for x, ch in enumerate(line):
            if ch in "XO":
                a = y * size + x
                for plane in ((0, 2) if ch == "X" else (1, 3)):
                    rec[plane, a >> 5] |= np.uint32(1 << (a & 31))
    rec[0, NW - 1] |= np.uint32(0x80000000)
    region = np.zeros(NW, np.uint32)
    for a in [y * size + x for y in range(h) for x in range(5)] + [(size - 1) * size, (size - 1) * size + 6]:
        region[a >> 5] |= np.uint32(1 << (a & 31))
    return rec.reshape(1, -1), ((size - 2) * size, (size - 2) * size + 3), region.reshape(1, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from sejonggo_amd import _lib as L
    from sejonggo_amd import race as rc
    from sejonggo_amd.records import DeviceRecords
    lib = L.require_gpu()
    n_entries, off, acts, cols, first = load_games(a.copies)
    total = int(n_entries.sum())
    n = total + len(n_entries)                                 # rows: every record of the chunk
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    T, N = rc.MAX_PAIRS, S * S
    index = torch.arange(n, dtype=torch.int32, device=dev)
    n_pairs = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = torch.zeros((n, T, 16), dtype=torch.int32, device=dev)
    regions = torch.zeros((n, T, be.NW), dtype=torch.int32, device=dev)
    s_targets = torch.zeros(n, dtype=torch.int32, device=dev)
    s_rows = torch.zeros((n, 64, 8), dtype=torch.int32, device=dev)
    s_regions = torch.zeros((n, 64, be.NW), dtype=torch.int32, device=dev)
    libs = torch.zeros((n, N), dtype=torch.uint8, device=dev)
    n_chains = torch.zeros(n, dtype=torch.int32, device=dev)
    chains = torch.zeros((n, 128, 8), dtype=torch.int32, device=dev)
    P = L.ptr

    def race():
        L.check(lib.sgo_race_dev(S, n, be.rec_ptr, be.cap, P(index), None, None, 1, 4, 8, 1024, T, P(n_pairs), P(rows), P(regions), L.stream_ptr()),
                "sgo_race_dev")

    def solve():
        L.check(lib.sgo_solve_dev(S, n, be.rec_ptr, be.cap, P(index), None, None, 1, 12, 4096, 64, P(s_targets), P(s_rows), P(s_regions),
                                  L.stream_ptr()), "sgo_solve_dev")

    def tactics():
        L.check(lib.sgo_tactics_dev(S, n, be.rec_ptr, be.cap, P(index), 128, P(libs), P(n_chains), P(chains), L.stream_ptr()), "sgo_tactics_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    # one asked pair whose longer racer spends its whole budget: (size, max_nodes) -> buffers
    single, single_out = {}, {}
    for size in (19, 9):
        rec, pq, region = block_case(size)
        rec, region = torch.from_numpy(rec.view(np.int32)).to(dev), torch.from_numpy(region.view(np.int32)).to(dev)
        ask = torch.tensor([pq], dtype=torch.int32, device=dev)
        for budget in (4096, rc.MAX_NODES):
            out = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((1, 1, 16), dtype=torch.int32, device=dev),
                   torch.zeros((1, 1, (size * size + 31) // 32), dtype=torch.int32, device=dev))
            single_out[(size, budget)] = out

            def one(size=size, rec=rec, ask=ask, region=region, budget=budget, out=out):
                L.check(lib.sgo_race_dev(size, 1, P(rec), 1, None, P(ask), P(region), 1, 8, 32, budget, 1, P(out[0]), P(out[1]), P(out[2]),
                                         L.stream_ptr()), "sgo_race_dev")
            single["one_pair_S%d_nodes%d" % (size, budget)] = one

    arms = {"replay": replay, "tactics": tactics, "solve": solve, "race": race}
    arms.update(single)
    for fn in arms.values():                                   # warm-up: code objects, the pinned staging block
        fn()
        torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    npr, rw = n_pairs.cpu().numpy(), rows.cpu().numpy()
    listed = np.arange(T)[None, :] < np.minimum(npr, T)[:, None]
    st = rw[:, :, 6][listed]
    words = [rc.verdict_of(s & 255) for s in st.tolist()] + [rc.verdict_of((s >> rc.WHITE_SHIFT) & 255) for s in st.tolist()]
    nodes = int(rw[:, :, 12:16][listed].sum())
    srw, snt = s_rows.cpu().numpy(), s_targets.cpu().numpy()
    s_listed = np.arange(64)[None, :] < np.minimum(snt, 64)[:, None]
    s_nodes = int(srw[:, :, 6][s_listed].sum() + srw[:, :, 7][s_listed].sum())
    out = {"what": "sgo_race_dev (k_race_pairs + k_race_read; rules 1, max_libs 4, max_region 8, max_nodes 1024, max_pairs 64, every pair in "
                   "contact enumerated) beside sgo_records_replay, sgo_tactics_dev and sgo_solve_dev (its Python defaults) on one 19x19 chunk, "
                   "and one asked pair whose longer racer spends its whole node budget (two one-eyed racers, a walled block of empty points) "
                   "at 19x19 and 9x9, one MI355X; HIP events around every call, arms interleaved",
           "board": S, "games": len(n_entries), "rows": n, "positions_with_pairs": int((npr > 0).sum()), "pairs_true": int(npr.sum()),
           "pairs_listed": int(listed.sum()), "pairs_cut_by_max_pairs": int((npr - np.minimum(npr, T)).sum()), "pairs_max": int(npr.max()),
           "pairs_per_position": float(npr.mean()), "nodes": nodes, "solve_nodes": s_nodes,
           "racer_share": {v: words.count(v) / float(max(1, len(words))) for v in rc.VERDICTS},
           "resources_gfx950": {"k_race_pairs": resources("sgo_race.hip", "k_race_pairs"), "k_race_read": resources("sgo_race.hip", "k_race_read"),
                                "k_solve_read": resources("sgo_solve.hip", "k_solve_read")},
           "arms": {}, "one_pair": {}}
    for k, v in ms.items():
        out["arms"][k] = stats(v)
    med = out["arms"]["race"]["median_us"]
    out["race_us_per_listed_pair"] = med / max(1, int(listed.sum()))
    out["race_nodes_per_us_whole_chip"] = nodes / med
    out["solve_nodes_per_us_whole_chip"] = s_nodes / out["arms"]["solve"]["median_us"]
    out["race_over_solve"] = med / out["arms"]["solve"]["median_us"]
    out["race_over_tactics"] = med / out["arms"]["tactics"]["median_us"]
    out["race_over_replay"] = med / out["arms"]["replay"]["median_us"]
    for (size, budget), o in single_out.items():
        row = o[1].cpu().numpy()[0, 0]
        longest = int(max(row[12] + row[13], row[14] + row[15]))     # the two racers run side by side: the launch lasts as long as the longer
        t = out["arms"]["one_pair_S%d_nodes%d" % (size, budget)]["median_us"]
        out["one_pair"]["S%d_nodes%d" % (size, budget)] = {"row": row.tolist(), "nodes_of_the_longer_racer": longest, "median_us": t,
                                                           "us_per_node": t / max(1, longest)}
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
