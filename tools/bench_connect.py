"""The connection reader on one 19x19 chunk and on single worst-case queries: the five records of tests/golden/sgf_S19.npz repeated
--copies times, replayed by sgo_records_replay, then every near pair of every record enumerated and read by sgo_connect_dev at the
Python defaults (rules 1, cut_libs 1, max_region 8, max_nodes 1024, max_pairs 64), beside sgo_race_dev on the same rows; the same
rows again at max_region 12 and 16 (what a larger default would cost and open up); and ONE query that spends its whole node budget
-- the peep of tests/connect_cases.py at cut_libs 2, nine empty points, which no budget up to the cap decides -- at 19x19 and at 9x9,
with max_nodes 4096 and SGO_CONNECT_MAX_NODES, with one half of the wave reading (one peep) and with both (two peeps in two corners,
enumerated): the time of one node, and the longest launch a single `sgo-connect` can cause.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, the listed pairs, the nodes read, the share of pairs per verdict, the groups beside the chains,
and the compiler's resource figures of the three kernels per board size.

    python tools/bench_connect.py [--reps 5] [--copies 8] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_chunk import S, load_games, resources, stats, timed  # noqa: E402

PEEP = ["", ".XO", "..X"]


def peep_case(size, both):
    """record uint32 [1, 16 * NW] at `size`, white to play: the peep in the top-left corner and, with `both`, a second one the same
    distance from the bottom-right corner (its region has nine empty points too)"""
    import numpy as np
    NW = (size * size + 31) // 32
    rec = np.zeros((16, NW), np.uint32)
    for ox in (0, size - 4) if both else (0,):
        for y, line in enumerate(PEEP):
            for x, ch in enumerate(line):
                if ch in "XO":
                    a = (ox + y) * size + ox + x
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
    from sejonggo_amd import connect as cn
    from sejonggo_amd.records import DeviceRecords
    import functools
    import vmcnt_isa_check
    vmcnt_isa_check.device_asm = functools.lru_cache(maxsize=None)(vmcnt_isa_check.device_asm)   # one listing serves the three kernels
    lib = L.require_gpu()
    n_entries, off, acts, cols, first = load_games(a.copies)
    total = int(n_entries.sum())
    n = total + len(n_entries)                                 # rows: every record of the chunk
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    T, N = cn.MAX_PAIRS, S * S
    index = torch.arange(n, dtype=torch.int32, device=dev)
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.int32), device=dev)   # noqa: E731
    outs = {r: (z(n), z(n, T, cn.WORDS), z(n, T, be.NW), z(n, N, dtype=torch.int16), z(n, 4)) for r in (8, 12, 16)}
    r_pairs, r_rows, r_regions = z(n), z(n, T, 16), z(n, T, be.NW)
    P = L.ptr

    def connect(region=8):
        o = outs[region]
        L.check(lib.sgo_connect_dev(S, n, be.rec_ptr, be.cap, P(index), None, None, 1, 1, region, 1024, T, P(o[0]), P(o[1]), P(o[2]), P(o[3]),
                                    P(o[4]), L.stream_ptr()), "sgo_connect_dev")

    def race():
        L.check(lib.sgo_race_dev(S, n, be.rec_ptr, be.cap, P(index), None, None, 1, 4, 8, 1024, T, P(r_pairs), P(r_rows), P(r_regions),
                                 L.stream_ptr()), "sgo_race_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    # one query (or two side by side) that spends its whole budget: (size, halves, max_nodes) -> buffers
    single, single_out = {}, {}
    for size in (19, 9):
        for halves in (1, 2):
            rec = torch.from_numpy(peep_case(size, halves == 2).view(np.int32)).to(dev)
            for budget in (4096, cn.MAX_NODES):
                nw = (size * size + 31) // 32
                out = (z(1), z(1, 2, cn.WORDS), z(1, 2, nw), z(1, size * size, dtype=torch.int16), z(1, 4))
                single_out[(size, halves, budget)] = out

                def one(size=size, rec=rec, budget=budget, out=out):
                    L.check(lib.sgo_connect_dev(size, 1, P(rec), 1, None, None, None, 1, 2, 9, budget, 2, P(out[0]), P(out[1]), P(out[2]), P(out[3]),
                                                P(out[4]), L.stream_ptr()), "sgo_connect_dev")
                single["peep_S%d_halves%d_nodes%d" % (size, halves, budget)] = one

    arms = {"replay": replay, "race": race, "connect": connect, "connect_region12": lambda: connect(12), "connect_region16": lambda: connect(16)}
    arms.update(single)
    for fn in arms.values():                                   # warm-up: code objects, the pinned staging block
        fn()
        torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))

    def figures(o):
        npr, rw, gc = o[0].cpu().numpy(), o[1].cpu().numpy(), o[4].cpu().numpy()
        listed = np.arange(T)[None, :] < np.minimum(npr, T)[:, None]
        words = [cn.verdict_of(s) for s in rw[:, :, 6][listed].tolist()]
        return {"positions_with_pairs": int((npr > 0).sum()), "pairs_true": int(npr.sum()), "pairs_listed": int(listed.sum()),
                "pairs_cut_by_max_pairs": int((npr - np.minimum(npr, T)).sum()), "pairs_max": int(npr.max()), "pairs_per_position": float(npr.mean()),
                "nodes": int(rw[:, :, 10:12][listed].sum()), "verdict_share": {v: words.count(v) / float(max(1, len(words))) for v in cn.VERDICTS},
                "chains_per_position": float(gc[:, 0].mean()), "groups_per_position": float(gc[:, 1].mean()),
                "positions_with_cut_table": int((gc[:, 3] & 1 != 0).sum()), "positions_with_undecided_pairs": int((gc[:, 3] & 2 != 0).sum())}

    # how many NEAR pairs there are whatever their region: enumerated at the largest region the interface takes, unread (one node)
    wide = (z(n), z(n, T, cn.WORDS), z(n, T, be.NW), z(n, N, dtype=torch.int16), z(n, 4))
    L.check(lib.sgo_connect_dev(S, n, be.rec_ptr, be.cap, P(index), None, None, 1, 1, 32, 1, T, *[P(t) for t in wide], L.stream_ptr()), "sgo_connect_dev")
    torch.cuda.synchronize()
    wide_pairs, wide_rows = wide[0].cpu().numpy(), wide[1].cpu().numpy()
    wl = np.arange(T)[None, :] < np.minimum(wide_pairs, T)[:, None]
    empties = wide_rows[:, :, 5][wl]
    out = {"what": "sgo_connect_dev (k_connect_pairs + k_connect_read + k_connect_groups; rules 1, cut_libs 1, max_region 8, max_nodes 1024, "
                   "max_pairs 64, every near pair enumerated) beside sgo_records_replay and sgo_race_dev (its Python defaults) on one 19x19 chunk, "
                   "the same at max_region 12 and 16, and one query that spends its whole node budget (the peep at cut_libs 2, nine empty "
                   "points) at 19x19 and 9x9 with one half of the wave reading and with both, one MI355X; HIP events around every call, arms "
                   "interleaved",
           "board": S, "games": len(n_entries), "rows": n, "defaults": figures(outs[8]), "max_region_12": figures(outs[12]),
           "max_region_16": figures(outs[16]),
           "near_pairs_with_region_up_to_32": {"listed": int(wl.sum()), "true": int(wide_pairs.sum()),
                                               "region_empty_histogram": np.bincount(empties, minlength=33).tolist()},
           "race_pairs_true": int(r_pairs.cpu().numpy().sum()),
           "resources_gfx950": {k: resources("sgo_connect.hip", k) for k in ("k_connect_pairs", "k_connect_read", "k_connect_groups")},
           "arms": {}, "one_query": {}}
    for k, v in ms.items():
        out["arms"][k] = stats(v)
    med = out["arms"]["connect"]["median_us"]
    out["connect_us_per_listed_pair"] = med / max(1, out["defaults"]["pairs_listed"])
    out["connect_nodes_per_us_whole_chip"] = out["defaults"]["nodes"] / med
    out["connect_over_race"] = med / out["arms"]["race"]["median_us"]
    out["connect_over_replay"] = med / out["arms"]["replay"]["median_us"]
    for (size, halves, budget), o in single_out.items():
        rows = o[1].cpu().numpy()[0]
        t = out["arms"]["peep_S%d_halves%d_nodes%d" % (size, halves, budget)]["median_us"]
        longest = int(rows[:, 10:12].sum(axis=1).max())          # the two halves run side by side: the launch lasts as long as the longer
        out["one_query"]["S%d_halves%d_nodes%d" % (size, halves, budget)] = {"n_pairs": int(o[0].cpu().numpy()[0]), "rows": rows.tolist(),
                                                                           "nodes_of_the_longer_half": longest, "median_us": t,
                                                                           "us_per_node": t / max(1, longest)}
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
