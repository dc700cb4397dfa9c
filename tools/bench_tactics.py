"""The chains-and-ladders kernels beside their neighbours in the records pipeline, on one 19x19 chunk: the five records of
tests/golden/sgf_S19.npz repeated --copies times, replayed by sgo_records_replay, then read by sgo_tactics_dev -- k_tactics_chains
and k_tactics_read apart (sgo_tactics_stage) and together -- and keyed by sgo_keys_dev on the same rows.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, rows/s, and the share of k_tactics_read's work items (rows x max_chains half-wavefronts) that
idle because the row lists fewer chains.

    python tools/bench_tactics.py [--reps 20] [--copies 8] [--max-chains 128] [--out profiles/tactics_ab.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_chunk import S, load_games, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--max-chains", type=int, default=128)
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
    n, mc = R, a.max_chains                                    # rows: every record of the chunk
    index = torch.arange(n, dtype=torch.int32, device=dev)
    libs = torch.zeros((n, S * S), dtype=torch.uint8, device=dev)
    n_chains = torch.zeros(n, dtype=torch.int32, device=dev)
    chains = torch.zeros((n, mc, 8), dtype=torch.int32, device=dev)
    key0, canon = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    P = L.ptr

    def tactics(stage):
        lib.sgo_tactics_stage(stage)
        L.check(lib.sgo_tactics_dev(S, n, be.rec_ptr, be.cap, P(index), mc, P(libs), P(n_chains), P(chains), L.stream_ptr()),
                "sgo_tactics_dev")

    def keys():
        L.check(lib.sgo_keys_dev(S, n, be.rec_ptr, be.cap, P(index), None, P(key0), P(canon), P(mask), None, L.stream_ptr()), "sgo_keys_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    # k_tactics_read alone runs on the table the chains arm in front of it has just written
    arms = {"replay": replay, "keys": keys, "tactics_chains": lambda: tactics(1), "tactics_read": lambda: tactics(2),
            "tactics_both": lambda: tactics(0)}
    try:
        for fn in arms.values():                               # warm-up: code objects, the pinned staging block
            fn()
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                ms[k].append(timed(fn))
    finally:
        lib.sgo_tactics_stage(0)
    nc = n_chains.cpu().numpy().astype(np.int64)
    rows = chains.cpu().numpy()
    stored = np.minimum(nc, mc)
    # node and unknown figures from a subsample of the rows (every copies-th), enough for two digits
    listed = np.concatenate([rows[i, :stored[i]] for i in range(0, n, max(1, a.copies))]) if n else np.zeros((0, 8), np.int32)
    out = {"what": "sgo_tactics_dev (k_tactics_chains, k_tactics_read) beside sgo_records_replay and sgo_keys_dev on one 19x19 chunk, "
                   "one MI355X; HIP events around every call, arms interleaved",
           "board": S, "games": len(n_entries), "rows": n, "max_chains": mc,
           "listed_chains_per_row_mean": float(nc.mean()), "listed_chains_per_row_max": int(nc.max()),
           "read_work_items": int(n) * mc, "read_work_items_idle_share": 1.0 - float(stored.sum()) / (float(n) * mc),
           "read_waves_with_work_share": float(np.ceil(stored / 2.0).sum()) / (float(n) * ((mc + 1) // 2)),
           "nodes_per_listed_chain_mean": float(listed[:, 7].mean()) if len(listed) else 0.0,
           "unknown_rows_share": float(((listed[:, 4] & 12) != 0).mean()) if len(listed) else 0.0, "arms": {}}
    for k, v in ms.items():
        st = stats(v)
        st["rows_per_s"] = n / (st["median_us"] * 1e-6)
        out["arms"][k] = st
    out["tactics_over_replay"] = out["arms"]["tactics_both"]["median_us"] / out["arms"]["replay"]["median_us"]
    out["tactics_over_keys"] = out["arms"]["tactics_both"]["median_us"] / out["arms"]["keys"]["median_us"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
