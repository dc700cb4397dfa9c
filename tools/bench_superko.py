"""The superko kernels beside their neighbours in the records pipeline, on one 19x19 chunk: the five records of
tests/golden/sgf_S19.npz repeated --copies times, replayed by sgo_records_replay, then read by sgo_superko_dev under both rules
(every record with its game as history), by sgo_moves_dev (side 0) and by sgo_keys_dev on the same rows; one sgo_superko_dev call
with n = 1 on a game's last record, what a single GTP query costs; and one row with a history of SGO_SUPERKO_MAX_HISTORY(19)
constructed records, alone.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, rows/s, per rule the positions with a non-empty `extra` and the largest `back`, the history
length per row, and the compiler's resource figures of the two kernels per board size.

    python tools/bench_superko.py [--reps 20] [--copies 8] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_chunk import S, load_games, resources, stats, timed  # noqa: E402


def long_history(np, H):
    """records uint32 [H, 16 * NW]: two stones that walk over the board, a different pair in every record; the last record is the
    current one.  Nothing repeats, so every lookup walks the whole history."""
    N, NW = S * S, (S * S + 31) // 32
    recs = np.zeros((H, 16, NW), np.uint32)
    for j in range(H):
        a, b = (5 * j) % N, (5 * j + 2 + 3 * (j // N)) % N
        recs[j, 0, a >> 5] |= np.uint32(1 << (a & 31))
        recs[j, 1, b >> 5] |= np.uint32(1 << (b & 31))
        if j % 2:
            recs[j, 0, NW - 1] |= np.uint32(0x80000000)
    return recs.reshape(H, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--copies", type=int, default=8)
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
    n = R                                                      # rows: every record of the chunk, with its game as history
    base = (off + np.arange(len(n_entries))).astype(np.int32)
    first_h = np.repeat(base, n_entries + 1).astype(np.int32)
    index = torch.arange(n, dtype=torch.int32, device=dev)
    first = torch.from_numpy(first_h).to(dev)
    last = int(base[0] + n_entries[0])
    one, one_first = torch.tensor([last], dtype=torch.int32, device=dev), torch.tensor([int(base[0])], dtype=torch.int32, device=dev)
    NW = be.NW
    keys = torch.zeros(be.cap, dtype=torch.int64, device=dev)
    sets = torch.zeros((n, 3, NW), dtype=torch.int32, device=dev)
    back = torch.zeros((n, S * S), dtype=torch.int16, device=dev)
    counts = torch.zeros((2, n, 8), dtype=torch.int32, device=dev)
    sets1, back1 = torch.zeros((1, 3, NW), dtype=torch.int32, device=dev), torch.zeros((1, S * S), dtype=torch.int16, device=dev)
    counts1 = torch.zeros((1, 8), dtype=torch.int32, device=dev)
    rows = torch.zeros((n, S * S, 8), dtype=torch.int16, device=dev)
    mcounts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    key0, canon = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    H = 4 * S * S + 1
    long_recs = torch.from_numpy(long_history(np, H).view(np.int32)).to(dev)
    long_keys = torch.zeros(H, dtype=torch.int64, device=dev)
    long_idx, long_first = torch.tensor([H - 1], dtype=torch.int32, device=dev), torch.tensor([0], dtype=torch.int32, device=dev)
    P = L.ptr

    def superko(rule):
        def call():
            L.check(lib.sgo_superko_dev(S, n, be.rec_ptr, R, P(index), P(first), rule, P(keys), P(sets), P(back), P(counts[rule]),
                                        L.stream_ptr()), "sgo_superko_dev")
        return call

    def superko_one():
        L.check(lib.sgo_superko_dev(S, 1, be.rec_ptr, last + 1, P(one), P(one_first), 0, P(keys), P(sets1), P(back1), P(counts1),
                                    L.stream_ptr()), "sgo_superko_dev")

    def superko_long():
        L.check(lib.sgo_superko_dev(S, 1, P(long_recs), H, P(long_idx), P(long_first), 0, P(long_keys), P(sets1), P(back1), P(counts1),
                                    L.stream_ptr()), "sgo_superko_dev")

    def moves():
        L.check(lib.sgo_moves_dev(S, n, be.rec_ptr, be.cap, P(index), 0, P(rows), P(mcounts), L.stream_ptr()), "sgo_moves_dev")

    def keys_arm():
        L.check(lib.sgo_keys_dev(S, n, be.rec_ptr, be.cap, P(index), None, P(key0), P(canon), P(mask), None, L.stream_ptr()), "sgo_keys_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    arms = {"replay": replay, "keys": keys_arm, "moves": moves, "superko_positional": superko(0), "superko_situational": superko(1),
            "superko_n1_last_record": superko_one, "superko_n1_full_history": superko_long}
    for fn in arms.values():                                   # warm-up: code objects, the pinned staging block
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    superko_long()
    torch.cuda.synchronize()
    long_counts = counts1.cpu().numpy()[0].tolist()
    assert long_counts[5] == H and long_counts[0] == 0 and long_counts[6] == 0
    got = counts.cpu().numpy()
    assert (got[:, :, 5] == np.concatenate([np.arange(k + 1) + 1 for k in n_entries])).all() and not got[:, :, 6].any() and not got[:, :, 7].any()
    assert (got[:, :, 1] <= mcounts.cpu().numpy()[:, 0]).all()   # extra lies inside the legal set sgo_moves_dev counts
    out = {"what": "sgo_superko_dev (k_superko_keys + k_superko) under both rules beside sgo_records_replay, sgo_keys_dev and sgo_moves_dev on "
                   "one 19x19 chunk, every record with its game as history; one call with n = 1 on the last record of the first game; "
                   "one call with n = 1 on a constructed history of SGO_SUPERKO_MAX_HISTORY(19) records in which nothing repeats; one "
                   "MI355X; HIP events around every call, arms interleaved",
           "board": S, "games": len(n_entries), "rows": n, "history_mean": float(got[0][:, 5].mean()), "history_max": int(got[0][:, 5].max()),
           "n1_last_record": {"record": last, "history": int(n_entries[0]) + 1}, "n1_full_history": {"history": H, "counts": long_counts},
           "rules": {}, "resources_gfx950": {"k_superko": resources("sgo_superko.hip", "k_superko"),
                                             "k_superko_keys": resources("sgo_superko.hip", "k_superko_keys")}, "arms": {}}
    for rule, name in ((0, "positional"), (1, "situational")):
        c = got[rule]
        out["rules"][name] = {"positions_with_extra": int((c[:, 1] > 0).sum()), "positions_with_repeat": int((c[:, 0] > 0).sum()),
                              "repeat_points": int(c[:, 0].sum()), "extra_points": int(c[:, 1].sum()), "max_back_over_extra": int(c[:, 2].max()),
                              "positions_seen_before": int((c[:, 4] > 0).sum())}
    for k, v in ms.items():
        st = stats(v)
        st["rows_per_s"] = (1 if "_n1_" in k else n) / (st["median_us"] * 1e-6)
        out["arms"][k] = st
    for k in ("moves", "keys", "replay"):
        out["superko_positional_over_" + k] = out["arms"]["superko_positional"]["median_us"] / out["arms"][k]["median_us"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
