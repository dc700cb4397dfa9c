"""The securing-move kernels beside their neighbours in the records pipeline, on one 19x19 chunk: the five records of
tests/golden/sgf_S19.npz repeated --copies times, replayed by sgo_records_replay, then read by sgo_secure_dev (side 0), by
sgo_life_dev and by sgo_moves_dev on the same rows; the two choices of k_secure's launch shape (sgo_secure_mode: the workgroups
per row, and the dealing by EMPTY-point rank or by point index); and one sgo_secure_dev call with n = 1 on a middle-game position
(the GTP case) under the same shapes.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, rows/s, the mean number of candidates (empty points) per row, the share of half-waves that idle
under either dealing, the summary of the rows (how many offer a securing move beside how many have anything proved), and the
compiler's resource figures of k_secure<S> and k_secure_sum<S> per board size.  The base counts of every row are checked against
sgo_life_dev's on the same rows, and every launch shape against the default's words.

    python tools/bench_secure.py [--reps 10] [--copies 8] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_chunk import S, load_games, resources, stats, timed  # noqa: E402

BY_POINT = 1 << 16
SHAPES = {"ch1": 1, "ch2": 2, "ch4": 4, "ch8": 8, "ch16": 16, "ch32": 32, "ch64": 64, "ch181": 181, "ch8_by_point": BY_POINT | 8,
          "ch181_by_point": BY_POINT | 181}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from sejonggo_amd import _lib as L
    from sejonggo_amd.records import DeviceRecords
    lib = L.require_gpu()
    n_entries, off, acts, cols, first = load_games(a.copies)
    total = int(n_entries.sum())
    R = total + len(n_entries)
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    n, N = R, S * S                                            # rows: every record of the chunk
    index = torch.arange(n, dtype=torch.int32, device=dev)
    table = torch.zeros((n, N, 4), dtype=torch.int16, device=dev)
    sets = torch.zeros((n, 4, be.NW), dtype=torch.int32, device=dev)
    counts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    lsets = torch.zeros((n, 4, be.NW), dtype=torch.int32, device=dev)
    lcounts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    mrows = torch.zeros((n, N, 8), dtype=torch.int16, device=dev)
    mcounts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    mid = int(np.cumsum(n_entries + 1)[0] // 2)                # the middle of the first game
    one = torch.tensor([mid], dtype=torch.int32, device=dev)
    table1 = torch.zeros((1, N, 4), dtype=torch.int16, device=dev)
    sets1 = torch.zeros((1, 4, be.NW), dtype=torch.int32, device=dev)
    counts1 = torch.zeros((1, 8), dtype=torch.int32, device=dev)
    P = L.ptr

    def secure():
        L.check(lib.sgo_secure_dev(S, n, be.rec_ptr, be.cap, P(index), 0, P(table), P(sets), P(counts), L.stream_ptr()), "sgo_secure_dev")

    def secure_one():
        L.check(lib.sgo_secure_dev(S, 1, be.rec_ptr, be.cap, P(one), 0, P(table1), P(sets1), P(counts1), L.stream_ptr()), "sgo_secure_dev")

    def life():
        L.check(lib.sgo_life_dev(S, n, be.rec_ptr, be.cap, P(index), P(lsets), P(lcounts), L.stream_ptr()), "sgo_life_dev")

    def moves():
        L.check(lib.sgo_moves_dev(S, n, be.rec_ptr, be.cap, P(index), 0, P(mrows), P(mcounts), L.stream_ptr()), "sgo_moves_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    def shaped(fn, mode):
        def run():
            lib.sgo_secure_mode(mode)
            try:
                fn()
            finally:
                lib.sgo_secure_mode(0)
        return run

    arms = {"replay": replay, "life": life, "moves": moves, "secure": secure, "secure_one": secure_one}
    for name, mode in SHAPES.items():
        arms["secure_" + name] = shaped(secure, mode)
        arms["secure_one_" + name] = shaped(secure_one, mode)
    replay()
    secure()
    secure_one()
    torch.cuda.synchronize()
    ref = [t.clone() for t in (table, sets, counts, table1, sets1, counts1)]
    for fn in arms.values():                                   # warm-up: code objects, the pinned staging block; and the same words
        fn()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(ref, (table, sets, counts, table1, sets1, counts1)))
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    # the base counts are sgo_life_dev's for the mover (side 0: the record's side to move)
    recs = be.records[:n].cpu().numpy().view(np.uint32)
    white = (recs[:, be.NW - 1] >> 31).astype(bool)
    c, lc = counts.cpu().numpy(), lcounts.cpu().numpy()
    for k in range(3):
        assert np.array_equal(c[:, k], np.where(white, lc[:, 2 * k + 1], lc[:, 2 * k])), k
    planes = recs[:, :2 * be.NW].copy()
    planes[:, be.NW - 1] &= np.uint32(0x7fffffff)
    stones = np.unpackbits(planes.view(np.uint8), axis=1, bitorder="little").reshape(n, 2, -1)[:, :, :N].sum(axis=(1, 2))
    empty = N - stones
    pairs_rank, pairs_point = (empty + 1) // 2, (N + 1) // 2
    base = c[:, 0] + c[:, 1]
    out = {"what": "sgo_secure_dev (k_secure + k_secure_sum, side 0) beside sgo_records_replay, sgo_life_dev and sgo_moves_dev on one 19x19 "
                   "chunk, and one call with n = 1 on a middle-game position, under the launch shapes of sgo_secure_mode (chK: K workgroups "
                   "per row; by_point: point 2k + h instead of the (2k + h)-th empty point), one MI355X; HIP events around every call, arms "
                   "interleaved; every shape writes the default's words, and the base counts equal sgo_life_dev's",
           "board": S, "games": len(n_entries), "rows": n, "one_row_record": mid, "one_row_empty_points": int(empty[mid]),
           "candidates_per_row_mean": float(empty.mean()), "candidates_total": int(empty.sum()),
           "idle_half_share_by_rank": float((empty % 2).sum() / (2.0 * pairs_rank.sum())),
           "idle_half_share_by_point": float((2 * pairs_point * n - empty.sum()) / (2.0 * pairs_point * n)),
           "rows_with_base_share": float((base > 0).mean()), "rows_with_securing_share": float((c[:, 4] > 0).mean()),
           "rows_with_best_gain_2_share": float((c[:, 5] >= 2).mean()), "rows_with_harmful_share": float((c[:, 7] > 0).mean()),
           "rows_securing_without_base_share": float(((c[:, 5] >= 2) & (base == 0)).mean()), "best_gain_max": int(c[:, 5].max()),
           "resources_gfx950": {"k_secure": resources("sgo_secure.hip", "k_secure"), "k_secure_sum": resources("sgo_secure.hip", "k_secure_sum")},
           "arms": {}}
    for k, v in ms.items():
        st = stats(v)
        rows = 1 if k.startswith("secure_one") else n
        st["rows_per_s"] = rows / (st["median_us"] * 1e-6)
        out["arms"][k] = st
    out["secure_us_per_candidate"] = out["arms"]["secure"]["median_us"] / float(empty.sum())
    out["secure_over_life"] = out["arms"]["secure"]["median_us"] / out["arms"]["life"]["median_us"]
    out["secure_over_moves"] = out["arms"]["secure"]["median_us"] / out["arms"]["moves"]["median_us"]
    out["secure_over_replay"] = out["arms"]["secure"]["median_us"] / out["arms"]["replay"]["median_us"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
