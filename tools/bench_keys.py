"""The position-key kernel beside its neighbours in the records pipeline, on one 19x19 chunk of about 2^18 records: the five
records of tests/golden/sgf_S19.npz repeated until the chunk is full, replayed by sgo_records_replay, then keyed by sgo_keys_dev in
both forms (z from the LDS table; z computed inline) and scored by sgo_records_score_dev on a uniform policy.

Every launch is bracketed by HIP events on the stream it runs on, the arms interleaved launch by launch after a warm-up; the
replay call (list packing, one copy, one launch, one wait) is also timed by the host clock, which is what a caller sees.  The report
has the median and the spread per arm, records/s, and for the key kernel the bytes it needs per record (two planes of 48 B, the
index and target words, the four outputs) over its time.

    python tools/bench_keys.py [--reps 30] [--out profiles/keys_ab.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_chunk import S, load_games, stats, timed  # noqa: E402
CHUNK = 1 << 18
BYTES_PER_RECORD = 2 * 48 + 4 + 4 + 8 + 8 + 4 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from sejonggo_amd import _lib as L
    from sejonggo_amd.records import DeviceRecords
    lib = L.require_gpu()
    copies = CHUNK // load_games(1)[4]
    n_entries, off, acts, cols, _ = load_games(copies)
    total = int(n_entries.sum())
    R = total + len(n_entries)
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    # rows: every entry, the record before it and the recorded move
    index = torch.from_numpy((np.arange(total) + np.repeat(np.arange(len(n_entries)), n_entries)).astype(np.int32)).to(dev)
    target = torch.from_numpy(acts).to(dev)
    n = total
    key0, canon = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    mask, action = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    A = S * S + 1
    policy = torch.full((n, A), 1.0 / A, dtype=torch.float32, device=dev)
    value = torch.zeros(n, dtype=torch.float32, device=dev)
    zs, bucket = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    rank, best = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    pt, flags = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    counters = torch.zeros((1, 8), dtype=torch.int64, device=dev)
    P = L.ptr

    def keys(mode):
        lib.sgo_keys_mode(mode)
        L.check(lib.sgo_keys_dev(S, n, be.rec_ptr, be.cap, P(index), P(target), P(key0), P(canon), P(mask), P(action), L.stream_ptr()),
                "sgo_keys_dev")

    def score():
        be.score(n, index, target, zs, bucket, 1, policy, value, 0, rank, best, pt, flags, counters)

    replay_wall = []

    def replay():
        t0 = time.perf_counter()
        status, _ = be.replay(n_entries, off, acts, cols)
        replay_wall.append(1e3 * (time.perf_counter() - t0))
        assert not status.any()

    arms = {"replay": replay, "keys_lds_table": lambda: keys(0), "keys_inline_sm": lambda: keys(1), "score": score}
    for fn in arms.values():                                   # warm-up: code objects, the pinned staging block
        fn()
        fn()
    torch.cuda.synchronize()
    keys(0)
    ref = (key0.clone(), canon.clone(), mask.clone(), action.clone())
    keys(1)
    same = all(bool(torch.equal(x, y)) for x, y in zip(ref, (key0, canon, mask, action)))
    del replay_wall[:]
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    lib.sgo_keys_mode(0)
    out = {"what": "sgo_keys_dev (k_keys) beside sgo_records_replay and sgo_records_score_dev on one 19x19 chunk, one MI355X; HIP events "
                   "around every call, arms interleaved",
           "board": S, "games": len(n_entries), "records": R, "rows": n, "bytes_needed_per_record": BYTES_PER_RECORD,
           "forms_bit_identical": same, "arms": {}}
    for k, v in ms.items():
        st = stats(v)
        st["rows_per_s"] = n / (st["median_us"] * 1e-6)
        if k.startswith("keys"):
            st["needed_bytes_per_s"] = BYTES_PER_RECORD * st["rows_per_s"]
        out["arms"][k] = st
    out["arms"]["replay"]["host_clock"] = stats(replay_wall)
    out["arms"]["replay"]["records_per_s"] = R / (out["arms"]["replay"]["median_us"] * 1e-6)
    out["keys_over_replay"] = out["arms"]["keys_lds_table"]["median_us"] / out["arms"]["replay"]["median_us"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
