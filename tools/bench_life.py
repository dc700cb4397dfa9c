"""The unconditional-life kernel beside its neighbours in the records pipeline, on one 19x19 chunk: the five records of
tests/golden/sgf_S19.npz repeated --copies times, replayed by sgo_records_replay, then read by sgo_life_dev, by k_tactics_chains
(sgo_tactics_dev at stage 1) and keyed by sgo_keys_dev on the same rows.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, rows/s, the removal passes per row and the share of rows with an alive stone (from the model,
tests/life_model.py, on the first copy of the games), and the compiler's resource figures of k_life<S> per board size.

    python tools/bench_life.py [--reps 20] [--copies 8] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from sejonggo_amd import _lib as L
    from sejonggo_amd.records import DeviceRecords
    from tests import life_model
    lib = L.require_gpu()
    n_entries, off, acts, cols, first = load_games(a.copies)
    total = int(n_entries.sum())
    R = total + len(n_entries)
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    n, mc = R, 128                                             # rows: every record of the chunk
    index = torch.arange(n, dtype=torch.int32, device=dev)
    sets = torch.zeros((n, 4, be.NW), dtype=torch.int32, device=dev)
    counts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    libs = torch.zeros((n, S * S), dtype=torch.uint8, device=dev)
    n_chains = torch.zeros(n, dtype=torch.int32, device=dev)
    chains = torch.zeros((n, mc, 8), dtype=torch.int32, device=dev)
    key0, canon = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    P = L.ptr

    def life():
        L.check(lib.sgo_life_dev(S, n, be.rec_ptr, be.cap, P(index), P(sets), P(counts), L.stream_ptr()), "sgo_life_dev")

    def tactics_chains():
        L.check(lib.sgo_tactics_dev(S, n, be.rec_ptr, be.cap, P(index), mc, P(libs), P(n_chains), P(chains), L.stream_ptr()),
                "sgo_tactics_dev")

    def keys():
        L.check(lib.sgo_keys_dev(S, n, be.rec_ptr, be.cap, P(index), None, P(key0), P(canon), P(mask), None, L.stream_ptr()), "sgo_keys_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    arms = {"replay": replay, "keys": keys, "tactics_chains": tactics_chains, "life": life}
    lib.sgo_tactics_stage(1)                                   # k_tactics_chains only
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
    got = counts.cpu().numpy()
    recs = be.records[:first].cpu().numpy().view(np.uint32)
    model = life_model.life(S, recs)
    assert np.array_equal(model["counts"], got[:first]) and np.array_equal(model["sets"], sets[:first].cpu().numpy().view(np.uint32))
    rounds = model["rounds"].max(axis=1)                       # the wavefront runs as long as its longer half
    out = {"what": "sgo_life_dev (k_life) beside sgo_records_replay, sgo_keys_dev and k_tactics_chains on one 19x19 chunk, one MI355X; "
                   "HIP events around every call, arms interleaved; the device rows of the first copy equal the model's",
           "board": S, "games": len(n_entries), "rows": n,
           "rounds_per_row_mean": float(rounds.mean()), "rounds_per_row_max": int(rounds.max()),
           "rows_with_alive_share": float((model["counts"][:, :2].sum(axis=1) > 0).mean()),
           "rows_settled_share": float((model["counts"][:, 6] == 0).mean()),
           "resources_gfx950": {"k_life": resources("sgo_life.hip", "k_life")}, "arms": {}}
    for k, v in ms.items():
        st = stats(v)
        st["rows_per_s"] = n / (st["median_us"] * 1e-6)
        out["arms"][k] = st
    out["life_over_tactics_chains"] = out["arms"]["life"]["median_us"] / out["arms"]["tactics_chains"]["median_us"]
    out["life_over_replay"] = out["arms"]["life"]["median_us"] / out["arms"]["replay"]["median_us"]
    out["life_over_keys"] = out["arms"]["life"]["median_us"] / out["arms"]["keys"]["median_us"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
