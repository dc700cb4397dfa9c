"""The move-outcome kernel beside its neighbours in the records pipeline, on one 19x19 chunk: the five records of
tests/golden/sgf_S19.npz repeated --copies times, replayed by sgo_records_replay, then read by sgo_moves_dev (side 0), by
k_tactics_chains (sgo_tactics_dev at stage 1) and by sgo_life_dev on the same rows; and one sgo_moves_dev call with n = 1 on a
middle-game position, what a single GTP query costs.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, rows/s, the contact points per row (the trips of the kernel's candidate loop: empty points next
to a stone, counted on the host from the replayed records) and the trips per wavefront (the larger of its two rows'), and the
compiler's resource figures of k_moves<S> per board size.  The device's `allowed` counts are checked against the legal bitsets the
replay wrote for the same records.

    python tools/bench_moves.py [--reps 20] [--copies 8] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_chunk import S, load_games, resources, stats, timed  # noqa: E402


def contact_points(records, np):
    """int [R]: the empty points next to a stone of packed 19x19 records uint32 [R, 16 * NW]"""
    N, NW = S * S, (S * S + 31) // 32
    w = np.ascontiguousarray(records[:, :2 * NW]).astype("<u4")
    bits = np.unpackbits(w.view(np.uint8).reshape(len(w), 2, 4 * NW), axis=-1, bitorder="little")[:, :, :N]
    stone = (bits[:, 0] | bits[:, 1]).reshape(-1, S, S).astype(bool)
    near = np.zeros_like(stone)
    near[:, 1:] |= stone[:, :-1]
    near[:, :-1] |= stone[:, 1:]
    near[:, :, 1:] |= stone[:, :, :-1]
    near[:, :, :-1] |= stone[:, :, 1:]
    return (near & ~stone).sum(axis=(1, 2))


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
    middle = int(n_entries[0]) // 2                            # a record of the first game, half way through
    total = int(n_entries.sum())
    R = total + len(n_entries)
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    n, mc = R, 128                                             # rows: every record of the chunk
    index = torch.arange(n, dtype=torch.int32, device=dev)
    one = torch.tensor([middle], dtype=torch.int32, device=dev)
    rows = torch.zeros((n, S * S, 8), dtype=torch.int16, device=dev)
    counts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    rows1 = torch.zeros((1, S * S, 8), dtype=torch.int16, device=dev)
    counts1 = torch.zeros((1, 8), dtype=torch.int32, device=dev)
    sets = torch.zeros((n, 4, be.NW), dtype=torch.int32, device=dev)
    lcounts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    libs = torch.zeros((n, S * S), dtype=torch.uint8, device=dev)
    n_chains = torch.zeros(n, dtype=torch.int32, device=dev)
    chains = torch.zeros((n, mc, 8), dtype=torch.int32, device=dev)
    P = L.ptr

    def moves():
        L.check(lib.sgo_moves_dev(S, n, be.rec_ptr, be.cap, P(index), 0, P(rows), P(counts), L.stream_ptr()), "sgo_moves_dev")

    def moves_one():
        L.check(lib.sgo_moves_dev(S, 1, be.rec_ptr, be.cap, P(one), 0, P(rows1), P(counts1), L.stream_ptr()), "sgo_moves_dev")

    def life():
        L.check(lib.sgo_life_dev(S, n, be.rec_ptr, be.cap, P(index), P(sets), P(lcounts), L.stream_ptr()), "sgo_life_dev")

    def tactics_chains():
        L.check(lib.sgo_tactics_dev(S, n, be.rec_ptr, be.cap, P(index), mc, P(libs), P(n_chains), P(chains), L.stream_ptr()),
                "sgo_tactics_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    arms = {"replay": replay, "tactics_chains": tactics_chains, "life": life, "moves": moves, "moves_n1": moves_one}
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
    recs = be.records[:n].cpu().numpy().view(np.uint32)
    legal = be.legal[:n].cpu().numpy().view(np.uint32).astype("<u4")
    lbits = np.unpackbits(legal.view(np.uint8), axis=-1, bitorder="little")[:, :S * S]
    assert np.array_equal(got[:, 0], lbits.sum(axis=1)), "allowed != the legal set the replay wrote"
    assert np.array_equal(rows[:, :, 0].cpu().numpy() & 1, lbits) and np.array_equal(counts1.cpu().numpy()[0], got[middle])
    contact = contact_points(recs, np)
    pairs = np.concatenate([contact, [0]])[:2 * ((n + 1) // 2)].reshape(-1, 2).max(axis=1)
    out = {"what": "sgo_moves_dev (k_moves, side 0) beside sgo_records_replay, k_tactics_chains and sgo_life_dev on one 19x19 chunk, and "
                   "one call with n = 1 on a middle-game position; one MI355X; HIP events around every call, arms interleaved; the "
                   "device's ALLOWED bits equal the legal sets the replay wrote for the same records",
           "board": S, "games": len(n_entries), "rows": n,
           "contact_points_per_row_mean": float(contact.mean()), "contact_points_per_row_max": int(contact.max()),
           "loop_trips_per_wave_mean": float(pairs.mean()), "loop_trips_per_wave_max": int(pairs.max()),
           "n1_position": {"record": int(middle), "contact_points": int(contact[middle]), "allowed": int(got[middle, 0])},
           "forbidden_sound_points": int(got[:, 7].sum()), "rows_with_forbidden_sound": int((got[:, 7] > 0).sum()),
           "resources_gfx950": {"k_moves": resources("sgo_moves.hip", "k_moves")}, "arms": {}}
    for k, v in ms.items():
        st = stats(v)
        st["rows_per_s"] = (1 if k == "moves_n1" else n) / (st["median_us"] * 1e-6)
        out["arms"][k] = st
    out["moves_over_tactics_chains"] = out["arms"]["moves"]["median_us"] / out["arms"]["tactics_chains"]["median_us"]
    out["moves_over_life"] = out["arms"]["moves"]["median_us"] / out["arms"]["life"]["median_us"]
    out["moves_over_replay"] = out["arms"]["moves"]["median_us"] / out["arms"]["replay"]["median_us"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
