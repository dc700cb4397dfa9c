"""The influence kernel beside its neighbours in the records pipeline, on one 19x19 chunk: the five records of
tests/golden/sgf_S19.npz repeated --copies times (8: 13 176 records), replayed by sgo_records_replay, then read by sgo_influence_dev
at the territory triple (5, 10, 21) and at the area triple (4, 0, 0), by sgo_life_dev and keyed by sgo_keys_dev on the same rows in
the same process; and one sgo_influence_dev call with n = 1.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median with the 10th and 90th percentile per arm, rows/s, the compiler's resource figures of k_influence<S> per board size, and
a description of the heuristic on the chunk: per bucket of 20 plies the share of positions whose margin has the sign of the margin
of the game's last position (no komi: the records carry none; nothing is lifted).  Every eighth row of the first copy is compared
with the model (tests/influence_model.py).

    python tools/bench_influence.py [--reps 20] [--copies 8] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_chunk import S, load_games, resources, stats, timed  # noqa: E402
TERRITORY, AREA = (5, 10, 21), (4, 0, 0)


def sign_agreement(margins, lengths, width=20):
    """[{"first_ply", "positions", "share"}]: per bucket of `width` plies the share of positions whose margin has the sign of the
    margin of the game's last position; margins = the rows of the games one after the other, lengths = entries per game"""
    import numpy as np
    hit, seen, base = {}, {}, 0
    for n in lengths:
        rows = np.sign(margins[base:base + n + 1])
        for k in range(n + 1):
            b = k // width
            seen[b] = seen.get(b, 0) + 1
            hit[b] = hit.get(b, 0) + int(rows[k] == rows[-1])
        base += n + 1
    return [{"first_ply": b * width, "positions": seen[b], "share": hit[b] / float(seen[b])} for b in sorted(seen)]


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
    from tests import influence_model
    lib = L.require_gpu()
    n_entries, off, acts, cols, first = load_games(a.copies)
    lengths = n_entries[:5].tolist()                           # the games of the first copy
    total = int(n_entries.sum())
    R = total + len(n_entries)
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    n = R                                                      # rows: every record of the chunk
    index = torch.arange(n, dtype=torch.int32, device=dev)
    values = torch.zeros((n, S * S), dtype=torch.int16, device=dev)
    sets = torch.zeros((n, 4, be.NW), dtype=torch.int32, device=dev)
    counts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    lsets, lcounts = torch.zeros_like(sets), torch.zeros_like(counts)
    key0, canon = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    P = L.ptr

    def influence(triple, rows=n):
        def call():
            L.check(lib.sgo_influence_dev(S, rows, be.rec_ptr, be.cap, P(index), None, triple[0], triple[1], triple[2], P(values), P(sets),
                                          P(counts), L.stream_ptr()), "sgo_influence_dev")
        return call

    def life():
        L.check(lib.sgo_life_dev(S, n, be.rec_ptr, be.cap, P(index), P(lsets), P(lcounts), L.stream_ptr()), "sgo_life_dev")

    def keys():
        L.check(lib.sgo_keys_dev(S, n, be.rec_ptr, be.cap, P(index), None, P(key0), P(canon), P(mask), None, L.stream_ptr()), "sgo_keys_dev")

    def replay():
        status, _ = be.replay(n_entries, off, acts, cols)
        assert not status.any()

    arms = {"replay": replay, "keys": keys, "life": life, "influence_area": influence(AREA), "influence_one_row": influence(TERRITORY, 1),
            "influence_territory": influence(TERRITORY)}         # the territory triple last: its outputs are the ones read below
    for fn in arms.values():                                   # warm-up: code objects, the pinned staging block
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    got = counts.cpu().numpy()
    pick = np.arange(0, first, 8)
    recs = be.records[:first].cpu().numpy().view(np.uint32)
    model = influence_model.influence(S, recs[pick], None, None, *TERRITORY)
    assert np.array_equal(model["counts"], got[pick]) and np.array_equal(model["values"], values[:first].cpu().numpy()[pick])
    assert np.array_equal(model["sets"], sets[:first].cpu().numpy().view(np.uint32)[pick])
    c = got[:first].astype(np.int64)
    out = {"what": "sgo_influence_dev (k_influence) at (5, 10, 21) and (4, 0, 0) beside sgo_records_replay, sgo_keys_dev and sgo_life_dev "
                   "(k_life) on one 19x19 chunk, one MI355X; HIP events around every call, arms interleaved; every eighth device row of "
                   "the first copy equals the model's",
           "board": S, "games": len(n_entries), "rows": n,
           "sign_of_final_margin_share": sign_agreement(c[:, 7], lengths),
           "neutral_mean": float(c[:, 6].mean()), "abs_margin_mean": float(np.abs(c[:, 7]).mean()),
           "resources_gfx950": {"k_influence": resources("sgo_influence.hip", "k_influence")}, "arms": {}}
    for k, v in ms.items():
        st = stats(v)
        st["rows_per_s"] = (1 if k == "influence_one_row" else n) / (st["median_us"] * 1e-6)
        out["arms"][k] = st
    t = out["arms"]["influence_territory"]["median_us"]
    out["territory_over_keys"] = t / out["arms"]["keys"]["median_us"]
    out["territory_over_life"] = t / out["arms"]["life"]["median_us"]
    out["territory_over_replay"] = t / out["arms"]["replay"]["median_us"]
    out["territory_over_area"] = t / out["arms"]["influence_area"]["median_us"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
