"""The shape-search kernel beside its neighbours in the records pipeline, on one 19x19 chunk: the five records of
tests/golden/sgf_S19.npz repeated --copies times, replayed by sgo_records_replay, then searched by sgo_shapes_dev for

  side_v0     a full-board-width side pattern (19 x 3 on the top edge, asymmetric, all four kinds of cell) as drawn only: its
              table cut down to the one variant v = 0;
  side_16     the same pattern with all sixteen variants;
  corner_16   a 5 x 5 corner pattern with all sixteen variants;

with sgo_keys_dev (k_keys) and sgo_life_dev (k_life) timed on the same rows in the same process as yardsticks.

Every call is bracketed by HIP events on the stream it runs on, the arms interleaved call by call after a warm-up.  The report has
the median and the spread per arm, rows/s, the share of rows each shape hits (the device rows of the first copy of the games equal
the model's, tests/shapes_model.py), and the compiler's resource figures of k_shapes<S> per board size.

    python tools/bench_shapes.py [--reps 20] [--copies 8] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_chunk import S, load_games, resources, stats, timed  # noqa: E402
SIDE = "+-------------------\n|..*..X..*....O..*..|\n|.*.X.O.......X.O.*.|\n|*.....*..........*.|"
CORNER = "+-----\n|.....\n|.....\n|...X.\n|.*...\n|....."        # a lone stone on the 3-4 point: the opening of some of the games


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
    from sejonggo_amd.shapes import Shape, compile_table
    from tests import shapes_model
    lib = L.require_gpu()
    n_entries, off, acts, cols, first = load_games(a.copies)
    total = int(n_entries.sum())
    R = total + len(n_entries)
    be = DeviceRecords(S, len(n_entries), total)
    dev = be.device
    status, _ = be.replay(n_entries, off, acts, cols)
    assert not status.any()
    n = R                                                      # rows: every record of the chunk
    index = torch.arange(n, dtype=torch.int32, device=dev)
    shapes = {"side": Shape.parse(SIDE), "corner": Shape.parse(CORNER)}
    tables = {"side_16": compile_table(S, shapes["side"]), "corner_16": compile_table(S, shapes["corner"])}
    assert int(tables["side_16"][1]) == 16 and int(tables["corner_16"][1]) == 16
    one = tables["side_16"].copy()                             # the shape as drawn only
    one[1], one[2] = 1, 1
    one[16 + 64:] = 0
    tables["side_v0"] = one
    d_tab = {k: torch.from_numpy(t.view(np.int32)).to(dev) for k, t in tables.items()}
    hits = {k: torch.zeros((n, 4), dtype=torch.int32, device=dev) for k in tables}
    cover = {k: torch.zeros((n, be.NW), dtype=torch.int32, device=dev) for k in tables}
    sets = torch.zeros((n, 4, be.NW), dtype=torch.int32, device=dev)
    counts = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    key0, canon = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    P = L.ptr

    def search(k):
        def run():
            L.check(lib.sgo_shapes_dev(S, n, be.rec_ptr, be.cap, P(index), P(d_tab[k]), P(hits[k]), P(cover[k]), L.stream_ptr()), "sgo_shapes_dev")
        return run

    def life():
        L.check(lib.sgo_life_dev(S, n, be.rec_ptr, be.cap, P(index), P(sets), P(counts), L.stream_ptr()), "sgo_life_dev")

    def keys():
        L.check(lib.sgo_keys_dev(S, n, be.rec_ptr, be.cap, P(index), None, P(key0), P(canon), P(mask), None, L.stream_ptr()), "sgo_keys_dev")

    arms = {"keys": keys, "life": life, "shapes_side_v0": search("side_v0"), "shapes_side_16": search("side_16"),
            "shapes_corner_16": search("corner_16")}
    for fn in arms.values():                                   # warm-up: code objects
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    recs = be.records[:first].cpu().numpy().view(np.uint32)
    share = {}
    for k, name in (("side_16", "side"), ("corner_16", "corner")):
        sh = shapes[name]
        model = shapes_model.shapes(S, recs, shapes_model.Shape(sh.w, sh.h, sh.edges, tuple(tuple(r) for r in sh.cells)))
        assert np.array_equal(model["hits"], hits[k][:first].cpu().numpy()), k
        assert np.array_equal(model["cover"], cover[k][:first].cpu().numpy().view(np.uint32)), k
        share[k] = float((model["hits"][:, 0] > 0).mean())
    got16, got1 = hits["side_16"][:first].cpu().numpy(), hits["side_v0"][:first].cpu().numpy()
    assert np.array_equal(got1[:, 2] != 0, (got16[:, 2] & 1) != 0)          # as drawn only: exactly the rows variant 0 hits
    share["side_v0"] = float((got1[:, 0] > 0).mean())
    out = {"what": "sgo_shapes_dev (k_shapes) beside sgo_keys_dev (k_keys) and sgo_life_dev (k_life) on one 19x19 chunk, one MI355X; HIP "
                   "events around every call, arms interleaved; the device rows of the first copy equal the model's",
           "board": S, "games": len(n_entries), "rows": n, "shapes": {"side": SIDE.split("\n"), "corner": CORNER.split("\n")},
           "rows_hit_share": share, "resources_gfx950": {"k_shapes": resources("sgo_shapes.hip", "k_shapes")}, "arms": {}}
    for k, v in ms.items():
        st = stats(v)
        st["rows_per_s"] = n / (st["median_us"] * 1e-6)
        out["arms"][k] = st
    for k in ("shapes_side_v0", "shapes_side_16", "shapes_corner_16"):
        out[k + "_over_keys"] = out["arms"][k]["median_us"] / out["arms"]["keys"]["median_us"]
        out[k + "_over_life"] = out["arms"][k]["median_us"] / out["arms"]["life"]["median_us"]
    be.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
