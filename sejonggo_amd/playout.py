"""Light playouts on the device (include/sgo.h "light playouts", csrc/sgo_playout.hip): per position `per_row` uniformly random
games that refuse to fill their own eyes, each played to its end inside one kernel -- no net, no host loop.  What comes out is an
ownership map, a score distribution and an all-moves-as-first table: an ESTIMATE of how the position ends, not a proof.

    from sejonggo_amd.playout import playouts
    v = playouts(19, records, per_row=256)             # packed records uint32 [R, 16 * NW], host or device
    v.score_mean(0), v.score_sd(0), v.capped_share(0)
    v.ownership(0)                                     # float [N] in [-1, 1]: +1 always black's at the end, -1 always white's
    v.move_values(0, min_count=8)                      # [(point, count, mean diff for the mover)], best first
    rollout.final_score(v.row(0), komi)                # a row has the shape of rollout.result_row

rules 1 ("sound", the default, as solve.py): a stone may also go where it has no empty neighbour and captures nothing as long as it
stands, which is what lets a ko be connected.  Under rules 0 (the inherited legal set) random playouts need not end on their own --
two kos and passes can cycle with one candidate per ply -- and the ply cap (default 3 * S * S) ends them; `capped_share` says how
often.  records.RecordSet.playouts() reads every position of a game collection, engine.SessionEngine.playouts the root positions of
session slots; GTP's `sgo-playouts` / `sgo-playout-moves` and `--score playouts`, `python -m sejonggo_amd.review --playouts` and
`python -m sejonggo_amd.records --playouts` stand on it."""
import ctypes as C

import numpy as np

from ._packed import device_records

SUMS = ("black_wins", "white_wins", "draws", "score_sum", "score_sq_sum", "plies_sum", "capped", "playouts")
MAX_PER_ROW = 65536
DEFAULT_PER_ROW = 256
RULES = 1                                                            # the default of solve.py


def check_args(size, per_row, rules, max_plies):
    if rules not in (0, 1):
        raise ValueError("rules must be 0 (inherited) or 1 (sound)")
    if not 1 <= int(per_row) <= MAX_PER_ROW:
        raise ValueError("per_row must be in [1, %d]" % MAX_PER_ROW)
    if int(max_plies) > 4 * size * size:
        raise ValueError("max_plies must be at most 4 * S * S (0: 3 * S * S)")


class Playouts(object):
    """own int32 [n, 2, N] (black's, white's), amaf int32 [n, 2, N] (count, score sum for the mover) or None, sums int64 [n, 8]
    (SUMS); white_to_play bool [n] or None: who the AMAF rows speak for."""

    def __init__(self, size, own, amaf, sums, white_to_play=None):
        self.S, self.N = size, size * size
        self.own, self.sums = np.asarray(own, dtype=np.int32), np.asarray(sums, dtype=np.int64)
        self.amaf = None if amaf is None else np.asarray(amaf, dtype=np.int32)
        self.white_to_play = None if white_to_play is None else np.asarray(white_to_play, dtype=bool)

    def __len__(self):
        return len(self.sums)

    def count(self, i, name):
        return int(self.sums[i, SUMS.index(name)])

    def row(self, i):
        """Row i shaped like rollout.result_row, so rollout.final_score / stone_status / point_owner work on it unchanged"""
        out = {"black_own": self.own[i, 0], "white_own": self.own[i, 1]}
        for j, name in enumerate(SUMS):
            out[name] = int(self.sums[i, j])
        out["rollouts"] = out["playouts"]
        return out

    def ownership(self, i):
        """float64 [N]: (black's - white's) / playouts, 0 for a row without playouts"""
        R = self.count(i, "playouts")
        return (self.own[i, 0].astype(np.float64) - self.own[i, 1]) / R if R else np.zeros(self.N)

    def score_mean(self, i):
        R = self.count(i, "playouts")
        return self.count(i, "score_sum") / float(R) if R else 0.0

    def score_sd(self, i):
        R = self.count(i, "playouts")
        if not R:
            return 0.0
        m = self.count(i, "score_sum") / float(R)
        return max(0.0, self.count(i, "score_sq_sum") / float(R) - m * m) ** 0.5

    def capped_share(self, i):
        R = self.count(i, "playouts")
        return self.count(i, "capped") / float(R) if R else 0.0

    def move_values(self, i, min_count=1):
        """[(point, count, mean)] of the points the side to move played first in at least min_count playouts, ranked by the mean
        final diff from that side's view (ties: the lower point)"""
        if self.amaf is None:
            raise ValueError("these playouts ran without an AMAF table")
        cnt, tot = self.amaf[i, 0], self.amaf[i, 1]
        pts = [(int(a), int(cnt[a]), int(tot[a]) / float(cnt[a])) for a in np.flatnonzero(cnt >= max(1, int(min_count)))]
        return sorted(pts, key=lambda t: (-t[2], t[0]))

    def format_board(self, i):
        """S lines from the top row down, one cell per point: black's share minus white's in per mille, signed"""
        o = np.rint(self.ownership(i) * 1000).astype(np.int64).reshape(self.S, self.S)
        return "\n".join(" ".join("%+5d" % v for v in line) for line in o)


def format_summary(v, i):
    """`sgo-playouts` head line: `score +3.4 +- 12.1 (black - white, komi-free)  capped 0.4%  playouts 256`"""
    return "score %+.1f +- %.1f  capped %.1f%%  playouts %d" % (v.score_mean(i), v.score_sd(i), 100.0 * v.capped_share(i), v.count(i, "playouts"))


def format_moves(v, i, k, vertex, min_count=1):
    """`sgo-playout-moves` text: one line `V count mean` per move, the K best first"""
    return "\n".join("%s %d %+.2f" % (vertex(a), c, m) for a, c, m in v.move_values(i, min_count)[:k])


def playout_dev(size, records, idx, n, per_row, seed, rules, max_plies, lib, rec_ptr=None, n_records=None, amaf=True):
    """sgo_playout_dev on device tensors: (own int32 [n, 2, N], amaf int32 [n, 2, N] or None, sums int64 [n, 8]) on the device; idx
    None: every record in order"""
    import torch
    from . import _lib
    check_args(size, per_row, rules, max_plies)
    R = int(records.shape[0]) if n_records is None else int(n_records)
    dev = records.device
    # the call zeroes its rows itself
    own = torch.empty((n, 2, size * size), dtype=torch.int32, device=dev)
    am = torch.empty((n, 2, size * size), dtype=torch.int32, device=dev) if amaf else None
    sums = torch.empty((n, 8), dtype=torch.int64, device=dev)
    _lib.check(lib.sgo_playout_dev(C.c_int(size), C.c_int(n), C.c_void_p(rec_ptr) if rec_ptr is not None else _lib.ptr(records), C.c_int(R),
                                   _lib.ptr(idx), C.c_int(int(per_row)), C.c_uint32(int(seed) & 0xFFFFFFFF), C.c_int(int(rules)),
                                   C.c_int(int(max_plies)), _lib.ptr(own), _lib.ptr(am), _lib.ptr(sums), _lib.stream_ptr()), "sgo_playout_dev")
    return own, am, sums


def playouts(size, records, index=None, per_row=DEFAULT_PER_ROW, seed=0, rules=RULES, max_plies=0):
    """sgo_playout_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Playouts with one row per
    entry of `index` (None: every record in order); an index outside [0, R) gives the zero row.  Playout j of row i draws with the
    id i * per_row + j: the same call gives the same numbers on every machine."""
    from . import _lib
    check_args(size, per_row, rules, max_plies)
    records, R, idx, n = device_records(size, records, index)
    own, am, sums = playout_dev(size, records, idx, n, per_row, seed, rules, max_plies, _lib.load())
    NW = (size * size + 31) // 32
    rows = records[idx.long().clamp(0, max(R - 1, 0))] if idx is not None else records
    wtp = ((rows[:, NW - 1].contiguous().cpu().numpy().view(np.uint32) >> 31) != 0) if R else np.zeros(n, bool)
    return Playouts(size, own.cpu().numpy(), am.cpu().numpy(), sums.cpu().numpy(), wtp)


# ---- game review and record statistics ----------------------------------------------------------------------------------------------
def lead_lines(names, leads, sds, vertex_of_move):
    """What `review --playouts` prints: per move the playout score lead (black - white, komi-free) of the position BEFORE it, the
    change the move made (seen from the mover: positive is good for the mover) and the three largest drops.  names: the movers
    ('B' / 'W'), leads / sds: one value per POSITION (len(names) + 1), vertex_of_move: the move texts."""
    lines, drops = [], []
    for j, who in enumerate(names):
        delta = (leads[j + 1] - leads[j]) * (1 if who == "B" else -1)
        lines.append("%4d %s %-4s lead %+6.1f +- %4.1f  change %+6.1f" % (j + 1, who, vertex_of_move[j], leads[j], sds[j], delta))
        drops.append((delta, j))
    worst = sorted(drops)[:3]
    lines.append("largest drops (estimate): " + ", ".join("move %d %s %s %+.1f" % (j + 1, names[j], vertex_of_move[j], d) for d, j in worst if d < 0))
    return lines


def bucket_table(ply, score_mean, score_sd, capped_share, width=20):
    """[{"from", "to", "positions", "abs_score", "sd", "capped"}] per bucket of `width` plies: the means over the positions of the
    bucket of |mean score|, of the score's standard deviation and of the capped share"""
    ply = np.asarray(ply, np.int64)
    out = []
    for b in sorted(set((ply // width).tolist())):
        sel = (ply // width) == b
        out.append({"from": int(b * width + 1), "to": int((b + 1) * width), "positions": int(sel.sum()),
                    "abs_score": float(np.abs(np.asarray(score_mean)[sel]).mean()), "sd": float(np.asarray(score_sd)[sel].mean()),
                    "capped": float(np.asarray(capped_share)[sel].mean())})
    return out


def format_report(games, table):
    lines = ["%s: playouts %+.1f +- %.1f at the last position, recorded %s" % (g["name"], g["lead"], g["sd"], g["result"]) for g in games]
    lines.append("moves      positions  |score|      sd  capped")
    for r in table:
        lines.append("%4d-%-4d  %9d  %7.1f  %6.1f  %5.1f%%" % (r["from"], r["to"], r["positions"], r["abs_score"], r["sd"], 100.0 * r["capped"]))
    return "\n".join(lines)
