"""Playout tree search on the device (include/sgo.h "playout tree search", csrc/sgo_uct.hip): which move?  Per position `trees`
independent Monte-Carlo tree searches of `sims` simulations each -- selection by a RAVE-blended value, expansion, a light playout
below the tree, back-propagation -- every search run from first to last inside one kernel: no net, no host loop.  What comes out is
the root's move table summed over the trees, and the move it favours: an ESTIMATE, not a proof.

    from sejonggo_amd.uct import search
    v = search(19, records, trees=256, sims=64, komi=7.5)   # packed records uint32 [R, 16 * NW], host or device
    v.best(0), v.winrate(0)                                 # the favoured move (N = pass; None for a row out of range), the mover's win rate
    v.move_table(0, 5)                                      # [(move, visits, win rate, rave visits, rave win rate)], most visited first
    v.ownership(0)                                          # float [N] in [-1, 1] over all simulations
    rollout.final_score(v.row(0), komi)                     # a row has the shape of rollout.result_row

The defaults below (TREES, SIMS, EXPAND_AT, RAVE_EQUIV, PRIOR) are UNTUNED: they are values in the range the literature uses for
RAVE without an exploration term, chosen so that the search runs; nobody has measured playing strength against them.
engine.SessionEngine.uct reads the root positions of session slots; GTP's `sgo-uct` and `--player uct` and
`python -m sejonggo_amd.review --uct` stand on it."""
import ctypes as C

import numpy as np

from ._packed import device_records
from .playout import RULES, SUMS

MAX_TREES, MAX_SIMS, MAX_DEPTH = 4096, 4096, 64
TREES = 64
SIMS = 128
EXPAND_AT = 2
RAVE_EQUIV = 256
PRIOR = 4


def komi2_of(komi):
    """komi as the integer 2 * komi the search compares 2 * (black - white) with"""
    k2 = int(round(2.0 * float(komi)))
    if abs(2.0 * float(komi) - k2) > 1e-9:
        raise ValueError("komi must be a multiple of 0.5")
    return k2


def check_args(size, trees, sims, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes):
    N = size * size
    if rules not in (0, 1):
        raise ValueError("rules must be 0 (inherited) or 1 (sound)")
    if not 1 <= int(trees) <= MAX_TREES:
        raise ValueError("trees must be in [1, %d]" % MAX_TREES)
    if not 1 <= int(sims) <= MAX_SIMS:
        raise ValueError("sims must be in [1, %d]" % MAX_SIMS)
    if int(max_plies) > 4 * N:
        raise ValueError("max_plies must be at most 4 * S * S (0: 3 * S * S)")
    if abs(int(komi2)) > 4 * N:
        raise ValueError("komi must be within +- 2 * S * S")
    if not 0 <= int(expand_at) <= int(sims):
        raise ValueError("expand_at must be in [0, sims]")
    if not 0 <= int(rave_equiv) <= 1 << 20:
        raise ValueError("rave_equiv must be in [0, 2^20]")
    if not 0 <= int(prior) <= 1024:
        raise ValueError("prior must be in [0, 1024]")
    if not 1 <= int(max_nodes) <= int(sims) + 1:
        raise ValueError("max_nodes must be in [1, sims + 1]")


class Search(object):
    """visits, wins2 int32 [n, N + 1] (index N: the pass), rave int32 [n, 2, N + 1] or None, own int32 [n, 2, N] or None, sums int64
    [n, 8] (playout.SUMS), info int32 [n, 4] (nodes, largest depth, trees refused a node, best), trace int32 [n * trees, sims] or
    None; white_to_play bool [n] or None: whose win rate the tables hold."""

    def __init__(self, size, visits, wins2, rave, own, sums, info, trace=None, white_to_play=None):
        self.S, self.N = size, size * size
        self.visits, self.wins2 = np.asarray(visits, dtype=np.int32), np.asarray(wins2, dtype=np.int32)
        self.rave = None if rave is None else np.asarray(rave, dtype=np.int32)
        self.own = None if own is None else np.asarray(own, dtype=np.int32)
        self.sums, self.info = np.asarray(sums, dtype=np.int64), np.asarray(info, dtype=np.int32)
        self.trace = None if trace is None else np.asarray(trace, dtype=np.int32)
        self.white_to_play = None if white_to_play is None else np.asarray(white_to_play, dtype=bool)

    def __len__(self):
        return len(self.sums)

    def count(self, i, name):
        return int(self.sums[i, SUMS.index(name)])

    def best(self, i):
        """the favoured move: a point, N for the pass, None for a row without a search"""
        b = int(self.info[i, 3])
        return None if b < 0 else b

    def winrate(self, i, move=None):
        """the win rate of the side to move after `move` (None: the favoured move) as the searches saw it: wins2 / (2 * visits);
        0.5 without a visit"""
        a = self.best(i) if move is None else int(move)
        if a is None or not self.visits[i, a]:
            return 0.5
        return int(self.wins2[i, a]) / (2.0 * int(self.visits[i, a]))

    def ranked(self, i, allowed=None):
        """the visited children, the most visited first (then the larger wins2, then the lower point): the order `best` heads;
        allowed: a predicate on the move, to skip children"""
        v, w = self.visits[i], self.wins2[i]
        pts = [int(a) for a in np.flatnonzero(v > 0) if allowed is None or allowed(int(a))]
        return sorted(pts, key=lambda a: (-int(v[a]), -int(w[a]), a))

    def move_table(self, i, k=None):
        """[(move, visits, win rate, rave visits, rave win rate)] of the visited children, best first; the rave columns are 0 and 0.5
        without a rave table"""
        out = []
        for a in self.ranked(i)[:k]:
            rn = int(self.rave[i, 0, a]) if self.rave is not None else 0
            rw = int(self.rave[i, 1, a]) if self.rave is not None else 0
            out.append((a, int(self.visits[i, a]), self.winrate(i, a), rn, rw / (2.0 * rn) if rn else 0.5))
        return out

    def ownership(self, i):
        """float64 [N]: (black's - white's) / simulations, 0 for a row without simulations"""
        if self.own is None:
            raise ValueError("this search ran without an ownership table")
        R = self.count(i, "playouts")
        return (self.own[i, 0].astype(np.float64) - self.own[i, 1]) / R if R else np.zeros(self.N)

    def row(self, i):
        """Row i shaped like rollout.result_row, so rollout.final_score / stone_status / point_owner work on it unchanged"""
        if self.own is None:
            raise ValueError("this search ran without an ownership table")
        out = {"black_own": self.own[i, 0], "white_own": self.own[i, 1]}
        for j, name in enumerate(SUMS):
            out[name] = int(self.sums[i, j])
        out["rollouts"] = out["playouts"]
        return out


def format_moves(v, i, k, vertex):
    """`sgo-uct` text: a head line `best V winrate 0.531 simulations 8192 nodes 4100 depth 7`, then one line `V visits winrate
    rave-visits rave-winrate` per move, the K most visited first"""
    b = v.best(i)
    lines = ["best %s winrate %.3f simulations %d nodes %d depth %d" % ("none" if b is None else vertex(b), v.winrate(i), v.count(i, "playouts"),
                                                                         int(v.info[i, 0]), int(v.info[i, 1]))]
    lines += ["%s %d %.3f %d %.3f" % (vertex(a), n, q, rn, rq) for a, n, q, rn, rq in v.move_table(i, k)]
    return "\n".join(lines)


def uct_dev(size, records, idx, n, trees, sims, seed, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes, lib, rec_ptr=None,
            n_records=None, rave=True, own=True, trace=False):
    """sgo_uct_dev on device tensors: (visits, wins2, rave or None, own or None, sums, info, trace or None) on the device; idx None:
    every record in order.  The workspace lives for the call."""
    import torch
    from . import _lib
    check_args(size, trees, sims, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes)
    R = int(records.shape[0]) if n_records is None else int(n_records)
    dev, N = records.device, size * size
    # the call zeroes its rows itself
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)                # noqa: E731
    visits, wins2, info = new(n, N + 1), new(n, N + 1), new(n, 4)
    rv, ow, tr = new(n, 2, N + 1) if rave else None, new(n, 2, N) if own else None, new(n * trees, sims) if trace else None
    sums = torch.empty((n, 8), dtype=torch.int64, device=dev)
    wb = _lib.check(int(lib.sgo_uct_workspace(size, n, int(trees), int(max_nodes))), "sgo_uct_workspace")
    work = torch.empty(max(wb, 4) // 4, dtype=torch.int32, device=dev)
    _lib.check(lib.sgo_uct_dev(C.c_int(size), C.c_int(n), C.c_void_p(rec_ptr) if rec_ptr is not None else _lib.ptr(records), C.c_int(R), _lib.ptr(idx),
                               int(trees), int(sims), C.c_uint32(int(seed) & 0xFFFFFFFF), int(rules), int(max_plies), int(komi2), int(expand_at),
                               int(rave_equiv), int(prior), int(max_nodes), _lib.ptr(visits), _lib.ptr(wins2), _lib.ptr(rv), _lib.ptr(ow),
                               _lib.ptr(sums), _lib.ptr(info), _lib.ptr(tr), _lib.ptr(work), C.c_int64(wb), _lib.stream_ptr()), "sgo_uct_dev")
    return visits, wins2, rv, ow, sums, info, tr


def search(size, records, index=None, trees=TREES, sims=SIMS, seed=0, rules=RULES, komi=0.0, max_plies=0, expand_at=EXPAND_AT,
           rave_equiv=RAVE_EQUIV, prior=PRIOR, max_nodes=None, trace=False):
    """sgo_uct_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Search with one row per entry of
    `index` (None: every record in order); an index outside [0, R) gives the zero row with best None.  komi is in points (a multiple
    of 0.5; black must lead by more to win); max_nodes None: sims + 1, a tree is never refused a node.  Simulation s of tree t of row
    i draws with the id (i * trees + t) * sims + s: the same call gives the same numbers on every machine.  The default trees, sims,
    expand_at, rave_equiv and prior are untuned."""
    from . import _lib
    max_nodes = int(sims) + 1 if max_nodes is None else int(max_nodes)
    komi2 = komi2_of(komi)
    check_args(size, trees, sims, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes)
    records, R, idx, n = device_records(size, records, index)
    out = uct_dev(size, records, idx, n, trees, sims, seed, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes, _lib.load(), trace=trace)
    NW = (size * size + 31) // 32
    rows = records[idx.long().clamp(0, max(R - 1, 0))] if idx is not None else records
    wtp = ((rows[:, NW - 1].contiguous().cpu().numpy().view(np.uint32) >> 31) != 0) if R else np.zeros(n, bool)
    host = [None if t is None else t.cpu().numpy() for t in out]
    return Search(size, *host, white_to_play=wtp)
