"""Game records as data (include/sgo.h "game records", csrc/sgo_records.hip): SGF collections replayed on the device into one
packed record per ply, written out as supervised samples, and a net scored on the recorded moves.

    python -m sejonggo_amd.records PATH [--size S] [--samples OUT] [--score] [--net best|hash|uniform|table]
                                        [--symmetry identity|random1|0..7] [--bucket N] [--json FILE] [--compat-unknown-result]
                                        [--book OUT.npz] [--book-plies N] [--duplicates] [--find SHAPE.txt] [--moves]
                                        [--influence] [--superko [positional|situational]] [--playouts R]

PATH is one .sgf file or a directory of them (default conf['KGS_DATA_DIR']).  The counterpart of the reference's
kgs_game_parser/KGSSelfPlayWorker.py: every record is replayed with make_play's rules, and every B / W move gives the board before
it, a one-hot policy target (the pass is the last entry) and the value target `+1 if winner == player else -1`, written as
OUT/KGS/<game>/move_%03d/sample.h5 where the number is the index of the move's node on the main line (root = 0), the reference's
`move_n`.  A game directory that exists is left alone, as the reference leaves it.

--score is the strength measure that needs no games: how often the net's policy puts the recorded move first or among the top
five of the candidates (the legal moves and the recorded one), the cross-entropy of the recorded moves, how often the sign of the
value head agrees with the result, per bucket of `--bucket` moves (default 20) and in total.  The net reads the packed records
the replay wrote (net.predict_packed); no input tensor is built for a net that can.

ORIENTATION.  The project's own is kept, as review.py has it: x = the column letter, y = the row letter counted from the top.
The reference feeds sgfmill's (row from the bottom, column) pairs into make_play(x, y): the same game under one fixed symmetry of
the board.  That is not reproduced.

RESULT.  The winner is read from RE ("B+..." / "W+..."); anything else is unknown.  The reference labels every move of such a
record -1.  Here such records give no samples by default and their rows enter the score with z = 0, outside the value figures;
--compat-unknown-result writes the reference's -1.

ONE DEVIATION in the positions: the reference places only the root's AB stones (as black plays) and ignores AW.  Every AB / AW
stone sgfload lists is placed here, in the node it stands in.

POSITION KEYS (include/sgo.h "position keys", csrc/sgo_keys.hip).  Every record of a replay has a 64-bit key that rotations and
reflections of the board do not change.  --book groups the recorded moves of the first --book-plies nodes (default 30) by
(canonical key, move in the canonical frame) and writes count / wins / losses per group as one .npz (Book); `gtp --device --book`
plays from it.  --duplicates lists the records whose key sequences are equal ply for ply: the same game, in any orientation.
Ko status and history are no part of a key.

SHAPE SEARCH (include/sgo.h "shape search", csrc/sgo_shapes.hip).  --find SHAPE.txt reads a picture of a local shape (shapes.py:
X O . and * for don't-care, `|` and lines of `-` for the board edges), searches every position of every record for it in all
sixteen variants, and prints the games matched / searched and, for the first matching position of each game, the table of the
moves recorded next -- on which cell of the shape as drawn, by the side drawn as X or O, elsewhere, or none -- sorted by count,
with the mover's wins and losses.

MOVE OUTCOMES (include/sgo.h "move outcomes", csrc/sgo_moves.hip).  --moves reads, for every position, what one ply on every point
would do, keeps the row of the move that was played, and prints per bucket of --bucket moves the share of the played moves that
capture / give atari / escape (a chain with one liberty gets two or more) / are self-atari, each beside the mean share of the
ALLOWED moves of the same positions that do -- what the players chose against what the board offered -- and the number of points
the inherited legal-move rule forbids although the stone would stand, with the positions that had any.

INFLUENCE (include/sgo.h "influence", csrc/sgo_influence.hip).  --influence reads Bouzy's dilation / erosion map of every position
(the classical territory triple; the stones unconditional life proves dead lifted first) and prints per bucket of --bucket plies the
mean |margin|, the mean number of neutral points and the mean moyo beyond territory per colour, and per game the estimate at the
last position (before komi: a Record keeps none).  An estimate, not a proof.

SUPERKO (include/sgo.h "superko", csrc/sgo_superko.hip).  --superko compares what every move of every position would give with
every earlier position of the SAME game (positional: equal stones; situational: and the same side to move) and prints per game the
first move that reached a position seen before (passes apart), every played move that repeats although the inherited one-ply ko
rule allowed it, the number of ko recaptures played through (a recorded move is played, not filtered), and per bucket of --bucket
plies the share of positions in which superko forbids a move that rule allows.

A file that does not parse, whose board is not the requested size or whose list is longer than the replay takes is counted and
skipped; a record that holds a move onto a stone or off the board is cut short there and reported.  PyTorch is plumbing here
(device memory, stream, the net)."""
import argparse
import collections
import ctypes as C
import json
import os
import random as pyrandom
import sys

import numpy as np

from . import sgfload
from .conf import conf

Record = collections.namedtuple("Record", "name size entries setup nodes winner")
COUNTERS = ("rows", "top1", "top5", "illegal", "value_rows", "value_agree")
P_FLOOR = 2.0 ** -149          # the smallest float32 above zero: what a target probability that is not positive counts as


def parse_record(text, name="game"):
    """Record of one SGF text: entries [(action, colour)] as sgfload.loads gives them, setup [bool], nodes [int] (main-line
    node index per entry), winner +1 / -1 / None."""
    game = sgfload.loads(text)
    nodes = sgfload.node_indices(text)
    assert len(nodes) == len(game.moves)
    return Record(name, game.size, list(game.moves), list(game.setup), nodes, sgfload.result_winner(sgfload.root_properties(text)))


def max_entries_of(size):
    return 4 * size * size           # SGO_SETUP_MAX_MOVES


def read_path(path, size):
    """(records, skipped) of a file or a directory (its *.sgf files, sorted).  skipped: {"unreadable": [names], "wrong_size":
    [names], "too_long": [names]}."""
    if os.path.isdir(path):
        files = [os.path.join(path, f) for f in sorted(os.listdir(path)) if f.lower().endswith(".sgf")]
    else:
        files = [path]
    records, skipped = [], {"unreadable": [], "wrong_size": [], "too_long": []}
    for f in files:
        name = os.path.basename(f).split(".")[0]       # KGSSelfPlayWorker.py:30
        try:
            with open(f, "r", errors="replace") as fh:
                rec = parse_record(fh.read(), name)
        except (ValueError, OSError, AssertionError):
            skipped["unreadable"].append(name)
            continue
        if rec.size != size:
            skipped["wrong_size"].append(name)
        elif len(rec.entries) > max_entries_of(size):
            skipped["too_long"].append(name)
        else:
            records.append(rec)
    return records, skipped


def value_targets(winner, colours, compat_unknown=False):
    """(z int32 [n], has_sample bool [n]) for moves of the given colours in a record won by `winner` (+1 / -1 / None).
    z = +1 if winner == colour else -1 (KGSSelfPlayWorker.py:97-99); an unknown result gives z = 0 and no sample, or with
    `compat_unknown` the reference's -1 and a sample."""
    colours = np.asarray(colours, dtype=np.int32)
    if winner is None:
        if compat_unknown:
            return np.full(len(colours), -1, np.int32), np.ones(len(colours), bool)
        return np.zeros(len(colours), np.int32), np.zeros(len(colours), bool)
    return np.where(colours == winner, 1, -1).astype(np.int32), np.ones(len(colours), bool)


def float_sums(p_target, value, z, bucket, n_buckets):
    """(ce_sum, se_sum) float64 [n_buckets]: per bucket, row after row in the order given, -log(p) of the float32 target
    probabilities taken to float64 (a p that is not positive counts as 2^-149, a p above 1 as 1) and (v - z)^2 over the rows with
    z != 0."""
    p = np.asarray(p_target, dtype=np.float32).astype(np.float64)
    q = np.where(p > 0.0, np.minimum(p, 1.0), P_FLOOR)
    ce_terms = -np.log(q)
    v = np.asarray(value, dtype=np.float32).astype(np.float64)
    zf = np.asarray(z, dtype=np.int32).astype(np.float64)
    se_terms = np.where(zf != 0.0, (v - zf) * (v - zf), 0.0)
    ce, se = np.zeros(n_buckets, np.float64), np.zeros(n_buckets, np.float64)
    b = np.asarray(bucket, dtype=np.int64)
    np.add.at(ce, b, ce_terms)                 # unbuffered: one addition per row, in row order
    np.add.at(se, b[zf != 0.0], se_terms[zf != 0.0])
    return ce, se


def tables(counters, ce_sum, se_sum, width):
    """(per-bucket rows, total row) as dicts from the int64 counters [n_buckets][8] and the float sums."""
    counters = np.asarray(counters, dtype=np.int64)

    def row(c, ce, se):
        d = {name: int(c[i]) for i, name in enumerate(COUNTERS)}
        d["ce_sum"], d["se_sum"] = float(ce), float(se)
        d["cross_entropy"] = float(ce) / d["rows"] if d["rows"] else None
        d["value_mse"] = float(se) / d["value_rows"] if d["value_rows"] else None
        return d
    buckets = []
    for b in range(len(counters)):
        d = row(counters[b], ce_sum[b], se_sum[b])
        d["bucket"], d["first_move"] = b, b * width
        buckets.append(d)
    tce = tse = 0.0
    for b in range(len(counters)):             # bucket after bucket: the order is part of the figure
        tce += float(ce_sum[b])
        tse += float(se_sum[b])
    return buckets, row(counters.sum(axis=0), tce, tse)


def sym_luts(size):
    """int32 [8, A]: the tables sgo_sym_lut(size, k) writes, k = 0..7 (symmetry.py:12-42), in integers."""
    m = size - 1
    y, x = np.divmod(np.arange(size * size), size)
    pts = [(x, y), (y, x), (m - x, y), (x, m - y), (m - y, x), (m - x, m - y), (y, m - x), (m - y, m - x)]     # (new x, new y)
    out = np.full((8, size * size + 1), size * size, np.int32)
    for k, (nx, ny) in enumerate(pts):
        out[k, :size * size] = nx + size * ny
    return out


def sm64(x):
    """sm of include/sgo.h "position keys" on uint64 arrays (wrapping)."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _host(a, dtype=None):
    """numpy array of a backend's output (a torch tensor or an array); int64 key tensors come back as uint64"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(dtype) if dtype is not None and a.dtype != dtype else a


def _tensor(a):
    """torch tensor of a backend's output; uint64 keys travel as the int64 of the same bits (torch has no unsigned sort)"""
    import torch
    if torch.is_tensor(a):
        return a
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)


class Book(object):
    """An opening book: per (canonical key, action in the canonical frame) how often the move was played and how it ended for the
    mover.  Entries are sorted by (key unsigned, action).  One .npz: size, key uint64, action int32, count / wins / losses int64."""

    def __init__(self, size, key, action, count, wins, losses):
        self.size = int(size)
        self.key, self.action = np.asarray(key, np.uint64), np.asarray(action, np.int32)
        self.count, self.wins, self.losses = (np.asarray(v, np.int64) for v in (count, wins, losses))
        order = np.lexsort((self.action, self.key))
        for name in ("key", "action", "count", "wins", "losses"):
            setattr(self, name, getattr(self, name)[order])
        self._luts = sym_luts(self.size)

    def __len__(self):
        return len(self.key)

    def __eq__(self, other):
        return isinstance(other, Book) and self.size == other.size and all(
            np.array_equal(getattr(self, n), getattr(other, n)) for n in ("key", "action", "count", "wins", "losses"))

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, size=np.int32(self.size), key=self.key, action=self.action, count=self.count, wins=self.wins,
                     losses=self.losses)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(int(z["size"]), z["key"], z["action"], z["count"], z["wins"], z["losses"])

    def moves(self, canon, mask):
        """[(a, count, wins, losses)] in the BOARD frame of a position with the given canonical key and symmetry mask
        (sgo_keys_dev / sgo_session_keys): for the smallest k of the mask, the a with L_k[a] == the entry's canonical action.
        Ordered by count descending, then a ascending."""
        mask = int(mask) & 255
        if not mask:
            return []
        k = (mask & -mask).bit_length() - 1
        canon = np.uint64(int(canon) & ((1 << 64) - 1))
        lo, hi = np.searchsorted(self.key, canon, "left"), np.searchsorted(self.key, canon, "right")
        back = np.empty(self.size * self.size + 1, np.int64)
        back[self._luts[k]] = np.arange(self.size * self.size + 1)
        rows = [(int(back[self.action[i]]), int(self.count[i]), int(self.wins[i]), int(self.losses[i])) for i in range(lo, hi)]
        return sorted(rows, key=lambda r: (-r[1], r[0]))


class DeviceRecords(object):
    """The sgo_records object of the library: replay, the record arrays as tensors, boards, the score launch."""

    def __init__(self, size, max_games, max_entries, device=0):
        import torch
        from . import _lib
        self.torch, self._lib = torch, _lib
        self.lib = _lib.require_gpu()
        self.S, self.N, self.A = size, size * size, size * size + 1
        self.max_games, self.max_entries = int(max_games), int(max_entries)
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.RW, self.NW = self.lib.sgo_packed_words(size), self.lib.sgo_plane_words(size)
        self.h = C.c_void_p(self.lib.sgo_records_create(size, self.max_games, self.max_entries, device))
        if not self.h:
            raise _lib.SgoError("sgo_records_create failed: %s" % self.lib.sgo_last_error().decode())
        rec, leg = C.c_void_p(), C.c_void_p()
        self.cap = _lib.check(self.lib.sgo_records_list(self.h, C.byref(rec), C.byref(leg)), "sgo_records_list")
        self.rec_ptr, self.legal_ptr = rec.value, leg.value
        self.records = self._view(rec.value, (self.cap, self.RW))
        self.legal = self._view(leg.value, (self.cap, self.NW))

    def _view(self, address, shape):
        class _Mem(object):
            pass
        m = _Mem()
        m.__cuda_array_interface__ = {"shape": shape, "typestr": "<i4", "data": (address, False), "version": 2}
        return self.torch.as_tensor(m, device=self.device)

    def close(self):
        if getattr(self, "h", None):
            self.records = self.legal = None
            self.lib.sgo_records_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def replay(self, n_entries, off, actions, colors):
        n_entries, off = np.ascontiguousarray(n_entries, np.int32), np.ascontiguousarray(off, np.int32)
        actions, colors = np.ascontiguousarray(actions, np.int32), np.ascontiguousarray(colors, np.int32)
        status, fail_at = np.zeros(len(n_entries), np.int32), np.full(len(n_entries), -1, np.int32)
        self._lib.check(self.lib.sgo_records_replay(self.h, len(n_entries), self._lib.ptr(n_entries), self._lib.ptr(off),
                                                    self._lib.ptr(actions), self._lib.ptr(colors), self._lib.ptr(status),
                                                    self._lib.ptr(fail_at), self._lib.stream_ptr()), "sgo_records_replay")
        return status, fail_at

    def boards(self, index, chunk=2048):
        """Board tensors int32 [n, S, S, 17] (host) of the listed records, through sgo_unpack_dev."""
        torch = self.torch
        index = np.asarray(index, dtype=np.int64)
        out = np.zeros((len(index), self.S, self.S, 17), np.int32)
        for lo in range(0, len(index), chunk):
            idx = torch.from_numpy(index[lo:lo + chunk]).to(self.device)
            packed = self.records.index_select(0, idx).contiguous()
            b17 = torch.empty((len(idx), self.S, self.S, 17), dtype=torch.int32, device=self.device)
            self._lib.check(self.lib.sgo_unpack_dev(C.c_int(self.S), C.c_int(len(idx)), self._lib.ptr(packed), self._lib.ptr(b17),
                                                    self._lib.stream_ptr()), "sgo_unpack_dev")
            out[lo:lo + chunk] = b17.cpu().numpy()
        return out

    def forward(self, net, index_dev, n, k, scratch):
        """(policy float32 [n, A], value float32 [n]) of the net on the records index_dev lists, evaluated under symmetry k."""
        torch = self.torch
        if getattr(net, "packed_ok", False):
            p, v = net.predict_packed(self.rec_ptr, index_dev.data_ptr(), n, k)
        else:                                   # a net that reads board tensors: the route of rollout.RolloutEngine._forward
            layout = 2 if getattr(net, "in_channels", 17) == 32 else 0
            if scratch.get("nn_in") is None or scratch["nn_in"].shape[0] < n:
                scratch["nn_in"] = torch.zeros((n, self.S, self.S, 32 if layout == 2 else 17), dtype=torch.float16, device=self.device)
            x = scratch["nn_in"]
            self._lib.check(self.lib.sgo_nn_pack_dev(C.c_int(self.S), C.c_int(n), C.c_void_p(self.rec_ptr), self._lib.ptr(index_dev),
                                                     C.c_int(k), C.c_int(layout), C.c_int(0), self._lib.ptr(x), self._lib.stream_ptr()),
                            "sgo_nn_pack_dev")
            p, v = net.predict_on_batch(x[:n])
        return p.to(torch.float32).contiguous(), v.to(torch.float32).reshape(n).contiguous()

    def score(self, n, index, target, z, bucket, n_buckets, policy, value, k, rank, best, p_target, flags, counters):
        P = self._lib.ptr
        self._lib.check(self.lib.sgo_records_score_dev(self.h, int(n), P(index), P(target), P(z), P(bucket), int(n_buckets), P(policy),
                                                       P(value), int(k), P(rank), P(best), P(p_target), P(flags), P(counters),
                                                       self._lib.stream_ptr()), "sgo_records_score_dev")

    def _index(self, index):
        """a list of record indices (a tensor or an array) as a contiguous int32 tensor on the device"""
        torch = self.torch
        index = (index if torch.is_tensor(index) else torch.from_numpy(np.ascontiguousarray(index, np.int32))).to(self.device, torch.int32)
        return index.contiguous()

    def _rows(self, index, words=slice(None)):
        """(the `words` of the listed records, ok): an index outside the object reads record 0 and is False in ok"""
        ok = (index >= 0) & (index < self.cap)
        return self.records[self.torch.where(ok, index, self.torch.zeros_like(index)).long(), words], ok

    def keys(self, index, target=None):
        """(key0, canon, mask, canon_action) device tensors of the listed records (sgo_keys_dev, one launch): the keys int64
        holding the uint64 bit patterns, mask / canon_action int32; canon_action is None without targets.  An index outside the
        object gives the zero row."""
        torch = self.torch
        index = self._index(index)
        n = int(index.shape[0])
        target = self._index(target) if target is not None else None
        assert target is None or int(target.shape[0]) == n
        key0, canon = torch.zeros(n, dtype=torch.int64, device=self.device), torch.zeros(n, dtype=torch.int64, device=self.device)
        mask = torch.zeros(n, dtype=torch.int32, device=self.device)
        action = torch.full((n,), -1, dtype=torch.int32, device=self.device) if target is not None else None
        if n:
            P = self._lib.ptr
            self._lib.check(self.lib.sgo_keys_dev(C.c_int(self.S), C.c_int(n), C.c_void_p(self.rec_ptr), C.c_int(self.cap), P(index),
                                                  P(target), P(key0), P(canon), P(mask), P(action), self._lib.stream_ptr()),
                            "sgo_keys_dev")
        return key0, canon, mask, action

    def tactics(self, index, max_chains=128):
        """(libs uint8 [n, N], n_chains int32 [n], chains int32 [n, max_chains, 8]) device tensors of the listed records
        (sgo_tactics_dev, two launches; include/sgo.h "chains and ladders").  Chain rows behind min(n_chains, max_chains) are zero;
        an index outside the object gives the zero row."""
        torch = self.torch
        index = self._index(index)
        n, mc = int(index.shape[0]), int(max_chains)
        libs = torch.zeros((n, self.N), dtype=torch.uint8, device=self.device)
        n_chains = torch.zeros(n, dtype=torch.int32, device=self.device)
        chains = torch.zeros((n, mc, 8), dtype=torch.int32, device=self.device)
        if n:
            P = self._lib.ptr
            self._lib.check(self.lib.sgo_tactics_dev(C.c_int(self.S), C.c_int(n), C.c_void_p(self.rec_ptr), C.c_int(self.cap), P(index),
                                                     C.c_int(mc), P(libs), P(n_chains), P(chains), self._lib.stream_ptr()),
                            "sgo_tactics_dev")
        return libs, n_chains, chains

    def life(self, index):
        """(sets int32 [n, 4, NW] holding the uint32 bit patterns, counts int32 [n, 8]) device tensors of the listed records
        (sgo_life_dev, one launch; include/sgo.h "unconditional life"); an index outside the object gives the zero row."""
        torch = self.torch
        index = self._index(index)
        n = int(index.shape[0])
        sets = torch.zeros((n, 4, self.NW), dtype=torch.int32, device=self.device)
        counts = torch.zeros((n, 8), dtype=torch.int32, device=self.device)
        if n:
            P = self._lib.ptr
            self._lib.check(self.lib.sgo_life_dev(C.c_int(self.S), C.c_int(n), C.c_void_p(self.rec_ptr), C.c_int(self.cap), P(index),
                                                  P(sets), P(counts), self._lib.stream_ptr()), "sgo_life_dev")
        return sets, counts

    def influence(self, index, dead=None, dilate=5, erode_moyo=10, erode_terr=21):
        """(values int16 [n, N], sets int32 [n, 4, NW] holding the uint32 bit patterns, counts int32 [n, 8]) device tensors of the
        listed records (sgo_influence_dev, one launch; include/sgo.h "influence"); an index outside the object gives the zero row.
        dead "life": the stones sgo_life_dev proves dead are lifted first (one more launch and two mask operations on the device);
        None: nothing is lifted; or a tensor / array [n, NW] of the rows' own."""
        from .influence import check_params, dead_from_life, influence_dev
        dilate, erode_moyo, erode_terr = check_params(dilate, erode_moyo, erode_terr)
        if isinstance(dead, str) and dead != "life":
            raise ValueError("influence: dead is None, \"life\" or an array of bitsets")
        index = self._index(index)
        n = int(index.shape[0])
        if isinstance(dead, str):
            life_sets, _ = self.life(index)
            planes, _ = self._rows(index, slice(0, 2 * self.NW))
            dead = dead_from_life(life_sets, planes[:, :self.NW], planes[:, self.NW:]).contiguous()
        return influence_dev(self.S, self.records, index, n, dead, dilate, erode_moyo, erode_terr, self.lib, self.rec_ptr, self.cap)

    def shapes(self, index, shape):
        """(hits int32 [n, 4], cover int32 [n, NW] holding the uint32 bit patterns) device tensors of the listed records for a
        shapes.Shape (sgo_shape_compile on the host, then sgo_shapes_dev, one launch; include/sgo.h "shape search"); an index
        outside the object gives {0, -1, 0, 0} and a zero cover."""
        from .shapes import compile_table
        torch = self.torch
        index = self._index(index)
        n = int(index.shape[0])
        table = torch.from_numpy(compile_table(self.S, shape).view(np.int32)).to(self.device)
        hits = torch.zeros((n, 4), dtype=torch.int32, device=self.device)
        cover = torch.zeros((n, self.NW), dtype=torch.int32, device=self.device)
        if n:
            P = self._lib.ptr
            self._lib.check(self.lib.sgo_shapes_dev(C.c_int(self.S), C.c_int(n), C.c_void_p(self.rec_ptr), C.c_int(self.cap), P(index),
                                                    P(table), P(hits), P(cover), self._lib.stream_ptr()), "sgo_shapes_dev")
        return hits, cover

    def to_play(self, index):
        """int8 [n] device tensor: the side to move of the listed records (+1 black, -1 white; 0 for an index outside the object)"""
        torch = self.torch
        index = self._index(index)
        if int(index.shape[0]) == 0:
            return torch.zeros(0, dtype=torch.int8, device=self.device)
        last, ok = self._rows(index, self.NW - 1)                        # the top bit of plane 0's last word
        return (torch.where(last < 0, -1, 1) * ok).to(torch.int8)

    def secure(self, index, side=0):
        """(table int16 [n, N, 4], sets int32 [n, 4, NW] holding the uint32 bit patterns, counts int32 [n, 8]) device tensors of the
        listed records (sgo_secure_dev, two launches; include/sgo.h "securing moves"); an index outside the object gives the zero
        row."""
        from .secure import secure_dev
        torch = self.torch
        index = self._index(index)
        if int(index.shape[0]) == 0:
            return (torch.zeros((0, self.N, 4), dtype=torch.int16, device=self.device),
                    torch.zeros((0, 4, self.NW), dtype=torch.int32, device=self.device), torch.zeros((0, 8), dtype=torch.int32, device=self.device))
        return secure_dev(self.S, self.records, index, side, self.lib)

    def solve(self, index, rules=1, max_region=12, max_nodes=4096, max_targets=16):
        """(n_targets int32 [n], rows int32 [n, max_targets, 8], regions int32 [n, max_targets, NW] holding the uint32 bit patterns)
        device tensors of the listed records, every enclosed chain enumerated (sgo_solve_dev, two launches; include/sgo.h "life and
        death").  Rows behind min(n_targets, max_targets) are zero; an index outside the object gives n_targets 0."""
        from .solve import solve_dev
        torch = self.torch
        index = self._index(index)
        if int(index.shape[0]) == 0:
            return (torch.zeros(0, dtype=torch.int32, device=self.device), torch.zeros((0, int(max_targets), 8), dtype=torch.int32, device=self.device),
                    torch.zeros((0, int(max_targets), self.NW), dtype=torch.int32, device=self.device))
        return solve_dev(self.S, self.records, index, None, None, rules, max_region, max_nodes, max_targets, self.lib)

    def race(self, index, rules=1, max_libs=4, max_region=8, max_nodes=1024, max_pairs=64):
        """(n_pairs int32 [n], rows int32 [n, max_pairs, 16], regions int32 [n, max_pairs, NW] holding the uint32 bit patterns)
        device tensors of the listed records, every pair in contact enumerated (sgo_race_dev, two launches; include/sgo.h "capturing
        races").  Rows behind min(n_pairs, max_pairs) are zero; an index outside the object gives n_pairs 0."""
        from .race import race_dev
        torch = self.torch
        index = self._index(index)
        if int(index.shape[0]) == 0:
            return (torch.zeros(0, dtype=torch.int32, device=self.device), torch.zeros((0, int(max_pairs), 16), dtype=torch.int32, device=self.device),
                    torch.zeros((0, int(max_pairs), self.NW), dtype=torch.int32, device=self.device))
        return race_dev(self.S, self.records, index, None, None, rules, max_libs, max_region, max_nodes, max_pairs, self.lib)

    def connect(self, index, rules=1, cut_libs=1, max_region=8, max_nodes=1024, max_pairs=64):
        """(n_pairs int32 [n], rows int32 [n, max_pairs, 12], regions int32 [n, max_pairs, NW] holding the uint32 bit patterns, groups
        int16 [n, N], group_counts int32 [n, 4]) device tensors of the listed records, every near pair enumerated (sgo_connect_dev,
        three launches; include/sgo.h "connections").  Rows behind min(n_pairs, max_pairs) are zero; an index outside the object
        gives n_pairs 0 and a map of -1."""
        from .connect import WORDS, connect_dev
        torch = self.torch
        index = self._index(index)
        if int(index.shape[0]) == 0:
            return (torch.zeros(0, dtype=torch.int32, device=self.device), torch.zeros((0, int(max_pairs), WORDS), dtype=torch.int32, device=self.device),
                    torch.zeros((0, int(max_pairs), self.NW), dtype=torch.int32, device=self.device),
                    torch.zeros((0, self.N), dtype=torch.int16, device=self.device), torch.zeros((0, 4), dtype=torch.int32, device=self.device))
        return connect_dev(self.S, self.records, index, None, None, rules, cut_libs, max_region, max_nodes, max_pairs, self.lib)

    def superko(self, index, first, rule=0, n_records=None):
        """(sets int32 [n, 3, NW] holding the uint32 bit patterns, back int16 [n, N], counts int32 [n, 8]) device tensors of the listed
        records, each with the history first[i] .. index[i] (sgo_superko_dev, two launches; include/sgo.h "superko").  An index
        outside the object, a negative first or one behind the record gives the zero row (back all -1).  n_records: how many
        records of the object are in use (the first stage keys them all; None: the whole object)."""
        from .superko import superko_dev
        torch = self.torch
        index, first = self._index(index), self._index(first)
        n = int(index.shape[0])
        assert int(first.shape[0]) == n
        if n == 0:
            return (torch.zeros((0, 3, self.NW), dtype=torch.int32, device=self.device), torch.zeros((0, self.N), dtype=torch.int16, device=self.device),
                    torch.zeros((0, 8), dtype=torch.int32, device=self.device))
        used = self.cap if n_records is None else max(0, min(self.cap, int(n_records)))
        return superko_dev(self.S, self.records, index, first, rule, self.lib, n_records=used)

    def playouts(self, index, per_row=16, seed=0, rules=1, max_plies=0, amaf=True):
        """(own int32 [n, 2, N], amaf int32 [n, 2, N] or None, sums int64 [n, 8]) device tensors of the listed records: per_row light
        playouts each (sgo_playout_dev, two launches; include/sgo.h "light playouts").  Playout j of row i draws with the id
        i * per_row + j.  An index outside the object gives the zero row."""
        from .playout import playout_dev
        torch = self.torch
        index = self._index(index)
        n = int(index.shape[0])
        if n == 0:
            z = torch.zeros((0, 2, self.N), dtype=torch.int32, device=self.device)
            return z, (z.clone() if amaf else None), torch.zeros((0, 8), dtype=torch.int64, device=self.device)
        return playout_dev(self.S, self.records, index, n, per_row, seed, rules, max_plies, self.lib, amaf=amaf)

    def uct(self, index, trees, sims, seed=0, rules=1, max_plies=0, komi2=0, expand_at=2, rave_equiv=256, prior=4, max_nodes=None):
        """(visits, wins2 int32 [n, N + 1], rave int32 [n, 2, N + 1], own int32 [n, 2, N], sums int64 [n, 8], info int32 [n, 4]) device
        tensors of the listed records: `trees` playout tree searches of `sims` simulations each (sgo_uct_dev, three launches;
        include/sgo.h "playout tree search").  An index outside the object gives the zero row with best -1."""
        from .uct import uct_dev
        torch = self.torch
        index = self._index(index)
        n = int(index.shape[0])
        if n == 0:
            z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=self.device)      # noqa: E731
            return z(0, self.N + 1), z(0, self.N + 1), z(0, 2, self.N + 1), z(0, 2, self.N), torch.zeros((0, 8), dtype=torch.int64, device=self.device), z(0, 4)
        max_nodes = int(sims) + 1 if max_nodes is None else max_nodes
        return uct_dev(self.S, self.records, index, n, trees, sims, seed, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes, self.lib)[:6]

    def moves(self, index, side=0, action=None, colour=None, rows_per_call=16384):
        """Move outcomes of the listed records (sgo_moves_dev, one launch per rows_per_call rows; include/sgo.h "move outcomes"); an
        index outside the object gives the zero row.  action None: (rows int16 [n, N, 8], counts int32 [n, 8]) device tensors, in
        one call.  With action int [n]: (played int16 [n, 8], counts, in_turn bool [n]) device tensors -- of the table only the row
        of the listed action is kept (rows[arange, action], gathered on the device; the zero row for a pass or an action off the
        board), so nothing of size n * N leaves the device; in_turn says that `colour` [n] (+1 black, -1 white; None: not asked,
        all True) is the colour side 0 moves for, i.e. the record's side to move."""
        from .moves import moves_dev
        torch = self.torch
        index = self._index(index)
        n = int(index.shape[0])
        if action is None:
            if n == 0:
                return (torch.zeros((0, self.N, 8), dtype=torch.int16, device=self.device), torch.zeros((0, 8), dtype=torch.int32, device=self.device))
            return moves_dev(self.S, self.records, index, side, self.lib)
        action = torch.from_numpy(np.ascontiguousarray(action, np.int64)).to(self.device)
        played = torch.zeros((n, 8), dtype=torch.int16, device=self.device)
        counts = torch.zeros((n, 8), dtype=torch.int32, device=self.device)
        for lo in range(0, n, int(rows_per_call)):
            hi = min(n, lo + int(rows_per_call))
            rows, c = moves_dev(self.S, self.records, index[lo:hi].contiguous(), side, self.lib)
            a = action[lo:hi]
            on = (a >= 0) & (a < self.N)
            picked = rows[torch.arange(hi - lo, device=self.device), torch.where(on, a, torch.zeros_like(a))]
            played[lo:hi] = picked * on[:, None].to(torch.int16)
            counts[lo:hi] = c
        in_turn = torch.ones(n, dtype=torch.bool, device=self.device)
        if colour is not None and n:
            last, ok = self._rows(index, self.NW - 1)
            flag = last < 0                                              # the top bit of plane 0's last word
            col = torch.from_numpy(np.ascontiguousarray(colour, np.int32)).to(self.device)
            in_turn = ok & (torch.where(flag, -1, 1) == col)
        return played, counts, in_turn

    def stones(self, index):
        """int8 [n, N] (host): +1 black, -1 white on the listed records; an index outside the object gives the empty board."""
        from .tactics import stones_of
        planes, ok = self._rows(self._index(index), slice(0, 2 * self.NW))
        return stones_of(self.S, planes.contiguous().cpu().numpy()) * ok.cpu().numpy()[:, None].astype(np.int8)


class Chunk(object):
    """What one replay call left on the device, one row per ENTRY of its games (set-up stones included): index (the record
    holding the position before the entry), game (index into RecordSet.records), node, action, colour, z, setup, valid (the entry
    was played: its game was not refused at or before it), sample (a move that gives a sample), plus status / fail_at per game."""
    FIELDS = ("index", "game", "node", "action", "colour", "z", "setup", "valid", "sample")

    def rows(self, mask):
        return {k: getattr(self, k)[mask] for k in self.FIELDS}

    def walk(self):
        """(i, g, base, off, n, played) per game of the chunk: its place in `games`, its index into RecordSet.records, its first
        record and its first entry row, the number of its entries and how many of them were played.  Records base .. base +
        played were written; entry row off + j stands between records base + j and base + j + 1."""
        base = off = 0
        for i, g in enumerate(self.games):
            n = int(self.n_entries[i])
            yield i, g, base, off, n, (int(self.fail_at[i]) if self.status[i] != 0 else n)
            base += n + 1
            off += n


class RecordSet(object):
    """Records of one board size on a replay backend (DeviceRecords, or anything with its replay / boards surface)."""

    def __init__(self, records, size=None, device=0, max_games=None, max_entries=None, compat_unknown_result=False, backend=None):
        self.records = list(records)
        self.S = size or conf['SIZE']
        self.N, self.A = self.S * self.S, self.S * self.S + 1
        self.compat_unknown_result = bool(compat_unknown_result)
        for r in self.records:
            if r.size != self.S or len(r.entries) > max_entries_of(self.S):
                raise ValueError("record %s does not fit a %dx%d replay" % (r.name, self.S, self.S))
            if any(c not in (1, -1) for _, c in r.entries):
                raise ValueError("record %s: every entry needs an explicit colour" % r.name)
        longest = max([len(r.entries) for r in self.records] + [1])
        total = sum(len(r.entries) for r in self.records)
        self.max_games = int(max_games or max(1, min(len(self.records), 4096)))
        self.max_entries = max(longest, int(max_entries or min(max(total, 1), 1 << 18)))
        self.backend = backend if backend is not None else DeviceRecords(self.S, self.max_games, self.max_entries, device)
        self.refused = []                      # (record name, status, fail_at) of the games a replay cut short

    def close(self):
        if self.backend is not None and hasattr(self.backend, "close"):
            self.backend.close()
        self.backend = None

    def _partition(self):
        out, cur, used = [], [], 0
        for g, r in enumerate(self.records):
            if cur and (len(cur) >= self.max_games or used + len(r.entries) > self.max_entries):
                out.append(cur)
                cur, used = [], 0
            cur.append(g)
            used += len(r.entries)
        if cur:
            out.append(cur)
        return out

    def replay(self):
        """Generator of Chunks: as many games per replay call as the object holds.  The device records of a chunk are valid until
        the next one is asked for."""
        self.refused = []
        for games in self._partition():
            n_entries = np.array([len(self.records[g].entries) for g in games], np.int32)
            off = np.concatenate([[0], np.cumsum(n_entries)[:-1]]).astype(np.int32)
            total = int(n_entries.sum())
            ch = Chunk()
            ch.games, ch.n_entries = games, n_entries
            ch.action, ch.colour = np.zeros(total, np.int32), np.zeros(total, np.int32)
            ch.node, ch.game = np.zeros(total, np.int32), np.zeros(total, np.int32)
            ch.setup, ch.z, has = np.zeros(total, bool), np.zeros(total, np.int32), np.zeros(total, bool)
            for i, g in enumerate(games):
                r = self.records[g]
                lo, hi = int(off[i]), int(off[i]) + len(r.entries)
                if hi > lo:
                    ch.action[lo:hi] = [a for a, _ in r.entries]
                    ch.colour[lo:hi] = [c for _, c in r.entries]
                    ch.node[lo:hi] = r.nodes
                    ch.setup[lo:hi] = r.setup
                    ch.z[lo:hi], has[lo:hi] = value_targets(r.winner, ch.colour[lo:hi], self.compat_unknown_result)
                ch.game[lo:hi] = g
            ch.status, ch.fail_at = self.backend.replay(n_entries, off, ch.action, ch.colour)
            ch.index = (np.arange(total) + np.repeat(np.arange(len(games)), n_entries)).astype(np.int32)    # base_g + j
            ch.valid = np.ones(total, bool)
            for i, g in enumerate(games):
                if ch.status[i] != 0:
                    ch.valid[int(off[i]) + int(ch.fail_at[i]):int(off[i]) + int(n_entries[i])] = False
                    self.refused.append((self.records[g].name, int(ch.status[i]), int(ch.fail_at[i])))
            ch.sample = ch.valid & ~ch.setup & has
            yield ch

    # ------------------------------------------------------------------ position keys, the opening book, duplicates
    def _keyed(self):
        """Generator of (chunk, (key0, canon, mask, canon_action)) as the backend gives them (device tensors on the device), one
        row per entry: the record before the entry, the entry's action as the target.  Rows that were not played key nothing."""
        for ch in self.replay():
            yield ch, self.backend.keys(np.where(ch.valid, ch.index, -1).astype(np.int32), ch.action)

    def keys(self):
        """Generator of Chunks as `replay` gives them, each with key0 / canon uint64 [rows], mask / canon_action int32 [rows]
        beside its fields: the position BEFORE each entry and the entry's action in the canonical frame (rows that were not
        played: 0, 0, 0, -1)."""
        for ch, (key0, canon, mask, action) in self._keyed():
            ch.key0, ch.canon = _host(key0, np.uint64), _host(canon, np.uint64)
            ch.mask, ch.canon_action = _host(mask), _host(action)
            yield ch

    # ------------------------------------------------------------------ one row per record: tactics, life, influence, shapes
    def _per_record(self, attr, call, wrap, stones=False, games=False):
        """Generator of Chunks as `replay` gives them, each with `attr` = wrap(*call(index)) over the records of the chunk (one
        backend call per chunk) and, with stones=True, ch.stones int8 [records, N] (+1 black, -1 white) of the same rows.
        games=True: call(index, first) with the first record of each record's game (-1 where index is)."""
        for ch in self.replay():
            index = self._record_index(ch)
            setattr(ch, attr, wrap(*(call(index, self._record_first(ch)) if games else call(index))))
            if stones:
                ch.stones = np.asarray(self.backend.stones(index), dtype=np.int8)
            yield ch

    def _record_index(self, ch):
        """int32 [records of the chunk]: the record's own index where the replay wrote it, -1 behind a refused entry"""
        index = np.full(len(ch.action) + len(ch.games), -1, np.int32)
        for _, _, base, _, _, played in ch.walk():
            index[base:base + played + 1] = np.arange(base, base + played + 1)
        return index

    def _record_first(self, ch):
        """int32 [records of the chunk]: the first record of the record's game (Chunk.walk's base), -1 behind a refused entry"""
        first = np.full(len(ch.action) + len(ch.games), -1, np.int32)
        for _, _, base, _, _, played in ch.walk():
            first[base:base + played + 1] = base
        return first

    def tactics(self, max_chains=128, stones=False):
        """Generator of Chunks as `replay` gives them, each with `tactics`, a tactics.Tactics with one row per RECORD of the
        chunk (one backend call per chunk): row ch.index[e] is the position before entry e, row ch.index[e] + 1 the position
        after it.  Records that were not written (behind a refused entry) give the zero row.  stones=True adds ch.stones, int8
        [records, N] (+1 black, -1 white), rows as in `tactics`.  The chain table takes 32 * max_chains bytes per record: for a
        large collection give the set a smaller max_entries (the chunk size) or a smaller max_chains."""
        from .tactics import Tactics
        return self._per_record("tactics", lambda index: self.backend.tactics(index, max_chains),
                                lambda libs, n_chains, chains: Tactics(self.S, _host(libs, np.uint8), _host(n_chains), _host(chains)), stones)

    def life(self, stones=False):
        """Generator of Chunks as `replay` gives them, each with `life`, a life.Life with one row per RECORD of the chunk (one
        backend call per chunk): row ch.index[e] is the position before entry e, row ch.index[e] + 1 the position after it.
        Records that were not written (behind a refused entry) give the zero row.  stones=True adds ch.stones as `tactics` does."""
        from .life import Life
        return self._per_record("life", self.backend.life, lambda sets, counts: Life(self.S, _host(sets, np.uint32), _host(counts)), stones)

    def influence(self, dead="life", stones=False, dilate=5, erode_moyo=10, erode_terr=21):
        """Generator of Chunks as `replay` gives them, each with `influence`, an influence.Influence with one row per RECORD of the
        chunk (one backend call per chunk), rows as in `life`.  dead "life": the stones unconditional life proves dead are lifted
        first; None: nothing is lifted.  Records that were not written give the zero row.  stones=True adds ch.stones as `tactics`
        does."""
        from .influence import Influence
        return self._per_record("influence", lambda index: self.backend.influence(index, dead, dilate, erode_moyo, erode_terr),
                                lambda values, sets, counts: Influence(self.S, _host(values, np.int16), _host(sets, np.uint32), _host(counts)),
                                stones)

    def shapes(self, shape):
        """Generator of Chunks as `replay` gives them, each with `shapes`, a shapes.Shapes with one row per RECORD of the chunk
        (one backend call per chunk), rows as in `life`.  Records that were not written give {0, -1, 0, 0}."""
        from .shapes import Shapes
        return self._per_record("shapes", lambda index: self.backend.shapes(index, shape),
                                lambda hits, cover: Shapes(self.S, _host(hits), _host(cover, np.uint32)))

    def secure(self, side=0):
        """Generator of Chunks as `replay` gives them, each with `secure`, a secure.Secure with one row per RECORD of the chunk (one
        backend call per chunk), rows as in `life`: what one more stone of the side to move (side 1: of the other colour) makes
        pass-alive.  Records that were not written give the zero row.  The table takes 8 * N bytes per record.  ch.to_play int8
        [records] is the side to move of each record (+1 black, -1 white; 0 for a record that was not written)."""
        from .secure import Secure
        for ch in self._per_record("secure", lambda index: self.backend.secure(index, side),
                                   lambda table, sets, counts: Secure(self.S, _host(table, np.int16), _host(sets, np.uint32), _host(counts))):
            ch.to_play = _host(self.backend.to_play(self._record_index(ch)), np.int8)
            yield ch

    def solve(self, rules=1, max_region=12, max_nodes=4096, max_targets=16, stones=False):
        """Generator of Chunks as `replay` gives them, each with `solve`, a solve.Solve with one row per RECORD of the chunk (one
        backend call per chunk), rows as in `life`: the enclosed chains of every position and what a bounded reader says of each.
        Records that were not written give n_targets 0.  stones=True adds ch.stones as `tactics` does."""
        from .solve import Solve
        return self._per_record("solve", lambda index: self.backend.solve(index, rules, max_region, max_nodes, max_targets),
                                lambda n_targets, rows, regions: Solve(self.S, _host(n_targets), _host(rows), _host(regions, np.uint32)), stones)

    def race(self, rules=1, max_libs=4, max_region=8, max_nodes=1024, max_pairs=64, stones=False):
        """Generator of Chunks as `replay` gives them, each with `race`, a race.Race with one row per RECORD of the chunk (one backend
        call per chunk), rows as in `life`: the pairs of chains in contact of every position and what a bounded reader says of each
        racer.  Records that were not written give n_pairs 0.  stones=True adds ch.stones as `tactics` does."""
        from .race import Race
        return self._per_record("race", lambda index: self.backend.race(index, rules, max_libs, max_region, max_nodes, max_pairs),
                                lambda n_pairs, rows, regions: Race(self.S, _host(n_pairs), _host(rows), _host(regions, np.uint32)), stones)

    def connect(self, rules=1, cut_libs=1, max_region=8, max_nodes=1024, max_pairs=64, stones=False):
        """Generator of Chunks as `replay` gives them, each with `connect`, a connect.Connect with one row per RECORD of the chunk (one
        backend call per chunk), rows as in `life`: the near pairs of chains of one colour of every position, what a bounded reader
        says of each, and the group map on top.  Records that were not written give n_pairs 0.  stones=True adds ch.stones as
        `tactics` does."""
        from .connect import Connect
        return self._per_record("connect", lambda index: self.backend.connect(index, rules, cut_libs, max_region, max_nodes, max_pairs),
                                lambda n_pairs, rows, regions, groups, counts: Connect(self.S, _host(n_pairs), _host(rows), _host(regions, np.uint32),
                                                                                       _host(groups, np.int16), _host(counts)), stones)

    def superko(self, rule=0):
        """Generator of Chunks as `replay` gives them, each with `superko`, a superko.Superko with one row per RECORD of the chunk (one
        backend call per chunk), rows as in `life`: which moves of every position would repeat an earlier position of ITS game --
        the history of a record is its game's records from the first (Chunk.walk's base) to itself.  Records that were not written
        give the zero row."""
        from .superko import Superko, rule_of
        rule = rule_of(rule)
        return self._per_record("superko", lambda index, first: self.backend.superko(index, first, rule, len(index)),
                                lambda sets, back, counts: Superko(self.S, _host(sets, np.uint32), _host(back, np.int16), _host(counts)), games=True)

    def playouts(self, per_row=16, seed=0, rules=1, max_plies=0, stones=False):
        """Generator of Chunks as `replay` gives them, each with `playouts`, a playout.Playouts with one row per RECORD of the chunk
        (one backend call per chunk), rows as in `life`: per_row light playouts from every position -- ownership, score
        distribution and the all-moves-as-first table of the side to move.  An ESTIMATE, not a proof.  The draws of a row depend
        on its place in the chunk.  Records that were not written give the zero row.  ch.to_play int8 [records] is the side to move
        of each record (+1 black, -1 white; 0 for a record that was not written)."""
        from .playout import Playouts, check_args
        check_args(self.S, per_row, rules, max_plies)
        for ch in self._per_record("playouts", lambda index: self.backend.playouts(index, per_row, seed, rules, max_plies),
                                   lambda own, amaf, sums: Playouts(self.S, _host(own), _host(amaf), _host(sums, np.int64)), stones):
            ch.to_play = _host(self.backend.to_play(self._record_index(ch)), np.int8)
            ch.playouts.white_to_play = ch.to_play < 0
            yield ch

    def uct(self, trees=None, sims=None, seed=0, rules=1, komi=0.0, max_plies=0):
        """Generator of Chunks as `replay` gives them, each with `uct`, a uct.Search with one row per RECORD of the chunk (one backend
        call per chunk), rows as in `life`: the playout tree search from every position -- the root's move table and the move it
        favours.  None: the untuned defaults of uct.py.  An ESTIMATE, not a proof.  The draws of a row depend on its place in the
        chunk.  Records that were not written give the zero row with best None.  ch.to_play as in `playouts`."""
        from . import uct as U
        trees, sims = U.TREES if trees is None else int(trees), U.SIMS if sims is None else int(sims)
        komi2, expand_at = U.komi2_of(komi), min(U.EXPAND_AT, sims)
        U.check_args(self.S, trees, sims, rules, max_plies, komi2, expand_at, U.RAVE_EQUIV, U.PRIOR, sims + 1)
        for ch in self._per_record("uct", lambda index: self.backend.uct(index, trees, sims, seed, rules, max_plies, komi2, expand_at, U.RAVE_EQUIV,
                                                                         U.PRIOR, sims + 1),
                                   lambda visits, wins2, rave, own, sums, info: U.Search(self.S, _host(visits), _host(wins2), _host(rave), _host(own),
                                                                                         _host(sums, np.int64), _host(info))):
            ch.to_play = _host(self.backend.to_play(self._record_index(ch)), np.int8)
            ch.uct.white_to_play = ch.to_play < 0
            yield ch

    # ------------------------------------------------------------------ move outcomes
    def moves(self, side=0):
        """Generator of Chunks as `replay` gives them, each with one row per ENTRY beside its fields (one backend call per chunk):
        played int16 [rows, 8], the row of the move-outcome table (include/sgo.h "move outcomes") for the entry's action in the
        position before it (zero for a pass); move_counts int32 [rows, 8], that position's counts; in_turn bool [rows], the entry's
        colour is the colour the rows were computed for (side 0: the record's side to move -- False for a set-up stone or a move out
        of turn, whose row then describes the other colour's stone).  The table itself, N rows per position, stays on the device:
        only the played rows are copied.  Rows that were not played are zero."""
        for ch in self.replay():
            played, counts, in_turn = self.backend.moves(np.where(ch.valid, ch.index, -1).astype(np.int32), side, ch.action,
                                                         ch.colour if side == 0 else -ch.colour)
            ch.played, ch.move_counts = _host(played, np.int16), _host(counts)
            ch.in_turn = _host(in_turn, bool) & ch.valid
            yield ch

    def find(self, shape):
        """Where a shapes.Shape first occurs in every game, and what was played next.  {"searched", "matched", "games": [{"name",
        "ply" (0 = the empty board, k = after entry k), "variant", "x0", "y0", "next" (a shapes.continuation key)}] of the games
        that hold the shape, "continuations": [{"key", "label", "count", "wins", "losses"}] sorted by count (ties by label)}.
        The move counted is the entry recorded from the first matching position, taken into the frame of the shape as drawn;
        wins / losses are the mover's, by value_targets, where the record has a result."""
        from .shapes import continuation, continuation_label
        games, tally, searched = [], {}, 0
        for ch in self.shapes(shape):
            v = ch.shapes
            for _, g, base, off, _, played in ch.walk():
                searched += 1
                rows = np.flatnonzero(v.hits[base:base + played + 1, 0] > 0)
                if len(rows):
                    ply = int(rows[0])
                    first = v.first(base + ply)
                    e = off + ply
                    has_move = ply < played
                    key = continuation(shape, self.S, first, int(ch.action[e]) if has_move else None, int(ch.colour[e]) if has_move else 0)
                    games.append({"name": self.records[g].name, "ply": ply, "variant": first[0], "x0": first[1], "y0": first[2], "next": key})
                    t = tally.setdefault(key, [0, 0, 0])
                    t[0] += 1
                    if has_move:
                        t[1] += int(ch.z[e] > 0)
                        t[2] += int(ch.z[e] < 0)
        rows = [{"key": k, "label": continuation_label(k), "count": t[0], "wins": t[1], "losses": t[2]} for k, t in tally.items()]
        rows.sort(key=lambda d: (-d["count"], d["label"]))
        return {"searched": searched, "matched": len(games), "games": games, "continuations": rows}

    def book(self, plies=30, min_count=1):
        """Book of the played B / W moves whose node index (the reference's move_n) is below `plies`, grouped by (canon,
        canon_action): count, wins (z = +1 for the mover), losses (z = -1); a record without a decided result counts in count
        only.  Groups with fewer than min_count rows are left out.  Grouped per chunk where the keys are (torch sort / unique),
        merged on the host: the result does not depend on how the set was chunked."""
        import torch
        parts = []
        for ch, (_, canon, _, action) in self._keyed():
            m = ch.valid & ~ch.setup & (ch.node < int(plies))
            if not m.any():
                continue
            winner = np.array([self.records[g].winner or 0 for g in ch.game], np.int32)
            z = np.where(winner == 0, 0, np.where(winner == ch.colour, 1, -1))
            canon, action = _tensor(canon), _tensor(action)
            sel = torch.from_numpy(np.flatnonzero(m)).to(canon.device)
            pair = torch.stack([canon.index_select(0, sel), action.index_select(0, sel).to(torch.int64)], dim=1)
            uniq, inv = torch.unique(pair, dim=0, return_inverse=True)
            tally = torch.from_numpy(np.stack([np.ones(int(m.sum()), np.int64), z[m] > 0, z[m] < 0], axis=1).astype(np.int64)).to(canon.device)
            sums = torch.zeros((uniq.shape[0], 3), dtype=torch.int64, device=canon.device).index_add_(0, inv.reshape(-1), tally)
            parts.append((uniq.cpu().numpy(), sums.cpu().numpy()))
        if not parts:
            return Book(self.S, [], [], [], [], [])
        pairs, sums = np.concatenate([p for p, _ in parts]), np.concatenate([t for _, t in parts])
        key, action = pairs[:, 0].copy().view(np.uint64), pairs[:, 1].astype(np.int32)
        order = np.lexsort((action, key))
        key, action, sums = key[order], action[order], sums[order]
        first = np.ones(len(key), bool)
        first[1:] = (key[1:] != key[:-1]) | (action[1:] != action[:-1])
        at = np.flatnonzero(first)
        sums = np.add.reduceat(sums, at, axis=0)
        keep = sums[:, 0] >= int(min_count)
        return Book(self.S, key[at][keep], action[at][keep], sums[keep, 0], sums[keep, 1], sums[keep, 2])

    def duplicates(self):
        """Groups (lists of record names, in the set's order) of records whose sequences of canonical keys are equal ply for ply:
        one key per record of the replay -- the empty board, the position after every entry, set-up entries included -- the
        same length and the same key everywhere.  A record that was cut short counts with the records it has.  Candidates are
        found by a signature folded on the host, sig = sm(sig ^ canon_j) from sig = 0, and confirmed on the sequences."""
        seqs = {}
        for ch in self.replay():
            games = list(ch.walk())                                                            # records base .. base + played
            index = np.concatenate([base + np.arange(played + 1) for _, _, base, _, _, played in games]).astype(np.int32)
            canon = _host(self.backend.keys(index, None)[1], np.uint64)
            at = 0
            for _, g, _, _, _, played in games:
                seqs[g] = canon[at:at + played + 1].copy()
                at += played + 1
        games = sorted(seqs)
        sig = np.zeros(len(games), np.uint64)
        length = np.array([len(seqs[g]) for g in games], np.int64)
        for j in range(int(length.max()) if len(games) else 0):
            live = np.flatnonzero(length > j)
            sig[live] = sm64(sig[live] ^ np.array([seqs[games[i]][j] for i in live], np.uint64))
        buckets = collections.OrderedDict()
        for i, g in enumerate(games):
            buckets.setdefault((int(length[i]), int(sig[i])), []).append(g)
        out = []
        for cand in buckets.values():
            while len(cand) > 1:                       # confirmed against the first; what differs waits for its own turn
                same = [g for g in cand if np.array_equal(seqs[g], seqs[cand[0]])]
                if len(same) > 1:
                    out.append(same)
                cand = [g for g in cand if g not in same]
        return [[self.records[g].name for g in group] for group in sorted(out)]

    # ------------------------------------------------------------------ the strength measure
    def score(self, net, batch=4096, symmetry="identity", bucket=20, seed=0, keep_policy=False):
        """Runs the net on every recorded move's position (slices of `batch` rows of the sample index list) and scores it.
        Returns {"buckets": [dict per bucket], "total": dict, "rows": {per-row numpy arrays}, "bucket_width", "net_calls"}.
        Rows: every played B / W move (set-up stones are no rows); z = 0 where the result is unknown."""
        import torch
        be = self.backend
        assert symmetry in ("identity", "random1") or symmetry in range(8)
        width = int(bucket)
        top = max([max([n for n, s in zip(r.nodes, r.setup) if not s] + [0]) for r in self.records] + [0])
        n_buckets = top // width + 1
        counters = torch.zeros((n_buckets, 8), dtype=torch.int64, device=be.device)
        rng = pyrandom.Random(seed)
        keep = {k: [] for k in ("index", "game", "node", "action", "z", "bucket", "rank", "best", "p_target", "flags", "value", "sym_k")}
        if keep_policy:
            keep["policy"] = []
        scratch, calls = {}, 0
        for ch in self.replay():
            m = ch.valid & ~ch.setup
            n = int(m.sum())
            if n == 0:
                continue
            z = ch.z[m].astype(np.int32)
            if self.compat_unknown_result:     # the compat label is a sample's, not a result: the rows of an unknown result stay z = 0
                unknown = np.array([self.records[g].winner is None for g in ch.game[m]], bool)
                z[unknown] = 0
            bk = (ch.node[m] // width).astype(np.int32)
            d_index, d_target = torch.from_numpy(ch.index[m]).to(be.device), torch.from_numpy(ch.action[m]).to(be.device)
            d_z, d_bucket = torch.from_numpy(z).to(be.device), torch.from_numpy(bk).to(be.device)
            d_rank, d_best = torch.empty(n, dtype=torch.int32, device=be.device), torch.empty(n, dtype=torch.int32, device=be.device)
            d_pt, d_flags = torch.empty(n, dtype=torch.float32, device=be.device), torch.empty(n, dtype=torch.int32, device=be.device)
            d_value = torch.empty(n, dtype=torch.float32, device=be.device)
            ks = np.zeros(n, np.int32)
            for lo in range(0, n, int(batch)):
                hi = min(n, lo + int(batch))
                k = 0 if symmetry == "identity" else (rng.randrange(8) if symmetry == "random1" else int(symmetry))
                p, v = be.forward(net, d_index[lo:hi], hi - lo, k, scratch)
                assert tuple(p.shape) == (hi - lo, self.A)
                d_value[lo:hi] = v
                be.score(hi - lo, d_index[lo:hi], d_target[lo:hi], d_z[lo:hi], d_bucket[lo:hi], n_buckets, p, v, k, d_rank[lo:hi],
                         d_best[lo:hi], d_pt[lo:hi], d_flags[lo:hi], counters)
                ks[lo:hi] = k
                calls += 1
                if keep_policy:
                    keep["policy"].append(p.cpu().numpy())
            for name, arr in (("index", ch.index[m]), ("game", ch.game[m]), ("node", ch.node[m]), ("action", ch.action[m]), ("z", z), ("bucket", bk),
                              ("rank", d_rank.cpu().numpy()), ("best", d_best.cpu().numpy()), ("p_target", d_pt.cpu().numpy()),
                              ("flags", d_flags.cpu().numpy()), ("value", d_value.cpu().numpy()), ("sym_k", ks)):
                keep[name].append(arr)
        empty = {"policy": np.zeros((0, self.A), np.float32), "p_target": np.zeros(0, np.float32), "value": np.zeros(0, np.float32)}
        rows = {k: (np.concatenate(v) if v else empty.get(k, np.zeros(0, np.int32))) for k, v in keep.items()}
        ce, se = float_sums(rows["p_target"], rows["value"], rows["z"], rows["bucket"], n_buckets)
        buckets, total = tables(counters.cpu().numpy(), ce, se, width)
        return {"buckets": buckets, "total": total, "rows": rows, "bucket_width": width, "net_calls": calls,
                "net": getattr(net, "name", str(net)), "refused": list(self.refused)}

    # ------------------------------------------------------------------ supervised samples
    def write_samples(self, root):
        """root/KGS/<game>/move_%03d/sample.h5 for every move that gives a sample.  Returns {"games", "samples", "existing":
        [names left alone], "empty": [names without a sample]}."""
        from .sgfsave import _write_sample_arrays
        out = {"games": 0, "samples": 0, "existing": [], "empty": []}
        for ch in self.replay():
            todo = []
            for g in ch.games:
                name = self.records[g].name
                rows = np.flatnonzero(ch.sample & (ch.game == g))
                if os.path.isdir(os.path.join(root, "KGS", name)):          # KGSSelfPlayWorker.py:32-33
                    out["existing"].append(name)
                elif len(rows) == 0:
                    out["empty"].append(name)
                else:
                    todo.append((name, rows))
            if not todo:
                continue
            allrows = np.concatenate([rows for _, rows in todo])
            boards = self.backend.boards(ch.index[allrows])
            at = 0
            for name, rows in todo:
                for r in rows:
                    directory = os.path.join(root, "KGS", name, "move_%03d" % int(ch.node[r]))
                    os.makedirs(directory, exist_ok=True)
                    pol = np.zeros(self.A, np.float32)
                    pol[int(ch.action[r])] = 1.0                             # the pass is the last entry
                    _write_sample_arrays(directory, boards[at:at + 1].astype(np.float32), pol, np.array(ch.z[r], dtype=np.float32))
                    at += 1
                out["games"] += 1
                out["samples"] += len(rows)
        return out


def life_lines(record_set):
    """[{"name", "plies", "first_alive", "unsettled"}] per game from one RecordSet.life pass: the number of entries played, the
    first ply (0 = the empty board, k = after entry k) whose position has a non-empty alive set (None: none), and `unsettled` of
    the position after the last played entry."""
    out = []
    for ch in record_set.life():
        for _, g, base, _, _, played in ch.walk():
            rows = ch.life.counts[base:base + played + 1]
            alive = np.flatnonzero((rows[:, 0] + rows[:, 1]) > 0)
            out.append({"name": record_set.records[g].name, "plies": played, "first_alive": int(alive[0]) if len(alive) else None,
                        "unsettled": int(rows[-1, 6])})
    return out


def influence_table(record_set, width=20, dead="life"):
    """The figures of `--influence` from one RecordSet.influence pass (the classical territory triple).  {"buckets": [{"first_ply",
    "positions", "abs_margin", "neutral", "moyo_beyond_black", "moyo_beyond_white"}] per `width` plies (ply 0 = the position before
    the first entry): the means of |margin|, of neutral and of |moyo| - |territory| per colour; "games": [{"name", "plies",
    "margin"}]: the margin (the estimate before komi; a Record keeps no komi) of the position after the last played entry}."""
    sums, games = {}, []
    for ch in record_set.influence(dead=dead):
        for _, g, base, _, _, played in ch.walk():
            rows = ch.influence.counts[base:base + played + 1].astype(np.int64)
            for k in range(0, played + 1, width):
                part = rows[k:k + width]
                s = sums.setdefault(k // width, np.zeros(5, np.int64))
                s += [len(part), int(np.abs(part[:, 7]).sum()), int(part[:, 6].sum()), int((part[:, 2] - part[:, 0]).sum()),
                      int((part[:, 3] - part[:, 1]).sum())]
            games.append({"name": record_set.records[g].name, "plies": played, "margin": int(rows[-1, 7])})
    buckets = [{"first_ply": b * width, "positions": int(s[0]), "abs_margin": float(s[1]) / int(s[0]), "neutral": float(s[2]) / int(s[0]),
                "moyo_beyond_black": float(s[3]) / int(s[0]), "moyo_beyond_white": float(s[4]) / int(s[0])} for b, s in sorted(sums.items())]
    return {"buckets": buckets, "games": games}


def moves_table(record_set, width=20):
    """The table of `--moves` (moves.bucket_table) from one RecordSet.moves pass: per bucket of `width` moves the share of the played
    moves that capture / give atari / escape / are self-atari beside the mean share of the allowed moves of the same positions
    that do, the forbidden-sound points and the positions that had any.  Set-up stones and moves out of turn are left out."""
    from .moves import bucket_table
    ply, action, played, counts = [], [], [], []
    for ch in record_set.moves():
        keep = ch.in_turn & ~ch.setup
        first = {}
        number = np.zeros(len(ch.action), np.int64)                  # the move number inside the game, set-up stones not counted
        for e in np.flatnonzero(ch.valid & ~ch.setup):
            g = int(ch.game[e])
            number[e] = first.get(g, 0)
            first[g] = number[e] + 1
        ply.append(number[keep])
        action.append(ch.action[keep])
        played.append(ch.played[keep])
        counts.append(ch.move_counts[keep])
    if not ply:
        return []
    return bucket_table(np.concatenate(ply), np.concatenate(action), np.concatenate(played), np.concatenate(counts), record_set.S, width)


def secure_table(record_set, width=20):
    """The table of `--secure` (secure.bucket_table) from one RecordSet.secure pass: per bucket of `width` moves the positions in
    which something is proved already, the positions that offer a securing move of gain >= 2, how often the recorded move took the
    best one or any, and the harmful moves played.  Set-up stones and moves out of turn are left out."""
    from .secure import bucket_table
    ply, action, played, counts = [], [], [], []
    for ch in record_set.secure():
        v = ch.secure
        first = {}
        for e in np.flatnonzero(ch.valid & ~ch.setup):
            g, r, a = int(ch.game[e]), int(ch.index[e]), int(ch.action[e])
            number = first.get(g, 0)
            first[g] = number + 1
            if int(ch.to_play[r]) != int(ch.colour[e]):
                continue
            ply.append(number)
            action.append(a)
            played.append(v.table[r, a] if 0 <= a < v.N else np.zeros(4, np.int16))
            counts.append(v.counts[r])
    if not ply:
        return []
    return bucket_table(np.array(ply), np.array(action), np.stack(played), np.stack(counts), record_set.S, width)


def solve_table(record_set, width=20, **kw):
    """The table of `--solve` (solve.bucket_table) from one RecordSet.solve pass: per bucket of `width` moves the positions that
    hold an unsettled enclosed chain, how often the recorded move was its kill or live move, and the share of unknown rows.  Set-up
    stones are left out."""
    from .solve import bucket_table
    ply, action, rows, n_targets = [], [], [], []
    for ch in record_set.solve(**kw):
        v = ch.solve
        first = {}
        for e in np.flatnonzero(ch.valid & ~ch.setup):
            g, r = int(ch.game[e]), int(ch.index[e])
            number = first.get(g, 0)
            first[g] = number + 1
            ply.append(number)
            action.append(int(ch.action[e]))
            rows.append(v.rows[r])
            n_targets.append(v.n_targets[r])
    if not ply:
        return []
    return bucket_table(np.array(ply), np.array(action), np.stack(rows), np.array(n_targets), width)


def race_table(record_set, width=20, **kw):
    """The table of `--race` (race.bucket_table) from one RecordSet.race pass: per bucket of `width` moves the pairs per position,
    the share of racers of each verdict, and how often the recorded move was a listed catching or saving move of the mover.  Set-up
    stones are left out."""
    from .race import bucket_table
    ply, action, colour, rows, n_pairs = [], [], [], [], []
    for ch in record_set.race(**kw):
        v = ch.race
        first = {}
        for e in np.flatnonzero(ch.valid & ~ch.setup):
            g, r = int(ch.game[e]), int(ch.index[e])
            number = first.get(g, 0)
            first[g] = number + 1
            ply.append(number)
            action.append(int(ch.action[e]))
            colour.append(int(ch.colour[e]))
            rows.append(v.rows[r])
            n_pairs.append(v.n_pairs[r])
    if not ply:
        return []
    return bucket_table(np.array(ply), np.array(action), np.array(colour), np.stack(rows), np.array(n_pairs), record_set.S * record_set.S, width)


def connect_table(record_set, width=20, **kw):
    """The table of `--connect` (connect.bucket_table) from one RecordSet.connect pass: per bucket of `width` moves the near pairs per
    position, the share of each verdict among them, and the groups per position beside the chains per position.  Set-up stones are
    left out."""
    from .connect import bucket_table
    ply, rows, n_pairs, counts = [], [], [], []
    for ch in record_set.connect(**kw):
        v = ch.connect
        first = {}
        for e in np.flatnonzero(ch.valid & ~ch.setup):
            g, r = int(ch.game[e]), int(ch.index[e])
            number = first.get(g, 0)
            first[g] = number + 1
            ply.append(number)
            rows.append(v.rows[r])
            n_pairs.append(v.n_pairs[r])
            counts.append(v.group_counts[r])
    if not ply:
        return []
    return bucket_table(np.array(ply), np.stack(rows), np.array(n_pairs), np.stack(counts), width)


def superko_report(record_set, rule=0, width=20):
    """What `--superko` prints, from one RecordSet.superko pass: {"rule", "games": [superko.game_report per game], "buckets":
    superko.bucket_table over every written record (ply = the number of entries before it), "positions_with_extra", "max_back"}."""
    from .superko import bucket_table, game_report, rule_of
    rule = rule_of(rule)
    games, ply, extra, max_back = [], [], [], 0
    for ch in record_set.superko(rule):
        v = ch.superko
        for _, g, base, off, _, played in ch.walk():
            games.append(game_report(record_set.records[g].name, v, base, played, ch.action[off:off + played]))
            ply += list(range(played + 1))
            extra += [int(c) for c in v.counts[base:base + played + 1, 1]]
            max_back = max([max_back] + [int(c) for c in v.counts[base:base + played + 1, 2]])
    return {"rule": ("positional", "situational")[rule], "games": games, "buckets": bucket_table(ply, extra, width) if ply else [],
            "positions_with_extra": int(sum(1 for c in extra if c > 0)), "max_back": max_back}


def playout_report(record_set, per_row=16, width=20, seed=0):
    """What `--playouts R` prints, from one RecordSet.playouts pass (rules 1, the default cap): {"per_row", "games": [{"name", "plies",
    "lead", "sd", "capped", "result"}] with the playout score (black - white, komi-free) of each game's LAST position beside the
    recorded result, "buckets": playout.bucket_table over every written record (ply = the number of entries before it)}.  An
    estimate from uniformly random playouts, not a verdict."""
    from .playout import bucket_table
    games, ply, mean, sd, capped = [], [], [], [], []
    for ch in record_set.playouts(per_row=per_row, seed=seed):
        v = ch.playouts
        for _, g, base, off, _, played in ch.walk():
            last = base + played
            w = record_set.records[g].winner
            games.append({"name": record_set.records[g].name, "plies": played, "lead": v.score_mean(last), "sd": v.score_sd(last),
                          "capped": v.capped_share(last), "result": "B" if w == 1 else "W" if w == -1 else "?"})
            for r in range(base, last + 1):
                ply.append(r - base)
                mean.append(v.score_mean(r))
                sd.append(v.score_sd(r))
                capped.append(v.capped_share(r))
    return {"per_row": int(per_row), "games": games, "buckets": bucket_table(ply, mean, sd, capped, width) if ply else []}


def format_bucket(d, label):
    def pct(a, b):
        return "%5.1f%%" % (100.0 * a / b) if b else "    - "
    ce = "%7.4f" % d["cross_entropy"] if d["cross_entropy"] is not None else "    -  "
    mse = "%6.4f" % d["value_mse"] if d["value_mse"] is not None else "   -  "
    return "%-9s rows %7d  top1 %s  top5 %s  illegal %5d  ce %s  value %s of %7d  mse %s" % (
        label, d["rows"], pct(d["top1"], d["rows"]), pct(d["top5"], d["rows"]), d["illegal"], ce,
        pct(d["value_agree"], d["value_rows"]), d["value_rows"], mse)


def _net(kind, size):
    if kind == "best":
        from .predicting_queue_worker import get_model, init_predicting_workers
        init_predicting_workers(conf['GPUs'][:1])
        return get_model("BEST")
    from .stub_nets import make_stub
    return make_stub(kind, size)


def main(argv=None, out=sys.stdout):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("path", nargs="?", default=None, help="an .sgf file or a directory of them (default: conf['KGS_DATA_DIR'])")
    ap.add_argument("--size", type=int, default=None, help="board size (default: conf['SIZE']); other records are skipped")
    ap.add_argument("--samples", default=None, help="write OUT/KGS/<game>/move_%%03d/sample.h5")
    ap.add_argument("--score", action="store_true", help="score the net on the recorded moves")
    ap.add_argument("--net", default="best", choices=["best", "hash", "uniform", "table"],
                    help="best: the model the configuration names; hash / uniform / table: the stub nets (no weights needed)")
    ap.add_argument("--symmetry", default="identity", help="identity, random1 (one of the eight per net call) or 0..7")
    ap.add_argument("--bucket", type=int, default=20, help="moves per bucket of the score table")
    ap.add_argument("--batch", type=int, default=4096, help="positions per net call")
    ap.add_argument("--json", default=None, help="write the counts and figures as one JSON document to this file")
    ap.add_argument("--compat-unknown-result", action="store_true",
                    help="label the moves of a record without a decided result -1, as the reference does, instead of leaving them out")
    ap.add_argument("--book", default=None, help="write the opening book of the records to this .npz")
    ap.add_argument("--book-plies", type=int, default=30, help="moves whose node index is below N enter the book (default 30)")
    ap.add_argument("--duplicates", action="store_true", help="list the records that are one game, in any orientation")
    ap.add_argument("--life", action="store_true",
                    help="per game: plies, the first ply with an unconditionally alive stone (or -), unsettled points at the last ply")
    ap.add_argument("--find", default=None, metavar="SHAPE.txt",
                    help="search every position for the shape drawn in this file (shapes.Shape.parse): games matched / searched and "
                         "the table of the moves played next")
    ap.add_argument("--moves", action="store_true",
                    help="per 20-move bucket: the share of the played moves that capture / give atari / escape / are self-atari beside "
                         "the mean share of the allowed moves of the same positions that do, and the points the inherited legal-move "
                         "rule forbids although the stone would stand")
    ap.add_argument("--secure", action="store_true",
                    help="per 20-move bucket: the positions that offer a securing move (one more stone that makes at least 2 more stones "
                         "and points pass-alive), how often the recorded move took the best one or any, and the harmful moves played")
    ap.add_argument("--solve", action="store_true",
                    help="life and death by a bounded reader: per 20-move bucket the positions that hold an unsettled enclosed chain, how "
                         "often the recorded move was its kill or live move, and the share of rows that ended unknown")
    ap.add_argument("--race", action="store_true",
                    help="capturing races by a bounded reader: per 20-move bucket the pairs of chains in contact per position, the share of "
                         "racers that are safe / unsettled / caught / unknown, and how often the recorded move was a listed catching or "
                         "saving move")
    ap.add_argument("--connect", action="store_true",
                    help="connections by a bounded reader: per 20-move bucket the near pairs of chains of one colour per position, the "
                         "share that is connected / unsettled / cut / unknown / open, and the groups per position beside the chains per "
                         "position")
    ap.add_argument("--influence", action="store_true",
                    help="Bouzy's influence map of every position (an estimate; proved-dead stones lifted): per 20-move bucket the "
                         "mean |margin|, mean neutral points and mean moyo beyond territory per colour; per game the estimate at "
                         "the last position")
    ap.add_argument("--superko", nargs="?", const="positional", default=None, choices=("positional", "situational"),
                    help="which moves would repeat an earlier position of their game: per game the first move that reached a position "
                         "seen before (passes apart) and every played move that the ko approximation let through although it repeats; "
                         "the ko recaptures played through; per 20-move bucket the share of positions where superko forbids a move "
                         "the inherited rule allows")
    ap.add_argument("--playouts", type=int, default=None, metavar="R",
                    help="R light playouts from every position (uniformly random moves that spare the mover's eyes, no net): per "
                         "20-move bucket the mean |score|, its standard deviation and the share of playouts the ply cap ended; per game "
                         "the estimate at the last position beside the recorded result.  An estimate, not a verdict")
    a = ap.parse_args(argv)
    size = a.size or conf['SIZE']
    symmetry = a.symmetry if a.symmetry in ("identity", "random1") else int(a.symmetry)
    records, skipped = read_path(a.path or conf['KGS_DATA_DIR'], size)
    out.write("records %d  skipped: unreadable %d, wrong size %d, too long %d\n" % (
        len(records), len(skipped["unreadable"]), len(skipped["wrong_size"]), len(skipped["too_long"])))
    doc = {"size": size, "records": len(records), "skipped": skipped}
    if not records:
        return 0
    rs = RecordSet(records, size, compat_unknown_result=a.compat_unknown_result)
    try:
        if a.samples:
            w = rs.write_samples(a.samples)
            out.write("samples %d of %d games  (%d game directories existed, %d games without a sample)\n" % (
                w["samples"], w["games"], len(w["existing"]), len(w["empty"])))
            doc["samples"] = w
        if a.score:
            net = _net(a.net, size)
            try:
                res = rs.score(net, batch=a.batch, symmetry=symmetry, bucket=a.bucket)
            finally:
                if a.net == "best":
                    from .predicting_queue_worker import destroy_predicting_workers
                    destroy_predicting_workers(conf['GPUs'][:1])
            for d in res["buckets"]:
                out.write(format_bucket(d, "%d-%d" % (d["first_move"], d["first_move"] + a.bucket - 1)) + "\n")
            out.write(format_bucket(res["total"], "total") + "\n")
            doc["score"] = {"net": res["net"], "bucket_width": a.bucket, "buckets": res["buckets"], "total": res["total"]}
        if a.book:
            book = rs.book(plies=a.book_plies)
            book.save(a.book)
            out.write("book %d entries in %d positions from %d moves (plies < %d) -> %s\n" % (
                len(book), len(np.unique(book.key)), int(book.count.sum()), a.book_plies, a.book))
            doc["book"] = {"file": a.book, "plies": a.book_plies, "entries": len(book), "positions": int(len(np.unique(book.key))),
                           "moves": int(book.count.sum())}
        if a.duplicates:
            groups = rs.duplicates()
            for names in groups:
                out.write("duplicates: %s\n" % " ".join(names))
            out.write("duplicate groups %d\n" % len(groups))
            doc["duplicates"] = groups
        if a.life:
            doc["life"] = life_lines(rs)
            for d in doc["life"]:
                out.write("life %s plies %d first_alive %s unsettled %d\n" % (
                    d["name"], d["plies"], "-" if d["first_alive"] is None else "%d" % d["first_alive"], d["unsettled"]))
        if a.find:
            from .shapes import Shape
            with open(a.find) as f:
                found = rs.find(Shape.parse(f.read()))
            out.write("find %s: games matched %d / searched %d\n" % (a.find, found["matched"], found["searched"]))
            for d in found["continuations"]:
                out.write("find next %-10s count %d wins %d losses %d\n" % (d["label"], d["count"], d["wins"], d["losses"]))
            doc["find"] = {"matched": found["matched"], "searched": found["searched"],
                           "games": [dict(d, next=list(d["next"])) for d in found["games"]],
                           "continuations": [dict(d, key=list(d["key"])) for d in found["continuations"]]}
        if a.secure:
            from .secure import format_bucket_table as format_secure_table
            doc["secure"] = secure_table(rs, a.bucket)
            if doc["secure"]:
                out.write(format_secure_table(doc["secure"]) + "\n")
            out.write("secure: %d of %d positions offer a securing move; the recorded move took the best %d times, any %d times; harmful moves played %d\n" % (
                sum(r["offered"] for r in doc["secure"]), sum(r["plies"] for r in doc["secure"]), sum(r["took_best"] for r in doc["secure"]),
                sum(r["took_any"] for r in doc["secure"]), sum(r["harmful_played"] for r in doc["secure"])))
        if a.solve:
            from .solve import format_bucket_table as format_solve_table
            doc["solve"] = solve_table(rs, a.bucket)
            if doc["solve"]:
                out.write(format_solve_table(doc["solve"]) + "\n")
            out.write("solve: %d of %d positions hold an unsettled enclosed chain; the recorded move was its kill or live move %d times; unknown rows %d of %d\n" % (
                sum(r["unsettled"] for r in doc["solve"]), sum(r["plies"] for r in doc["solve"]), sum(r["took"] for r in doc["solve"]),
                sum(r["unknown"] for r in doc["solve"]), sum(r["rows"] for r in doc["solve"])))
        if a.race:
            from .race import format_bucket_table as format_race_table
            doc["race"] = race_table(rs, a.bucket)
            if doc["race"]:
                out.write(format_race_table(doc["race"]) + "\n")
            out.write("race: %d pairs in %d positions; %d positions offered the mover a catching or saving move; the recorded move was one %d times; unknown racers %d of %d\n" % (
                sum(r["pairs"] for r in doc["race"]), sum(r["plies"] for r in doc["race"]), sum(r["chances"] for r in doc["race"]),
                sum(r["took"] for r in doc["race"]), sum(r["unknown"] for r in doc["race"]), sum(r["racers"] for r in doc["race"])))
        if a.connect:
            from .connect import format_bucket_table as format_connect_table
            doc["connect"] = connect_table(rs, a.bucket)
            if doc["connect"]:
                out.write(format_connect_table(doc["connect"]) + "\n")
            tot = lambda k: sum(r[k] for r in doc["connect"])                            # noqa: E731
            out.write("connect: %d pairs in %d positions (%d found, %d tables cut); connected %d unsettled %d cut %d unknown %d open %d; %d chains in %d groups\n" % (
                tot("pairs"), tot("plies"), tot("found"), tot("cut_tables"), tot("connected"), tot("unsettled"), tot("cut"), tot("unknown"),
                tot("open"), tot("chains"), tot("groups")))
        if a.moves:
            from .moves import format_bucket_table
            doc["moves"] = moves_table(rs, a.bucket)
            if doc["moves"]:
                out.write(format_bucket_table(doc["moves"]) + "\n")
            out.write("moves: forbidden-sound points %d in %d positions\n" % (
                sum(r["forbidden_sound"] for r in doc["moves"]), sum(r["positions_forbidden"] for r in doc["moves"])))
        if a.influence:
            from .influence import score_text
            doc["influence"] = influence_table(rs, a.bucket)
            for d in doc["influence"]["buckets"]:
                out.write("influence %d-%d positions %d  |margin| %.1f  neutral %.1f  moyo beyond territory black %.1f white %.1f\n" % (
                    d["first_ply"], d["first_ply"] + a.bucket - 1, d["positions"], d["abs_margin"], d["neutral"], d["moyo_beyond_black"],
                    d["moyo_beyond_white"]))
            for d in doc["influence"]["games"]:
                out.write("influence %s plies %d estimate %s\n" % (d["name"], d["plies"], score_text(d["margin"])))
        if a.superko:
            from .superko import format_report
            from .review import vertex
            doc["superko"] = superko_report(rs, a.superko, a.bucket)
            out.write("superko (%s)\n" % doc["superko"]["rule"])
            out.write(format_report(doc["superko"]["games"], doc["superko"]["buckets"], lambda p: vertex(p, size)) + "\n")
        if a.playouts:
            from .playout import format_report as format_playouts
            doc["playouts"] = playout_report(rs, a.playouts, a.bucket)
            out.write("playouts (%d per position; an estimate)\n" % a.playouts)
            out.write(format_playouts(doc["playouts"]["games"], doc["playouts"]["buckets"]) + "\n")
        doc["refused"] = [list(t) for t in rs.refused]
        for name, status, at in rs.refused:
            out.write("record %s cut short at entry %d (status %d)\n" % (name, at, status))
    finally:
        rs.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
