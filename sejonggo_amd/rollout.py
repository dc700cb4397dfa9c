"""Policy rollouts on the device (include/sgo.h "policy rollouts", csrc/sgo_rollout.hip): how a game ended.

A position is played out many times with the net's policy -- thousands of tree-less games advance one sampled move per net
call -- and every point is counted for the colour that holds it at the end.  `RolloutEngine.run` drives the loop
list -> net -> step; the functions below turn one source's counts into the answers of GTP's final_score and
final_status_list with integer thresholds.  PyTorch is plumbing here (device memory, stream, the net); the rollouts are HIP.
"""
import ctypes as C
import random as pyrandom

import numpy as np

from . import _lib
from .conf import conf

SUMS = ("black_wins", "white_wins", "draws", "score_sum", "score_sq_sum", "plies_sum", "capped", "rollouts")


class RolloutEngine(object):
    """`max_rollouts` resident rollouts from at most `max_sources` positions at once.  net: the model contract of the engine
    (engine.SelfPlayEngine): `predict_packed` when the net reads packed records, `predict_on_batch` on board tensors otherwise.
    symmetry: "identity", "random1" (one of the seven SYMMETRIES per step, drawn from the run's seed) or a fixed k."""

    def __init__(self, net, size=None, max_rollouts=4096, max_sources=None, device=0, symmetry="identity"):
        import torch
        self.torch = torch
        self.lib = _lib.require_gpu()
        self.net = net
        self.S = size or conf['SIZE']
        self.N = self.S * self.S
        self.A = self.N + 1
        self.max_rollouts = int(max_rollouts)
        self.max_sources = int(max_sources or max_rollouts)
        assert symmetry in ("identity", "random1") or symmetry in range(8)
        self.symmetry = symmetry
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.RW = self.lib.sgo_packed_words(self.S)
        self.h = C.c_void_p(self.lib.sgo_rollout_create(self.S, self.max_rollouts, self.max_sources, device))
        if not self.h:
            raise _lib.SgoError("sgo_rollout_create failed: %s" % self.lib.sgo_last_error().decode())
        self.packed = bool(getattr(net, "packed_ok", False))
        self.layout = 2 if getattr(net, "in_channels", 17) == 32 else 0
        self.nn_in = None                      # the board-tensor route's input, allocated on first use
        self.status = _lib.RolloutStatus()
        self.n_net_calls = 0
        self.n_net_positions = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.sgo_rollout_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ the three starts
    def start(self, records, per_src, seed=0, max_plies=None):
        """HOST packed records uint32 [n_src, RW]."""
        records = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, self.RW)
        _lib.check(self.lib.sgo_rollout_start(self.h, len(records), _lib.ptr(records), int(per_src), int(seed) & 0xFFFFFFFF,
                                              int(max_plies or 0), _lib.stream_ptr()), "sgo_rollout_start")
        return len(records)

    def start_dev(self, records, index, per_src, seed=0, max_plies=None, n_src=None):
        """DEVICE records (a uint32 / int32 tensor [m, RW]) and an optional int32 index tensor: source s = record index[s]."""
        n = int(n_src if n_src is not None else (len(index) if index is not None else records.shape[0]))
        _lib.check(self.lib.sgo_rollout_start_dev(self.h, n, _lib.ptr(records), _lib.ptr(index), int(per_src), int(seed) & 0xFFFFFFFF,
                                                  int(max_plies or 0), _lib.stream_ptr()), "sgo_rollout_start_dev")
        return n

    def start_sessions(self, session_engine, slots, per_src, seed=0, max_plies=None):
        """The root positions of holding session slots of an engine.SessionEngine.  Returns the status per slot; raises SgoError
        (nothing starts) when one of them is not a holding session."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        self.session_status = np.zeros(len(slots), np.int32)
        _lib.check(self.lib.sgo_rollout_start_sessions(self.h, session_engine.ctx, len(slots), _lib.ptr(slots), int(per_src),
                                                       int(seed) & 0xFFFFFFFF, int(max_plies or 0), _lib.ptr(self.session_status),
                                                       _lib.stream_ptr()), "sgo_rollout_start_sessions")
        return len(slots)

    def source_records(self, n_src, per_src):
        """The source positions as packed records uint32 [n_src, RW], read from the first clone of each.  Valid between a start
        and the first step (the steps overwrite the clones)."""
        class _Mem(object):
            pass
        rec = C.c_void_p()
        _lib.check(self.lib.sgo_rollout_list(self.h, C.byref(rec), None), "sgo_rollout_list")
        m = _Mem()
        m.__cuda_array_interface__ = {"shape": (n_src, per_src, self.RW), "typestr": "<i4", "data": (rec.value, False), "version": 2}
        t = self.torch.as_tensor(m, device=self.device)[:, 0, :]
        return t.cpu().numpy().view(np.uint32).reshape(n_src, self.RW)

    # ------------------------------------------------------------------ the loop
    def _forward(self, n, k):
        torch = self.torch
        rec, idx = C.c_void_p(), C.c_void_p()
        _lib.check(self.lib.sgo_rollout_list(self.h, C.byref(rec), C.byref(idx)), "sgo_rollout_list")
        self.n_net_calls += 1
        self.n_net_positions += n
        if self.packed:
            p, _ = self.net.predict_packed(rec.value, idx.value, n, k)
        else:
            if self.nn_in is None:
                self.nn_in = torch.zeros((self.max_rollouts, self.S, self.S, 32 if self.layout == 2 else 17), dtype=torch.float16,
                                         device=self.device)
            _lib.check(self.lib.sgo_nn_pack_dev(C.c_int(self.S), C.c_int(n), rec, idx, C.c_int(k), C.c_int(self.layout), C.c_int(0),
                                                _lib.ptr(self.nn_in), _lib.stream_ptr()), "sgo_nn_pack_dev")
            p, _ = self.net.predict_on_batch(self.nn_in[:n])
        return p.to(torch.float32).contiguous()

    def step(self, k=0):
        """One ply of every live rollout: the net on the list, then sgo_rollout_step.  Returns the status."""
        n = self.status.n_live
        policy = self._forward(n, k)
        assert tuple(policy.shape) == (n, self.A)
        _lib.check(self.lib.sgo_rollout_step(self.h, _lib.ptr(policy), int(k), _lib.stream_ptr(), C.byref(self.status)),
                   "sgo_rollout_step")
        return self.status

    def result(self, n_src, steps=0):
        black, white = np.zeros((n_src, self.N), np.int32), np.zeros((n_src, self.N), np.int32)
        sums = np.zeros((n_src, 8), np.int64)
        _lib.check(self.lib.sgo_rollout_result(self.h, int(n_src), _lib.ptr(black), _lib.ptr(white), _lib.ptr(sums)),
                   "sgo_rollout_result")
        out = {"black_own": black, "white_own": white, "sums": sums, "steps": int(steps)}
        for j, name in enumerate(SUMS):
            out[name] = sums[:, j].copy()
        return out

    def run(self, records=None, sessions=None, per_src=None, seed=0, max_plies=None, device_records=None):
        """Plays `per_src` rollouts from every source to the end.  Sources: `records` (host packed records), `sessions` =
        (session_engine, slots), or `device_records` = (records tensor, index tensor or None).  Returns a dict of numpy arrays --
        black_own / white_own int32 [n_src, S*S], sums int64 [n_src, 8] and its columns by name (SUMS) -- plus `steps` and `records`,
        the packed source records uint32 [n_src, RW] (engine.unpack_positions expands them)."""
        per_src = int(per_src or conf.get('ROLLOUTS', 64))
        if (records is not None) + (sessions is not None) + (device_records is not None) != 1:
            raise ValueError("run: exactly one of records, sessions, device_records")
        if records is not None:
            n_src = self.start(records, per_src, seed, max_plies)
        elif sessions is not None:
            n_src = self.start_sessions(sessions[0], sessions[1], per_src, seed, max_plies)
        else:
            n_src = self.start_dev(device_records[0], device_records[1], per_src, seed, max_plies)
        sources = self.source_records(n_src, per_src)
        rng = pyrandom.Random(seed)
        self.status.n_live, self.status.n_done, self.status.steps = n_src * per_src, 0, 0
        while self.status.n_live > 0:
            k = 0 if self.symmetry == "identity" else (rng.randrange(7) if self.symmetry == "random1" else int(self.symmetry))
            self.step(k)
        out = self.result(n_src, self.status.steps)
        out["records"] = sources
        return out


# ---------------------------------------------------------------------- pure functions on one source's counts
def result_row(result, i):
    """Source i of a `run` result as a dict of its own: black_own / white_own [S*S], the sums by name."""
    row = {"black_own": np.asarray(result["black_own"][i]), "white_own": np.asarray(result["white_own"][i])}
    for name in SUMS:
        row[name] = int(result[name][i])
    return row


def point_owner(row):
    """int8 [S*S]: +1 black's, -1 white's, 0 unsettled.  With R rollouts a point is black's if 3 * black_own >= 2 * R, white's
    likewise (the two cannot both hold: black_own + white_own <= R)."""
    R = int(row["rollouts"])
    b, w = np.asarray(row["black_own"], dtype=np.int64), np.asarray(row["white_own"], dtype=np.int64)
    out = np.zeros(b.shape, dtype=np.int8)
    if R > 0:
        out[3 * b >= 2 * R] = 1
        out[3 * w >= 2 * R] = -1
    return out


def stone_status(row, board):
    """{"alive", "dead", "seki"}: sets of actions (y * S + x) of the stones on `board` (+1 black, -1 white, 0 empty; any shape
    with S*S entries).  A stone is dead if its point is the opponent's, alive if its own colour's, seki if unsettled."""
    owner = point_owner(row)
    stones = np.asarray(board).reshape(-1)
    out = {"alive": set(), "dead": set(), "seki": set()}
    for a in np.flatnonzero(stones):
        c = 1 if stones[a] > 0 else -1
        out["alive" if owner[a] == c else ("dead" if owner[a] == -c else "seki")].add(int(a))
    return out


def score_lead(row, komi):
    """black points - white points - komi over the settled points."""
    owner = point_owner(row)
    return int((owner > 0).sum()) - int((owner < 0).sum()) - float(komi)


def final_score(row, komi):
    """GTP final_score text: B+x.x / W+x.x / 0."""
    lead = score_lead(row, komi)
    if lead == 0:
        return "0"
    return "%s+%.1f" % ("B" if lead > 0 else "W", abs(lead))


def real_board(board17):
    """Stones of a board tensor [1, S, S, 17] in absolute colours: int8 [S, S], +1 black, -1 white."""
    b = np.asarray(board17)[0]
    d = (b[:, :, 0] - b[:, :, 1]).astype(np.int8)
    return d if int(b[0, 0, 16]) == 1 else -d
