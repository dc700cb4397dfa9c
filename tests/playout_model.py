"""CPU model of the light playouts (include/sgo.h "light playouts"), written from the header's text on the oracle's rules: every
ALLOWED of rules = 0 is oracle.legal_moves on a board tensor whose plane 2 is `prev`, every ply is oracle.make_play, the sound set
of rules = 1 is found by PLAYING the ply and looking for the stone, the score is tests/rollout_model.owners (oracle.get_real_board /
color_board / get_winner) and the draw tests/rollout_model.draw.  The eye rule is plain Python on the board.  No code of the
package takes part.  Everything is integer: the GPU results must match word for word.

FAULT SWITCHES -- each the kind of slip the kernel could hold (tests/test_playout_model_power.py shows that the case set of
tests/playout_cases.py notices every one).  Model and test helper only; no library code reads them.
  edge_T2             an edge or corner eye is judged with T = 2
  empty_diag_counts   empty diagonals are counted as the other colour's
  offboard_diag       diagonals beyond the edge are counted as the other colour's
  pick_round_up       t = ceil(r * k / 2^32) (clamped to k - 1) where the header has the floor
  ko_across_pass      a mover that passes keeps its ko ban for its next turn
  prev_wrong_plane    `prev` of the first ply is read from the other colour's plane
  touched_unseeded    `touched` starts empty: a replayed starting point counts in AMAF
  amaf_any_touch      AMAF counts a point whenever the starting side plays it, not only when it is first touched
  amaf_black_view     the AMAF score is black - white for a white mover too
  owner_no_exclusion  an empty point reached by both colours is counted for both
  history_passes      two records in a row with the same stones count as a pass already made
  cap_off_by_one      the playout ends at ply == max_plies + 1
  g_ignores_row       g = j
  sound_ignores_ko    the sound set of rules = 1 holds the ko point when its stone would stand"""
import numpy as np

from oracle import oracle
from tests import rollout_model as RM
from tests import tactics_model as T

FAULTS = ("edge_T2", "empty_diag_counts", "offboard_diag", "pick_round_up", "ko_across_pass", "prev_wrong_plane", "touched_unseeded",
          "amaf_any_touch", "amaf_black_view", "owner_no_exclusion", "history_passes", "cap_off_by_one", "g_ignores_row",
          "sound_ignores_ko")
SIZES = T.SIZES
SUMS = ("black_wins", "white_wins", "draws", "score_sum", "score_sq_sum", "plies_sum", "capped", "playouts")
MAX_PER_ROW = 65536
build_record = T.build_record


def default_plies(S):
    return 3 * S * S


def _board(S, own, opp, prev, mover):
    """board tensor with `mover` (+1 / -1) to move: plane 0 its stones, plane 1 the other's, plane 2 its `prev` (bool [N] each)"""
    flat = np.zeros((S * S, 17), np.int32)
    flat[:, 0], flat[:, 1], flat[:, 2] = own, opp, prev
    flat[:, 16] = mover
    return np.ascontiguousarray(flat.reshape(1, S, S, 17))


def ko_point(own, prev):
    gone = np.flatnonzero(prev & ~own)
    return int(gone[0]) if len(gone) == 1 else -1


_ON = {}


def _diag(m, S):
    """per point the number of set diagonal neighbours of a padded plane [S + 2, S + 2]"""
    return m[:S, :S].astype(np.int8) + m[:S, 2:] + m[2:, :S] + m[2:, 2:]


def eyes(S, own, opp, fault=None):
    """EYE of the header for the mover `own`: bool [N].  A neighbour beyond the edge is no neighbour."""
    if S not in _ON:
        inside = np.zeros((S + 2, S + 2), bool)
        inside[1:-1, 1:-1] = True
        _ON[S] = _diag(inside, S)
    on = _ON[S]
    o1, p1 = np.ones((S + 2, S + 2), bool), np.zeros((S + 2, S + 2), bool)
    o1[1:-1, 1:-1], p1[1:-1, 1:-1] = own.reshape(S, S), opp.reshape(S, S)
    all4 = o1[:-2, 1:-1] & o1[2:, 1:-1] & o1[1:-1, :-2] & o1[1:-1, 2:]     # only ON-BOARD neighbours must be the mover's
    bad = _diag(p1, S)
    if fault == "empty_diag_counts":
        n1 = np.zeros((S + 2, S + 2), bool)
        n1[1:-1, 1:-1] = ~own.reshape(S, S)
        bad = _diag(n1, S)
    if fault == "offboard_diag":
        bad = bad + (4 - on)
    T_ = np.where(on == 4, 2, 2 if fault == "edge_T2" else 1)
    return (~(own | opp).reshape(S, S) & all4 & (bad < T_)).reshape(-1)


def allowed(S, own, opp, prev, mover, rules, fault=None):
    """ALLOWED of the "life and death" section: bool [N]"""
    N = S * S
    board = _board(S, own, opp, prev, mover)
    out = np.asarray(oracle.legal_moves(board))[:N] == 0
    if rules:
        ko = ko_point(own, prev)
        for a in np.flatnonzero(~(out | own | opp)):
            if a == ko and fault != "sound_ignores_ko":
                continue
            child = board.copy()
            oracle.make_play(int(a % S), int(a // S), child)
            if child[0, a // S, a % S, 1]:                           # the stone stands: it is the new mover's opponent's
                out[a] = True
    return out


def pick(cand, r, fault=None):
    """the (t + 1)-th lowest point of cand (bool [N], not empty)"""
    pts = np.flatnonzero(cand)
    k = len(pts)
    t = (int(r) * k) >> 32
    if fault == "pick_round_up":
        t = min(k - 1, -((-int(r) * k) >> 32))
    return int(pts[t])


def _mask(N, pts):
    m = np.zeros(N, bool)
    m[np.asarray(pts, dtype=np.int64)] = True
    return m


def play_out(S, rec, seed, g, rules, max_plies, fault=None, trace=None):
    """One playout of one record.  Returns (black_owned bool [N], white_owned bool [N], first bool [N], plies, capped)."""
    N = S * S
    black, white, pblack, pwhite, wtp = T.record_sets(S, rec)
    black, white, pblack, pwhite = (_mask(N, s) for s in (black, white, pblack, pwhite))
    start = -1 if wtp else 1
    mover = start
    own, opp = (black, white) if mover == 1 else (white, black)
    prev = pblack if (mover == 1) != (fault == "prev_wrong_plane") else pwhite
    touched = np.zeros(N, bool) if fault == "touched_unseeded" else (black | white)
    first = np.zeros(N, bool)
    cap = max_plies if max_plies > 0 else default_plies(S)
    if fault == "cap_off_by_one":
        cap += 1
    ply = passes = 0
    if fault == "history_passes" and (black == pblack).all() and (white == pwhite).all():
        passes = 1
    kept = {}                                                        # ko_across_pass: the `prev` a passing mover keeps
    while True:
        if fault == "ko_across_pass" and mover in kept:
            prev = kept.pop(mover)
        cand = allowed(S, own, opp, prev, mover, rules, fault) & ~eyes(S, own, opp, fault)
        board = _board(S, own, opp, prev, mover)
        if not cand.any():
            a = N
            oracle.make_play(0, S, board)
            passes += 1
            if fault == "ko_across_pass":
                kept[mover] = prev
        else:
            a = pick(cand, RM.draw(seed, g, ply), fault)
            oracle.make_play(a % S, a // S, board)
            passes = 0
            if mover == start and (not touched[a] or fault == "amaf_any_touch"):
                first[a] = True
            touched[a] = True
        if trace is not None:
            trace.append(a)
        flat = board.reshape(N, 17)
        prev = opp                                                   # the next mover's stones one ply ago
        own, opp, mover = flat[:, 0] != 0, flat[:, 1] != 0, -mover
        ply += 1
        if passes >= 2 or ply >= cap:
            break
    end = _board(S, own, opp, own, mover)
    bo, wo = RM.owners(end, "owner_no_exclusion" if fault == "owner_no_exclusion" else None)
    return bo, wo, first, ply, passes < 2


def playouts(S, records, index=None, per_row=1, seed=0, rules=1, max_plies=0, fault=None):
    """The outputs of sgo_playout_dev for n rows: {"own" int32 [n, 2, N], "amaf" int32 [n, 2, N], "sums" int64 [n, 8]}.  records
    uint32 [R, 16 * NW]; index None = rows 0 .. R - 1; a row outside [0, R) gives zeros."""
    records = np.asarray(records, dtype=np.uint32)
    R, N = len(records), S * S
    index = list(range(R)) if index is None else [int(r) for r in index]
    n = len(index)
    own, amaf, sums = np.zeros((n, 2, N), np.int32), np.zeros((n, 2, N), np.int32), np.zeros((n, 8), np.int64)
    for i, r in enumerate(index):
        if not 0 <= r < R:
            continue
        wtp = bool(records[r].reshape(16, -1)[0, -1] >> 31)
        for j in range(per_row):
            g = (j if fault == "g_ignores_row" else i * per_row + j) & 0xFFFFFFFF
            bo, wo, first, plies, capped = play_out(S, records[r], seed, g, rules, max_plies, fault)
            own[i, 0] += bo
            own[i, 1] += wo
            diff = int(bo.sum()) - int(wo.sum())
            view = -diff if (wtp and fault != "amaf_black_view") else diff
            amaf[i, 0] += first
            amaf[i, 1] += np.where(first, view, 0).astype(np.int32)
            sums[i] += [diff > 0, diff < 0, diff == 0, diff, diff * diff, plies, capped, 1]
    return {"own": own, "amaf": amaf, "sums": sums}
