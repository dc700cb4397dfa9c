"""CPU model of the game-records kernels (include/sgo.h "game records"), written from the header's text on top of the oracle's
rules (oracle.make_play / legal_moves / sym_lut).  No rules code of the package takes part.  Everything is integer or a verbatim
float: the GPU results must match word for word and bit for bit.

FAULT SWITCHES -- each the kind of slip k_records_replay / k_records_score could hold (tests/test_records_model_power.py shows that
the cases of the GPU tests notice them).  Model and test helper only; no library code reads them.
  tie_high             a tie at the target's key is broken towards the HIGHER index
  nan_first            a NaN ranks above everything instead of as -inf
  no_pass_bit          the pass is left out of the legal candidates
  sym_not_inverted     the policy row is read without mapping it back through the symmetry
  target_not_candidate an illegal target is not added to the candidates: it ranks behind every legal move
  best_any             `best` ranges over all actions instead of the legal ones
  write_after_refusal  the record after a refused entry is written (a copy of the last valid one)
  in_turn_only         an out-of-turn colour is played as the side to move
  agree_ge             a value of exactly 0 agrees with z > 0"""
import numpy as np

from oracle import oracle
from tests import rollout_model as rm

FAULTS = ("tie_high", "nan_first", "no_pass_bit", "sym_not_inverted", "target_not_candidate", "best_any", "write_after_refusal",
          "in_turn_only", "agree_ge")
OK, ERR_OCCUPIED, ERR_RANGE = 0, -101, -102


def legal_words(board):
    """The legal bitset of a board tensor as uint32 [NW]: bit a = action a is legal, the pass bit set."""
    S = board.shape[1]
    A = S * S + 1
    NW = (S * S + 31) // 32
    ok = oracle.legal_moves(board)[:A] == 0
    bits = np.zeros(NW * 32, np.uint8)
    bits[:A] = ok
    bits[A - 1] = 1
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def replay(S, games, fault=None):
    """games: [(actions, colours)] (colours may be None: all 0).  Returns a dict: records uint32 [T + G, RW], legal uint32
    [T + G, NW], written bool [T + G] (the records the call must write; every other word stays as it was), status / fail_at int32
    [G], boards {record index: board tensor}."""
    N, A = S * S, S * S + 1
    NW = (N + 31) // 32
    total = sum(len(a) for a, _ in games)
    R = total + len(games)
    rec, leg = np.zeros((R, 16 * NW), np.uint32), np.zeros((R, NW), np.uint32)
    written = np.zeros(R, bool)
    status, fail_at = np.zeros(len(games), np.int32), np.full(len(games), -1, np.int32)
    boards = {}
    off = 0
    for g, (actions, colours) in enumerate(games):
        base = off + g
        board, _ = oracle.game_init(S)
        rec[base], leg[base], written[base] = rm.pack_boards(board)[0], legal_words(board), True
        boards[base] = board.copy()
        for j, a in enumerate(actions):
            col = 0 if colours is None else int(colours[j])
            a = int(a)
            rc = OK
            if a < 0 or a >= A:
                rc = ERR_RANGE
            elif a < N and board[0, a // S, a % S, :2].any():
                rc = ERR_OCCUPIED
            if rc:
                status[g], fail_at[g] = rc, j
                if fault == "write_after_refusal":
                    rec[base + j + 1], leg[base + j + 1], written[base + j + 1] = rec[base + j], leg[base + j], True
                break
            if fault == "in_turn_only":
                col = 0
            x, y = (a % S, a // S) if a < N else (0, S)
            oracle.make_play(x, y, board, None if col == 0 else col)
            r = base + j + 1
            rec[r], leg[r], written[r] = rm.expected_record(rec[r - 1], board), legal_words(board), True
            boards[r] = board.copy()
        off += len(actions)
    return {"records": rec, "legal": leg, "written": written, "status": status, "fail_at": fail_at, "boards": boards}


def lists_of(games):
    """(n_entries, off, actions, colours) int32 arrays of a game list, back to back."""
    n = np.array([len(a) for a, _ in games], np.int32)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32)
    acts = np.array([x for a, _ in games for x in a], np.int32)
    cols = np.array([x for a, c in games for x in (c if c is not None else [0] * len(a))], np.int32)
    return n, off, acts, cols


def _keys(p, fault):
    k = np.asarray(p, dtype=np.float32).astype(np.float64)
    return np.where(np.isnan(k), np.inf if fault == "nan_first" else -np.inf, k)


def score(S, legal, index, target, z, bucket, n_buckets, policy, value, sym_k, fault=None):
    """The outputs of sgo_records_score_dev.  legal: the object's whole legal array uint32 [cap, NW]; policy float32 [n, A] as the
    net produced it under sym_k; value float32 [n].  Returns rank / best / flags int32 [n], p_target float32 [n], counters int64
    [n_buckets, 8]."""
    A = S * S + 1
    n = len(index)
    lut = np.arange(A) if fault == "sym_not_inverted" else oracle.sym_lut(S, sym_k).astype(np.int64)
    policy = np.asarray(policy, dtype=np.float32).reshape(n, A)
    value = np.asarray(value, dtype=np.float32).reshape(n)
    rank, best, flags = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    p_target = np.zeros(n, np.float32)
    counters = np.zeros((n_buckets, 8), np.int64)
    acts = np.arange(A)
    for i in range(n):
        r, t, b = int(index[i]), int(target[i]), int(bucket[i])
        if r < 0 or r >= len(legal) or t < 0 or t >= A or b < 0 or b >= n_buckets:
            rank[i], best[i], flags[i] = -1, -1, 2
            continue
        lg = np.unpackbits(np.asarray(legal[r], dtype="<u4").view(np.uint8), bitorder="little")[:A].astype(bool)
        if fault == "no_pass_bit":
            lg[A - 1] = False
        p = policy[i][lut]
        key = _keys(p, fault)
        t_legal = bool(lg[t])
        cand = lg.copy()
        cand[t] = False
        kt = key[t]
        if fault == "target_not_candidate" and not t_legal:
            kt = -np.inf
            ahead = cand & ((key > kt) | (key == kt))
        elif fault == "tie_high":
            ahead = cand & ((key > kt) | ((key == kt) & (acts > t)))
        else:
            ahead = cand & ((key > kt) | ((key == kt) & (acts < t)))
        rank[i] = int(ahead.sum())
        pool = np.ones(A, bool) if fault == "best_any" else lg
        if pool.any():
            kk = np.where(pool, key, -np.inf)
            top = kk.max()
            best[i] = int(np.flatnonzero(pool & (kk == top))[0])
        else:
            best[i] = -1
        p_target[i] = p[t]
        flags[i] = 1 if t_legal else 0
        c = counters[b]
        c[0] += 1
        c[1] += rank[i] == 0
        c[2] += rank[i] < 5
        c[3] += not t_legal
        zi, v = int(z[i]), value[i]
        if zi != 0:
            c[4] += 1
            pos = v >= 0 if fault == "agree_ge" else v > 0
            c[5] += bool((pos and zi > 0) or (v < 0 and zi < 0))
    return {"rank": rank, "best": best, "flags": flags, "p_target": p_target, "counters": counters}


def float_sums(p_target, value, z, bucket, n_buckets):
    """(ce_sum, se_sum) float64 [n_buckets] as records.float_sums defines them, one addition per row in row order."""
    ce, se = [0.0] * n_buckets, [0.0] * n_buckets
    for p, v, zi, b in zip(np.asarray(p_target, np.float32), np.asarray(value, np.float32), z, bucket):
        p, v = float(p), float(v)
        q = min(p, 1.0) if p > 0.0 else 2.0 ** -149
        ce[int(b)] = ce[int(b)] + float(-np.log(np.float64(q)))
        if int(zi) != 0:
            d = v - float(int(zi))
            se[int(b)] = se[int(b)] + d * d
    return np.array(ce, np.float64), np.array(se, np.float64)


# ---- constructed games: (actions, colours) at a size S >= 5; points are y * S + x ----------------------------------------------
def pt(S, x, y):
    return y * S + x


def constructed_games(S):
    """{name: (actions, colours)}: the shapes the issue lists, built from coordinates so that they exist at every size."""
    N = S * S
    P = lambda x, y: pt(S, x, y)                                                        # noqa: E731
    g = {}
    g["empty"] = ([], [])
    g["one"] = ([P(2, 2)], [1])
    seq = [P(x, y) for y in range(S) for x in range(S)]
    g["seven"] = (seq[:7], [1, -1, 1, -1, 1, -1, 1])
    g["eight"] = (seq[1:9], [1, -1] * 4)
    g["nine"] = (seq[2:11], ([1, -1] * 5)[:9])
    # passes, two in a row, play goes on
    g["passes"] = ([P(1, 1), N, N, P(3, 3), N, P(2, 1), N, N, N, P(0, 4)], [1, -1, 1, -1, 1, -1, 1, -1, 1, -1])
    # capture in the corner: white a1, black b1 + a2 takes it
    g["capture"] = ([P(1, 0), P(0, 0), P(0, 1), P(4, 4)], [1, -1, 1, -1])
    # ko: black (1,0) (0,1) (1,2) + white (2,0)... the classic shape around (1,1)/(2,1); white retakes at once, which the legal set
    # refuses and the replay plays
    ko_a = [P(1, 0), P(2, 0), P(0, 1), P(3, 1), P(1, 2), P(2, 2), P(2, 1), P(1, 1), P(2, 1)]
    g["ko_retake"] = (ko_a, [1, -1, 1, -1, 1, -1, 1, -1, 1])
    # suicide: white b1 and a2, black plays a1 (executed: the stone is removed again)
    g["suicide"] = ([P(1, 0), P(2, 2), P(0, 1), P(3, 3), P(0, 0)], [-1, 1, -1, 1, 1])
    # handicap stones as explicit black entries, then white moves; and a white set-up stone among black's
    g["handicap"] = ([P(1, 1), P(3, 3), P(3, 1), P(2, 2), P(0, 2)], [1, 1, 1, -1, 1])
    g["white_setup"] = ([P(1, 1), P(3, 3), P(4, 0), P(2, 2)], [1, -1, -1, 0])
    g["same_colour_twice"] = ([P(0, 0), P(1, 0), P(2, 0), P(3, 0), P(3, 1)], [1, 1, -1, -1, 0])
    g["colour_zero"] = (seq[3:9], [0] * 6)
    # refusals: entry 0 (off the board), the middle (occupied), the last (occupied; off the board)
    g["refuse_first"] = ([N + 1, P(1, 1)], [0, 0])
    g["refuse_negative"] = ([P(0, 0), -1, P(1, 1)], [0, 0, 0])
    g["refuse_middle"] = ([P(0, 0), P(1, 1), P(0, 0), P(2, 2), P(3, 3)], [1, -1, 1, -1, 1])
    g["refuse_last"] = ([P(0, 0), P(1, 1), P(2, 2), P(1, 1)], [0, 0, 0, 0])
    # a long game: every point row by row (captures on the way), then passes up to the cap of a list
    full = []
    board, _ = oracle.game_init(S)
    rng = np.random.RandomState(100 + S)
    while len(full) < 4 * N:
        empty = np.flatnonzero(~board[0, :, :, :2].any(axis=-1).reshape(-1))
        a = int(rng.choice(empty)) if len(empty) and rng.rand() > 0.05 else N
        full.append(a)
        oracle.make_play(a % S if a < N else 0, a // S if a < N else S, board)
    g["max_length"] = (full, None)
    g["long"] = (full[:3 * N // 2], None)
    return g


def shape_prefix_games(S, limit=6):
    """Games that reach the STONES of positions of tests/golden/rule_shapes_S*.npz: black's stones, then white's, as explicit
    entries, then a pass when the side to move has to change.  Only positions whose stones can be placed one at a time without a
    capture on the way; the fixture's history planes are not reproduced (the record's history is the set-up's own)."""
    from tests import rule_shapes as rs
    f = rs.load_shapes(S)
    out = []
    for i in range(f.P):
        b = f.boards[i]
        to_play = int(f.colour[i])
        own, opp = np.flatnonzero(b[..., 0].reshape(-1)), np.flatnonzero(b[..., 1].reshape(-1))
        if len(own) + len(opp) < 4:
            continue
        black, white = (own, opp) if to_play == 1 else (opp, own)
        acts = [int(a) for a in black] + [int(a) for a in white]
        cols = [1] * len(black) + [-1] * len(white)
        board, _ = oracle.game_init(S)
        ok = True
        for a, c in zip(acts, cols):
            if board[0, a // S, a % S, :2].any():
                ok = False
                break
            oracle.make_play(a % S, a // S, board, c)
        if not ok:
            continue
        if int(board[0, 0, 0, 16]) != to_play:
            acts.append(S * S)
            cols.append(0)
            oracle.make_play(0, S, board)
        if not np.array_equal(board[0, :, :, :2], b[:, :, :2]):
            continue
        out.append((f.names[i], (acts, cols)))
        if len(out) >= limit:
            break
    return out
