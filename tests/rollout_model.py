"""CPU model of the policy rollouts (include/sgo.h "policy rollouts"), written from the header's text on top of the oracle's
rules (oracle.legal_moves / make_play / get_real_board / color_board / sym_board / sym_policy_inverse) and stub nets on numpy.
No rules code of the package takes part.  All integer: the GPU results must match bit for bit."""
import numpy as np

from oracle import oracle

M32 = 0xFFFFFFFF
SUMS = ("black_wins", "white_wins", "draws", "score_sum", "score_sq_sum", "plies_sum", "capped", "rollouts")


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw(seed, g, ply):
    return mix((mix((seed ^ (g * 0x9E3779B9)) & M32) + ply * 0x85EBCA6B) & M32)


def weights_arr(p, fault=None):
    """floor(clamp(p) * 2^20) + 1 per float32 entry, int64 (float32 -> float64 and the scaling by 2^20 are exact)."""
    v = np.asarray(p, dtype=np.float32).astype(np.float64)
    if fault == "neg_as_abs":
        v = np.abs(v)
    pos = v > 0.0                                    # False for NaN, negatives, +-0
    c = np.where(pos, v, 0.0)
    if fault == "nan_as_one":
        c = np.where(np.isnan(v), 1.0, c)
    c = np.minimum(c, 2048.0 if fault == "no_clamp_hi" else 1.0)     # above 1, +inf (the fault still saturates: 2^31)
    x = c * 1048576.0
    w = np.floor(x + 0.5 if fault == "round_not_floor" else x).astype(np.int64)
    return w if fault == "no_plus_one" else w + 1


def weights(p):
    """weights_arr as a list of python ints."""
    return weights_arr(p).tolist()


def pick(w, r):
    """The smallest a with w[0] + ... + w[a] > t, t = (r * total) >> 32."""
    cum = np.cumsum(np.asarray(w, dtype=np.int64))
    assert cum[-1] > 0, "no weight"
    t = (int(r) * int(cum[-1])) >> 32
    return int(np.searchsorted(cum, t, side="right"))


# ---- fault switches: each the kind of slip k_rollout_step could hold (tests/test_rollout_step_power.py shows that the cases
# of tests/rollout_cases.py notice them).  Model and test helper only; no library code reads them.
#   pick_ge            c >= t where the kernel has c > t (among the legal points)
#   no_plus_one        the weight without its + 1
#   round_not_floor    round to nearest where the header says floor
#   no_clamp_hi        p > 1 is not clamped
#   nan_as_one         NaN weighs like 1.0
#   neg_as_abs         a negative weighs like its absolute value
#   row_boundary_lt    a row owns excl < t <= incl where the kernel has excl <= t < incl
#   scan_wraps_28      prefix sums taken mod 2^28
#   fill_capped        the scoring fill stops after FILL_CAP trips, the deepest the whole-game rollout cases need
#   owner_no_exclusion rb where the kernel has rb & ~rw
#   seed_unmasked      the fill seed without & emp
#   history_from_out   planes 2..15 are taken from the new pair (and what follows it) instead of the record read
#   meta_not_flipped   the to-play bit stays as it was
FAULTS = ("pick_ge", "no_plus_one", "round_not_floor", "no_clamp_hi", "nan_as_one", "neg_as_abs", "row_boundary_lt",
          "scan_wraps_28", "fill_capped", "owner_no_exclusion", "seed_unmasked", "history_from_out", "meta_not_flipped")
WEIGHT_FAULTS = ("no_plus_one", "round_not_floor", "no_clamp_hi", "nan_as_one", "neg_as_abs")
PICK_FAULTS = ("pick_ge", "row_boundary_lt", "scan_wraps_28")
FILL_FAULTS = ("fill_capped", "owner_no_exclusion", "seed_unmasked")
FILL_CAP = 4


def pick_faulty(w, r, S, fault):
    """pick with one of PICK_FAULTS, in the kernel's form: a row of the board claims t, then a point of that row does.  Always
    a point with a weight, so that the model can play it."""
    w = np.asarray(w, dtype=np.int64)
    mod = (1 << 28) if fault == "scan_wraps_28" else (1 << 62)
    cum = np.cumsum(w) % mod
    t = (int(r) * int(cum[-1])) >> 32
    on = np.flatnonzero(w)
    if fault == "row_boundary_lt":
        rows = sorted(set(int(a) // S for a in on))
        mine = rows[0]
        for y in rows:
            excl = int(cum[y * S - 1]) if y else 0
            if excl < t <= int(cum[y * S + S - 1]):
                mine = y
                break
        here = [int(a) for a in on if a // S == mine]
        return next((a for a in here if cum[a] > t), here[-1])
    for a in on:
        if (cum[a] >= t) if fault == "pick_ge" else (cum[a] > t):
            return int(a)
    return int(on[-1])


def pack_boards(boards):
    """Board tensors int32 [n, S, S, 17] -> packed records uint32 [n, 16 * NW] (include/sgo.h "packed")."""
    boards = np.asarray(boards, dtype=np.int32)
    n, S = boards.shape[0], boards.shape[1]
    N = S * S
    NW = (N + 31) // 32
    out = np.zeros((n, 16, NW), dtype=np.uint32)
    for i in range(n):
        white = boards[i, 0, 0, 16] == -1
        for c in range(16):
            bits = boards[i, :, :, c ^ 1 if white else c].reshape(N)
            for a in np.flatnonzero(bits):
                out[i, c, a >> 5] |= np.uint32(1 << (a & 31))
        if white:
            out[i, 0, NW - 1] |= np.uint32(0x80000000)
    return out.reshape(n, 16 * NW)


def pack_pairs(boards):
    """Planes 0 / 1 (black, white) of the packed records of board tensors [n, S, S, 17], with the to-play bit: uint32 [n, 2 * NW]."""
    boards = np.asarray(boards, dtype=np.int32)
    n, S = boards.shape[0], boards.shape[1]
    N = S * S
    NW = (N + 31) // 32
    white = boards[:, 0, 0, 16] == -1
    own, opp = boards[..., 0].reshape(n, N) != 0, boards[..., 1].reshape(n, N) != 0
    bits = np.zeros((n, 2, NW * 32), dtype=np.uint8)
    bits[:, 0, :N] = np.where(white[:, None], opp, own)
    bits[:, 1, :N] = np.where(white[:, None], own, opp)
    bits[:, 0, NW * 32 - 1] = white
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view("<u4").astype(np.uint32).reshape(n, 2 * NW)


def expected_records(prev_records, pairs, fault=None):
    """The records a step must write, uint32 [n, 16 * NW], from the records it read and the new planes 0 / 1 (pack_pairs of
    the model's boards): planes 2..15 are words 0 .. 14*NW-1 of the record read, verbatim -- spare bits ride along."""
    prev_records = np.asarray(prev_records, dtype=np.uint32)
    NW = prev_records.shape[1] // 16
    out = np.empty_like(prev_records)
    out[:, :2 * NW] = pairs
    out[:, 2 * NW:] = prev_records[:, :14 * NW]
    if fault == "history_from_out":
        out[:, 2 * NW:4 * NW] = pairs
    if fault == "meta_not_flipped":
        meta = np.uint32(0x80000000)
        out[:, NW - 1] = (out[:, NW - 1] & ~meta) | (prev_records[:, NW - 1] & meta)
    return out


def expected_record(prev_record, new_board, fault=None):
    """One record: planes 0 / 1 and the to-play bit from the model's board after the ply, the history from the record read."""
    return expected_records(np.asarray(prev_record, dtype=np.uint32)[None], pack_pairs(new_board), fault)[0]


def regions(board):
    """(black stones or reached by black, the same for white, empty) as bool [N] of a board tensor, from the oracle."""
    real = oracle.get_real_board(board)
    cb, cw = oracle.color_board(real, 1).reshape(-1) != 0, oracle.color_board(real, -1).reshape(-1) != 0
    return cb, cw, real.reshape(-1) == 0


def owners(board, fault=None):
    """(black_owned bool [N], white_owned bool [N]) of a board tensor: stones, and empty points reached by one colour only.
    With one of FILL_FAULTS the row-form fill of tests/rule_shapes.py takes the oracle's place."""
    if fault in FILL_FAULTS:
        return owners_rows(board, fault)[:2]
    real = oracle.get_real_board(board)
    total = oracle.color_board(real, 1).astype(np.int32) + oracle.color_board(real, -1).astype(np.int32)
    bo, wo = (total > 0).reshape(-1), (total < 0).reshape(-1)
    _, black, white = oracle.get_winner(board, 0)
    assert int(bo.sum()) == black and int(wo.sum()) == int(white)        # the invariant of the issue
    return bo, wo


def owners_rows(board, fault=None):
    """The scoring of k_rollout_step restated on rows of bits: flood(nbr4(nb) & emp, emp) twice, then rb & ~rw.  Returns
    (black_owned, white_owned, trips of the deeper fill)."""
    return owners_rows_real(oracle.get_real_board(board), fault)


def owners_rows_real(real, fault=None):
    """owners_rows on the stones themselves: int [S, S], +1 black, -1 white."""
    from tests import rule_shapes as rs
    S = real.shape[0]
    M = (1 << S) - 1
    nb, nw = rs.rows_of(real == 1), rs.rows_of(real == -1)
    emp = [~(nb[y] | nw[y]) & M for y in range(S)]
    reach, deepest = [], 0
    for mine in (nb, nw):
        seed = rs.nbr4(mine, M)
        if fault != "seed_unmasked":
            seed = [seed[y] & emp[y] for y in range(S)]
        got, trips = rs.flood(seed, emp, FILL_CAP if fault == "fill_capped" else None)
        reach.append(got)
        deepest = max(deepest, trips)
    rb, rw = reach
    if fault == "owner_no_exclusion":
        bo, wo = [nb[y] | rb[y] for y in range(S)], [nw[y] | rw[y] for y in range(S)]
    else:
        bo, wo = [nb[y] | (rb[y] & ~rw[y]) for y in range(S)], [nw[y] | (rw[y] & ~rb[y]) for y in range(S)]
    return rs.plane_of(bo, S).reshape(-1) != 0, rs.plane_of(wo, S).reshape(-1) != 0, deepest


def step_row(board, row, r, fault=None, legal=None):
    """One ply of one rollout from an explicit policy row: float32 [A] (or [N]) in board orientation, r the draw.  Returns
    (action, new board); the board given is left as it is.  The oracle only: legal_moves, weights, pick, make_play.
    `legal` (bool [N]) may carry oracle.legal_moves(board)[:N] == 0 when the caller has it already."""
    S = board.shape[1]
    N = S * S
    if legal is None:
        legal = oracle.legal_moves(board)[:N] == 0
    w = None
    if legal.any():
        w = np.where(legal, weights_arr(np.asarray(row, dtype=np.float32)[:N], fault if fault in WEIGHT_FAULTS else None), 0)
    if w is None or (fault == "no_plus_one" and not w.any()):        # a total of 0 is a pass in the kernel
        a = N
    else:
        a = pick_faulty(w, r, S, fault) if fault in PICK_FAULTS else pick(w, r)
    new = np.ascontiguousarray(board, dtype=np.int32).copy()
    if a == N:
        oracle.make_play(0, S, new)
    else:
        oracle.make_play(a % S, a // S, new)
    return a, new


def play_out(net, board, seed, g, sym_k=0, max_plies=None):
    """One rollout from a board tensor [1, S, S, 17].  Returns (final board, plies, capped)."""
    S = board.shape[1]
    N = S * S
    cap = max_plies if max_plies and max_plies > 0 else 2 * N
    board = np.ascontiguousarray(board, dtype=np.int32).copy()
    ply = passes = 0
    while True:
        legal = oracle.legal_moves(board)[:N] == 0
        row = None
        if legal.any():                                               # a rollout that must pass never asks the net
            p, _ = net.predict_on_batch(oracle.sym_board(sym_k, board))
            row = oracle.sym_policy_inverse(S, sym_k, np.asarray(p, dtype=np.float32))[0]
        a, board = step_row(board, row, draw(seed, g, ply), legal=legal)
        passes = passes + 1 if a == N else 0
        ply += 1
        if passes >= 2 or ply >= cap:
            return board, ply, passes < 2


def run(net, boards, per_src, seed, sym_k=0, max_plies=None):
    """What sgo_rollout_result gives for the source boards [n_src, S, S, 17]: black_own / white_own int32 [n_src, N],
    sums int64 [n_src, 8]; plus the per-rollout (plies, black, white, capped) rows."""
    boards = np.asarray(boards, dtype=np.int32)
    n_src, S = boards.shape[0], boards.shape[1]
    N = S * S
    black_own, white_own = np.zeros((n_src, N), np.int32), np.zeros((n_src, N), np.int32)
    sums = np.zeros((n_src, 8), np.int64)
    rows = []
    for s in range(n_src):
        for j in range(per_src):
            g = s * per_src + j
            end, plies, capped = play_out(net, boards[s:s + 1], seed, g, sym_k, max_plies)
            bo, wo = owners(end)
            black_own[s] += bo
            white_own[s] += wo
            diff = int(bo.sum()) - int(wo.sum())
            sums[s] += [diff > 0, diff < 0, diff == 0, diff, diff * diff, plies, capped, 1]
            rows.append((plies, int(bo.sum()), int(wo.sum()), bool(capped)))
    return {"black_own": black_own, "white_own": white_own, "sums": sums, "rows": rows}


def fixture_f1(S=5):
    """F1: black fills columns 0-2 except (0,0) and (0,4), white fills columns 3-4 except (4,0) and (4,4); points are (x, y).
    Returns (black points, white points) as action lists."""
    black = [y * S + x for x in range(3) for y in range(S) if (x, y) not in ((0, 0), (0, 4))]
    white = [y * S + x for x in (3, 4) for y in range(S) if (x, y) not in ((4, 0), (4, 4))]
    return black, white


def fixture_f2(S=5):
    """F2: F1 with (0,1) also empty and a white stone on (0,0)."""
    black, white = fixture_f1(S)
    black.remove(1 * S + 0)
    return black, white + [0]


def board_of(S, black, white, to_play=1):
    """A board tensor [1, S, S, 17] with the given stones, no history, `to_play` to move."""
    b = np.zeros((1, S, S, 17), dtype=np.int32)
    own, opp = (black, white) if to_play == 1 else (white, black)
    for a in own:
        b[0, a // S, a % S, 0] = 1
    for a in opp:
        b[0, a // S, a % S, 1] = 1
    b[0, :, :, 16] = to_play
    return b
