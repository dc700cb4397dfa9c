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


def weights(p):
    """floor(clamp(p) * 2^20) + 1 per float32 entry, as python ints (the scaling by 2^20 is exact)."""
    out = []
    for v in np.asarray(p, dtype=np.float32):
        v = float(v)
        if not v > 0.0:          # NaN, negatives, +-0
            c = 0.0
        elif v > 1.0:            # above 1, +inf
            c = 1.0
        else:
            c = v
        out.append(int(np.floor(c * 1048576.0)) + 1)
    return out


def pick(w, r):
    """The smallest a with w[0] + ... + w[a] > t, t = (r * total) >> 32."""
    t = (int(r) * int(sum(w))) >> 32
    c = 0
    for a, v in enumerate(w):
        c += v
        if c > t:
            return a
    raise AssertionError("no weight")


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


def owners(board):
    """(black_owned bool [N], white_owned bool [N]) of a board tensor: stones, and empty points reached by one colour only."""
    real = oracle.get_real_board(board)
    total = oracle.color_board(real, 1).astype(np.int32) + oracle.color_board(real, -1).astype(np.int32)
    bo, wo = (total > 0).reshape(-1), (total < 0).reshape(-1)
    _, black, white = oracle.get_winner(board, 0)
    assert int(bo.sum()) == black and int(wo.sum()) == int(white)        # the invariant of the issue
    return bo, wo


def play_out(net, board, seed, g, sym_k=0, max_plies=None):
    """One rollout from a board tensor [1, S, S, 17].  Returns (final board, plies, capped)."""
    S = board.shape[1]
    N = S * S
    cap = max_plies if max_plies and max_plies > 0 else 2 * N
    board = np.ascontiguousarray(board, dtype=np.int32).copy()
    ply = passes = 0
    while True:
        legal = oracle.legal_moves(board)[:N] == 0
        if not legal.any():
            a = N
            passes += 1
        else:
            p, _ = net.predict_on_batch(oracle.sym_board(sym_k, board))
            p = oracle.sym_policy_inverse(S, sym_k, np.asarray(p, dtype=np.float32))[0]
            w = [wi if ok else 0 for wi, ok in zip(weights(p[:N]), legal)]
            a = pick(w, draw(seed, g, ply))
            passes = 0
        if a == N:
            oracle.make_play(0, S, board)
        else:
            oracle.make_play(a % S, a // S, board)
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
