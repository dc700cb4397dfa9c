"""Constructed cases for one ply of k_rollout_step (csrc/sgo_rollout.hip) and what the CPU model tests/rollout_model.py expects
of them: the action, the record written, the survivors and the accumulated result of every rollout, ply by ply.

Plain numpy on top of the oracle and the fixtures tests/golden/rule_shapes_S*.npz; deterministic.  tests/test_gpu_rollout_step.py
runs the cases on the device, tests/test_rollout_step_power.py shows on the CPU that they notice the faults of
rollout_model.FAULTS and that they reach what they were built for.

A CASE is one start: source boards, an index list (source s = board index[s]), per_src, seed, max_plies, the symmetry of every
step and one policy row per rollout for the first ply (in the orientation the step receives).  Later plies take the same row
again ("same") or the HashNet's row on the model's board ("hash").  The global id of a rollout, g = src * per_src + j, is also
the row of everything below."""
import functools

import numpy as np

from oracle import oracle
from tests import rollout_model as M
from tests import rule_shapes as rs

SIZES = rs.SIZES
BOUNDARY_SIZES = (5, 13, 19)
W_MAX = (1 << 20) + 1
MAX_TOTAL = 361 * W_MAX
F32 = np.float32
VALUES = (("nan", np.nan), ("-0", -0.0), ("+0", 0.0), ("-1", -1.0), ("-inf", -np.inf), ("+inf", np.inf), ("1", 1.0),
          ("above 1", np.nextafter(F32(1), F32(2))), ("below 1", np.nextafter(F32(1), F32(0))), ("2", 2.0),
          ("2^-20", 2.0 ** -20), ("below 2^-20", np.nextafter(F32(2.0 ** -20), F32(0))), ("min denormal", 2.0 ** -149),
          ("max denormal", 2.0 ** -126 - 2.0 ** -149))
KINDS = ("first_two", "last_two", "row_end", "gap_row", "t0", "t_last")


class Case(object):
    pass


class Expect(object):
    pass


# ---- symmetry ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sym_index(S, k):
    """idx with oracle.sym_policy_inverse(S, k, row)[a] == row[idx[a]] (the entries of arange are exact in float32)."""
    return oracle.sym_policy_inverse(S, k, np.arange(S * S + 1, dtype=np.float32)).astype(np.int64)


def to_step(S, k, rows):
    """Rows in board orientation -> the rows the step must be given under sym_k = k: sym_policy_inverse maps them back."""
    out = np.empty_like(rows)
    out[:, sym_index(S, k)] = rows
    return out


# ---- source records -----------------------------------------------------------------------------------------------------------
def source_table(boards, salt):
    """Packed records of the boards with every word the rules do not read made random: planes 4..15 whole, and the spare bits
    of planes 1..3 (plane 0's is the to-play bit).  A step has to move all of it verbatim."""
    rec = M.pack_boards(boards)
    n, S = len(boards), boards.shape[1]
    N = S * S
    NW = (N + 31) // 32
    rng = np.random.RandomState(1000 * S + salt)
    rec = rec.reshape(n, 16, NW)
    rec[:, 4:, :] = rng.randint(0, 1 << 32, size=(n, 12, NW), dtype=np.uint64).astype(np.uint32)
    spare = np.uint32((0xFFFFFFFF << (N - 32 * (NW - 1))) & 0xFFFFFFFF)
    rec[:, 1:4, NW - 1] |= rng.randint(0, 1 << 32, size=(n, 3), dtype=np.uint64).astype(np.uint32) & spare
    return rec.reshape(n, 16 * NW)


def make_case(name, S, boards, index, per_src, seed, max_plies, rows_board, sym=(0,), later="same", pad=5, salt=0):
    c = Case()
    c.name, c.S, c.N, c.A, c.NW = name, S, S * S, S * S + 1, (S * S + 31) // 32
    c.boards = np.ascontiguousarray(boards, dtype=np.int32)
    c.index = np.asarray(index, dtype=np.int32)
    c.n_src, c.per_src, c.n_total = len(c.index), int(per_src), len(c.index) * int(per_src)
    c.seed, c.max_plies, c.sym, c.later = int(seed), int(max_plies), tuple(sym), later
    c.max_rollouts = c.n_total + pad              # the second half of the record array does not start at n_total
    rows_board = np.ascontiguousarray(rows_board, dtype=np.float32)
    assert rows_board.shape == (c.n_total, c.A) and max_plies >= 1
    c.rows0 = rows_board if c.sym[0] == 0 else to_step(S, c.sym[0], rows_board)
    c.records = source_table(c.boards, salt)
    c.meta = None
    return c


def expect(c, fault=None):
    """The model's account of a case: per ply t and rollout g the row given (rows[t]), the action (-1: not live), the new
    planes 0 / 1 (pair), whether it lives on; the end position's stones; the per-source result."""
    from sejonggo_amd import stub_nets
    S, N, T, n = c.S, c.N, c.max_plies, c.n_total
    e = Expect()
    e.rows = [c.rows0] + [c.rows0 if c.later == "same" else np.zeros((n, c.A), np.float32) for _ in range(T - 1)]
    e.action = np.full((T, n), -1, dtype=np.int32)
    e.pair = np.zeros((T, n, 2 * c.NW), dtype=np.uint32)
    e.live_after = np.zeros((T, n), dtype=bool)
    e.end_real = np.zeros((n, N), dtype=np.int8)
    e.plies = np.zeros(n, dtype=np.int32)
    e.both = np.zeros(n, dtype=bool)
    e.black_own, e.white_own = np.zeros((c.n_src, N), np.int32), np.zeros((c.n_src, N), np.int32)
    e.sums = np.zeros((c.n_src, 8), np.int64)
    net = stub_nets.HashNet(S) if c.later == "hash" else None
    legal0 = {}
    for g in range(n):
        s = g // c.per_src
        b = int(c.index[s])
        if b not in legal0:
            legal0[b] = oracle.legal_moves(c.boards[b:b + 1])[:N] == 0
        board, legal = c.boards[b:b + 1], legal0[b]
        ply = passes = 0
        while True:
            k = c.sym[ply % len(c.sym)]
            if ply and net is not None:
                e.rows[ply][g] = net.predict_on_batch(oracle.sym_board(k, board))[0][0]
            row = e.rows[ply][g]
            if k:
                row = oracle.sym_policy_inverse(S, k, row)
            a, board = M.step_row(board, row, M.draw(c.seed, g, ply), fault, legal)
            legal = None
            passes = passes + 1 if a == N else 0
            e.action[ply, g] = a
            e.pair[ply, g] = M.pack_pairs(board)[0]
            ply += 1
            if passes >= 2 or ply >= T:
                break
            e.live_after[ply - 1, g] = True
        bo, wo = M.owners(board, fault)
        cb, cw, emp = M.regions(board)
        e.both[g] = (cb & cw & emp).any()
        e.end_real[g] = oracle.get_real_board(board).reshape(-1)
        e.plies[g] = ply
        e.black_own[s] += bo
        e.white_own[s] += wo
        diff = int(bo.sum()) - int(wo.sum())
        e.sums[s] += [diff > 0, diff < 0, diff == 0, diff, diff * diff, ply, passes < 2, 1]
    return e


@functools.lru_cache(maxsize=None)
def expected(key):
    """expect() of the case group(key[0])(*key[1:]), computed once and shared (treat it as read-only)."""
    return expect(case(key))


@functools.lru_cache(maxsize=None)
def case(key):
    return GROUPS[key[0]](*key[1:])


def fill_depth(real_flat, S):
    """Trips of the deeper of the two scoring fills on an end position (rule_shapes.flood counts as the kernel's loop does)."""
    return M.owners_rows_real(np.asarray(real_flat).reshape(S, S))[2]


# ---- shape probes and chains --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_items(S):
    """(movers, passers): lists of (position, point) over the fixture of size S -- every empty point and two occupied ones of
    every position; passers are those of the positions whose side to move has no legal board point."""
    f = rs.load_shapes(S)
    movers, passers = [], []
    for p in range(f.P):
        stones = ((f.boards[p, :, :, 0] != 0) | (f.boards[p, :, :, 1] != 0)).reshape(-1)
        emp, occ = np.flatnonzero(~stones), np.flatnonzero(stones)
        pts = [int(a) for a in emp] + ([int(occ[0]), int(occ[-1])] if len(occ) else [])
        (passers if f.legal[p][:f.N].all() else movers).extend((p, a) for a in pts)
    return movers, passers


def _one_hot(items, A):
    rows = np.zeros((len(items), A), dtype=np.float32)
    rows[np.arange(len(items)), [a for _, a in items]] = 1.0
    return rows


def probes(S, passers):
    """One rollout per probe, one source each.  Movers play one ply and are scored (max_plies 1); passers pass, the other side
    answers from the same row, and the second ply ends them (two passes, or the cap)."""
    f = rs.load_shapes(S)
    items = probe_items(S)[1 if passers else 0]
    return make_case("probes_S%d_%s" % (S, "pass" if passers else "move"), S, f.boards, [p for p, _ in items], 1, 11 + S,
                     2 if passers else 1, _one_hot(items, f.A), pad=7, salt=1 + int(passers))


def chains(S):
    """A fixed 1-in-8 subset of the moving probes continued to three plies with HashNet rows, a symmetry per step: the ping-pong
    back into the first record and a history of three plies."""
    f = rs.load_shapes(S)
    items = probe_items(S)[0][3::8]
    return make_case("chains_S%d" % S, S, f.boards, [p for p, _ in items], 1, 23 + S, 3, _one_hot(items, f.A), sym=(0, 3, 6),
                     later="hash", pad=3, salt=3)


# ---- pick boundaries ----------------------------------------------------------------------------------------------------------
def _spread(total, k):
    base, extra = divmod(total, k) if k else (0, 0)
    return [base + 1] * extra + [base] * (k - extra)


def boundary_weights(L, r, j, T, hit):
    """Integer weights in [1, 2^20 + 1] over the legal list L that sum to T such that, with t = (r * T) >> 32, the prefix sum
    through L[j] is t + 1 (hit: L[j] is the pick) or t (not hit: L[j + 1] is).  None when no such weights exist."""
    n = len(L)
    t = (int(r) * int(T)) >> 32
    k, head = j + 1, (t + 1 if hit else t)
    m, tail = n - k, T - head
    if not (0 <= j < n and k <= head <= k * W_MAX and m <= tail <= m * W_MAX) or (not hit and m == 0):
        return None
    return _spread(head, k) + _spread(tail, m)


def encode(w, how):
    """float32 policy values of integer weights: 'exact' p = (w - 1) / 2^20, 'below' the largest float32 below w / 2^20 (floors
    to the same weight), 'mixed' the two alternating."""
    w = np.asarray(w, dtype=np.float64)
    exact = ((w - 1) / 1048576.0).astype(np.float32)
    below = np.nextafter((w / 1048576.0).astype(np.float32), F32(0))
    if how == "exact":
        return exact
    if how == "below":
        return below
    return np.where(np.arange(len(w)) % 2 == 0, exact, below)


def legal_list(board):
    N = board.shape[1] ** 2
    return [int(a) for a in np.flatnonzero(oracle.legal_moves(board)[:N] == 0)]


def boundary_rows(S, board, n, seed):
    """n policy rows (board orientation) for rollouts g = 0..n-1 of one position, and what each was built for:
    meta[g] = (kind, hit, total class, encoding, j, expected action).  The draws decide where t = 0 and t = T - 1 can be had
    (small totals only); every other g takes the next task of a fixed cycle whose weights exist for its draw."""
    A = S * S + 1
    L = legal_list(board)
    nL = len(L)
    assert nL >= 2
    ys = [a // S for a in L]
    js = {"first_two": 0, "last_two": nL - 2,
          "row_end": next((j for j in range(nL - 1) if ys[j + 1] == ys[j] + 1), None),
          "gap_row": next((j for j in range(nL - 1) if ys[j + 1] > ys[j] + 1), None)}
    totals = (("mid", nL * 1024 + 517), ("big", nL * (1 << 19) + 12345), ("small", nL + 3))
    tasks = [(kind, hit, enc) for kind in KINDS[:4] if js[kind] is not None for hit in (True, False)
             for enc in ("exact", "below", "mixed")]
    rows = np.zeros((n, A), dtype=np.float32)
    meta, nxt, n_t0, n_tl = [], 0, 0, 0
    illegal = np.ones(S * S, dtype=bool)
    illegal[L] = False
    for g in range(n):
        r = M.draw(seed, g, 0)
        got = None
        for T in ((nL, nL + 3) if (n_t0 + n_tl) % 2 == 0 else (nL + 3, nL)):
            t = (r * T) >> 32
            if got is None and t == 0 and n_t0 < 6:
                got, n_t0 = ("t0", True, "small", "exact", 0, T, boundary_weights(L, r, 0, T, True)), n_t0 + 1
            if got is None and t == T - 1 and n_tl < 6:
                got, n_tl = ("t_last", False, "small", "below", nL - 2, T, boundary_weights(L, r, nL - 2, T, False)), n_tl + 1
        tries = 0
        while got is None and tries < len(tasks):
            kind, hit, enc = tasks[(nxt + tries) % len(tasks)]
            for o in range(len(totals)):
                cls, T = totals[(g + o) % len(totals)]
                w = boundary_weights(L, r, js[kind], T, hit)
                if w is not None:
                    got = (kind, hit, cls, enc, js[kind], T, w)
                    break
            tries += 1
        if got is None:                                  # cannot happen with nL >= 2: the small total always admits a task
            got = ("plain", True, "ones", "exact", 0, nL, [1] * nL)
        else:
            nxt += tries
        kind, hit, cls, enc, j, T, w = got
        rows[g, L] = encode(w, enc)
        rows[g, :S * S][illegal] = 1.0 if g % 2 == 0 else 0.5           # must weigh nothing
        rows[g, A - 1] = np.nan if g % 2 else np.inf                   # the pass entry must never matter
        meta.append((kind, hit, cls, enc, j, T, L[j] if hit else L[j + 1]))
    return rows, meta


@functools.lru_cache(maxsize=None)
def boundary_positions(S):
    """{"empty" | "dense" | "ko": board}: the empty board, the fixture position with a row without a legal point between two
    that have some (a 'dense' one where there is one) and the most legal points, and the ko position with the most."""
    f = rs.load_shapes(S)
    best = {}
    for p in range(f.P):
        lg = f.legal[p][:f.N] == 0
        ys = sorted(set(np.flatnonzero(lg) // S))
        gap = any(b - a > 1 for a, b in zip(ys, ys[1:]))
        own, prev = f.boards[p, :, :, 0] != 0, f.boards[p, :, :, 2] != 0
        score = (f.names[p].startswith("dense"), int(lg.sum()))
        ko = (prev & ~own).sum() == 1
        if gap and not ko and score > best.get("dense", (None, (False, 1)))[1]:
            best["dense"] = (p, score)
        if ko and score[1] > best.get("ko", (None, (False, 1)))[1][1]:
            best["ko"] = (p, (False, score[1]))
    out = {"empty": oracle.game_init(S)[0]}
    for k in ("dense", "ko"):
        out[k] = f.boards[best[k][0]:best[k][0] + 1].copy()
    return out


def boundaries(S, where, sym_k=0):
    n = {5: 384, 13: 768, 19: 1536}[S] if where == "empty" else 192
    board = boundary_positions(S)[where]
    rows, meta = boundary_rows(S, board, n, 31 + S)
    c = make_case("boundaries_S%d_%s_k%d" % (S, where, sym_k), S, board, [0] * n, 1, 31 + S, 1, rows, sym=(sym_k,), pad=9, salt=4)
    c.meta = meta
    return c


def max_total():
    """All weights 2^20 + 1 on the empty 19x19 board, from 1.0, the float above it, 2.0 and +inf: the largest total.  Its
    boundaries cannot be adjusted; the model predicts the picks."""
    S, n = 19, 256
    board = oracle.game_init(S)[0]
    vals = np.array([1.0, np.nextafter(F32(1), F32(2)), 2.0, np.inf], dtype=np.float32)
    rows = vals[(np.arange(n)[:, None] + np.arange(S * S + 1)[None, :]) % 4]
    return make_case("max_total", S, board, [0] * n, 1, 77, 1, rows, pad=1, salt=5)


# ---- special values -----------------------------------------------------------------------------------------------------------
def specials(S, where):
    """Row i gives point a the value VALUES[(a + i) % 14]: every legal point carries every value in turn, 4 draws per row.
    Nine more rows do the same with the nine values that weigh 1 or 2 alone: beside a weight of 2^20 their weights hardly
    ever decide a pick, among themselves each of them does."""
    board = boundary_positions(S)[where]
    A, reps = S * S + 1, 4
    vals = np.array([v for _, v in VALUES], dtype=np.float32)
    small = vals[np.array(M.weights(vals)) <= 2]
    pts = np.arange(A)[None, :]
    rows = np.concatenate([v[(pts + (np.arange(len(v) * reps) // reps)[:, None]) % len(v)] for v in (vals, small)])
    n = len(rows)
    rows[:, A - 1] = np.where(np.arange(n) % 2 == 0, np.nan, np.inf)
    return make_case("specials_S%d_%s" % (S, where), S, board, [0] * n, 1, 41 + S, 1, rows, pad=2, salt=6)


# ---- wave neighbours ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deepest_probe(S):
    """(position, point, trips) of the moving probe with the deepest scoring fill among those of the four positions whose
    unmoved fill is deepest."""
    f = rs.load_shapes(S)
    e, items = expected(("probes", S, False)), probe_items(S)[0]
    unmoved = [fill_depth(oracle.get_real_board(f.boards[p:p + 1]).reshape(-1), S) for p in range(f.P)]
    top = set(np.argsort(unmoved)[-4:].tolist())
    best = (None, None, 0)
    for g, (p, a) in enumerate(items):
        if p in top:
            d = fill_depth(e.end_real[g], S)
            if d > best[2]:
                best = (p, a, d)
    return best


def quiet_board(S):
    """Black on every point but two corner eyes, black to play: no legal board point (the rollout passes and, with max_plies 1,
    is scored as it stands) and scoring fills that end on their first trip."""
    return M.board_of(S, list(range(1, S * S - 1)), [], to_play=1)


def neighbours(S, order):
    """The deepest-fill probe D and the quiet board E side by side: `order` is a string over 'D' / 'E', list position i of the
    step = its i-th letter (list[0] is the identity after a start)."""
    f = rs.load_shapes(S)
    p, a, _ = deepest_probe(S)
    boards = np.concatenate([f.boards[p:p + 1], quiet_board(S)])
    rows = np.zeros((len(order), f.A), dtype=np.float32)
    rows[:, a] = 1.0
    return make_case("neighbours_S%d_%s" % (S, order), S, boards, [0 if ch == "D" else 1 for ch in order], 1, 51 + S, 1, rows,
                     pad=1, salt=7)


NEIGHBOUR_ORDERS = ("DEED", "DED", "EDE", "D", "E")


# ---- contention ---------------------------------------------------------------------------------------------------------------
def contention(n_src, per_src, first=0):
    """F1 (nobody has a legal board point: two passes) and its colour mirror, both sides to move: every rollout of a source
    adds to the same counters on step 2."""
    black, white = M.fixture_f1()
    boards = np.concatenate([M.board_of(5, black, white, 1), M.board_of(5, white, black, 1), M.board_of(5, black, white, -1),
                             M.board_of(5, white, black, -1)])
    n = n_src * per_src
    rows = np.full((n, 26), 0.25, dtype=np.float32)
    return make_case("contention_%dx%d_%d" % (n_src, per_src, first), 5, boards, [(s + first) % 4 for s in range(n_src)], per_src, 61, 2, rows,
                     pad=11, salt=8)


GROUPS = {"probes": probes, "chains": chains, "boundaries": boundaries, "max_total": max_total, "specials": specials,
          "neighbours": neighbours, "contention": contention}
