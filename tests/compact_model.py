"""A plain model of the engine step's LIST COMPACTION (k_compact of sejonggo_amd/csrc/sgo_engine.hip): what one step's per-game
requests become.  No code of the package takes part.

INPUT, per game g of G (arrays of G entries, payloads [G, E]): n_req (0 .. E requests), req_kind (LEAF = 1: positions that
board_advance has to make first; anything else, ROOT = 0 here: a position that exists), cur_model, the payloads of request j --
req_blk (the block to evaluate), req_parent and req_move (leaf requests: the block it is made from and the move) --, phase and error.

OUTPUT: eval_base and list_base [G]; the dense evaluation list eval_idx with its model column eval_model [n_eval]; the leaf list
leaf_in (parent), leaf_mv (move), leaf_out (out-block) [n_leaf]; and the status words n_eval, n_leaf, n_root, n_active (games in
PH_WAIT_ROOT or PH_SEARCH), n_done (PH_DONE), error_game (the LOWEST slot with an error, -1 without one) and error (its code, 0).

ORDER: game-major.  The requests of game g stand before those of game g + 1, request j of a game before its request j + 1:
eval_base[g] = sum of n_req over the games below g; list_base[g] is the same sum over the games below g OF g's KIND (leaf and root
requests are counted apart: the leaf list holds the leaf requests only, in the same order).

compact() is that definition, by running sums.  compact_block() computes the same through the SHAPE the kernel has -- one workgroup
of 1 024 threads in 16 waves, thread t owning the run of per = ceil(G / 1024) consecutive games [t * per, t * per + per), a scan
inside each wave, a scan over the 16 wave totals, then every thread walking its run with a running base -- because only that shape
can hold the slips below.  Unwritten words keep FILL.

FAULT SWITCHES of compact_block -- each the kind of slip a block-wide scan with several games per thread could hold
(tests/test_compact_model_power.py shows on which tables each one shows, and which ones a lockstep table cannot see).  Model and
test helper only; no library code reads them.
  one_per_thread    every thread owns one game: games at or above 1 024 contribute nothing (no base, no rows, no count)
  run_base_stuck    all games of one thread's run get the run's first base: the running base is not advanced inside the run
  wave_total_last   a wave's total counts only the LAST game of each run (the bases inside a wave are right, every later wave's
                    base and the totals are short)
  kinds_share_scan  leaf and root requests share one base: list_base is eval_base
  err_last          error_game is not the lowest failing slot: the LAST failing game of a run, and the HIGHEST wave with one
  fold_first_only   n_active / n_done count the first game of a run only"""
import numpy as np

FAULTS = ("one_per_thread", "run_base_stuck", "wave_total_last", "kinds_share_scan", "err_last", "fold_first_only")
EVAL_LIST_FAULTS = ("one_per_thread", "run_base_stuck", "wave_total_last")       # the ones that move rows of the evaluation list
THREADS, WAVE = 1024, 64
LEAF, ROOT = 1, 0
PH_IDLE, PH_WAIT_ROOT, PH_SEARCH, PH_DONE, PH_HOLD = 0, 1, 2, 3, 4
FILL = -7
NONE = 0x7fffffff
KEYS = ("eval_base", "list_base", "eval_idx", "eval_model", "leaf_in", "leaf_mv", "leaf_out", "n_eval", "n_leaf", "n_root", "n_active",
        "n_done", "error_game", "error")


def per_thread(G):
    """games per thread of the one workgroup"""
    return (G + THREADS - 1) // THREADS


def run_of(G, t):
    """the games [g0, g1) of thread t"""
    per = per_thread(G)
    g0 = min(G, t * per)
    return g0, min(G, g0 + per)


def table(G, E, n_req, req_kind=LEAF, cur_model=0, phase=PH_SEARCH, error=0, seed=0):
    """a request table from per-game columns (scalars are broadcast); the payloads are distinct numbers, so that every row of a
    list names its game and its request: req_blk = g * 64 + j, req_parent = 1 000 000 + that, req_move = (g + 3 j) % 26"""
    col = lambda v: np.broadcast_to(np.asarray(v, np.int64), (G,)).copy()        # noqa: E731
    t = {"G": G, "E": E, "n_req": col(n_req), "req_kind": col(req_kind), "cur_model": col(cur_model), "phase": col(phase), "error": col(error)}
    assert E <= 64 and (t["n_req"] >= 0).all() and (t["n_req"] <= E).all()
    g, j = np.meshgrid(np.arange(G, dtype=np.int64), np.arange(E, dtype=np.int64), indexing="ij")
    t["req_blk"] = g * 64 + j
    t["req_parent"] = 1000000 + t["req_blk"]
    t["req_move"] = (g + 3 * j) % 26
    return t


def _lists(t, eval_base, list_base, listed, n_eval, n_leaf):
    """the second phase: every (game, request) pair writes its row; rows nobody writes keep FILL, a row written twice keeps the
    higher game's word.  The lists are as long as the totals say, at least as long as the highest row written."""
    G, E, n_req, kind = t["G"], t["E"], t["n_req"], t["req_kind"]
    top_e = max([n_eval] + [int(eval_base[g] + n_req[g]) for g in range(G) if listed[g] and n_req[g]])
    top_l = max([n_leaf] + [int(list_base[g] + n_req[g]) for g in range(G) if listed[g] and n_req[g] and kind[g] == LEAF])
    out = {"eval_idx": np.full(top_e, FILL, np.int64), "eval_model": np.full(top_e, FILL, np.int64)}
    for k in ("leaf_in", "leaf_mv", "leaf_out"):
        out[k] = np.full(top_l, FILL, np.int64)
    for g in range(G):
        if not listed[g]:
            continue
        k, be = int(n_req[g]), int(eval_base[g])
        out["eval_idx"][be:be + k] = t["req_blk"][g, :k]
        out["eval_model"][be:be + k] = t["cur_model"][g]
        if kind[g] == LEAF:
            bl = int(list_base[g])
            out["leaf_in"][bl:bl + k] = t["req_parent"][g, :k]
            out["leaf_mv"][bl:bl + k] = t["req_move"][g, :k]
            out["leaf_out"][bl:bl + k] = t["req_blk"][g, :k]
    return out


def compact(t):
    """the definition: running sums in game order"""
    G, n_req = t["G"], t["n_req"]
    leaf = t["req_kind"] == LEAF
    eval_base = np.cumsum(n_req) - n_req
    nl, nr = np.where(leaf, n_req, 0), np.where(leaf, 0, n_req)
    list_base = np.where(leaf, np.cumsum(nl) - nl, np.cumsum(nr) - nr)
    failing = np.flatnonzero(t["error"] != 0)
    out = {"eval_base": eval_base, "list_base": list_base, "n_eval": int(n_req.sum()), "n_leaf": int(nl.sum()), "n_root": int(nr.sum()),
           "n_active": int(((t["phase"] == PH_WAIT_ROOT) | (t["phase"] == PH_SEARCH)).sum()), "n_done": int((t["phase"] == PH_DONE).sum()),
           "error_game": int(failing[0]) if len(failing) else -1, "error": int(t["error"][failing[0]]) if len(failing) else 0}
    out.update(_lists(t, eval_base, list_base, np.ones(G, bool), out["n_eval"], out["n_leaf"]))
    return out


def compact_block(t, fault=None):
    """the same through the kernel's shape: runs of games per thread, waves of 64 threads, 16 wave totals"""
    assert fault is None or fault in FAULTS
    G, n_req, kind, phase, error = t["G"], t["n_req"], t["req_kind"], t["phase"], t["error"]
    W = THREADS // WAVE
    runs = [(t_, min(G, t_ + 1)) if fault == "one_per_thread" else run_of(G, t_) for t_ in range(THREADS)]
    runs = [(min(a, G), b) for a, b in runs]
    # first pass: every thread folds its run
    ne, nl, nr = np.zeros(THREADS, np.int64), np.zeros(THREADS, np.int64), np.zeros(THREADS, np.int64)
    last = np.zeros((3, THREADS), np.int64)                                  # the last game of the run alone
    act, done, err = np.zeros(THREADS, np.int64), np.zeros(THREADS, np.int64), np.full(THREADS, NONE, np.int64)
    for t_, (g0, g1) in enumerate(runs):
        for g in range(g0, g1):
            k = int(n_req[g])
            ne[t_] += k
            nl[t_] += k if kind[g] == LEAF else 0
            nr[t_] += 0 if kind[g] == LEAF else k
            last[:, t_] = (k, k if kind[g] == LEAF else 0, 0 if kind[g] == LEAF else k)
            if fault != "fold_first_only" or g == g0:
                act[t_] += phase[g] in (PH_WAIT_ROOT, PH_SEARCH)
                done[t_] += phase[g] == PH_DONE
            if error[g] and (err[t_] == NONE or fault == "err_last"):
                err[t_] = g
    # the scan inside each wave, the scan over the wave totals
    base = np.zeros((3, THREADS), np.int64)
    tot = np.zeros(3, np.int64)
    for c, v in enumerate((ne, nl, nr)):
        incl = np.concatenate([np.cumsum(v[w * WAVE:(w + 1) * WAVE]) for w in range(W)])
        wave_total = incl[WAVE - 1::WAVE] if fault != "wave_total_last" else last[c].reshape(W, WAVE).sum(axis=1)
        wave_base = np.cumsum(wave_total) - wave_total
        base[c] = np.repeat(wave_base, WAVE) + incl - v
        tot[c] = wave_total.sum()
    wave_err = err.reshape(W, WAVE).min(axis=1)
    if fault == "err_last":
        have = wave_err[wave_err != NONE]
        eg = int(have.max()) if len(have) else NONE
    else:
        eg = int(wave_err.min())
    # phase 1: every thread walks its run with a running base
    eval_base, list_base, listed = np.full(G, FILL, np.int64), np.full(G, FILL, np.int64), np.zeros(G, bool)
    for t_, (g0, g1) in enumerate(runs):
        be, bl, br = (int(b) for b in base[:, t_])
        for g in range(g0, g1):
            eval_base[g] = be
            list_base[g] = be if fault == "kinds_share_scan" else (bl if kind[g] == LEAF else br)
            listed[g] = True
            if fault != "run_base_stuck":
                k = int(n_req[g])
                be += k
                bl += k if kind[g] == LEAF else 0
                br += 0 if kind[g] == LEAF else k
    out = {"eval_base": eval_base, "list_base": list_base, "n_eval": int(tot[0]), "n_leaf": int(tot[1]), "n_root": int(tot[2]),
           "n_active": int(act.sum()), "n_done": int(done.sum()), "error_game": -1 if eg == NONE else eg, "error": 0 if eg == NONE else int(error[eg])}
    out.update(_lists(t, eval_base, list_base, listed, out["n_eval"], out["n_leaf"]))
    return out


def differs(a, b, keys=KEYS):
    """the outputs in which two results differ"""
    return [k for k in keys if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


def from_counts(counts, E, blocks=None):
    """the request table of one recorded step: counts[g] rows of game g in the evaluation list read back from the device (and the
    listed blocks, in order, as payload).  The kind is not recorded -- the evaluation list does not depend on it -- so every request
    counts as a leaf request."""
    counts = np.asarray(counts, np.int64)
    t = table(len(counts), E, counts)
    if blocks is not None:
        blocks = np.asarray(blocks, np.int64)
        assert len(blocks) == counts.sum()
        at = 0
        for g, k in enumerate(counts):
            t["req_blk"][g, :k] = blocks[at:at + k]
            at += k
    return t
