"""Batch review of a game record on the device engine: every reviewed position of an SGF file is one session slot, all of
them set up in one launch (engine.SessionEngine.setup), searched together without moving (analyze: one net call per round for
all positions) and read back in one launch (report).

    python -m sejonggo_amd.review game.sgf [--sims N] [--every k] [--top K] [--depth D] [--net best|hash|uniform]
                                           [--energy E] [--games n] [--json FILE] [--rollouts R] [--tactics] [--life]
                                           [--find SHAPE.txt] [--moves] [--influence] [--secure] [--solve] [--race] [--connect] [--superko [RULE]]
                                           [--playouts R] [--uct [TREES SIMS]]

One line per reviewed position: the move number, the move played there, its share of the root's visits and its mean value, the
engine's best move with its mean, and the principal variation.  Position m is the board BEFORE move m of the record (set-up
stones placed); with --every k the positions before moves 1, 1 + k, 1 + 2k, ... are reviewed.  Means are the search's own
(the root player's view).  --rollouts R plays every reviewed position out R times with the net's policy (rollout.py; all
positions of a chunk in one batch) and adds the score lead (mean of black - white over the rollouts, minus komi), black's share
of the rollouts won on the board (komi aside) and the number of stones judged dead.  --tactics reads the chains and ladders of
every position of the record in one call (records.RecordSet.tactics) and flags a move `ladder` when it runs out a chain that was
dead even with its owner to move and is still capturable afterwards, `missed` when it leaves an opponent chain of three or more
stones standing that could have been caught.  --life reads the unconditional life of every position of the record in one call
(records.RecordSet.life): each row gains life = {settled, black, white} (the points safe for either colour, for black, for white, in
the position before the move), a move is flagged `inside` when it is played on a point that lay in either colour's territory and
`decided` at the first position without an unsettled point.  --find SHAPE.txt searches every position of the record for the shape
drawn in the file (shapes.Shape.parse, records.RecordSet.shapes): the move after which it first occurs is flagged `appears`, the
first move after which it is gone again `disappears`.  --moves reads what one ply on every point of every position would do
(records.RecordSet.moves; include/sgo.h "move outcomes") and flags each played move from its row in the position before it:
`captures N`, `atari` (it leaves an opponent chain next to it with one liberty), `escape` (a chain of the mover's with one liberty
gets two or more), `self-atari` (two or more stones left with one liberty, nothing captured; a one-stone throw-in is not flagged) and
`missed-capture K at V` (it captured nothing while V would have taken K >= 3 stones).  These are flags, not verdicts: one ply is
looked at and nothing is read out.  --influence reads Bouzy's influence map of every position of the record in one call
(records.RecordSet.influence; include/sgo.h "influence"; the stones unconditional life proves dead are lifted first): each row gains
`estimate` (live stones + territory of black minus white's, minus the record's komi, in front of the move) and `gain` (the change of
that margin across the move in the mover's favour), and a last line names the three moves with the highest and the three with the
lowest gain.  An estimate, and numbers, not verdicts.  Given without --sims, --net and --rollouts it searches nothing and loads no
net: the lines then hold the move and the two figures only.  --superko [positional|situational] compares what every move of every
position would give with every earlier position of the game (records.RecordSet.superko; include/sgo.h "superko") and flags a played
move `repeats K` when it recreated the position K records before the one it was played from (1: a ko recapture), and a position
`superko-forbidden V ...` with the moves superko forbids although the inherited ko rule allows them; like --influence it loads no
net when nothing else asks for one.  --playouts R puts the mean score of R light playouts (records.RecordSet.playouts; include/sgo.h
"light playouts": uniformly random moves that spare the mover's eyes, no net; black - white, komi-free) in front of every move with
its change across the move in the mover's favour, and a last line names the three largest drops: an estimate, not a verdict, and
again no net is loaded for it.  --uct [TREES SIMS] puts `uct V W` in front of every move -- the move the playout tree search favours
there (records.RecordSet.uct; include/sgo.h "playout tree search") and the win rate W of the side to move at the game's komi -- and
flags the move `uct-agrees` or `uct-prefers V`: flags from an estimate, not verdicts, and no net is loaded.  More positions than --games slots run in chunks: one setup, one analyze, one report per chunk."""
import argparse
import contextlib
import json
import string
import sys

import numpy as np

from .conf import conf


def vertex(action, size):
    """GTP vertex of an action (letters skip 'I', rows count from the bottom), as gtp.GTPEngine.print_move."""
    if action < 0:
        return "none"
    if action >= size * size:
        return "pass"
    x, y = action % size, action // size
    return string.ascii_uppercase[x + 1 if x >= 8 else x] + str(size - y)


def positions_of(game, every=1):
    """[(move number m, the (action, colour) list in front of move m, move m itself)] for m = 1, 1 + every, ..."""
    out = []
    for m in range(1, game.n_moves + 1, max(1, int(every))):
        before = game.prefix(m - 1)
        out.append((m, before, game.prefix(m)[-1]))
    return out


def review(engine, game, sims=None, every=1, top=3, depth=8, rollouts=0, komi=None, rollout_seed=0):
    """Reviews `game` (sgfload.SgfGame) on `engine` (engine.SessionEngine; its board size must be the record's).  Returns one
    dict per reviewed position: move_number, colour, played, played_visits, played_share, played_mean, best, best_visits,
    best_mean, root_value, visits, top [{move, visits, mean, prior, pv}] -- or, for a position whose set-up was refused or whose
    search failed, move_number, colour, played, error (the SGO_ERR_* code) and fail_at (the refused entry; -1: the search).
    rollouts > 0 adds rollout_lead, rollout_black_wins and rollout_dead (the module's text; komi None: the record's, else the
    configuration's)."""
    S = engine.S
    if game.size != S:
        raise ValueError("the record is {0}x{0}, the engine plays {1}x{1}".format(game.size, S))
    todo, rows = positions_of(game, every), []
    engine.open(np.arange(min(engine.G, len(todo)), dtype=np.int32))       # the slots become sessions once; setup re-uses them
    for c0 in range(0, len(todo), engine.G):
        chunk = todo[c0:c0 + engine.G]
        slots = np.arange(len(chunk), dtype=np.int32)
        status, fail_at = engine.setup(slots, [[a for a, _ in before] for _, before, _ in chunk],
                                       [[c for _, c in before] for _, before, _ in chunk])
        good = [int(s) for s in slots[status == 0]]
        played_out = _rollouts(engine, good, rollouts, komi, rollout_seed) if good and rollouts > 0 else {}
        if good:
            _search(engine, good, sims)
        r = engine.report(slots, top=top, depth=depth)
        failed = [int(s) for s in good if r["status"][s] != 0]
        codes = dict(zip(failed, engine.results(failed)["done"])) if failed else {}
        if failed:
            engine.open(failed)                         # a failed slot takes no set-up: it serves the next chunk as a new session
        for i, (m, _, (played, colour)) in enumerate(chunk):
            if status[i] != 0 or r["status"][i] != 0:
                # a refused set-up (fail_at = the entry) or a search that failed (fail_at -1; e.g. -201: out of tree blocks)
                rows.append({"move_number": m, "colour": "B" if colour > 0 else "W", "played": vertex(played, S),
                             "error": int(status[i] or codes.get(i) or r["status"][i]), "fail_at": int(fail_at[i])})
                continue
            N, Q, P = r["N"][i], r["Q"][i], r["P"][i]
            visits = int(N[N > 0].sum())
            best = int(r["top_action"][i][0]) if top > 0 else -1
            # the mean of a move that is not the mover's to play (a record with two moves of one colour in a row) has no entry
            in_tree = int(r["to_play"][i]) == colour and N[played] >= 0
            rows.append({
                "move_number": m, "colour": "B" if colour > 0 else "W", "played": vertex(played, S),
                "played_visits": int(N[played]) if in_tree else 0,
                "played_share": (float(N[played]) / visits) if in_tree and visits else 0.0,
                "played_mean": float(Q[played]) if in_tree else 0.0,
                "best": vertex(best, S), "best_visits": int(N[best]) if best >= 0 else 0,
                "best_mean": float(Q[best]) if best >= 0 else 0.0,
                "root_value": float(r["root_value"][i]), "visits": visits,
                "top": [{"move": vertex(int(a), S), "visits": int(N[a]), "mean": float(Q[a]), "prior": float(P[a]),
                         "pv": [vertex(int(v), S) for v in r["pv"][i][k] if v >= 0]}
                        for k, a in enumerate(r["top_action"][i]) if a >= 0]})
            rows[-1].update(played_out.get(i, {}))
    return rows


def _rollouts(engine, slots, per_src, komi, seed):
    """{slot: the rollout fields of its row}: one batch over all listed slots (sgo_rollout_start_sessions); the slots are only
    read, so the search that follows starts from what the set-up left."""
    from .engine import unpack_positions
    from .rollout import real_board, result_row, stone_status
    res = engine.rollouts(slots, per_src=per_src, seed=seed)
    boards = unpack_positions(res["records"], engine.S)
    out = {}
    for k, s in enumerate(slots):
        row = result_row(res, k)
        R = max(1, row["rollouts"])
        out[s] = {"rollout_lead": row["score_sum"] / float(R) - float(komi),
                  "rollout_black_wins": row["black_wins"] / float(R),
                  "rollout_dead": len(stone_status(row, real_board(boards[k:k + 1]))["dead"])}
    return out


def _search(engine, slots, sims):
    """analyze, except that a slot whose search fails (its tree outgrew its blocks) does not end the review: the other slots
    search on to the end, the failed one does not hold afterwards and its report says so."""
    from ._lib import SgoError
    keep = getattr(engine, "raise_on_error", True)
    engine.raise_on_error = False
    try:
        engine.analyze(slots, sims)
    except SgoError:
        pass                # the step bound ran out on the failed slots; the others have recorded and hold
    finally:
        engine.raise_on_error = keep


@contextlib.contextmanager
def _record_set_of(game, record_set):
    """the record set given, or a device RecordSet that holds the game as its only record and is closed on exit"""
    if record_set is not None:
        yield record_set
        return
    from .records import Record, RecordSet
    entries = [(int(a), int(c)) for a, c in game.moves]
    record_set = RecordSet([Record("game", game.size, entries, list(game.setup), list(range(1, len(entries) + 1)), None)], game.size)
    try:
        yield record_set
    finally:
        record_set.close()


def played_moves(game, ch):
    """(m, e, r, action, colour) of the B / W moves of `game` that chunk `ch` of a one-record set played: the move number (set-up
    entries are not counted), the entry's row, the record of the position before it (r + 1: after it) and the move."""
    m = 0
    for e, ((action, colour), is_setup) in enumerate(zip(game.moves, game.setup)):
        if is_setup:
            continue
        m += 1
        if ch.valid[e]:
            yield m, e, int(ch.index[e]), int(action), int(colour)


def move_flags(game, record_set):
    """{move number: ["ladder", "missed"]} of the B / W moves of `game` (tactics.review_flags) from one RecordSet.tactics pass over
    a set that holds the game as its only record."""
    from .tactics import review_flags
    out = {}
    for ch in record_set.tactics(stones=True):
        t = ch.tactics
        for m, _, r, action, colour in played_moves(game, ch):
            out[m] = review_flags(game.size, action, colour, ch.stones[r], t.chains_of(r), ch.stones[r + 1], t.chains_of(r + 1), t.libs[r + 1])
    return out


def add_tactics(rows, game, record_set=None):
    """Adds `tactics` (the flag list of move_flags) to every row of a review.  record_set None: a device RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        flags = move_flags(game, rs)
    for row in rows:
        row["tactics"] = flags.get(row["move_number"], [])
    return rows


def life_rows(game, record_set):
    """{move number: {"settled", "black", "white", "flags"}} of the B / W moves of `game` (life.review_flags) from one RecordSet.life
    pass over a set that holds the game as its only record: the figures of the position BEFORE the move."""
    from .life import review_flags
    out = {}
    for ch in record_set.life():
        v, decided = ch.life, False
        for m, _, r, action, _ in played_moves(game, ch):
            c = v.counts[r]
            flags = review_flags(game.size, action, v, r, decided)
            decided = decided or v.settled(r)
            out[m] = {"settled": game.size * game.size - int(c[6]), "black": int(c[0]) + int(c[2]), "white": int(c[1]) + int(c[3]),
                      "flags": flags}
    return out


def add_life(rows, game, record_set=None):
    """Adds `life` ({settled, black, white}) and `life_flags` to every row of a review.  record_set None: a device RecordSet of
    the game."""
    with _record_set_of(game, record_set) as rs:
        found = life_rows(game, rs)
    for row in rows:
        d = found.get(row["move_number"])
        if d is not None:
            row["life"] = {k: d[k] for k in ("settled", "black", "white")}
            row["life_flags"] = list(d["flags"])
    return rows


def find_rows(game, record_set, shape):
    """{move number: {"hits", "flags"}} of the B / W moves of `game` from one RecordSet.shapes pass over a set that holds the game
    as its only record: `hits` = n_hits of the position AFTER the move, `flags` = shapes.review_flags of the positions around it,
    each flag given once (the first appearance, the first disappearance after it)."""
    from .shapes import review_flags
    out = {}
    for ch in record_set.shapes(shape):
        v, seen, gone = ch.shapes, False, False
        for m, _, r, _, _ in played_moves(game, ch):
            before, after = v.n_hits(r) > 0, v.n_hits(r + 1) > 0
            flags = [f for f in review_flags(before, after) if not (seen if f == "appears" else gone)]
            seen, gone = seen or before or after, gone or "disappears" in flags
            out[m] = {"hits": v.n_hits(r + 1), "flags": flags}
    return out


def add_find(rows, game, shape, record_set=None):
    """Adds `find` (n_hits of the position after the move) and `find_flags` to every row of a review.  record_set None: a device
    RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        found = find_rows(game, rs, shape)
    for row in rows:
        d = found.get(row["move_number"])
        if d is not None:
            row["find"] = d["hits"]
            row["find_flags"] = list(d["flags"])
    return rows


def moves_rows(game, record_set):
    """{move number: flags} of the B / W moves of `game` (moves.review_flags) from one RecordSet.moves pass over a set that holds the
    game as its only record: the row of the played move in the position BEFORE it.  A move out of turn gets no flag: the table is
    the side to move's."""
    from .moves import review_flags
    out = {}
    for ch in record_set.moves():
        for m, e, _, action, _ in played_moves(game, ch):
            out[m] = review_flags(game.size, action, ch.played[e], ch.move_counts[e], lambda a: vertex(a, game.size)) if ch.in_turn[e] else []
    return out


def add_moves(rows, game, record_set=None):
    """Adds `moves_flags` to every row of a review.  record_set None: a device RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        found = moves_rows(game, rs)
    for row in rows:
        row["moves_flags"] = list(found.get(row["move_number"], []))
    return rows


def secure_rows(game, record_set):
    """{move number: flags} of the B / W moves of `game` (secure.review_flags) from one RecordSet.secure pass over a set that holds
    the game as its only record: the row of the played move in the position BEFORE it.  A move out of turn gets no flag: the table
    is the side to move's."""
    from .secure import review_flags
    out = {}
    for ch in record_set.secure():
        v = ch.secure
        for m, _, r, action, colour in played_moves(game, ch):
            in_turn = int(ch.to_play[r]) == colour
            out[m] = review_flags(game.size, action, v.table[r, min(action, v.N - 1)], v.counts[r], lambda a: vertex(a, game.size)) if in_turn else []
    return out


def add_secure(rows, game, record_set=None):
    """Adds `secure_flags` to every row of a review.  record_set None: a device RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        found = secure_rows(game, rs)
    for row in rows:
        row["secure_flags"] = list(found.get(row["move_number"], []))
    return rows


def superko_rows(game, record_set, rule=0):
    """{move number: flags} of the B / W moves of `game` (superko.review_flags) from one RecordSet.superko pass over a set that holds
    the game as its only record: `repeats K` for a played move that recreated an earlier position of the game, `superko-forbidden V
    ...` for a position in which superko forbids moves the inherited rule allows.  The table is the side to move's: a stone placed
    out of turn is read as that side's."""
    from .superko import review_flags
    out = {}
    for ch in record_set.superko(rule):
        v = ch.superko
        for m, _, r, action, colour in played_moves(game, ch):
            out[m] = review_flags(v, r, action, lambda a: vertex(a, game.size))
    return out


def add_superko(rows, game, record_set=None, rule=0):
    """Adds `superko_flags` to every row of a review.  record_set None: a device RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        found = superko_rows(game, rs, rule)
    for row in rows:
        row["superko_flags"] = list(found.get(row["move_number"], []))
    return rows


def solve_rows(game, record_set):
    """{move number: flags} of the B / W moves of `game` (solve.review_flags) from one RecordSet.solve pass over a set that holds
    the game as its only record: the verdicts of the same chain in the position before and after the move."""
    from .solve import review_flags
    out = {}
    for ch in record_set.solve(stones=True):
        v = ch.solve
        for m, _, r, action, colour in played_moves(game, ch):
            out[m] = review_flags(game.size, action, colour, ch.stones[r], v.targets_of(r), ch.stones[r + 1], v.targets_of(r + 1),
                                  lambda a: vertex(a, game.size))
    return out


def add_solve(rows, game, record_set=None):
    """Adds `solve_flags` to every row of a review.  record_set None: a device RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        found = solve_rows(game, rs)
    for row in rows:
        row["solve_flags"] = list(found.get(row["move_number"], []))
    return rows


def race_rows(game, record_set):
    """{move number: flags} of the B / W moves of `game` (race.review_flags) from one RecordSet.race pass over a set that holds the
    game as its only record: each played move against the pairs of the position in front of it."""
    from .race import review_flags
    out = {}
    for ch in record_set.race():
        v = ch.race
        for m, _, r, action, colour in played_moves(game, ch):
            out[m] = review_flags(game.size, action, colour, v.pairs_of(r), lambda a: vertex(a, game.size))
    return out


def add_race(rows, game, record_set=None):
    """Adds `race_flags` to every row of a review.  record_set None: a device RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        found = race_rows(game, rs)
    for row in rows:
        row["race_flags"] = list(found.get(row["move_number"], []))
    return rows


def connect_rows(game, record_set):
    """{move number: flags} of the B / W moves of `game` (connect.review_flags) from one RecordSet.connect pass over a set that holds
    the game as its only record: each played move against the pairs of the position in front of it."""
    from .connect import review_flags
    out = {}
    for ch in record_set.connect():
        v = ch.connect
        for m, _, r, action, colour in played_moves(game, ch):
            out[m] = review_flags(game.size, action, colour, v.pairs_of(r), lambda a: vertex(a, game.size))
    return out


def add_connect(rows, game, record_set=None):
    """Adds `connect_flags` to every row of a review.  record_set None: a device RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        found = connect_rows(game, rs)
    for row in rows:
        row["connect_flags"] = list(found.get(row["move_number"], []))
    return rows


def influence_rows(game, record_set, komi=0.0, dead="life"):
    """{move number: {"estimate", "gain"}} of the B / W moves of `game` (influence.review_fields) from one RecordSet.influence pass
    over a set that holds the game as its only record: the estimate in front of the move, and what the move did to the margin."""
    from .influence import review_fields
    out = {}
    for ch in record_set.influence(dead=dead):
        for m, _, r, _, colour in played_moves(game, ch):
            out[m] = review_fields(ch.influence, r, r + 1, colour, komi)
    return out


def add_influence(rows, game, record_set=None, komi=None):
    """Adds `estimate` (Bouzy's area-score estimate of the position in front of the move, proved-dead stones lifted, minus komi;
    positive = black) and `gain` (the change of the margin across the move in the mover's favour) to every row of a review.
    komi None: the record's, 0 when it has none.  record_set None: a device RecordSet of the game.  Numbers, not verdicts."""
    if komi is None:
        komi = game.komi if game.komi is not None else 0.0
    with _record_set_of(game, record_set) as rs:
        found = influence_rows(game, rs, komi)
    for row in rows:
        d = found.get(row["move_number"])
        if d is not None:
            row["estimate"], row["gain"] = d["estimate"], d["gain"]
    return rows


def playout_rows(game, record_set, per_row, seed=0):
    """{move number: (lead, sd, change, capped share)} of the B / W moves of `game` from one RecordSet.playouts pass over a set that
    holds the game as its only record: the mean playout score (black - white, komi-free) of the position in front of the move, its
    standard deviation, and the change of the mean across the move in the mover's favour.  An estimate from uniformly random
    playouts (include/sgo.h "light playouts"), not a verdict."""
    out = {}
    for ch in record_set.playouts(per_row=per_row, seed=seed):
        v = ch.playouts
        for m, _, r, action, colour in played_moves(game, ch):
            out[m] = (v.score_mean(r), v.score_sd(r), (v.score_mean(r + 1) - v.score_mean(r)) * (1 if colour > 0 else -1), v.capped_share(r))
    return out


def add_playouts(rows, game, per_row, record_set=None, seed=0):
    """Adds `playout_lead`, `playout_sd`, `playout_change` and `playout_capped` to every row of a review.  record_set None: a device
    RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        found = playout_rows(game, rs, per_row, seed)
    for row in rows:
        lead, sd, change, capped = found.get(row["move_number"], (None, None, None, None))
        row["playout_lead"], row["playout_sd"], row["playout_change"], row["playout_capped"] = lead, sd, change, capped
    return rows


def uct_rows(game, record_set, trees=None, sims=None, seed=0):
    """{move number: (best move text, win rate of the side to move, flag)} of the B / W moves of `game` from one RecordSet.uct pass
    over a set that holds the game as its only record: what the playout tree search (include/sgo.h "playout tree search") favours
    in the position in front of the move at the game's komi, and `uct-agrees` or `uct-prefers V`.  A flag from an estimate, not a
    verdict."""
    out = {}
    for ch in record_set.uct(trees=trees, sims=sims, seed=seed, komi=game.komi if game.komi is not None else conf['KOMI']):
        v = ch.uct
        for m, _, r, action, colour in played_moves(game, ch):
            best = v.best(r)
            if best is not None:
                text = vertex(best, game.size)
                out[m] = (text, v.winrate(r), "uct-agrees" if best == action else "uct-prefers " + text)
    return out


def add_uct(rows, game, trees=None, sims=None, record_set=None, seed=0):
    """Adds `uct_best`, `uct_winrate` and `uct_flags` to every row of a review.  record_set None: a device RecordSet of the game."""
    with _record_set_of(game, record_set) as rs:
        found = uct_rows(game, rs, trees, sims, seed)
    for row in rows:
        best, winrate, flag = found.get(row["move_number"], (None, None, None))
        row["uct_best"], row["uct_winrate"], row["uct_flags"] = best, winrate, [flag] if flag else []
    return rows


def playout_summary(rows, top=3):
    """`playouts (estimate): largest drops M C V (-d) ...` of the rows add_playouts filled: the moves after which the mean playout
    score fell most for the mover"""
    drops = sorted((row["playout_change"], row["move_number"], row["colour"], row["played"]) for row in rows
                   if row.get("playout_change") is not None and row["playout_change"] < 0)[:top]
    return "playouts (estimate): largest drops " + (" ".join("%d %s %s (%+.1f)" % (m, c, v, d) for d, m, c, v in drops) or "-")


def influence_summary(rows, top=3):
    """`influence: highest gain M (+g) ...; lowest gain M (-g) ...` of the rows add_influence filled"""
    from .influence import review_summary
    gains = {row["move_number"]: row.get("gain") for row in rows}
    best, worst = review_summary(sorted(gains.items()), top)
    part = lambda ms: " ".join("%d (%+d)" % (m, gains[m]) for m in ms) or "-"            # noqa: E731
    return "influence: highest gain %s; lowest gain %s" % (part(best), part(worst))


def bare_rows(game, every=1):
    """the rows of a review without a search: move_number, colour, played"""
    return [{"move_number": m, "colour": "B" if colour > 0 else "W", "played": vertex(played, game.size)}
            for m, _, (played, colour) in positions_of(game, every)]


def format_row(row):
    text = _format_row(row)
    if row.get("estimate") is not None:
        from .influence import score_text
        text += "  | estimate %s gain %s" % (score_text(row["estimate"]), "-" if row.get("gain") is None else "%+d" % row["gain"])
    if row.get("playout_lead") is not None:
        text += "  | playouts %+.1f +- %.1f change %+.1f" % (row["playout_lead"], row["playout_sd"], row["playout_change"])
    if row.get("uct_best") is not None:
        text += "  | uct %s %.3f" % (row["uct_best"], row["uct_winrate"])
    flags = list(row.get("tactics") or []) + list(row.get("life_flags") or []) + list(row.get("find_flags") or []) + \
        list(row.get("moves_flags") or []) + list(row.get("secure_flags") or []) + list(row.get("solve_flags") or []) + \
        list(row.get("race_flags") or []) + list(row.get("connect_flags") or []) + list(row.get("superko_flags") or []) + list(row.get("uct_flags") or [])
    if flags:
        text += "  | " + " ".join(flags)
    return text


def _format_row(row):
    if "error" in row and row["fail_at"] < 0:
        return "%4d %s %-4s  search failed (%d)" % (row["move_number"], row["colour"], row["played"], row["error"])
    if "error" in row:
        return "%4d %s %-4s  set-up refused (%d at entry %d)" % (row["move_number"], row["colour"], row["played"], row["error"],
                                                                 row["fail_at"])
    if "top" not in row:                                    # a review without a search (bare_rows)
        return "%4d %s %-4s" % (row["move_number"], row["colour"], row["played"])
    pv = " ".join(row["top"][0]["pv"]) if row["top"] else ""
    text = "%4d %s %-4s share %5.1f%% mean %+.4f  best %-4s mean %+.4f  pv %s" % (
        row["move_number"], row["colour"], row["played"], 100.0 * row["played_share"], row["played_mean"], row["best"],
        row["best_mean"], pv)
    if "rollout_lead" in row:
        text += "  | lead %+.1f black wins %5.1f%% dead %d" % (row["rollout_lead"], 100.0 * row["rollout_black_wins"], row["rollout_dead"])
    return text


def document(game, rows, sims, energy, net_name, rollouts=0):
    """The review as one JSON-serialisable document."""
    doc = {"size": game.size, "komi": game.komi, "moves": game.n_moves, "sims": sims, "energy": energy, "net": net_name,
           "positions": rows}
    if rollouts:
        doc["rollouts"] = rollouts
    return doc


def _net(kind, size):
    if kind == "best":
        from .predicting_queue_worker import get_model, init_predicting_workers
        init_predicting_workers(conf['GPUs'][:1])
        return get_model("BEST")
    from .stub_nets import make_stub
    return make_stub(kind, size)


def main(argv=None, out=sys.stdout):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("sgf")
    ap.add_argument("--sims", type=int, default=None, help="simulations per position (default: conf['MCTS_SIMULATIONS'])")
    ap.add_argument("--every", type=int, default=1, help="review every k-th position")
    ap.add_argument("--top", type=int, default=3)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--net", default=None, choices=["best", "hash", "uniform"],
                    help="best (default): the model the configuration names; hash / uniform: the stub nets (no weights needed)")
    ap.add_argument("--influence", action="store_true",
                    help="per move: Bouzy's estimate in front of it (proved-dead stones lifted, minus the record's komi) and the gain "
                         "of the margin across it; a summary of the three highest and lowest gains.  Given without --sims, --net "
                         "and --rollouts, nothing is searched and no net is loaded")
    ap.add_argument("--energy", type=int, default=None)
    ap.add_argument("--games", type=int, default=None, help="session slots = positions per chunk (default: as many as reviewed, at most 1024)")
    ap.add_argument("--symmetry", default="random1", choices=["random1", "avg8", "identity"])
    ap.add_argument("--rollouts", type=int, default=0, help="policy rollouts per position: score lead, black's win share, dead stones")
    ap.add_argument("--tactics", action="store_true", help="flag moves that run out a dead ladder or miss a capturable chain")
    ap.add_argument("--life", action="store_true", help="flag moves played inside settled territory and the position that settled the board")
    ap.add_argument("--find", default=None, metavar="SHAPE.txt", help="flag the moves after which the shape drawn in this file first appears and disappears")
    ap.add_argument("--moves", action="store_true",
                    help="flag what each played move did in one ply: captures N, atari, escape, self-atari, missed-capture K at V "
                         "(flags, not verdicts: nothing is read out)")
    ap.add_argument("--secure", action="store_true",
                    help="flag what each played move proved in one ply: secures K (stones and points made pass-alive), missed-secure K "
                         "at V, destroys K (flags from a proof about one ply, not verdicts: the answer is not read).  Like "
                         "--influence it loads no net when nothing else asks for one")
    ap.add_argument("--solve", action="store_true",
                    help="flag what each played move did to the enclosed chains a bounded life-and-death reader decides: kills V, saves "
                         "V, missed-kill V at K, missed-save V at K (flags from a bounded reader, not verdicts).  Like --influence it "
                         "loads no net when nothing else asks for one")
    ap.add_argument("--race", action="store_true",
                    help="flag each played move against the capturing races a bounded reader decides in the position in front of it: "
                         "wins-race V (the catching or saving move of an unsettled racer V), missed-race V at K (flags from a bounded "
                         "reader, not verdicts).  Like --influence it loads no net when nothing else asks for one")
    ap.add_argument("--connect", action="store_true",
                    help="flag each played move against the connections a bounded reader decides in the position in front of it: cuts V "
                         "(the cut_move of an unsettled pair V of the opponent), joins V, missed-cut V at K, missed-join V at K (flags "
                         "from a bounded reader, not verdicts).  Like --influence it loads no net when nothing else asks for one")
    ap.add_argument("--superko", nargs="?", const="positional", default=None, choices=("positional", "situational"),
                    help="flag every played move that recreated an earlier position of the game (repeats K: K records back from the "
                         "position it was played in) and every position in which superko forbids moves the inherited ko rule allows "
                         "(superko-forbidden V ...).  Like --influence it loads no net when nothing else asks for one")
    ap.add_argument("--playouts", type=int, default=None, metavar="R",
                    help="put the mean score of R light playouts (uniformly random moves that spare the mover's eyes, no net; black - "
                         "white, komi-free) in front of every move, with its change across the move in the mover's favour, and name the "
                         "three largest drops.  An estimate, not a verdict.  Like --influence it loads no net when nothing else asks for one")
    ap.add_argument("--uct", nargs="*", type=int, default=None, metavar="N",
                    help="--uct [TREES SIMS]: put the best move and the win rate (of the side to move, at the game's komi) of the playout "
                         "tree search in front of every move, and flag it uct-agrees or uct-prefers V (flags from an estimate, not "
                         "verdicts; default: the untuned trees and sims of uct.py).  Like --influence it loads no net when nothing else "
                         "asks for one")
    ap.add_argument("--json", default=None, help="write the review as one JSON document to this file")
    a = ap.parse_args(argv)
    if a.uct is not None and len(a.uct) not in (0, 2):
        ap.error("--uct takes no values or TREES SIMS")
    from .engine import SessionEngine
    from .sgfload import load_file
    game = load_file(a.sgf)
    # --influence with nothing that asks for a search or a net: the record kernels alone
    searched = not ((a.influence or a.secure or a.solve or a.race or a.connect or a.superko or a.playouts or a.uct is not None) and a.sims is None and a.net is None and not a.rollouts)
    a.net = a.net or "best"
    sims = a.sims or conf['MCTS_SIMULATIONS']
    energy = a.energy or min(conf['ENERGY'], sims)
    n_pos = len(positions_of(game, a.every))
    net = _net(a.net, game.size) if searched else None
    if searched:
        eng = SessionEngine(net, size=game.size, n_games=a.games or max(1, min(1024, n_pos)), sims=sims, energy=energy,
                            komi=game.komi if game.komi is not None else conf['KOMI'], symmetry=a.symmetry)
        try:
            rows = review(eng, game, sims=sims, every=a.every, top=a.top, depth=a.depth, rollouts=a.rollouts, komi=eng.komi)
        finally:
            eng.close()
            if a.net == "best":
                from .predicting_queue_worker import destroy_predicting_workers
                destroy_predicting_workers(conf['GPUs'][:1])
    else:
        rows, sims, energy = bare_rows(game, a.every), 0, 0
    if a.tactics:
        add_tactics(rows, game)
    if a.life:
        add_life(rows, game)
    if a.find:
        from .shapes import Shape
        with open(a.find) as f:
            add_find(rows, game, Shape.parse(f.read()))
    if a.moves:
        add_moves(rows, game)
    if a.secure:
        add_secure(rows, game)
    if a.solve:
        add_solve(rows, game)
    if a.race:
        add_race(rows, game)
    if a.connect:
        add_connect(rows, game)
    if a.superko:
        add_superko(rows, game, rule=a.superko)
    if a.influence:
        add_influence(rows, game)
    if a.playouts:
        add_playouts(rows, game, a.playouts)
    if a.uct is not None:
        add_uct(rows, game, *(a.uct or (None, None)))
    for row in rows:
        out.write(format_row(row) + "\n")
    if a.influence:
        out.write(influence_summary(rows) + "\n")
    if a.playouts:
        out.write(playout_summary(rows) + "\n")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(document(game, rows, sims, energy, getattr(net, "name", a.net) if searched else None, a.rollouts), f, indent=1,
                      sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
