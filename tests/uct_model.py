"""CPU model of the playout tree search (include/sgo.h "playout tree search"), written from the header's text on the model of the light
playouts (tests/playout_model.py: `allowed`, `eyes`, `pick`, every ply oracle.make_play) and on tests/rollout_model.py (`draw`, `mix`,
`owners`).  The tree is plain Python: a node is an object with dicts per child.  No code of the package takes part.  Everything is
integer: the GPU results must match word for word, the trace of every simulation included.

FAULT SWITCHES -- each the kind of slip the kernel could hold (tests/test_uct_model_power.py shows that the case set of
tests/uct_cases.py notices every one).  Model and test helper only; no library code reads them.
  w_black_view        w is counted from black's view at a white node
  amaf_second         a point played by both colours below the tree is credited to the colour that played it second
  amaf_unmasked       the AMAF update is not masked by the node's child set
  path_not_in_F       the move of a path step does not enter F
  beta_swapped        beta with n and rn' exchanged in the numerator
  no_prior            the prior is left out (P = 0)
  no_hash             the tie hash is ignored: the lowest point wins a tie
  expand_off_by_one   a node is created when the child's n is above expand_at
  depth_64_node       a node is created at depth SGO_UCT_MAX_DEPTH
  pool_overflow       a node is created with the pool full
  node_for_ended      a position in which the game has ended gets a node
  gs_is_s             gs = s: every tree draws alike
  komi_vs_diff        komi2 is compared with diff where the header has 2 * diff
  best_by_wins        best is decided by wins2 first
  skip_last_tree      the sums over the trees skip the last tree"""
import numpy as np

from oracle import oracle
from tests import playout_model as PM
from tests import rollout_model as RM
from tests import tactics_model as T

FAULTS = ("w_black_view", "amaf_second", "amaf_unmasked", "path_not_in_F", "beta_swapped", "no_prior", "no_hash", "expand_off_by_one",
          "depth_64_node", "pool_overflow", "node_for_ended", "gs_is_s", "komi_vs_diff", "best_by_wins", "skip_last_tree")
SIZES = PM.SIZES
MAX_TREES, MAX_SIMS, MAX_DEPTH = 4096, 4096, 64
M32 = 0xFFFFFFFF


class Node(object):
    def __init__(self, children):
        self.children = list(children)
        self.n = dict.fromkeys(self.children, 0)
        self.w, self.rn, self.rw = dict(self.n), dict(self.n), dict(self.n)
        self.link = {}


def value(n, w, rn, rw, P, E, fault=None):
    """v of the header for one child"""
    if fault == "no_prior":
        P = 0
    rn1, rw1 = rn + P, rw + P
    rq = (rw1 << 16) // rn1 if (E and rn1) else 65536
    q = (w << 16) // n if n else rq
    if n == 0:
        beta = 65536
    elif E and rn1:
        beta = ((n if fault == "beta_swapped" else rn1) << 16) // (rn1 + n + rn1 * n // E)
    else:
        beta = 0
    return (beta * rq + (65536 - beta) * q) >> 16


def select(node, r, P, E, fault=None):
    best = None
    for a in node.children:
        key = (value(node.n[a], node.w[a], node.rn[a], node.rw[a], P, E, fault), 0 if fault == "no_hash" else RM.mix((r + a) & M32), -a)
        if best is None or key > best[0]:
            best = (key, a)
    return best[1]


def children_of(cand, N):
    pts = np.flatnonzero(cand).tolist()
    return pts if pts else [N]


def run_tree(S, rec, seed, g, sims, rules, max_plies, komi2, expand_at, E, P, max_nodes, fault=None):
    """One tree.  Returns {"root": Node, "own" int [2, N], "sums" int [8], "nodes", "deepest", "refused", "trace" [sims]}."""
    N = S * S
    black, white, pblack, pwhite, wtp = T.record_sets(S, rec)
    black, white, pblack, pwhite = (PM._mask(N, s) for s in (black, white, pblack, pwhite))
    start = -1 if wtp else 1
    cap = max_plies if max_plies > 0 else PM.default_plies(S)
    own0, opp0 = (black, white) if start == 1 else (white, black)
    prev0 = pblack if start == 1 else pwhite
    root = Node(children_of(PM.allowed(S, own0, opp0, prev0, start, rules) & ~PM.eyes(S, own0, opp0), N))
    nodes, deepest, refused = 1, 0, 0
    own_acc, sums, trace = np.zeros((2, N), np.int64), np.zeros(8, np.int64), []
    for s in range(sims):
        gs = (s if fault == "gs_is_s" else g * sims + s) & M32
        mover, own, opp, prev = start, own0, opp0, prev0
        ply = passes = 0
        node, path, D = root, [], None
        F = {1: set(), -1: set()}
        while True:
            cand = PM.allowed(S, own, opp, prev, mover, rules) & ~PM.eyes(S, own, opp)
            r = RM.draw(seed, gs, ply)
            board = PM._board(S, own, opp, prev, mover)
            in_tree = D is None
            if in_tree:
                assert node.children == children_of(cand, N)
                a = select(node, r, P, E, fault)
            else:
                a = PM.pick(cand, r) if cand.any() else N
            if a == N:
                oracle.make_play(0, S, board)
                passes += 1
            else:
                oracle.make_play(a % S, a // S, board)
                passes = 0
                if not in_tree:
                    if fault == "amaf_second":
                        F[mover].add(a)
                        F[-mover].discard(a)
                    elif a not in F[1] and a not in F[-1]:
                        F[mover].add(a)
            flat = board.reshape(N, 17)
            prev = opp
            own, opp = flat[:, 0] != 0, flat[:, 1] != 0
            ply += 1
            ended = passes >= 2 or ply >= cap
            if in_tree:
                path.append((node, a, mover))
                if a in node.link and not ended:
                    node = node.link[a]
                else:
                    D = ply
                    if a not in node.link:
                        want = node.n[a] > expand_at if fault == "expand_off_by_one" else node.n[a] >= expand_at
                        want = want and (D < MAX_DEPTH or (fault == "depth_64_node" and D == MAX_DEPTH)) and (not ended or fault == "node_for_ended")
                        if want and nodes >= max_nodes and fault != "pool_overflow":
                            refused, want = 1, False
                        if want:
                            nodes += 1
                            if ended:                                # node_for_ended: never visited, its child set means nothing
                                node.link[a] = Node([N])
                            else:
                                node.link[a] = Node(children_of(PM.allowed(S, own, opp, prev, -mover, rules) & ~PM.eyes(S, own, opp), N))
            mover = -mover
            if ended:
                break
        end = PM._board(S, own, opp, own, mover)
        bo, wo = RM.owners(end)
        diff = int(bo.sum()) - int(wo.sum())
        lhs = diff if fault == "komi_vs_diff" else 2 * diff
        result2 = 2 if lhs > komi2 else (1 if lhs == komi2 else 0)
        for nd, a, c in reversed(path):
            r2 = result2 if (c == 1 or fault == "w_black_view") else 2 - result2
            if a < N and fault != "path_not_in_F":
                F[c].add(a)
                F[-c].discard(a)
            nd.n[a] += 1
            nd.w[a] += r2
            for b in F[c]:
                if b in nd.rn:
                    nd.rn[b] += 1
                    nd.rw[b] += r2
                elif fault == "amaf_unmasked":
                    nd.rn[b], nd.rw[b] = 1, r2
        capped = passes < 2
        own_acc[0] += bo
        own_acc[1] += wo
        sums += [diff > 0, diff < 0, diff == 0, diff, diff * diff, ply, capped, 1]
        deepest = max(deepest, D)
        trace.append(path[0][1] | (D << 9) | (result2 << 16) | (int(capped) << 18))
    return {"root": root, "own": own_acc, "sums": sums, "nodes": nodes, "deepest": deepest, "refused": refused, "trace": trace}


def best_of(visits, wins2, fault=None):
    if not visits.any():
        return -1
    key = (lambda a: (wins2[a], visits[a], -a)) if fault == "best_by_wins" else (lambda a: (visits[a], wins2[a], -a))
    return max(range(len(visits)), key=key)


def search(S, records, index=None, trees=1, sims=16, seed=0, rules=1, max_plies=0, komi2=0, expand_at=2, rave_equiv=64, prior=4,
           max_nodes=None, fault=None):
    """The outputs of sgo_uct_dev for n rows: {"visits" int32 [n, N + 1], "wins2" int32 [n, N + 1], "rave" int32 [n, 2, N + 1], "own"
    int32 [n, 2, N], "sums" int64 [n, 8], "info" int32 [n, 4], "trace" int32 [n * trees, sims]}.  records uint32 [R, 16 * NW]; index
    None = rows 0 .. R - 1; a row outside [0, R) gives zeros and best = -1."""
    records = np.asarray(records, dtype=np.uint32)
    R, N = len(records), S * S
    max_nodes = sims + 1 if max_nodes is None else max_nodes
    index = list(range(R)) if index is None else [int(r) for r in index]
    n = len(index)
    out = {"visits": np.zeros((n, N + 1), np.int32), "wins2": np.zeros((n, N + 1), np.int32), "rave": np.zeros((n, 2, N + 1), np.int32),
           "own": np.zeros((n, 2, N), np.int32), "sums": np.zeros((n, 8), np.int64), "info": np.zeros((n, 4), np.int32),
           "trace": np.zeros((n * trees, sims), np.int32)}
    for i, r in enumerate(index):
        if not 0 <= r < R:
            out["info"][i, 3] = -1
            continue
        for t in range(trees):
            g = i * trees + t
            tr = run_tree(S, records[r], seed, g, sims, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes, fault)
            out["trace"][g] = tr["trace"]
            if fault == "skip_last_tree" and trees > 1 and t == trees - 1:
                continue
            root = tr["root"]
            for a in root.rn:                                        # amaf_unmasked may have added points beyond the child set
                out["rave"][i, 0, a] += root.rn[a]
                out["rave"][i, 1, a] += root.rw[a]
            for a in root.children:
                out["visits"][i, a] += root.n[a]
                out["wins2"][i, a] += root.w[a]
            out["own"][i] += tr["own"].astype(np.int32)
            out["sums"][i] += tr["sums"]
            out["info"][i, 0] += tr["nodes"]
            out["info"][i, 1] = max(out["info"][i, 1], tr["deepest"])
            out["info"][i, 2] += tr["refused"]
        out["info"][i, 3] = best_of(out["visits"][i], out["wins2"][i], fault)
    return out
