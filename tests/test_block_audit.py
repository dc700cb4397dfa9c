"""CPU: proof that tests/block_audit.py can fail.

A plain-integer restatement of the engine's block allocator (csrc/sgo_engine.hip k_start and the k_compact merge,
csrc/sgo_search.hpp alloc / back / the graft in back_propagate / reroot / adopt_other_tree / release_on_error,
csrc/sgo_engine_state.hpp pool_release) writes dumps in the format of the hooks, for several games on one shared pool.  The
search itself is replaced by seeded random growth that builds what the accounting finds hard: chains deeper than 64 levels (so
the re-root's pointer jumping needs 7 passes), wide fans, a kept child chosen at random, an other-player tree that sometimes
follows the move and sometimes is rebuilt, restarts in mid-search, a pool that runs dry.  The correct model audits clean after
every step; each of twelve single faults must be reported, with its own kind of violation."""
import numpy as np
import pytest

from tests import block_audit as BA

A, APAD, NW, F = 5, 32, 1, 16
PH_IDLE, PH_WAIT_ROOT, PH_SEARCH, PH_DONE = 0, 1, 2, 3
KEEP, DROP = -3, -4
ERR_CAPACITY = -201

FAULTS = {
    1: "the other root is not marked KEEP",
    2: "pointer jumping is stopped after 4 passes",
    3: "the stale parents of free ids are not dropped before the mark",
    4: "Lu is taken as cap only: overflow ids are never swept",
    5: "a freed overflow id is not released",
    6: "the merge does not reset the return count",
    7: "the merge drops the last returned entry",
    8: "the rebuild runs in ascending order",
    9: "a pop does not lower free_top",
    10: "k_start does not release the old game's map row",
    11: "a second leaf is grafted onto a slot that already has a child",
    12: "release_on_error is skipped",
}


class Model(object):
    """G games on one context.  Device arrays as integer arrays, indexed by PHYSICAL block like the engine's."""

    def __init__(self, G, cap, ovf_cap, pool, E, rounds, moves, two_model, seed, fault=None):
        self.G, self.cap, self.ovf_cap, self.L, self.pool, self.E = G, cap, ovf_cap, cap + ovf_cap, pool, E
        self.rounds, self.moves, self.two_model, self.fault = rounds, moves, two_model, fault
        self.rng = np.random.RandomState(seed)
        nb = G * cap + pool
        # hipMemset(0) of ctx_alloc: child arrays start as zeros, not as -1 -- unexpanded blocks carry stale child arrays
        self.bParent, self.bSlot = np.zeros(nb, np.int32), np.zeros(nb, np.int32)
        self.cB, self.legal = np.zeros((nb, APAD), np.int32), np.zeros((nb, NW), np.uint32)
        self.freeList = np.zeros((G, self.L), np.int32)
        self.ovfMap = np.full((G, max(1, ovf_cap)), -1, np.int32)
        self.poolFree = np.arange(pool - 1, -1, -1, dtype=np.int32)                # pops give 0, 1, 2, ...
        self.poolRet = np.zeros(max(1, pool), np.int32)
        self.ctl = [pool, 0, pool]
        self.fParent, self.fSlot, self.fBlk, self.fEvaluated = (np.zeros((G, F), np.int32) for _ in range(4))
        self.gs = [dict(phase=PH_IDLE, error=0, root_blk=0, other_root=0, free_top=0, min_free=0, ovf_hi=0, fifo_head=0,
                        fifo_tail=0, rounds_left=0, move_n=0) for _ in range(G)]
        self.max_passes = self.followed = self.fresh = self.mid_search_restarts = self.failures = self.dry_pops = 0

    # ------------------------------------------------------------------ Eng::ph, pool_release, back, alloc
    def ph(self, g, blk):
        if blk < self.cap:
            return g * self.cap + blk
        return self.G * self.cap + int(self.ovfMap[g, blk - self.cap])

    def pool_release(self, g, j):
        ob = int(self.ovfMap[g, j])
        if ob >= 0:
            self.poolRet[self.ctl[1]] = ob
            self.ctl[1] += 1
            self.ovfMap[g, j] = -1

    def back(self, g, blk):
        st = self.gs[g]
        t = self.ctl[0]
        self.ctl[0] -= 1
        ok = t > 0
        if ok:
            self.ctl[2] = min(self.ctl[2], t - 1)
            self.ovfMap[g, blk - self.cap] = self.poolFree[t - 1]
        else:
            self.ctl[0] += 1
            self.dry_pops += 1
        st["ovf_hi"] = max(st["ovf_hi"], blk - self.cap + 1)
        return ok

    def alloc(self, g):
        st = self.gs[g]
        if st["free_top"] <= 0:
            return -1
        nb = int(self.freeList[g, st["free_top"] - 1])
        if nb >= self.cap and not self.back(g, nb):
            return -1
        if self.fault != 9:
            st["free_top"] -= 1
        st["min_free"] = min(st["min_free"], st["free_top"])
        return nb

    # ------------------------------------------------------------------ k_start
    def start(self, g):
        old = self.gs[g]
        if old["phase"] == PH_SEARCH and old["fifo_tail"] > old["fifo_head"]:
            self.mid_search_restarts += 1
        if self.fault != 10:
            for j in range(self.ovf_cap):
                self.pool_release(g, j)
        self.freeList[g, :self.L - 1] = self.L - 1 - np.arange(self.L - 1)
        self.gs[g] = dict(phase=PH_WAIT_ROOT, error=0, root_blk=0, other_root=-1, free_top=self.L - 1, min_free=self.L - 1,
                          ovf_hi=0, fifo_head=0, fifo_tail=0, rounds_left=0, move_n=0)
        gb0 = g * self.cap
        self.legal[gb0, 0] = (1 << A) - 1
        self.bParent[gb0], self.bSlot[gb0] = -1, -2

    # ------------------------------------------------------------------ the tree, as the descent sees it
    def is_legal(self, pb, s):
        return (int(self.legal[pb, 0]) >> s) & 1

    def tree(self, g, root):
        """[(block, depth)] of the expanded blocks below `root`, over cB on legal slots"""
        if self.bSlot[self.ph(g, root)] == -2:
            return []
        out, stack = [], [(root, 0)]
        while stack:
            b, dep = stack.pop()
            out.append((b, dep))
            pb = self.ph(g, b)
            for s in range(A):
                c = int(self.cB[pb, s])
                if self.is_legal(pb, s) and c >= 0:
                    stack.append((c, dep + 1))
        return out

    def expand(self, g, blk):
        self.cB[self.ph(g, blk), :] = -1

    def fail(self, g, code):
        st = self.gs[g]
        if not st["error"]:
            st["error"] = code
        st["phase"] = PH_DONE
        self.failures += 1

    # ------------------------------------------------------------------ one launch of k_search for game g
    def search(self, g):
        st = self.gs[g]
        if st["phase"] in (PH_IDLE, PH_DONE):
            return
        if st["phase"] == PH_WAIT_ROOT:
            pr = self.ph(g, st["root_blk"])
            if self.bSlot[pr] == -2:
                self.expand(g, st["root_blk"])
                self.bSlot[pr] = -1
            st["rounds_left"] = self.rounds
            st["phase"] = PH_SEARCH
        else:
            for fi in range(st["fifo_head"], st["fifo_tail"]):           # consume_leaf_evals
                if not self.fEvaluated[g, fi % F]:
                    self.expand(g, int(self.fBlk[g, fi % F]))
                    self.fEvaluated[g, fi % F] = 1
            while st["fifo_head"] < st["fifo_tail"]:                     # close_round: back_propagate's graft, FIFO order
                i = st["fifo_head"] % F
                self.cB[self.ph(g, int(self.fParent[g, i])), int(self.fSlot[g, i])] = self.fBlk[g, i]
                st["fifo_head"] += 1
            st["rounds_left"] -= 1
        if st["rounds_left"] == 0:
            self.play_move(g)
        else:
            self.select_round(g)
        if st["error"] and st["ovf_hi"] > 0 and self.fault != 12:         # release_on_error
            for j in range(st["ovf_hi"]):
                self.pool_release(g, j)
            st["ovf_hi"] = 0

    def select_round(self, g):
        st, rng = self.gs[g], self.rng
        busy = set()
        for _ in range(self.E):
            blocks = self.tree(g, st["root_blk"])
            cand = []
            for b, dep in blocks:
                pb = self.ph(g, b)
                free = [s for s in range(A) if self.is_legal(pb, s) and self.cB[pb, s] < 0 and (b, s) not in busy]
                if self.fault == 11 and rng.random_sample() < 0.05:
                    free = [s for s in range(A) if self.is_legal(pb, s) and self.cB[pb, s] >= 0 and (b, s) not in busy] or free
                if free:
                    cand.append((dep, b, free))
            if not cand:
                break
            u = rng.random_sample()
            if u < 0.55:
                dep, pb_, free = max(cand)                                # the deepest block: chains
            elif u < 0.8:
                dep, pb_, free = min(cand)                                # the shallowest: wide fans
            else:
                dep, pb_, free = cand[rng.randint(len(cand))]
            slot = free[rng.randint(len(free))]
            nb = self.alloc(g)
            if nb < 0:
                self.fail(g, ERR_CAPACITY)
                return
            busy.add((pb_, slot))
            p = self.ph(g, nb)
            self.bParent[p], self.bSlot[p] = pb_, slot
            self.legal[p, 0] = rng.randint(1, 1 << A)                     # board_advance: the leaf's legal words
            i = st["fifo_tail"] % F
            self.fParent[g, i], self.fSlot[g, i], self.fBlk[g, i], self.fEvaluated[g, i] = pb_, slot, nb, 0
            st["fifo_tail"] += 1

    # ------------------------------------------------------------------ play_move: reroot, adopt_other_tree
    def play_move(self, g):
        st, rng = self.gs[g], self.rng
        pr = self.ph(g, st["root_blk"])
        kids = [s for s in range(A) if self.is_legal(pr, s) and self.cB[pr, s] >= 0]
        if not kids:
            self.fail(g, -3)
            return
        selected = kids[rng.randint(len(kids))]
        if rng.random_sample() < 0.75:                                    # mostly keep the child with the deepest chain below it
            deep = max(self.tree(g, st["root_blk"]), key=lambda t: t[1])[0]
            while self.bParent[self.ph(g, deep)] != st["root_blk"]:
                deep = int(self.bParent[self.ph(g, deep)])
            selected = int(self.bSlot[self.ph(g, deep)])
        nr = int(self.cB[pr, selected])
        onr = self.reroot(g, selected, nr)
        if self.two_model and not self.adopt_other_tree(g, onr):
            return
        st["move_n"] += 1
        st["phase"] = PH_DONE if st["move_n"] >= self.moves else PH_WAIT_ROOT

    def other_tree_follows(self, g, selected):
        st = self.gs[g]
        if self.two_model and st["other_root"] >= 0 and self.bSlot[self.ph(g, st["other_root"])] != -2:
            po = self.ph(g, st["other_root"])
            return int(self.cB[po, selected]) if self.is_legal(po, selected) else -1
        return -1

    def reroot(self, g, selected, nr):
        st, cap, L, f = self.gs[g], self.cap, self.L, self.fault
        onr = self.other_tree_follows(g, selected)
        st["root_blk"] = nr
        self.bParent[self.ph(g, nr)], self.bSlot[self.ph(g, nr)] = -1, -1
        if onr >= 0:
            self.bParent[self.ph(g, onr)], self.bSlot[self.ph(g, onr)] = -1, -1
        Lu = cap + (0 if f == 4 else st["ovf_hi"])
        base = L - Lu
        par = [DROP] * L                      # the LDS copy; ids beyond Lu are never written (read as DROP here)
        for b in range(Lu):
            pv = DROP
            if b < cap:
                pv = int(self.bParent[g * cap + b])
            else:
                ob = int(self.ovfMap[g, b - cap])
                if ob >= 0:
                    pv = int(self.bParent[self.G * cap + ob])
            par[b] = DROP if pv < 0 else pv
        if f != 3:
            for i in range(base, st["free_top"]):
                par[int(self.freeList[g, i])] = DROP
        par[nr] = KEEP
        if onr >= 0 and f != 1:
            par[onr] = KEEP
        passes = 0
        while True:                           # every pass reads the previous pass's array: the slowest order the lanes can take
            new, open_ = list(par), False
            for b in range(Lu):
                if par[b] >= 0:
                    new[b] = par[par[b]]
                    open_ |= new[b] >= 0
            par = new
            passes += 1
            if not open_ or (f == 2 and passes >= 4):
                break
        self.max_passes = max(self.max_passes, passes)
        ft = base
        for b in (range(Lu) if f == 8 else range(Lu - 1, -1, -1)):
            if par[b] != KEEP:
                self.freeList[g, ft] = b
                ft += 1
                if b >= cap and f != 5:
                    self.pool_release(g, b - cap)
        st["free_top"] = ft
        return onr

    def adopt_other_tree(self, g, onr):
        st = self.gs[g]
        nr = st["root_blk"]
        if onr < 0:
            onr = self.alloc(g)
            if onr < 0:
                self.fail(g, ERR_CAPACITY)
                return False
            po = self.ph(g, onr)
            self.legal[po] = self.legal[self.ph(g, nr)]
            self.bParent[po], self.bSlot[po] = -1, -2
            self.fresh += 1
        else:
            self.followed += 1
        st["root_blk"], st["other_root"] = onr, nr
        return True

    # ------------------------------------------------------------------ k_compact's merge
    def merge(self):
        nret, top = self.ctl[1], self.ctl[0]
        n = max(0, nret - 1) if self.fault == 7 else nret
        self.poolFree[top:top + n] = self.poolRet[:n]
        if nret > 0:
            self.ctl[0] = top + n
            if self.fault != 6:
                self.ctl[1] = 0

    # ------------------------------------------------------------------ the hooks' format
    def block_state(self, g):
        st, cap = self.gs[g], self.cap
        omap = self.ovfMap[g, :self.ovf_cap].copy()
        hi = int(np.flatnonzero(omap >= 0)[-1]) + 1 if np.any(omap >= 0) else 0
        rows = 0 if st["error"] else cap + hi
        d = {k: st[k] for k in ("phase", "error", "root_blk", "other_root", "free_top", "min_free", "ovf_hi", "fifo_head", "fifo_tail")}
        d.update(cap=cap, L=self.L, ovf_cap=self.ovf_cap, APAD=APAD, NW=NW, E=self.E, rows=rows, A=A, F=F, ovfMap=omap)
        if st["error"]:
            return d
        phys = np.array([g * cap + b if b < cap else self.G * cap + omap[b - cap] for b in range(rows)], np.int64)
        ok = np.array([b < cap or omap[b - cap] >= 0 for b in range(rows)], bool)
        phys[~ok] = 0
        d["freeList"] = self.freeList[g].copy()
        d["bParent"] = np.where(ok, self.bParent[phys], -9)
        d["bSlot"] = np.where(ok, self.bSlot[phys], -9)
        d["cB"] = np.where(ok[:, None], self.cB[phys], -9)
        d["legal"] = np.where(ok[:, None], self.legal[phys], 0).astype(np.uint32)
        d["fParent"], d["fSlot"], d["fBlk"], d["fEvaluated"] = (a[g].copy() for a in (self.fParent, self.fSlot, self.fBlk, self.fEvaluated))
        return d

    def pool_state(self):
        return {"poolCtl": list(self.ctl), "pool_blocks": self.pool, "poolFree": self.poolFree[:self.pool].copy(),
                "poolRet": self.poolRet[:self.pool].copy()}

    def audit(self, tally=None):
        games = [self.block_state(g) for g in range(self.G)]
        v = BA.audit(games, self.pool_state())
        return v if tally is None else tally.add(v, games)


CONFIGS = {
    # name: G, cap, ovf_cap, pool, E, rounds per move, moves per game, two_model
    "self_play": (3, 6, 420, 3 * 420, 4, 20, 6, False),
    "two_model": (3, 6, 420, 3 * 420, 4, 20, 6, True),
    "dry_pool": (4, 6, 300, 260, 4, 12, 5, True),
    "private": (2, 160, 300, 600, 4, 20, 6, False),      # most blocks private: only those keep a stale parent while free
}


def drive(name, seed, fault=None, steps=150):
    """Restart / step / merge, an audit after the restarts and one after the merge.  Returns (model, tally, the first
    non-empty Violations or None)."""
    m = Model(*CONFIGS[name], seed=seed, fault=fault)
    tally = BA.Tally()
    rng = np.random.RandomState(seed + 1000)
    for g in range(m.G):
        m.start(g)
    for step in range(steps):
        v = m.audit(tally)                                  # right after k_start: returns still on poolRet
        if v:
            return m, tally, v
        for g in range(m.G):
            m.search(g)
        m.merge()
        v = m.audit(tally)
        if v:
            return m, tally, v
        for g in range(m.G):
            st = m.gs[g]
            mid = st["phase"] == PH_SEARCH and st["fifo_tail"] > st["fifo_head"] and rng.random_sample() < 0.01
            if mid or (st["phase"] == PH_DONE and rng.random_sample() < 0.3):
                m.start(g)
    return m, tally, None


@pytest.fixture(scope="module")
def clean_runs():
    return {name: drive(name, seed) for name, seed in (("self_play", 5), ("two_model", 6), ("dry_pool", 7), ("private", 8))}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_correct_model_audits_clean_at_every_step(clean_runs, name):
    m, tally, v = clean_runs[name]
    print(tally.line("model/" + name), "passes", m.max_passes, "followed", m.followed, "fresh", m.fresh, "mid-search restarts",
          m.mid_search_restarts, "failures", m.failures, "dry pops", m.dry_pops)
    assert v is None, v[:10]
    assert tally.audits == 2 * 150 and tally.audits_fifo > 0 and tally.audits_empty > 0
    assert tally.backed > 0 and m.mid_search_restarts > 0


def test_the_driver_reaches_what_the_faults_need(clean_runs):
    """Chains deeper than 64 levels under the kept child (7 jumping passes), both fates of the other tree, a dry pool."""
    assert max(m.max_passes for m, _, _ in clean_runs.values()) >= 7
    assert max(t.deepest for _, t, _ in clean_runs.values()) > 64
    m, tally, _ = clean_runs["two_model"]
    assert m.followed > 0 and m.fresh > 0
    assert tally.followed > 0 and tally.fresh > 0           # ... and the audit's own count of them sees both (on the new root)
    assert clean_runs["self_play"][1].followed == clean_runs["self_play"][1].fresh == 0
    m, tally, _ = clean_runs["dry_pool"]
    assert m.dry_pops > 0 and m.failures > 0 and tally.failed_slots > 0


# fault -> (the configuration that reaches it, the kind of violation that names it and must be among those reported)
EXPECT = {
    1: ("two_model", {"root-free"}),         # the other tree followed the move and is the searched tree now: its root was swept
    2: ("self_play", {"linked-free:root"}),
    3: ("private", {"leak-unlinked"}),
    4: ("self_play", {"free-backed"}),
    5: ("self_play", {"free-backed"}),
    6: ("self_play", {"pool-dup"}),
    7: ("self_play", {"pool-missing"}),
    8: ("self_play", {"free-order"}),
    9: ("self_play", {"inflight-free"}),
    10: ("self_play", {"ovf-hi"}),
    11: ("self_play", {"leak-overwritten"}),
    12: ("dry_pool", {"failed-holds"}),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_each_single_fault_is_reported_with_its_kind(fault):
    name, kinds = EXPECT[fault]
    m, tally, v = drive(name, seed=20 + fault, fault=fault)
    assert v, "fault %d (%s) went unreported in %d audits" % (fault, FAULTS[fault], tally.audits)
    print("fault %d (%s): after %d audits: %s" % (fault, FAULTS[fault], tally.audits, v[:3]))
    assert kinds & set(v.kinds()), (FAULTS[fault], v.kinds(), v[:5])


def test_violations_name_kind_block_and_game():
    m, _, v = drive("self_play", seed=29, fault=9)
    assert all(s.split(": ")[1] in BA.KINDS for s in v) and any(s.startswith("game ") for s in v)


def test_the_golden_game_of_the_gpu_audit_gets_deep_enough():
    """tests/test_gpu_block_audit.py audits async_05 step by step and requires a chain of at least 33 blocks below the root
    (six jumping passes in the re-root) and rounds without a best leaf.  The oracle establishes both for that game."""
    from oracle import oracle as ora
    from sejonggo_amd.stub_nets import make_stub
    from tests.helpers import load
    z = load("async_05.npz")
    S, nm = int(z["size"]), int(z["num_moves"])
    assert S == 5 and int(z["none_events"]) > 0
    net = make_stub(bytes(z["net"]).decode(), S)
    ora.build()
    g = ora.Game(S, int(z["sims"]), int(z["energy"]), int(z["stop_exploration"]), None if nm < 0 else nm, komi=float(z["komi"]),
                 uniforms=z["uniforms"], noises=z["noises"])
    deepest = 0
    while g.phase != ora.PH_DONE:
        p, v = net.predict_on_batch(g.pending())
        g.submit(p, v)
        deepest = max(deepest, g.tree_depth())
    assert g.n_moves == len(z["move_index"]) and g.counters()["none_events"] == int(z["none_events"])
    assert deepest >= 33, deepest
