"""The tree-block accounting invariant (the comments of csrc/sgo_engine_state.hpp), checked on raw dumps.

Pure Python / numpy; no GPU, no engine import.  The dumps come from SelfPlayEngine.block_state(slot) / pool_state() (the hooks
sgo_debug_block_state / sgo_debug_pool_state copy device state and interpret nothing) or, in tests/test_block_audit.py, from a
plain-integer model of the allocator that writes the same format.  `audit(games, pool)` returns the list of violations, empty
when the accounting is exact.  It is written against the data model, not against k_search's control flow:

  per game   the free stack [0, free_top) of `freeList`, the overflow map, the child links `cB` (what sgo_tree_serialize and
             top_one walk), the parent view `bParent` / `bSlot` (what the re-root's mark walks) and the FIFO of leaves in flight
             describe ONE set of blocks: every local id of [0, cap + ovf_hi) is either on the free stack, or linked exactly once
             below the root (or the other player's root), or in flight -- and never two of these
  per context  every shared block is in exactly one place: on poolFree, on poolRet, or behind one game's overflow id

Every violation is a string "<where>: <kind>: <detail>"; KINDS lists the kinds (tests assert kinds, never just non-emptiness).
"""
import numpy as np

PH_IDLE, PH_WAIT_ROOT = 0, 1

KINDS = (
    "range",            # free_top / min_free / ovf_hi / FIFO counters outside their bounds
    "ovf-hi",           # a backed map index at or above ovf_hi
    "free-range",       # a free-stack entry outside [0, L), or above the bottom part one outside [0, cap + ovf_hi)
    "free-dup",         # an id twice on the free stack
    "free-bottom",      # the never-used bottom of the stack is not k_start's L - 1 - b
    "free-order",       # a private id below an overflow id, or overflow ids not descending towards the top
    "free-backed",      # a free overflow id that still holds a shared block
    "inuse-unbacked",   # an overflow id in use without a shared block
    "link-range",       # a root, child link or FIFO block that is no id in use or has no row
    "stale-link",       # an expanded block with a child pointer on a slot that is not legal
    "dup-link",         # a block reached twice: two links, or linked and in flight, or in both trees
    "dup-inflight",     # a block twice in the FIFO
    "linked-free:root", "linked-free:other", "inflight-free",    # a block of the tree / the other tree / the FIFO on the free stack
    "root-free",        # the root block itself (of either tree) is on the free stack
    "leak-overwritten", # in use, outside every set; its parent is reached and that slot links ANOTHER block
    "leak-unlinked",    # ... its parent is reached and that slot links nothing
    "leak-detached",    # ... its parent is not reached either (or is no block)
    "parent-mismatch",  # cB[p][s] == b but bParent[b] != p or bSlot[b] != s
    "root-parent",      # a root whose bParent is not -1
    "fifo-view", "fifo-parent", "fifo-slot",   # FIFO entry vs bParent / bSlot; its parent not reached; its slot not legal there
    "failed-holds",     # a failed (or never started) slot with a backed map entry
    "pool-range",       # poolCtl outside its bounds, or a shared id outside [0, pool_blocks)
    "pool-missing",     # a shared id in none of the three places
    "pool-dup",         # a shared id in two places
)


class Violations(list):
    """The violations of one audit (empty = clean); `.stats` carries that audit's measurements."""

    def kinds(self):
        return sorted(set(v.split(": ")[1] for v in self))


class Tally(object):
    """Measurements over the audits of one test, for its BLOCK_AUDIT line."""

    def __init__(self):
        self.audits = self.in_use = self.in_flight = self.deepest = self.backed = 0
        self.audits_fifo = self.audits_empty = self.followed = self.fresh = self.failed_slots = 0

    def add(self, v, games=None):
        """v: the Violations of one audit; games: its dumps, for the count of what became of the other player's tree"""
        s = v.stats
        self.audits += 1
        self.in_use = max(self.in_use, s["in_use"])
        self.in_flight = max(self.in_flight, s["in_flight"])
        self.deepest = max(self.deepest, s["deepest"])
        self.backed = max(self.backed, s["backed"])
        self.audits_fifo += s["in_flight"] > 0
        self.audits_empty += s["in_flight"] == 0
        if games is not None:
            followed, fresh = other_tree_fates(games)
            self.followed += followed
            self.fresh += fresh
        self.failed_slots = max(self.failed_slots, s["failed"])
        return v

    def line(self, name):
        return ("BLOCK_AUDIT %s: audits=%d blocks_in_use_max=%d in_flight_max=%d deepest_chain=%d overflow_backed_max=%d"
                % (name, self.audits, self.in_use, self.in_flight, self.deepest, self.backed))


def other_tree_fates(games):
    """A measurement, no part of the invariant: in how many two-model games of these dumps (a list, or a dict slot -> dump) the
    other player's tree has just (followed the move, been rebuilt from a fresh block).  play_move swaps the two trees before its
    launch ends, so the tree that was the other player's during the move is the ROOT of the first dump after it, while the slot
    waits for that root's evaluation: expanded when it followed the move, an unexpanded fresh block (bSlot == -2) when it did
    not hold it.  other_root is the mover's chosen child by then and always expanded."""
    followed = fresh = 0
    for d in (games.values() if isinstance(games, dict) else games):
        if d["error"] != 0 or d["phase"] != PH_WAIT_ROOT or d["other_root"] < 0 or "bSlot" not in d:
            continue
        if 0 <= d["root_blk"] < len(d["bSlot"]):
            if d["bSlot"][d["root_blk"]] == -2:
                fresh += 1
            else:
                followed += 1
    return followed, fresh


def _legal_matrix(d):
    rows = d["cB"].shape[0]
    w = np.asarray(d["legal"], dtype=np.uint32).reshape(rows, d["NW"])
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    return bits.reshape(rows, 32 * d["NW"])[:, :d["A"]].astype(bool)


def audit_game(slot, d, stats=None):
    """Items 1-7 for one slot's dump.  A dump without the block arrays (block_state(slot, blocks=False)) gets items 1-3."""
    out = []
    st = stats if stats is not None else {}
    for k in ("in_use", "in_flight", "deepest", "backed", "failed"):
        st.setdefault(k, 0)

    def bad(kind, detail):
        assert kind in KINDS, kind
        out.append("game %d: %s: %s" % (slot, kind, detail))

    omap = np.asarray(d["ovfMap"], dtype=np.int64)
    backed_idx = np.flatnonzero(omap >= 0)
    if d["error"] != 0 or d["phase"] == PH_IDLE:
        if d["error"] != 0:
            st["failed"] += 1
        if len(backed_idx):
            bad("failed-holds", "%s slot holds shared blocks behind overflow indices %s"
                % ("failed" if d["error"] else "never started", backed_idx[:8].tolist()))
        return out
    cap, L, ovf_cap, A, F = d["cap"], d["L"], d["ovf_cap"], d["A"], d["F"]
    ft, Lu = d["free_top"], d["cap"] + d["ovf_hi"]
    st["backed"] += len(backed_idx)
    # 1. the counters
    if not (0 <= d["ovf_hi"] <= ovf_cap and 0 <= L - Lu <= ft <= L):
        bad("range", "free_top %d, ovf_hi %d: want 0 <= L - Lu = %d <= free_top <= L = %d" % (ft, d["ovf_hi"], L - Lu, L))
        return out
    if not d["min_free"] <= ft:
        bad("range", "min_free %d > free_top %d" % (d["min_free"], ft))
    if len(backed_idx) and d["ovf_hi"] < backed_idx[-1] + 1:
        bad("ovf-hi", "overflow index %d is backed, ovf_hi is %d" % (backed_idx[-1], d["ovf_hi"]))
    if not (0 <= d["fifo_head"] <= d["fifo_tail"] <= d["fifo_head"] + F):
        bad("range", "fifo_head %d, fifo_tail %d, ring of %d" % (d["fifo_head"], d["fifo_tail"], F))
        return out
    # 2. the free stack
    free = np.asarray(d["freeList"][:ft], dtype=np.int64)
    nb = L - Lu
    if np.any((free < 0) | (free >= L)):
        bad("free-range", "entries %s" % free[(free < 0) | (free >= L)][:8].tolist())
        return out
    cnt = np.bincount(free, minlength=L)
    if np.any(cnt > 1):
        bad("free-dup", "ids %s are on the free stack more than once" % np.flatnonzero(cnt > 1)[:8].tolist())
    if not np.array_equal(free[:nb], L - 1 - np.arange(nb)):
        i = int(np.flatnonzero(free[:nb] != L - 1 - np.arange(nb))[0])
        bad("free-bottom", "entry %d holds %d, k_start put %d there" % (i, free[i], L - 1 - i))
    top = free[nb:]
    if np.any(top >= Lu):
        bad("free-range", "ids %s above the never-used bottom are beyond cap + ovf_hi = %d" % (top[top >= Lu][:8].tolist(), Lu))
    is_ovf = top >= cap
    if is_ovf.any() and (~is_ovf).any() and np.flatnonzero(is_ovf)[-1] > np.flatnonzero(~is_ovf)[0]:
        bad("free-order", "overflow id %d lies above private id %d: it would pop first"
            % (top[np.flatnonzero(is_ovf)[-1]], top[np.flatnonzero(~is_ovf)[0]]))
    ov = top[is_ovf]
    if len(ov) > 1 and np.any(np.diff(ov) >= 0):
        i = int(np.flatnonzero(np.diff(ov) >= 0)[0])
        bad("free-order", "free overflow ids do not descend towards the top: %d below %d" % (ov[i], ov[i + 1]))
    # 3. in use <=> backed
    is_free = cnt > 0
    in_use = np.flatnonzero(~is_free[:Lu])
    st["in_use"] += len(in_use)
    ids = cap + np.arange(ovf_cap)
    used_o = np.zeros(ovf_cap, bool)
    used_o[:d["ovf_hi"]] = ~is_free[cap:Lu]
    if np.any(used_o & (omap < 0)):
        bad("inuse-unbacked", "overflow ids %s are in use and not backed" % ids[used_o & (omap < 0)][:8].tolist())
    if np.any(~used_o & (omap >= 0)):
        bad("free-backed", "overflow ids %s are free (or never used) and hold shared blocks %s"
            % (ids[~used_o & (omap >= 0)][:8].tolist(), omap[~used_o & (omap >= 0)][:8].tolist()))
    if "cB" not in d:
        return out
    # 4. the child-link view
    cB, bP, bS = np.asarray(d["cB"]), np.asarray(d["bParent"]), np.asarray(d["bSlot"])
    rows = cB.shape[0]
    legal = _legal_matrix(d)

    def has_row(b):
        return 0 <= b < rows and (b < cap or omap[b - cap] >= 0)

    free_kind = {"root": "linked-free:root", "other": "linked-free:other", "fifo": "inflight-free"}

    def usable(b, name, what):
        """a block some view refers to: an id of [0, Lu) with a row; a freed overflow id has none (its block was released)"""
        if 0 <= b < Lu and has_row(b):
            return True
        if 0 <= b < Lu and is_free[b]:
            bad("root-free" if what == "root block" else free_kind[name], "%s %d (%s) is on the free stack, its shared block released" % (what, b, name))
        else:
            bad("link-range", "%s %d (%s) is no block of this game" % (what, b, name))
        return False

    owner = {}                     # block -> the set that reached it first
    deepest = 0
    # every link of every row at once (rows of free or in-flight blocks hold stale links: the walk never follows those)
    lp, ls = np.nonzero(legal & (cB[:, :A] >= 0))
    lc = cB[lp, ls]
    first = np.searchsorted(lp, np.arange(rows + 1))
    stale = ~legal & (cB[:, :A] != -1)

    def walk(root, name):
        nonlocal deepest
        if not usable(root, name, "root block"):
            return
        if root in owner:
            bad("dup-link", "%s block %d is already in %s" % (name, root, owner[root]))
            return
        owner[root] = name
        if bP[root] != -1:
            bad("root-parent", "%s block %d has bParent %d" % (name, root, bP[root]))
        if bS[root] == -2:         # an unexpanded root: its child arrays are stale
            return
        stack = [(root, 0)]
        while stack:
            b, depth = stack.pop()
            deepest = max(deepest, depth)
            if stale[b].any():
                s = int(np.flatnonzero(stale[b])[0])
                bad("stale-link", "block %d (%s) has cB %d on slot %d, which is not legal" % (b, name, cB[b, s], s))
            for i in range(first[b], first[b + 1]):
                s, c = int(ls[i]), int(lc[i])
                if not usable(c, name, "cB[%d][%d] =" % (b, s)):
                    continue
                if c in owner:
                    bad("dup-link", "block %d linked from %d slot %d is already in %s" % (c, b, s, owner[c]))
                    continue
                owner[c] = name
                if bP[c] != b or bS[c] != s:
                    bad("parent-mismatch", "cB[%d][%d] = %d, but bParent / bSlot of %d are %d / %d" % (b, s, c, c, bP[c], bS[c]))
                stack.append((c, depth + 1))

    walk(d["root_blk"], "root")
    if d["other_root"] >= 0:
        walk(d["other_root"], "other")
    st["deepest"] = max(st["deepest"], deepest)
    # 5. the leaves in flight, and 7. their two views
    fP, fS, fB = d["fParent"], d["fSlot"], d["fBlk"]
    n_fly = 0
    for fi in range(d["fifo_head"], d["fifo_tail"]):
        i = fi % F
        b, p, s = int(fB[i]), int(fP[i]), int(fS[i])
        n_fly += 1
        if not usable(b, "fifo", "FIFO entry %d: block" % fi):
            continue
        if b in owner:
            bad("dup-inflight" if owner[b] == "fifo" else "dup-link", "FIFO entry %d: block %d is already in %s" % (fi, b, owner[b]))
            continue
        owner[b] = "fifo"
        if bP[b] != p or bS[b] != s:
            bad("fifo-view", "FIFO entry %d: block %d has bParent / bSlot %d / %d, the entry says %d / %d" % (fi, b, bP[b], bS[b], p, s))
        if owner.get(p) not in ("root", "other"):
            bad("fifo-parent", "FIFO entry %d: parent %d of block %d is not in a tree" % (fi, p, b))
        elif not (0 <= s < A and legal[p, s]):
            bad("fifo-slot", "FIFO entry %d: slot %d is not legal in block %d" % (fi, s, p))
    st["in_flight"] += n_fly
    # 6. the partition
    for b, name in sorted(owner.items()):
        if is_free[b]:
            bad("root-free" if name != "fifo" and b in (d["root_blk"], d["other_root"]) else free_kind[name],
                "block %d (%s) is on the free stack" % (b, name))
    for b in in_use:
        b = int(b)
        if b in owner:
            continue
        p, s = (int(bP[b]), int(bS[b])) if has_row(b) else (-9, -9)
        if owner.get(p) in ("root", "other") and 0 <= s < A:
            c = int(cB[p, s])
            bad("leak-overwritten" if c >= 0 else "leak-unlinked",
                "block %d is in use, neither linked nor in flight; its parent %d (%s) holds %d on slot %d" % (b, p, owner[p], c, s))
        else:
            bad("leak-detached", "block %d is in use, neither linked nor in flight; its bParent / bSlot are %d / %d" % (b, p, s))
    return out


def audit_pool(games, pool):
    """The context partition.  `games` maps slot -> dump, ALL slots of the context (the map rows are what counts)."""
    out = []

    def bad(kind, detail):
        assert kind in KINDS, kind
        out.append("pool: %s: %s" % (kind, detail))

    c0, c1, c2 = pool["poolCtl"][:3]
    n = pool["pool_blocks"]
    if not (0 <= c2 <= c0 <= n and 0 <= c1 <= n):
        bad("pool-range", "poolCtl = %s with %d pool blocks" % ([c0, c1, c2], n))
        return out
    where = [("poolFree", np.asarray(pool["poolFree"][:c0], dtype=np.int64)), ("poolRet", np.asarray(pool["poolRet"][:c1], dtype=np.int64))]
    for slot, d in sorted(games.items()):
        m = np.asarray(d["ovfMap"], dtype=np.int64)
        where.append(("game %d" % slot, m[m >= 0]))
    cnt = np.zeros(n, np.int64)
    for name, ids in where:
        if np.any((ids < 0) | (ids >= n)):
            bad("pool-range", "%s holds shared ids %s" % (name, ids[(ids < 0) | (ids >= n)][:8].tolist()))
            return out
        cnt += np.bincount(ids, minlength=n)
    if np.any(cnt == 0):
        miss = np.flatnonzero(cnt == 0)
        bad("pool-missing", "%d shared blocks are nowhere: %s" % (len(miss), miss[:8].tolist()))
    for b in np.flatnonzero(cnt > 1)[:8]:
        bad("pool-dup", "shared block %d is held by %s" % (b, " and ".join(nm for nm, ids in where for _ in range(int(np.sum(ids == b))))))
    return out


def audit(games, pool):
    """games: the dumps of ALL slots of one context (a list indexed by slot, or a dict slot -> dump); pool: its pool_state().
    Returns the Violations (a list; empty = clean).  Dumps without block arrays get items 1-3 and count in the pool partition."""
    if not isinstance(games, dict):
        games = dict(enumerate(games))
    v = Violations()
    v.stats = {}
    for slot in sorted(games):
        v.extend(audit_game(slot, games[slot], v.stats))
    v.extend(audit_pool(games, pool))
    return v


def dump_engine(eng, full=None):
    """The dumps of every slot of a SelfPlayEngine: block arrays for the slots in `full` (default: all), counters / free stack /
    map row for the rest."""
    G = eng.pool_info()["games"]
    return {s: eng.block_state(s, blocks=(full is None or s in full)) for s in range(G)}, eng.pool_state()
