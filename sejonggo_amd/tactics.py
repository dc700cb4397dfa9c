"""Chains, liberties and ladders on the device (include/sgo.h "chains and ladders", csrc/sgo_tactics.hip): per position the liberty
count of the chain on every point, the chains with one or two liberties, and for each of them whether an exhaustive reader
catches it -- with the attacker moving first (`capturable`) and even with the defender moving first (`dead`).

    from sejonggo_amd.tactics import tactics
    t = tactics(19, records)                 # packed records uint32 [R, 16 * NW], host or device
    for c in t.chains_of(0): print(c.anchor, c.liberties, c.capturable, c.dead, c.attack_move, c.defend_move)

records.RecordSet.tactics() reads every position of a game collection, engine.SessionEngine.tactics(slots) the positions of
session slots; GTP's `sgo-ladders` and `python -m sejonggo_amd.review --tactics` stand on them."""
import collections
import ctypes as C

import numpy as np

from ._packed import device_records

A_CAPTURED, D_CAPTURED, A_UNKNOWN, D_UNKNOWN, D_RAN = 1, 2, 4, 8, 16


class Chain(collections.namedtuple("Chain", "anchor colour size liberties status attack_move defend_move nodes")):
    """One row of the chain table.  colour +1 black / -1 white; attack_move / defend_move -1: none."""
    __slots__ = ()

    @property
    def capturable(self):
        """caught when the attacker moves first"""
        return bool(self.status & A_CAPTURED)

    @property
    def dead(self):
        """caught even when the defender moves first"""
        return bool(self.status & D_CAPTURED)

    @property
    def unknown(self):
        """a query ran out of its node or depth budget"""
        return bool(self.status & (A_UNKNOWN | D_UNKNOWN))


class Tactics(object):
    """libs uint8 [n, N], n_chains int32 [n] (the true number), chains int32 [n, max_chains, 8] (the first min(n_chains,
    max_chains) rows of each position)."""

    def __init__(self, size, libs, n_chains, chains):
        self.S, self.libs, self.n_chains, self.chains = size, libs, n_chains, chains

    def chains_of(self, i):
        k = min(int(self.n_chains[i]), self.chains.shape[1])
        return [Chain(*(int(v) for v in row)) for row in self.chains[i, :k]]


def tactics(size, records, index=None, max_chains=128):
    """sgo_tactics_dev on packed records (a numpy array or a device tensor, [R, 16 * NW] 32-bit words): a Tactics with one row per
    entry of `index` (None: every record in order); an index outside [0, R) gives the zero row."""
    import torch
    from . import _lib
    records, R, idx, n = device_records(size, records, index)
    lib, dev = _lib.load(), records.device
    libs = torch.zeros((n, size * size), dtype=torch.uint8, device=dev)
    n_chains = torch.zeros(n, dtype=torch.int32, device=dev)
    chains = torch.zeros((n, int(max_chains), 8), dtype=torch.int32, device=dev)
    _lib.check(lib.sgo_tactics_dev(C.c_int(size), C.c_int(n), _lib.ptr(records), C.c_int(R), _lib.ptr(idx), C.c_int(int(max_chains)),
                                   _lib.ptr(libs), _lib.ptr(n_chains), _lib.ptr(chains), _lib.stream_ptr()), "sgo_tactics_dev")
    return Tactics(size, libs.cpu().numpy(), n_chains.cpu().numpy(), chains.cpu().numpy())


def format_chain(c, vertex):
    """`sgo-ladders` line of a Chain: `D4 black size 3 liberties 2 capturable attack E4 defend none`"""
    move = lambda a: vertex(a) if a >= 0 else "none"                                     # noqa: E731
    return "%s %s size %d liberties %d %s attack %s defend %s" % (
        vertex(c.anchor), "black" if c.colour > 0 else "white", c.size, c.liberties, "dead" if c.dead else "capturable",
        move(c.attack_move), move(c.defend_move))


# ---- game review: which moves ran out a ladder that does not work, which left a capturable chain standing ----------------------
def chain_points(size, stones, start):
    """the points of the chain on `start`: stones int8 [N], +1 black / -1 white / 0 empty"""
    N, seen, todo = size * size, {start}, [start]
    while todo:
        a = todo.pop()
        x = a % size
        for b in (a - 1 if x else -1, a + 1 if x < size - 1 else -1, a - size, a + size):
            if 0 <= b < N and b not in seen and stones[b] == stones[start]:
                seen.add(b)
                todo.append(b)
    return seen


def review_flags(size, action, colour, stones_before, chains_before, stones_after, chains_after, libs_after):
    """Flags of one move from the stones (int8 [N]) and chain lists (Tactics.chains_of) of the position before and after it:
    `ladder`  the move is a liberty of one of the mover's own chains that was dead even with the defender first, and the chain
              holding the stone after the move is capturable;
    `missed`  an opponent chain of three or more stones was capturable before the move and still stands after it with two or more
              liberties.
    A pass gets no `ladder`."""
    flags = []
    N = size * size
    if 0 <= action < N and stones_after[action] == colour:
        x = action % size
        near = {a for a in (action - 1 if x else -1, action + 1 if x < size - 1 else -1, action - size, action + size) if 0 <= a < N}
        ran = any(c.colour == colour and c.dead and near & chain_points(size, stones_before, c.anchor) for c in chains_before)
        if ran:
            anchor = min(chain_points(size, stones_after, action))
            if any(c.anchor == anchor and c.capturable for c in chains_after):
                flags.append("ladder")
    for c in chains_before:
        if c.colour == -colour and c.size >= 3 and c.capturable and stones_after[c.anchor] == -colour and libs_after[c.anchor] >= 2:
            flags.append("missed")
            break
    return flags


def stones_of(size, planes):
    """int8 [n, N] (+1 black, -1 white) from the first two planes of packed records, uint32 [n, >= 2 * NW]"""
    N, NW = size * size, (size * size + 31) // 32
    w = np.ascontiguousarray(np.asarray(planes)[:, :2 * NW]).view(np.uint32).astype("<u4")
    bits = np.unpackbits(w.view(np.uint8).reshape(len(w), 2, 4 * NW), axis=-1, bitorder="little")[:, :, :N]
    return bits[:, 0].astype(np.int8) - bits[:, 1].astype(np.int8)
