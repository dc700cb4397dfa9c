"""Shared helpers for the parity tests (fixture loading, canonical tree hashing)."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def sha8(arr):
    return np.frombuffer(hashlib.sha1(np.ascontiguousarray(arr).tobytes()).digest()[:8], dtype=np.uint8)


def unpack_mask(bits, A):
    return np.unpackbits(bits)[:A]


def name_of(z, key):
    return bytes(z[key]).decode()


# 08 = BASELINE config 5 (19x19, 1600 sims, 32-leaf rounds); 09..11 and 18 are the two-model games; 12..14: 13x13 / 7x7,
# energies 4 / 16; 15..17: full-mantissa priors (stub_nets.TableNet) at 9x9, 5x5 and 19x19 / 400 sims
ASYNC_FILES = ["async_%02d.npz" % i for i in list(range(9)) + [12, 13, 14, 15, 16, 17]]
TWO_MODEL_FILES = ["async_09.npz", "async_10.npz", "async_11.npz", "async_18.npz"]


def selector_tables(name):
    """[(A, {P, N, Q, V, EX, F64, out_vl, out_one, out_top[, cls, I, J]}, class names)] of a selector fixture: puct.npz is one
    table set of A = 82; puct_ties.npz holds one set per size, its arrays suffixed _<A>."""
    z = load(name)
    keys = ("P", "N", "Q", "V", "EX", "F64", "out_vl", "out_one", "out_top")
    if "sizes" not in z.files:
        return [(z["P"].shape[1], {k: z[k] for k in keys}, None)]
    names = bytes(z["cls_names"]).decode().split("\n")
    return [(int(A), {k: z["%s_%d" % (k, A)] for k in keys + ("cls", "I", "J")}, names) for A in z["sizes"]]


def dict_tree_hash(root):
    """Canonical serialisation of a host dict tree (same record as tests/golden/gen_golden.py:_tree_hash and
    oracle ora_game_tree_serialize): pre-order, ascending action, <i a, i count, f value, f mean, d p, i vloss, i expanded>."""
    import struct
    h = hashlib.sha1()
    n_nodes = [0]

    def rec(node):
        for a in node["subtree"]:
            c = node["subtree"][a]
            h.update(struct.pack("<iiffdii", int(a), int(c["count"]), float(c["value"]), float(c["mean_value"]),
                                 float(c["p"]), int(c.get("virtual_loss", 0)), 1 if c["subtree"] else 0))
            n_nodes[0] += 1
            if c["subtree"]:
                rec(c)
    rec(root)
    return h.digest()[:16], n_nodes[0]


SYNC_FILES = ["sync_%02d.npz" % i for i in range(4)]


# ---- the reference's unit tests recorded as data (tests/golden/units_S9.npz, gen_golden.py child_units) ----------
_TYPES = {0: int, 1: float, 2: np.float32, 3: np.float64, 4: int}


def deser_tree(ints, flts):
    """Rebuilds a dict tree from gen_golden.ser_tree rows, with the recorded key set and scalar types per node."""
    root = None
    stack = []
    for (depth, action, m, index, count, vloss, has_parent, tv, tm, tp), (value, mean, p) in zip(ints, flts):
        node = {}
        if m & 1:
            node['index'] = int(index)
        if m & 2:
            node['count'] = int(count)
        if m & 4:
            node['virtual_loss'] = int(vloss)
        if m & 8:
            node['value'] = _TYPES[int(tv)](value)
        if m & 16:
            node['mean_value'] = _TYPES[int(tm)](mean)
        if m & 32:
            node['p'] = _TYPES[int(tp)](p)
        node['subtree'] = None if m & 128 else {}
        del stack[int(depth):]
        if stack:
            stack[-1]['subtree'][int(action)] = node
            if m & 64:
                node['parent'] = stack[-1] if has_parent else None
        else:
            root = node
            if m & 64:
                node['parent'] = None
        stack.append(node)
    return root


def ser_tree(root):
    """Same rows as tests/golden/gen_golden.py:ser_tree (kept in step with it)."""
    def tcode(v):
        if isinstance(v, np.float32):
            return 2
        if isinstance(v, np.float64):
            return 3
        if isinstance(v, np.integer):
            return 4
        if isinstance(v, float):
            return 1
        return 0
    ints, flts = [], []

    def row(node, depth, action):
        m = 0
        for bit, k in ((1, "index"), (2, "count"), (4, "virtual_loss"), (8, "value"), (16, "mean_value"), (32, "p"), (64, "parent")):
            if k in node:
                m |= bit
        if node.get("subtree") is None:
            m |= 128
        ints.append([depth, action, m, node.get("index", 0), node.get("count", 0), node.get("virtual_loss", 0),
                     1 if node.get("parent") is not None else 0,
                     tcode(node.get("value", 0)), tcode(node.get("mean_value", 0)), tcode(node.get("p", 0))])
        flts.append([float(node.get("value", 0)), float(node.get("mean_value", 0)), float(node.get("p", 0))])
        for a, c in (node.get("subtree") or {}).items():
            row(c, depth + 1, int(a))

    row(root, 0, -1)
    return np.array(ints, dtype=np.int64), np.array(flts, dtype=np.float64)


def unit_calls(z):
    """The recorded rule / symmetry calls: dicts {fn, test, ins: [(kind, array)], out: (kind, array)}."""
    out = []
    for i in range(int(z["n_calls"])):
        p = "c%03d_" % i
        ins = [(int(z[p + "in%d_k" % j]), z[p + "in%d" % j]) for j in range(int(z[p + "nin"]))]
        out.append({"fn": name_of(z, p + "fn"), "test": name_of(z, p + "test"), "ins": ins,
                    "out": (int(z[p + "out_k"]), z[p + "out"])})
    return out


def unit_value(kv):
    """(kind, array) -> python value: 0 None, 1 ndarray, 2 int, 3 list of tuples, 4 dict, 5 float"""
    kind, arr = kv
    if kind == 0:
        return None
    if kind == 1:
        return np.array(arr)
    if kind == 2:
        return int(arr)
    if kind == 3:
        return [tuple(int(t) for t in e) for e in arr]
    if kind == 4:
        return {int(k): int(v) for k, v in arr}
    return float(arr)


def read_sample(path):
    """(board, policy_target, value_target) of a sample.h5, through whatever HDF5 reader exists: h5py, the HDF5 C library
    (h5lite), or -- for files of the pure-Python writer only -- hdf5_min's own reader."""
    try:
        import h5py as mod
    except Exception:
        from sejonggo_amd import h5lite as mod
        if not mod.available():
            from sejonggo_amd.hdf5_min import read_datasets
            r = read_datasets(path)
            return r['board'], r['policy_target'], r['value_target']
    with mod.File(path, "r") as f:
        return f['board'][...], f['policy_target'][...], f['value_target'][()]


class PackedProbe(object):
    """A stub net behind the resident net's PACKED-RECORD input contract (engine route: net.predict_packed -> sgo_stem_packed_dev),
    built so that the evaluation stays rounding-free: the real stem kernel runs with 0/1 weights that copy plane c of tap t into
    output channel 16 t + c (and the colour term into channel 144), the full S x S x 17 board tensor is re-assembled from those
    (S-2)^2 x 145 values -- every board point is under some tap of some output pixel -- and handed to the hash net.  Any wrong bit,
    tap, symmetry, colour flip or list index in the kernel changes the game."""
    packed_ok = True

    def __init__(self, net, S):
        import torch
        from sejonggo_amd import _lib
        self.net, self.name, self.S, self.t = net, net.name, S, S - 2
        self._lib, self.lib = _lib, _lib.require_gpu()
        w10 = torch.zeros(256, 10, 16)
        for t in range(9):
            for c in range(16):
                w10[16 * t + c, t, c] = 1.0
        self.w10 = w10.half().cuda().contiguous()
        self.bias = torch.zeros(256, dtype=torch.float16, device="cuda")
        wcol = torch.zeros(256)
        wcol[144] = 1.0                                   # relu(+1) = 1 black to play, relu(-1) = 0 white to play
        self.wcol = wcol.cuda().contiguous()
        ys = torch.arange(S)
        o = (ys - 1).clamp(0, S - 3)                      # an output pixel row whose window covers board row y, and the tap row
        d = ys - o
        self.oy, self.ox = o.cuda()[:, None].expand(S, S), o.cuda()[None, :].expand(S, S)
        self.tap = (d[:, None] * 3 + d[None, :]).cuda()

    def predict_packed(self, records_ptr, index_ptr, n, k=0, k_dev_ptr=None):
        import torch
        S, t = self.S, self.t
        y = torch.full((n, t, t, 256), 7.0, dtype=torch.float16, device="cuda")
        self._lib.check(self.lib.sgo_stem_packed_dev(S, n, records_ptr, index_ptr, int(k), k_dev_ptr, self.w10.data_ptr(),
                                                     self.bias.data_ptr(), self.wcol.data_ptr(), y.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), "sgo_stem_packed_dev")
        capturing = torch.cuda.is_current_stream_capturing()      # captured rounds: no host read-backs inside the graph
        if not capturing:
            assert float(y[..., 145:].abs().max()) == 0.0
        g = y[:, self.oy, self.ox, :]                                                  # [n, S, S, 256]
        ch = (self.tap[..., None] * 16 + torch.arange(16, device="cuda"))[None].expand(n, S, S, 16)
        planes = torch.gather(g, 3, ch)
        col = (2.0 * y[:, 0, 0, 144] - 1.0)[:, None, None, None].expand(n, S, S, 1)
        X = torch.cat([planes, col.to(planes.dtype)], dim=3)
        if not capturing:
            assert bool(((X[..., :16] == 0) | (X[..., :16] == 1)).all())
        return self.net.predict_on_batch(X)

    def predict_on_batch(self, X):
        raise AssertionError("the engine must take the packed-record route for this net")
