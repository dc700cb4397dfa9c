"""Deterministic stand-in policy/value nets (the reference's tests use the same idea:
``DummyModel`` in test/tests.py:34-49).

Every net here honours the model contract of the reference (model.py:57,80,90):
``predict_on_batch(X[n,S,S,17]) -> [policy float32[n,S*S+1], value float32[n,1]]`` and a
``.name``.  They exist so that self-play can be driven without trained weights and so that the
GPU engine, the CPU oracle and the Python reference can be fed *bit-identical* priors:

* ``UniformNet``   p = 1/(S*S+1), v = 0             (BASELINE.json configs[0] "uniform-random stub")
* ``DummyNet``     p ∝ reversed(range(1, A+1)), v=1 (restates DummyModel, tests.py:34-49)
* ``HashNet``      p, v are dyadic rationals computed from an integer hash of the 17 planes, so
                   no floating-point rounding happens anywhere and numpy / torch-CPU /
                   torch-ROCm agree to the bit.
* ``TableNet``     row ``hash(position) mod K`` of a fixed table of what a trained head emits: full 24-bit
                   mantissas at several sharpnesses, exact zeros, float32 denormals, v = +-1.0 / +-0.0.
                   Integer hash plus one gather, so the three back-ends still agree to the bit.

Each class works on numpy arrays and on torch tensors (any device); the arithmetic is integer
until the final exact scaling.
"""
import numpy as np

_HASH_MOD = 1000003


def _hash_weights(size):
    """Fixed integer weight table [S,S,17], values in [1, 2^20)."""
    n = size * size * 17
    w = np.empty(n, dtype=np.int64)
    s = 88172645463325252 & 0xFFFFFFFFFFFFFFFF
    for i in range(n):  # xorshift64, seed fixed
        s ^= (s << 13) & 0xFFFFFFFFFFFFFFFF
        s ^= s >> 7
        s ^= (s << 17) & 0xFFFFFFFFFFFFFFFF
        w[i] = (s >> 11) % ((1 << 20) - 1) + 1
    return w.reshape(size, size, 17)


class _Base(object):
    def __init__(self, size, name):
        self.size = size
        self.A = size * size + 1
        self.name = name

    def predict(self, X):
        p, v = self.predict_on_batch(X)
        return p[0], v[0]

    def _on(self, device):
        """The constant prior vector on `device`, copied there once (a per-call host-to-device copy would also be illegal inside
        a captured launch chain)."""
        import torch
        cache = self.__dict__.setdefault("_dev", {})
        if device not in cache:
            cache[device] = torch.from_numpy(self._p).to(device)
        return cache[device]


class UniformNet(_Base):
    def __init__(self, size, name="uniform_stub"):
        _Base.__init__(self, size, name)
        self._p = np.full((self.A,), np.float32(1.0) / np.float32(self.A), dtype=np.float32)

    def predict_on_batch(self, X):
        n = X.shape[0]
        if isinstance(X, np.ndarray):
            return np.tile(self._p, (n, 1)), np.zeros((n, 1), dtype=np.float32)
        import torch
        p = self._on(X.device)
        return p.unsqueeze(0).repeat(n, 1), torch.zeros((n, 1), dtype=torch.float32, device=X.device)


class DummyNet(_Base):
    def __init__(self, size, name="dummy_model"):
        _Base.__init__(self, size, name)
        pol = np.zeros((1, self.A), dtype=np.float32)
        pol[0, :] = list(reversed(range(1, self.A + 1)))
        pol[:, :] /= np.sum(pol, axis=1)[:, np.newaxis]
        self._p = pol[0].copy()

    def predict_on_batch(self, X):
        n = X.shape[0]
        if isinstance(X, np.ndarray):
            return np.tile(self._p, (n, 1)), np.ones((n, 1), dtype=np.float32)
        import torch
        p = self._on(X.device)
        return p.unsqueeze(0).repeat(n, 1), torch.ones((n, 1), dtype=torch.float32, device=X.device)


class HashNet(_Base):
    """Board-dependent, rounding-free pseudo net."""

    def __init__(self, size, name="hash_stub", variant=0):
        _Base.__init__(self, size, name)
        self._w = _hash_weights(size)
        if variant:                           # a second, different pseudo net (two-model evaluation games)
            self._w = np.roll(self._w.reshape(-1), 7 * variant).reshape(self._w.shape) + variant
        self._mul = (np.arange(self.A, dtype=np.int64) * (7919 + 2 * variant) + 13 + variant)
        self._wt = {}

    def predict_on_batch(self, X):
        if isinstance(X, np.ndarray):
            x = X.astype(np.int64).reshape(X.shape[0], -1)
            h = x @ self._w.reshape(-1)
            base = np.mod(h, _HASH_MOD)
            raw = np.mod((base[:, None] + 1) * self._mul[None, :], 1009) + 1
            p = raw.astype(np.float32) * np.float32(2.0 ** -19)
            v = (np.mod(base, 2049) - 1024).astype(np.float32) * np.float32(2.0 ** -10)
            return p, v.reshape(-1, 1)
        import torch
        dev = X.device
        if dev not in self._wt:
            self._wt[dev] = (torch.from_numpy(self._w.reshape(-1)).to(dev),
                             torch.from_numpy(self._mul).to(dev))
        w, mul = self._wt[dev]
        x = X.to(torch.int64).reshape(X.shape[0], -1)
        h = (x * w.unsqueeze(0)).sum(dim=1)
        base = torch.remainder(h, _HASH_MOD)
        raw = torch.remainder((base.unsqueeze(1) + 1) * mul.unsqueeze(0), 1009) + 1
        p = raw.to(torch.float32) * (2.0 ** -19)
        v = (torch.remainder(base, 2049) - 1024).to(torch.float32) * (2.0 ** -10)
        return p, v.reshape(-1, 1)


def _table(size, K):
    """(T float32[K, A], V float32[K]) of TableNet.  Every value is assembled from a float32 BIT PATTERN (sign, exponent field,
    23 random mantissa bits drawn with RandomState.randint): no libm call and no floating-point reduction takes part, so every
    host builds the same bytes (tests/test_host_logic.py pins their SHA-256)."""
    A = size * size + 1
    rng = np.random.RandomState(977 + size)
    e0 = 127 - int(A).bit_length()                     # exponent field of [2^-ceil(log2 A), 2 * that): a flat row sums to about 1
    hot = (size * size) // 2                           # the centre point: it is taken within the first plies of most games

    def f32(expo, mant, sign=0):
        bits = (np.asarray(sign, np.int64) << 31) | (np.asarray(expo, np.int64) << 23) | np.asarray(mant, np.int64)
        return bits.astype(np.uint32).view(np.float32)

    T = np.zeros((K, A), dtype=np.float32)
    for k in range(K):
        mant = rng.randint(0, 1 << 23, size=A)
        kind = k % 8
        peak = int(rng.randint(0, A))
        if kind == 0:                                  # flat: one binade
            row = f32(np.full(A, e0), mant)
        elif kind == 1:                                # mild: four binades
            row = f32(e0 + rng.randint(-3, 1, size=A), mant)
        elif kind == 2:                                # sharp: twenty binades and a few large entries
            row = f32(e0 + rng.randint(-20, 1, size=A), mant)
            big = rng.randint(0, A, size=3)
            row[big] = f32(rng.randint(122, 126, size=3), rng.randint(0, 1 << 23, size=3))
        elif kind in (3, 4, 5):
            # near one-hot (softmax of logit gaps up to and beyond 87): the rest is a mix of exact zeros, denormals (exponent
            # field 0) and tiny normals; kind 4 puts the peak on the centre point, kind 5 on the pass
            cls = rng.randint(0, 3, size=A)
            expo = np.where(cls == 2, rng.randint(1, 60, size=A), 0)
            row = f32(expo, np.where(cls == 0, 0, mant))
            peak = {3: peak, 4: hot, 5: A - 1}[kind]
            row[peak] = f32(126, (1 << 23) - 1 - int(rng.randint(0, 256)))
        elif kind == 6:                                # two close rivals, full mantissas, over a flat floor
            row = f32(np.full(A, e0 - 4), mant)
            a, b = rng.choice(A, size=2, replace=False)
            m = int(rng.randint(0, (1 << 23) - 1))
            row[a], row[b] = f32(125, m), f32(125, m + 1)
        else:                                          # every entry the same value
            row = np.full(A, np.float32(1.0) / np.float32(A), dtype=np.float32)
        T[k] = row
    V = f32(rng.randint(117, 127, size=K), rng.randint(0, 1 << 23, size=K), rng.randint(0, 2, size=K))
    V[:4] = np.array([1.0, -1.0, 0.0, -0.0], dtype=np.float32)
    V[4:8] = f32([126, 126, 1, 0], [(1 << 23) - 1, (1 << 23) - 1, 0, 1], [0, 1, 0, 1])   # +-(1 - 2^-24), smallest normal, a denormal
    return T, V


class TableNet(_Base):
    """Board-dependent net with the value domain of a trained policy / value head: row ``hash mod K`` of _table()."""
    K = 128

    def __init__(self, size, name="table_stub"):
        _Base.__init__(self, size, name)
        self._w = _hash_weights(size)
        self._T, self._V = _table(size, self.K)
        self._wt = {}

    def predict_on_batch(self, X):
        if isinstance(X, np.ndarray):
            x = X.astype(np.int64).reshape(X.shape[0], -1)
            h = np.mod(np.mod(x @ self._w.reshape(-1), _HASH_MOD), self.K)
            return self._T[h], self._V[h].reshape(-1, 1)
        import torch
        dev = X.device
        if dev not in self._wt:
            self._wt[dev] = (torch.from_numpy(self._w.reshape(-1)).to(dev), torch.from_numpy(self._T).to(dev),
                             torch.from_numpy(self._V).to(dev))
        w, T, V = self._wt[dev]
        x = X.to(torch.int64).reshape(X.shape[0], -1)
        h = torch.remainder(torch.remainder((x * w.unsqueeze(0)).sum(dim=1), _HASH_MOD), self.K)
        return T.index_select(0, h), V.index_select(0, h).reshape(-1, 1)


def make_stub(kind, size):
    if kind == "table":
        return TableNet(size)
    if kind == "hash2":
        return HashNet(size, name="hash_stub_2", variant=1)
    return {"uniform": UniformNet, "dummy": DummyNet, "hash": HashNet}[kind](size)
