"""Whole-net parity on calibrated nets (tests/netcal.py): the resident fp16 net on its own routes against a float64 forward of
the same fp16 weights, with bounds that a wrong kernel cannot pass (tests/test_net_parity_power.py shows, on CPU, that every
fault of netcal.MUTATIONS moves the logit metric by >= 2 * LOGIT_TOL while the fp16 rounding model stays within LOGIT_TOL / 2).

* engine route (predict_packed: packed records -> sgo_stem_packed_dev -> tower -> heads) at 19x19 x 20 blocks and at 9x9, 5x5,
  7x7 and 13x13 x 4 blocks (every size size_ok() accepts; the last three calibrated with centred heads, so that all four head
  channels are alive), on positions board_advance itself played from the opening to a nearly full board (a playout passes
  when nothing else is legal, so the late 5x5 plies are valid), all 8 symmetries, ragged batches
  (1 and 37 rows through an index list, 64 rows whole) and the headline 8 192 at 19x19 (sampled rows, first and last
  included), on each tower kernel: k_conv4w (the default), k_conv8w and k_conv4r;
* tensor route (predict_on_batch on the channel-padded tensor: k_stem -> tower -> heads) on the same positions;
* negative controls on the real kernels with valid but wrong data: the reference under symmetry k + 1, and the net with one
  conv's filter bank taps rolled -- each must exceed 2 * LOGIT_TOL.

One NET_PARITY line per configuration reports the measured errors.
"""
import numpy as np
import pytest

from tests import netcal
from tests.test_gpu_baseline_nets import _playout_records

pytestmark = pytest.mark.gpu

CONFIGS = [(19, 20, (0, 30, 120, 250)), (9, 4, (0, 10, 30, 60)),
           (5, 4, (0, 4, 10, 16)), (7, 4, (0, 6, 16, 32)), (13, 4, (0, 20, 60, 110))]     # tower shapes 3x3, 5x5 and 11x11
KERNELS = ("k_conv4w", "k_conv8w", "k_conv4r")
N = 64
P_STATED = 2e-3          # SURVEY.md 8c's probability bound, which the calibrated nets meet as well


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


class _Case(object):
    """A calibrated net, its device-side weights for the reference, the played records and the float64 reference per
    (ply, symmetry, route), computed once and shared by the three tower kernels."""

    def __init__(self, L, S, blocks, plies):
        import torch
        self.L, self.lib = L, L.load()
        self.S, self.blocks, self.plies = S, blocks, plies
        self.key = (S, blocks)
        self.net = netcal.calibrated(S, blocks)
        self.fnet = netcal.fused_net(self.net)
        assert self.fnet.packed_ok
        self.W = netcal.Weights(self.net, device="cuda")
        self.recs = {ply: _playout_records(L, S, N, ply, seed=2000 + ply) for ply in plies}
        self._ref = {}
        self.torch = torch

    def planes(self, recs, k, idx=None, n=N, padded=False):
        """The network input of `recs` under symmetry k: [n, S, S, 17] float32, or [n, S, S, 32] fp16 (the tensor route's)."""
        torch, S = self.torch, self.S
        if padded:
            x = torch.zeros((n, S, S, 32), dtype=torch.float16, device="cuda")
            layout, dtype = 2, 0
        else:
            x = torch.zeros((n, S, S, 17), dtype=torch.float32, device="cuda")
            layout, dtype = 0, 1
        self.L.check(self.lib.sgo_nn_pack_dev(S, n, self.L.ptr(recs), None if idx is None else self.L.ptr(idx), k, layout,
                                              dtype, self.L.ptr(x), self.L.stream_ptr()))
        return x

    def ref(self, ply, k, route="packed"):
        key = (ply, k, route)
        if key not in self._ref:
            self._ref[key] = netcal.forward(self.W, self.planes(self.recs[ply], k).double(), route=route)
        return self._ref[key]


_CASES = {}


def shared_case(L, S, blocks):
    """the case of configuration (S, blocks) of CONFIGS, built once and shared (also by tests/test_gpu_conv_epilogue.py)"""
    plies = {(s, b): p for s, b, p in CONFIGS}[(S, blocks)]
    if (S, blocks) not in _CASES:
        _CASES.clear()                      # one 20-block net + its references at a time
        _CASES[(S, blocks)] = _Case(L, S, blocks, plies)
    return _CASES[(S, blocks)]


@pytest.fixture(scope="module", params=CONFIGS, ids=["%dx%d_%dblock" % (c[0], c[0], c[1]) for c in CONFIGS])
def case(request, L):
    S, blocks, plies = request.param
    return shared_case(L, S, blocks)


class _Tower(object):
    """Routes the net's tower through one kernel for the duration of a `with`, and restores the switches."""

    def __init__(self, case, name):
        self.case, self.name = case, name

    def __enter__(self):
        lib, fnet = self.case.lib, self.case.fnet
        self.old = lib.sgo_conv_tower_kernel(0 if self.name == "k_conv8w" else 1)
        if self.name == "k_conv4r":
            assert fnet.use_packed_tower(True)
        return self

    def __exit__(self, *exc):
        self.case.fnet.use_packed_tower(False)
        self.case.lib.sgo_conv_tower_kernel(self.old)
        return False


class _Worst(object):
    def __init__(self):
        self.logit = self.value = self.dp = 0.0
        self.rows = 0

    def add(self, p, v, ref, rows=None):
        import torch
        lr, vr = ref
        if rows is not None:
            lr, vr = lr[rows], vr[rows]
        # a NaN / inf anywhere in the batch fails here: the metrics below would otherwise fold it away with max()
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all()), "non-finite policy / value"
        self.logit = max(self.logit, netcal.logit_error(torch.log(p.double()), lr))
        self.value = max(self.value, netcal.value_error(v, vr))
        self.dp = max(self.dp, float((p.double() - lr.exp()).abs().max()))
        self.rows += p.shape[0]

    def check(self, what, case):
        tol_l, tol_v = netcal.LOGIT_TOL[case.key], netcal.V_TOL[case.key]
        print("\nNET_PARITY S=%d blocks=%d %s rows=%d: logit %.3e (tol %.1e) value %.3e (tol %.1e) max|dp| %.3e (stated %.0e)"
              % (case.S, case.blocks, what, self.rows, self.logit, tol_l, self.value, tol_v, self.dp, P_STATED))
        assert self.logit <= tol_l and self.value <= tol_v and self.dp <= P_STATED, (what, self.logit, self.value, self.dp)


@pytest.mark.parametrize("kernel", KERNELS)
def test_engine_route_matches_the_float64_reference(case, kernel):
    """predict_packed on 64 / 37 / 1 rows (the last two through an index list) of every ply under every symmetry."""
    torch = case.torch
    g = torch.Generator().manual_seed(case.S)
    worst = _Worst()
    with _Tower(case, kernel):
        for ply in case.plies:
            recs = case.recs[ply]
            for k in range(8):
                ref = case.ref(ply, k)
                p, v = case.fnet.predict_packed(recs.data_ptr(), None, N, k)
                assert p.shape == (N, case.S * case.S + 1) and v.shape == (N, 1)
                worst.add(p, v, ref)
                for n in (37, 1):
                    rows = torch.randperm(N, generator=g)[:n].cuda()
                    idx = rows.to(torch.int32)
                    p, v = case.fnet.predict_packed(recs.data_ptr(), idx.data_ptr(), n, k)
                    worst.add(p, v, ref, rows)
    worst.check("route=packed kernel=%s batches=(64,37,1) plies=%s x 8 symmetries" % (kernel, case.plies), case)


@pytest.mark.parametrize("kernel", KERNELS)
def test_tensor_route_matches_the_float64_reference(case, kernel):
    """predict_on_batch on the channel-padded fp16 tensor of the same records (k_stem reads all 17 planes with fp16 weights)."""
    worst = _Worst()
    with _Tower(case, kernel):
        for ply in case.plies:
            for k in range(8):
                x = case.planes(case.recs[ply], k, padded=True)
                p, v = case.fnet.predict_on_batch(x)
                worst.add(p, v, case.ref(ply, k, route="tensor"))
                p, v = case.fnet.predict_on_batch(x[:37])
                worst.add(p, v, case.ref(ply, k, route="tensor"), slice(0, 37))
                p, v = case.fnet.predict_on_batch(x[k + 40:k + 41])
                worst.add(p, v, case.ref(ply, k, route="tensor"), slice(k + 40, k + 41))
    worst.check("route=tensor kernel=%s batches=(64,37,1) plies=%s x 8 symmetries" % (kernel, case.plies), case)


def test_headline_batch_matches_the_float64_reference_on_sampled_rows(L):
    """8 192 positions at 19x19 through the 20-block net on each tower kernel (the bench's launch), compared on sampled rows:
    the first and last ones, rows spread over the batch and random ones."""
    import torch
    S, blocks, n, k = 19, 20, 8192, 5
    c = _CASES.get((S, blocks)) or _Case(L, S, blocks, ())
    recs = _playout_records(L, S, n, 150, seed=4242)
    sample = sorted(set([0, 1, n - 2, n - 1] + [int((j + f) * n / 8) for j in range(8) for f in (0.0, 0.5, 0.999)]
                        + [int(r) for r in np.random.RandomState(5).randint(0, n, size=16)]))
    rows = torch.tensor(sample, device="cuda")
    x = c.planes(recs, k, idx=rows.to(torch.int32), n=len(sample))
    ref = netcal.forward(c.W, x.double())
    for kernel in KERNELS:
        worst = _Worst()
        with _Tower(c, kernel):
            p, v = c.fnet.predict_packed(recs.data_ptr(), None, n, k)
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all()), kernel     # every row, not just the sampled
        worst.add(p[rows], v[rows], ref)
        del p, v
        worst.check("route=packed kernel=%s batch=%d sampled_rows=%d" % (kernel, n, len(sample)), c)


@pytest.mark.parametrize("kernel", KERNELS)
def test_negative_controls_exceed_twice_the_tolerance(case, kernel):
    """The check fails on real kernels fed valid but wrong data: (a) the net under symmetry k, the reference under k + 1;
    (b) one middle conv1's filter bank with its taps rolled (OHWI copy for k_conv4w / k_conv8w; for k_conv4r a fragment-order
    bank prepacked from the rolled weights, registered for an UNROLLED OHWI copy, so the fault shows only if the bank is what
    the kernel reads).  Mid-game positions, so that no symmetry of the board hides the fault."""
    torch = case.torch
    tol = netcal.LOGIT_TOL[case.key]
    ply = case.plies[2]
    recs = case.recs[ply]
    fnet = case.fnet
    mid = len(fnet.blocks) // 2
    with _Tower(case, kernel):
        p, v = fnet.predict_packed(recs.data_ptr(), None, N, 2)
        wrong_sym = netcal.logit_error(torch.log(p.double()), case.ref(ply, 3)[0])
        saved = fnet.blocks[mid]
        w_rolled = netcal.roll_taps(saved[0]).contiguous(memory_format=torch.channels_last)
        w1 = saved[0].clone(memory_format=torch.channels_last) if kernel == "k_conv4r" else w_rolled
        try:
            fnet.blocks[mid] = (w1,) + tuple(saved[1:])
            if kernel == "k_conv4r":
                bank = torch.empty(case.lib.sgo_conv3x3_tower_packed_bytes(), dtype=torch.uint8, device="cuda")
                case.L.check(case.lib.sgo_conv3x3_tower_prepack_dev(w_rolled.data_ptr(), bank.data_ptr(), case.L.stream_ptr()))
                fnet._banks[w1.data_ptr()] = bank
            p, v = fnet.predict_packed(recs.data_ptr(), None, N, 2)
        finally:
            fnet.blocks[mid] = saved
            fnet._banks.pop(w1.data_ptr(), None)
        rolled = netcal.logit_error(torch.log(p.double()), case.ref(ply, 2)[0])
        # and with the weights restored the same launch is back within the bound
        p, v = fnet.predict_packed(recs.data_ptr(), None, N, 2)
        restored = netcal.logit_error(torch.log(p.double()), case.ref(ply, 2)[0])
    print("\nNET_PARITY_NEGATIVE S=%d blocks=%d kernel=%s: wrong symmetry %.3e, rolled taps %.3e, restored %.3e (2 x tol %.1e)"
          % (case.S, case.blocks, kernel, wrong_sym, rolled, restored, 2 * tol))
    assert wrong_sym >= 2 * tol and rolled >= 2 * tol and restored <= tol, (wrong_sym, rolled, restored)
