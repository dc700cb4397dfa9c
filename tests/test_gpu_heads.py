"""k_heads (csrc/sgo_heads.hpp, sgo_heads_dev): the policy / value heads as one kernel.

1. exact on integers: inputs chosen so that every logit and the pre-tanh value are exact in fp32 in ANY summation order, with
   weights in which a swapped (pixel, channel, output) index changes an integer; every board size, batch sizes that straddle the
   16-position tile, guard rows behind the outputs;
2. calibrated nets (tests/netcal.py): the kernel and the framework route on the SAME tower output against the float64 heads --
   the kernel's error within 1.25 x the framework route's (tests/test_heads_rounding_model.py shows on CPU that its rounding model
   is the better one: 0.12 .. 0.95 of the framework's there, 0.12 .. 0.43 on the 4-block nets of 5x5, 7x7 and 13x13; the quarter
   is for accumulation order and the maximum over more rows), at every board size,
   a channels-first flatten as the negative control, and a logit bias of 3e4;
3. the whole net on the engine's route with the fused heads against netcal.forward in float64, as tests/test_gpu_net_parity.py,
   at 9x9 and, with all four head channels alive (netcal.CALIBRATION), at 5x5, 7x7 and 13x13.

Measured on MI355X (logit / value error): 9x9 x 4 blocks: torch route 1.87e-3 / 1.98e-3, k_heads 4.34e-4 / 1.10e-3; 19x19 x 2
blocks: torch route 3.53e-3 / 1.50e-3, k_heads 2.29e-3 / 1.14e-3; channels-first reference 3.5 / 9.2; 5x5, 7x7, 13x13 x 4 blocks:
torch route 1.72e-3 / 2.87e-3, 1.82e-3 / 1.56e-3, 2.34e-3 / 3.70e-4, k_heads 4.04e-4 / 3.91e-4, 4.82e-4 / 3.94e-4, 1.10e-3 / 1.52e-4,
channels-first reference 1.8 / 2.4 / 5.5; exact-integer cases: policy within 2.0e-7 relative, value within 1.3e-8.
"""
import numpy as np
import pytest

from tests import netcal

pytestmark = pytest.mark.gpu

SIZES = (5, 7, 9, 13, 19)
BATCHES = (1, 15, 16, 17, 33, 70)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


def run_heads(L, S, n, y, head_w, head_b, bank, p_fc_b, v_fc1_b, v_fc2_w, v_fc2_b, guard=2):
    """(policy [n + guard, A], value [n + guard]) with the guard rows holding SENTINEL."""
    import torch
    A = S * S + 1
    pol = torch.full((n + guard, A), SENTINEL, dtype=torch.float32, device="cuda")
    val = torch.full((n + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    L.check(L.load().sgo_heads_dev(S, n, y.data_ptr(), head_w.data_ptr(), head_b.data_ptr(), bank.data_ptr(), p_fc_b.data_ptr(),
                                   v_fc1_b.data_ptr(), v_fc2_w.data_ptr(), v_fc2_b.data_ptr(), pol.data_ptr(), val.data_ptr(),
                                   L.stream_ptr()), "sgo_heads_dev")
    torch.cuda.synchronize()
    return pol, val


def make_bank(L, S, p_fc_w, v_fc1_w):
    import torch
    lib = L.load()
    bank = torch.empty(lib.sgo_heads_packed_bytes(S), dtype=torch.uint8, device="cuda")
    L.check(lib.sgo_heads_prepack_dev(S, p_fc_w.data_ptr(), v_fc1_w.data_ptr(), bank.data_ptr(), L.stream_ptr()), "sgo_heads_prepack_dev")
    return bank


# ---------------------------------------------------------------------------------------------------------- 1. exact integers
class _IntCase(object):
    """Integer-valued inputs for board size S (70 rows) and their float64 results.  All tensors are exact in fp16."""

    def __init__(self, L, S):
        import torch
        g = torch.Generator().manual_seed(1000 + S)
        n, t = max(BATCHES), S - 2
        T2, A = t * t, S * S + 1
        K = 2 * T2
        y = (torch.rand((n, t, t, 256), generator=g) < 0.08).double()                       # sparse {0, 1}
        head_w = torch.randint(-1, 2, (4, 256), generator=g).double()
        head_b = torch.tensor([3.0, 2.0, 4.0, 1.0], dtype=torch.float64)
        h = torch.relu(torch.einsum("nhwc,kc->nhwk", y, head_w) + head_b)                   # [n, t, t, 4] integers
        assert 8 <= float(h.max()) <= 40
        hp = h[..., 0:2].reshape(n, K)                                                      # flatten order pixel * 2 + channel
        hv = h[..., 2:4].reshape(n, K)
        wp_int = torch.randint(-4, 5, (A, K), generator=g).double()
        bp_int = torch.randint(-8, 9, (A,), generator=g).double()
        lg_int = hp @ wp_int.t() + bp_int
        assert float((hp @ wp_int.abs().t()).max()) + 8 < 2 ** 24                          # every partial sum is exact in fp32
        shift = int(np.ceil(np.log2(float(lg_int.abs().max()) / 8.0)))                      # logits span about +-8
        scale = 2.0 ** -shift
        wv = torch.randint(-1, 2, (256, K), generator=g).double()
        bv = torch.randint(-3, 4, (256,), generator=g).double()
        v1 = torch.relu(hv @ wv.t() + bv)
        assert float((hv @ wv.abs().t()).max()) + 3 < 2 ** 24
        w2_int = torch.randint(-500, 501, (256,), generator=g).double()
        b2_int = torch.tensor([37.0], dtype=torch.float64)
        assert float((v1 @ w2_int.abs()).max()) + 37 < 2 ** 24
        pre = (v1 @ w2_int + b2_int) * 2.0 ** -20
        self.logits = lg_int * scale
        self.policy = torch.softmax(self.logits, dim=1)
        self.value = torch.tanh(pre)
        assert 4.0 < float(self.logits.abs().max()) <= 8.0 and float(pre.abs().max()) > 0.05

        def dev(x):
            x16 = x.to(torch.float16)
            assert bool((x16.double() == x).all()), "not exact in fp16"
            return x16.contiguous().cuda()

        self.S, self.A = S, A
        self.y, self.head_w, self.head_b = dev(y), dev(head_w), dev(head_b)
        self.p_fc_w, self.p_fc_b = dev(wp_int * scale), dev(bp_int * scale)
        self.v_fc1_w, self.v_fc1_b = dev(wv), dev(bv)
        self.v_fc2_w, self.v_fc2_b = dev(w2_int * 2.0 ** -20), dev(b2_int * 2.0 ** -20)
        self.bank = make_bank(L, S, self.p_fc_w, self.v_fc1_w)


_INT = {}


def int_case(L, S):
    """the integer case of board size S, built once per session (also used by tests/test_gpu_conv_epilogue.py)"""
    if S not in _INT:
        _INT[S] = _IntCase(L, S)
    return _INT[S]


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("S", SIZES)
def test_exact_on_integers(L, S, n):
    import torch
    c = int_case(L, S)
    pol, val = run_heads(L, S, n, c.y, c.head_w, c.head_b, c.bank, c.p_fc_b, c.v_fc1_b, c.v_fc2_w, c.v_fc2_b)
    assert bool((pol[n:] == SENTINEL).all()) and bool((val[n:] == SENTINEL).all()), "rows >= n were written"
    p, v = pol[:n].double().cpu(), val[:n].double().cpu()
    rel = float(((p - c.policy[:n]).abs() / c.policy[:n]).max())
    dv = float((v - c.value[:n]).abs().max())
    print("\nHEADS_EXACT S=%d n=%d: policy rel %.2e value %.2e" % (S, n, rel, dv))
    assert rel <= 1e-5, rel
    assert dv <= 1e-6, dv


# ---------------------------------------------------------------------------------------------------------- 2. calibrated nets
def tower_output(L, fnet, recs_ptr, idx_ptr, n, k, k_dev_ptr=None):
    """The tower output through FusedInferenceNet's own stem and _conv calls: [n, 256, t, t] fp16, channels-last memory."""
    import torch
    y = torch.empty((n, fnet.channels, fnet.t, fnet.t), dtype=torch.float16, device=fnet.device, memory_format=torch.channels_last)
    L.check(fnet.lib.sgo_stem_packed_dev(fnet.size, n, recs_ptr, idx_ptr, int(k), k_dev_ptr, fnet.stem_w10.data_ptr(),
                                         fnet.stem_b.data_ptr(), fnet.stem_wcol.data_ptr(), y.data_ptr(), L.stream_ptr()),
            "sgo_stem_packed_dev")
    for (w1, b1, w2, b2) in fnet.blocks:
        z = fnet._conv(y, w1, b1, 1)
        y = fnet._conv(z, w2, b2, 1, skip=y)
    return y


def torch_heads(fnet, y):
    """The default heads of FusedInferenceNet (the framework route) on a tower output: its own code, with the tower skipped."""
    saved, was = fnet.blocks, fnet.fused_heads
    try:
        fnet.blocks, fnet.fused_heads = [], False
        return fnet._tower_and_heads(y)
    finally:
        fnet.blocks, fnet.fused_heads = saved, was


HEADS_CONFIGS = [(9, 4, (0, 10, 30, 60)), (19, 2, (0, 30, 120, 250)), (5, 4, (0, 4, 10, 16)), (7, 4, (0, 6, 16, 32)), (13, 4, (0, 20, 60, 110))]


@pytest.mark.parametrize("S,blocks,plies", HEADS_CONFIGS, ids=["%dx%d_%dblock" % (c[0], c[0], c[1]) for c in HEADS_CONFIGS])
def test_calibrated_heads_against_float64_and_the_torch_route(L, S, blocks, plies):
    import torch
    from tests.test_gpu_baseline_nets import _playout_records
    from tests.test_heads_rounding_model import heads
    net = netcal.calibrated(S, blocks)
    fnet = netcal.fused_net(net)
    W = netcal.Weights(net, device="cuda")
    recs = torch.cat([_playout_records(L, S, 16, ply, seed=3000 + ply) for ply in plies])          # 64 rows
    n = recs.shape[0]
    y = tower_output(L, fnet, recs.data_ptr(), None, n, 0)
    y64 = y.double().contiguous()                                                                   # [n, 256, t, t] values
    lp_ref, v_ref = heads(W, y64, "f64")
    lp_cf, _ = heads(W, y64, "f64", channels_first=True)

    p_t, v_t = torch_heads(fnet, y)
    assert fnet.use_fused_heads(True)
    p_f, v_f = fnet._heads_kernel(y)
    assert p_f.shape == (n, S * S + 1) and v_f.shape == (n, 1) and p_f.dtype == v_f.dtype == torch.float32
    assert bool(torch.isfinite(p_f).all()) and bool(torch.isfinite(v_f).all())
    e_torch = (netcal.logit_error(torch.log(p_t.double()), lp_ref), netcal.value_error(v_t, v_ref))
    e_fused = (netcal.logit_error(torch.log(p_f.double()), lp_ref), netcal.value_error(v_f, v_ref))
    wrong = netcal.logit_error(torch.log(p_f.double()), lp_cf)
    print("\nHEADS_PARITY S=%d blocks=%d rows=%d: torch route logit %.3e value %.3e | fused logit %.3e value %.3e | "
          "channels-first reference %.3e" % ((S, blocks, n) + e_torch + e_fused + (wrong,)))
    assert e_fused[0] <= 1.25 * e_torch[0], (e_fused, e_torch)
    assert e_fused[1] <= 1.25 * e_torch[1], (e_fused, e_torch)
    assert wrong > 100.0 * e_torch[0], (wrong, e_torch)
    assert float((p_f.sum(dim=1) - 1).abs().max()) < 1e-5

    # a logit bias of 3e4 on one move: p = 1 there, finite everywhere
    j = S * S // 2
    pb = fnet.p_fc_b.clone()
    pb[j] = 3e4
    pol, val = run_heads(L, S, n, y, fnet.head_w, fnet.head_b, fnet._heads_bank, pb, fnet.v_fc1_b, fnet.v_fc2_w, fnet.v_fc2_b)
    assert bool(torch.isfinite(pol[:n]).all()) and bool(torch.isfinite(val[:n]).all())
    assert bool((pol[:n, j] == 1.0).all()) and float(pol[:n].sum(dim=1).max()) == 1.0
    assert torch.equal(val[:n], v_f.reshape(n))


# ---------------------------------------------------------------------------------------------------------- 3. whole net
@pytest.mark.parametrize("S,blocks", [(9, 4), (5, 4), (7, 4), (13, 4)], ids=["9x9_4block", "5x5_4block", "7x7_4block", "13x13_4block"])
def test_whole_net_with_fused_heads_matches_the_float64_reference(L, S, blocks):
    """predict_packed with use_fused_heads(True) on the 4-block nets of tests/test_gpu_net_parity.py: 64 / 37 / 1 rows (the last
    two through an index list) of every ply under every symmetry, within the bounds of that module."""
    import torch
    from tests import test_gpu_net_parity as tp
    case = tp.shared_case(L, S, blocks)
    fnet = case.fnet
    g = torch.Generator().manual_seed(S)
    worst = tp._Worst()
    assert fnet.use_fused_heads(True)
    try:
        for ply in case.plies:
            recs = case.recs[ply]
            for k in range(8):
                ref = case.ref(ply, k)
                p, v = fnet.predict_packed(recs.data_ptr(), None, tp.N, k)
                assert p.shape == (tp.N, S * S + 1) and v.shape == (tp.N, 1)
                worst.add(p, v, ref)
                for n in (37, 1):
                    rows = torch.randperm(tp.N, generator=g)[:n].cuda()
                    idx = rows.to(torch.int32)
                    p, v = fnet.predict_packed(recs.data_ptr(), idx.data_ptr(), n, k)
                    worst.add(p, v, ref, rows)
    finally:
        fnet.use_fused_heads(False)
    worst.check("route=packed heads=k_heads batches=(64,37,1) plies=%s x 8 symmetries" % (case.plies,), case)
