"""The whole-net parity check has power (CPU, no GPU needed).

tests/test_gpu_net_parity.py holds the resident fp16 net to LOGIT_TOL / V_TOL (tests/netcal.py) against a float64 forward of
the same fp16 weights.  This module shows, on the same calibrated nets and on CPU, that those bounds separate rounding from
faults: the kernels' rounding model (fp16 weights and activations, fp32 accumulation) stays within TOL / 2 of the reference,
and every fault of netcal.MUTATIONS -- a lost K-chunk, zeroed output channels, rolled taps, a dropped bias, a misplaced skip,
misread stem planes, the wrong symmetry, the wrong flatten order -- moves the logits by >= 2 * TOL.  So a GPU run that passes
the bound rules each of these faults out, at the 20-block 19x19 net of the reference and the 4-block 9x9 net of config 2.
"""
import numpy as np
import pytest
import torch

from tests import netcal


def _rows(S):
    """Played positions from the opening to a crowded board, each under two symmetries (identity and a rotation, so that a
    symmetry fault cannot hide behind the empty board's invariance): 32 rows at 9x9, 16 at 19x19 (fp64 on CPU)."""
    from oracle import oracle as ora
    per_ply = 4 if S == 9 else 2
    boards = netcal.playout_boards(S, (0, S * S // 6, S * S // 2, S * S * 3 // 4), per_ply, seed=9)
    return torch.as_tensor(np.concatenate([boards, ora.sym_board(3, boards)]), dtype=torch.float64)


@pytest.fixture(scope="module", params=[(9, 4), (19, 20)], ids=["9x9_4block", "19x19_20block"])
def calibrated(request):
    S, blocks = request.param
    net = netcal.build_calibrated_net(S, blocks)
    W = netcal.Weights(net)
    X = _rows(S)
    return (S, blocks), net, W, X, netcal.forward(W, X)


def test_calibrated_net_is_in_the_intended_regime(calibrated):
    """Policy neither uniform nor one-hot, value informative and not saturated -- unlike the default init, whose probabilities
    all lie within a factor ~2 of 1/A and whose value sits near 0."""
    (S, blocks), net, W, X, (lr, vr) = calibrated
    A = S * S + 1
    pmax_lo, pmax_hi, sd, vmax = netcal.regime(lr, vr)
    assert 1.5 <= sd <= 2.5, sd                                  # centred logits: std ~2 per row
    assert pmax_lo >= 5.0 / A and pmax_hi <= 0.9, (pmax_lo, pmax_hi)
    assert vmax <= 0.999 and float(vr.std()) >= 0.2, (vmax, float(vr.std()))
    # the calibration is a property of the module: its own fp32 forward agrees with the reference up to fp16 weight rounding
    with torch.no_grad():
        p32, v32 = net.fused(torch.float32).predict_on_batch(X.float())
    assert netcal.logit_error(torch.log(p32.double()), lr) <= netcal.LOGIT_TOL[(S, blocks)]


@pytest.mark.parametrize("route", ["packed", "tensor"])
def test_rounding_model_stays_within_half_the_tolerance(calibrated, route):
    (S, blocks), net, W, X, (lr, vr) = calibrated
    le, ve = netcal.forward(W, X, route=route, emulate=True)
    dl, dv = netcal.logit_error(le, lr), netcal.value_error(ve, vr)
    print("\nNOISE S=%d blocks=%d route=%s rows=%d: logit %.3e (tol %.1e) value %.3e (tol %.1e)"
          % (S, blocks, route, X.shape[0], dl, netcal.LOGIT_TOL[(S, blocks)], dv, netcal.V_TOL[(S, blocks)]))
    assert dl <= netcal.LOGIT_TOL[(S, blocks)] / 2, dl
    assert dv <= netcal.V_TOL[(S, blocks)] / 2, dv
    # the stated probability bound also holds on the calibrated net
    assert float((le.exp() - lr.exp()).abs().max()) <= 2e-3


@pytest.mark.parametrize("mutation", netcal.MUTATIONS)
def test_every_listed_fault_exceeds_twice_the_tolerance(calibrated, mutation):
    (S, blocks), net, W, X, (lr, vr) = calibrated
    le, ve = netcal.forward(W, X, emulate=True, mutation=mutation)
    dl, dv = netcal.logit_error(le, lr), netcal.value_error(ve, vr)
    print("\nMUTATION S=%d blocks=%d %s: logit %.3e (2 x tol %.1e) value %.3e"
          % (S, blocks, mutation, dl, 2 * netcal.LOGIT_TOL[(S, blocks)], dv))
    assert dl >= 2 * netcal.LOGIT_TOL[(S, blocks)], (mutation, dl)
    # a mutation works on copies: the weights the reference reads are untouched
    assert netcal.logit_error(netcal.forward(W, X[:2])[0], lr[:2]) <= 1e-9


def test_logit_metric_ignores_a_constant_shift_and_sees_one_move():
    """The metric is blind to what softmax is blind to (a per-row constant) and sees a single wrong logit."""
    g = torch.Generator().manual_seed(0)
    ref = torch.log_softmax(2.0 * torch.randn(4, 82, generator=g, dtype=torch.float64), dim=1)
    assert netcal.logit_error(ref + 3.0, ref) <= 1e-12
    bad = ref.clone()
    bad[2, 17] += 0.05
    bad = torch.log_softmax(bad, dim=1)
    assert 0.045 <= netcal.logit_error(bad, ref) <= 0.05
    # moves the reference gives (almost) no probability are left out
    ref2 = ref.clone()
    ref2[1, 5] = -40.0
    wild = ref2.clone()
    wild[1, 5] = -20.0
    assert netcal.logit_error(wild, ref2) <= 1e-12
    wild[1, 5] = -float("inf")                      # even p == 0 there
    assert netcal.logit_error(wild, ref2) <= 1e-12


def test_metrics_fail_on_non_finite_values():
    """A NaN or inf anywhere in a batch makes the metric infinite: a NaN would otherwise compare false with every bound and be
    lost by a max() over batches."""
    ref = torch.log_softmax(torch.randn(3, 82, generator=torch.Generator().manual_seed(1), dtype=torch.float64), dim=1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        lp = ref.clone()
        lp[2, 40] = bad
        assert netcal.logit_error(lp, ref) == float("inf")
        v = torch.zeros(3, 1, dtype=torch.float64)
        v[1, 0] = bad
        assert netcal.value_error(v, torch.zeros(3, 1)) == float("inf")
    assert max(0.0, netcal.logit_error(torch.full_like(ref, float("nan")), ref)) == float("inf")
