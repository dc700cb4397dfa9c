"""The whole-net parity check has power (CPU, no GPU needed).

tests/test_gpu_net_parity.py holds the resident fp16 net to LOGIT_TOL / V_TOL (tests/netcal.py) against a float64 forward of
the same fp16 weights.  This module shows, on the same calibrated nets and on CPU, that those bounds separate rounding from
faults: the kernels' rounding model (fp16 weights and activations, fp32 accumulation) stays within TOL / 2 of the reference,
and every fault of netcal.MUTATIONS -- a lost K-chunk, zeroed output channels, rolled taps, a dropped bias, a misplaced skip,
misread stem planes, the wrong symmetry, the wrong flatten order -- moves the logits by >= 2 * TOL.  So a GPU run that passes
the bound rules each of these faults out, at the 20-block 19x19 net of the reference, the 4-block 9x9 net of config 2 and
4-block nets at the three other board sizes, 5, 7 and 13.

The three new nets are calibrated with centred heads (netcal.CALIBRATION): all four head channels are alive on 10 .. 90 % of
the (row, pixel) pairs, and the faults of netcal.HEAD_MUTATIONS -- the columns of p_fc or v_fc1 that multiply one head channel
zeroed -- move the logit metric by >= 2 * LOGIT_TOL (p_fc) or the value metric by >= 2 * V_TOL (v_fc1).  The 9x9 and 19x19
nets are not centred (their tolerances rest on published numbers), and test_old_nets_have_a_dead_head_channel documents what
they cannot see.
"""
import numpy as np
import pytest
import torch

from tests import netcal


def _rows(S):
    """Played positions from the opening to a crowded board, each under two symmetries (identity and a rotation, so that a
    symmetry fault cannot hide behind the empty board's invariance): 16 rows at 19x19, 32 at every other size (fp64 on CPU)."""
    from oracle import oracle as ora
    per_ply = 2 if S == 19 else 4
    boards = netcal.playout_boards(S, (0, S * S // 6, S * S // 2, S * S * 3 // 4), per_ply, seed=9)
    return torch.as_tensor(np.concatenate([boards, ora.sym_board(3, boards)]), dtype=torch.float64)


CONFIGS = [(9, 4), (19, 20), (5, 4), (7, 4), (13, 4)]


@pytest.fixture(scope="module", params=CONFIGS, ids=["%dx%d_%dblock" % (S, S, b) for S, b in CONFIGS])
def calibrated(request):
    S, blocks = request.param
    net = netcal.calibrated(S, blocks)
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


def test_centred_nets_have_four_live_head_channels(calibrated):
    """On the power test's rows every head channel of a centred configuration is non-zero on 10 .. 90 % of the (row, pixel)
    pairs: no column of p_fc or v_fc1 multiplies zeros only."""
    (S, blocks), net, W, X, (lr, vr) = calibrated
    live = netcal.head_liveness(net, X)
    print("\nLIVENESS S=%d blocks=%d centred=%s rows=%d: policy ch0 %.2f ch1 %.2f value ch0 %.2f ch1 %.2f"
          % ((S, blocks, netcal.centred(S, blocks), X.shape[0]) + live))
    if netcal.centred(S, blocks):
        assert all(0.1 <= s <= 0.9 for s in live), live


@pytest.mark.parametrize("mutation", sorted(netcal.HEAD_MUTATIONS))
def test_every_head_fault_exceeds_twice_the_tolerance_on_centred_nets(calibrated, mutation):
    (S, blocks), net, W, X, (lr, vr) = calibrated
    le, ve = netcal.forward(W, X, emulate=True, mutation=mutation)
    dl, dv = netcal.logit_error(le, lr), netcal.value_error(ve, vr)
    print("\nMUTATION S=%d blocks=%d centred=%s %s: logit %.3e (2 x tol %.1e) value %.3e (2 x tol %.1e)"
          % (S, blocks, netcal.centred(S, blocks), mutation, dl, 2 * netcal.LOGIT_TOL[(S, blocks)], dv, 2 * netcal.V_TOL[(S, blocks)]))
    if netcal.centred(S, blocks):
        if mutation.startswith("v_fc1"):
            assert dv >= 2 * netcal.V_TOL[(S, blocks)], (mutation, dv)
        else:
            assert dl >= 2 * netcal.LOGIT_TOL[(S, blocks)], (mutation, dl)
    assert netcal.logit_error(netcal.forward(W, X[:2])[0], lr[:2]) <= 1e-9


@pytest.mark.parametrize("calibrated", [(9, 4), (19, 20)], ids=["9x9_4block", "19x19_20block"], indirect=True)
def test_old_nets_have_a_dead_head_channel(calibrated):
    """A known limit of the two uncentred nets, kept as they are because published numbers rest on their tolerances.

    (19, 20): value-head channel 1 is zero on every (row, pixel) pair, and zeroing the v_fc1 columns that multiply it leaves the
    value metric at the rounding noise, below V_TOL / 2 (4.9e-3 against 1e-2).  A head that misreads those columns passes every
    whole-net check on this net.
    (9, 4): policy-head channel 1 is non-zero on 3 of the 1 568 (row, pixel) pairs of these rows (1 of 1 568 on the calibration
    rows), never above 0.04.  Zeroing the p_fc columns that multiply it stays below LOGIT_TOL / 2 on 29 of the 32 rows; the three
    rows with one live pixel each move by 2.2e-2, 3.2e-2 and 1.2e-1, so the metric as a whole, a maximum over the rows, does
    exceed the bound here -- by one pixel in ten rows, where the centred nets show the same fault by 0.73 .. 3.0.
    Whoever recalibrates the two nets so that this test fails should move them into netcal.CALIBRATION's centred set, hold them
    to HEAD_MUTATIONS as well, and delete it."""
    (S, blocks), net, W, X, (lr, vr) = calibrated
    live = netcal.head_liveness(net, X)
    if (S, blocks) == (9, 4):
        le, ve = netcal.forward(W, X, emulate=True, mutation="p_fc_cols_of_ch1_zeroed")
        rows = netcal.logit_error_per_row(le, lr)
        hidden = float((rows < netcal.LOGIT_TOL[(S, blocks)] / 2).float().mean())
        print("\nDEAD_CHANNEL S=9 blocks=4: policy ch1 alive on %.4f of the pairs; its p_fc columns zeroed: logit metric %.3e, below "
              "tol / 2 = %.1e on %.2f of the rows" % (live[1], float(rows.max()), netcal.LOGIT_TOL[(S, blocks)] / 2, hidden))
        assert live[1] <= 0.01 and hidden >= 0.9, (live, hidden)
    else:
        le, ve = netcal.forward(W, X, emulate=True, mutation="v_fc1_cols_of_ch1_zeroed")
        d = netcal.value_error(ve, vr)
        print("\nDEAD_CHANNEL S=19 blocks=20: value ch1 alive on %.4f of the pairs; its v_fc1 columns zeroed: value metric %.3e "
              "(tol / 2 %.1e)" % (live[3], d, netcal.V_TOL[(S, blocks)] / 2))
        assert live[3] == 0.0 and d < netcal.V_TOL[(S, blocks)] / 2, (live, d)


def test_degenerate_calibration_fails_loudly():
    """Uncentred, seed 11 leaves both value-head channels of the 4-block 7x7 net at zero on every calibration row: an assertion
    naming the size and the seed, where there used to be a NaN value downstream."""
    with pytest.raises(AssertionError, match=r"S=7, blocks=4, seed=11\): dead value head"):
        netcal.build_calibrated_net(7, 4)


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
