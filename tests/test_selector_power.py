"""CPU-only: what tests/golden/puct_ties.npz can see that puct.npz and the whole-game fixtures cannot.

The PUCT score of the reference under numpy >= 2 (play.py:308-323) is

    float32 priors:        fl32(q + fl32(fl32(p * fl32(tn)) / fl32(1 + n)))
    float64 root priors:   q + (p * tn) / (1 + n)                                  (all float64)

A selector that computes the same quantity with another rounding -- a hoisted tn / (1 + n), p / (1 + n) first, a widened
product, the wrong regime at the root -- picks another child only when two scores lie within an ulp of each other, which
random tables and short games almost never produce.  The formulas are restated here in numpy (independently of the
generator's copy in tests/golden/gen_golden.py) and run over the fixtures: every wrong one must lose at least 20 cases per
table size of its regime on puct_ties.npz, the reference formula none; on puct.npz the two reassociations that were measured
to pass the whole CPU suite must indeed lose nothing."""
import math

import numpy as np
import pytest

from tests.helpers import selector_tables

f32, f64_ = np.float32, np.float64


def _reference(P, N, Q, tn, root64):
    if root64:
        return Q.astype(f64_) + P * tn / (1. + N)
    return Q + (P.astype(f32) * f32(tn)) / (1. + N).astype(f32)


def _f32_hoisted_ratio(P, N, Q, tn):
    return Q + P.astype(f32) * (f32(tn) / (1. + N).astype(f32))


def _f32_prior_over_count_first(P, N, Q, tn):
    return Q + (P.astype(f32) / (1. + N).astype(f32)) * f32(tn)


def _f32_in_f64_rounded_once(P, N, Q, tn):
    return (Q.astype(f64_) + P.astype(f32).astype(f64_) * tn / (1. + N)).astype(f32)


def _f32_product_with_f64_tn(P, N, Q, tn):
    return Q + (P.astype(f32).astype(f64_) * tn).astype(f32) / (1. + N).astype(f32)


def _f64_hoisted_ratio(P, N, Q, tn):
    return Q.astype(f64_) + P * (tn / (1. + N))


def _f64_prior_over_count_first(P, N, Q, tn):
    return Q.astype(f64_) + (P / (1. + N)) * tn


def _f64_scored_in_f32(P, N, Q, tn):
    return _reference(P.astype(f32).astype(f64_), N, Q, tn, False)


WRONG = {0: {"f32_hoisted_ratio": _f32_hoisted_ratio, "f32_prior_over_count_first": _f32_prior_over_count_first,
             "f32_in_f64_rounded_once": _f32_in_f64_rounded_once, "f32_product_with_f64_tn": _f32_product_with_f64_tn},
         1: {"f64_hoisted_ratio": _f64_hoisted_ratio, "f64_prior_over_count_first": _f64_prior_over_count_first,
             "f64_scored_in_f32": _f64_scored_in_f32}}


def _losses(z, score):
    """How many cases of one table set the selector built on `score(P, N, Q, tn, root64)` gets wrong (top_one_with_virtual_loss:
    first index of the largest score among the children that are not busy, -1 when all are)."""
    bad = {0: 0, 1: 0}
    for c in range(len(z["F64"])):
        ex, root64 = z["EX"][c] > 0, int(z["F64"][c])
        P, N, Q = z["P"][c], np.where(ex, z["N"][c], 0), np.where(z["N"][c] > 0, z["Q"][c], f32(0))
        tn = math.sqrt(int(N.sum())) or 1
        free = np.flatnonzero(ex & (z["V"][c] == 0))
        got = int(free[np.argmax(score(P, N, Q, tn, root64)[free])]) if len(free) else -1
        bad[root64] += got != z["out_vl"][c]
    return bad


@pytest.fixture(scope="module")
def ties():
    return selector_tables("puct_ties.npz")


def test_reference_formula_loses_no_case(ties):
    for A, z, _ in ties + selector_tables("puct.npz"):
        assert _losses(z, _reference) == {0: 0, 1: 0}, A


def test_every_wrong_formula_loses_at_least_20_cases_per_size(ties):
    for A, z, _ in ties:
        for regime in (0, 1):
            n_cases = int((z["F64"] == regime).sum())
            for name, fn in sorted(WRONG[regime].items()):
                lost = _losses(z, lambda P, N, Q, tn, r64: fn(P, N, Q, tn) if r64 == regime else _reference(P, N, Q, tn, r64))
                print("puct_ties A=%3d %s: %-28s loses %3d of %d cases" % (A, ("float32", "float64 root")[regime], name,
                                                                           lost[regime], n_cases))
                assert lost[1 - regime] == 0 and lost[regime] >= 20, (A, name, lost)


def test_the_old_fixture_cannot_see_them(ties):
    """Why puct_ties.npz exists.  The hoisted ratio and the float64 evaluation of the float32 score passed all of puct.npz, the
    games and the tree tables when put into the oracle; here the same two lose no case of puct.npz.  The other formulas may
    lose a few of its 600 random tables, and always fewer than on the near-tie tables."""
    (A, old, _), = selector_tables("puct.npz")
    for regime in (0, 1):
        for name, fn in sorted(WRONG[regime].items()):
            score = lambda P, N, Q, tn, r64: fn(P, N, Q, tn) if r64 == regime else _reference(P, N, Q, tn, r64)
            lost_old = _losses(old, score)[regime]
            lost_new = sum(_losses(z, score)[regime] for _, z, _ in ties)
            print("puct.npz: %-28s loses %d of %d cases (puct_ties.npz: %d)" % (name, lost_old, int((old["F64"] == regime).sum()),
                                                                                lost_new))
            if name in ("f32_hoisted_ratio", "f32_in_f64_rounded_once"):
                assert lost_old == 0, name
            assert lost_old < lost_new, name


def test_fixture_covers_the_device_geometries_and_edges(ties):
    """What the fixture has to contain, whatever the generator's random stream gave: both regimes, the three table sizes, the
    pair in one lane / neighbouring lanes / slot 0 / last point / pass, exact ties, every busy pattern, zero and large counts,
    p = 0, a denormal p, q = +-1 and q = -0.0."""
    assert [A for A, _, _ in ties] == [26, 82, 362]
    tiny = np.finfo(f32).tiny
    for A, z, names in ties:
        cls = [names[k] for k in z["cls"]]
        I, J = z["I"], z["J"]
        assert set(z["F64"]) == {0, 1}
        for regime in (0, 1):
            r = z["F64"] == regime
            have = {c for c, k in zip(cls, r) if k}
            assert have >= set(names) - ({"same_lane"} if A <= 64 else set()), (A, regime, set(names) - have)
            pair = r & (I != J)
            assert (A <= 64) == (not np.any(pair & ((J - I) % 64 == 0)))              # one lane of the selecting wave
            assert np.any(pair & (J - I == 1)) and np.any(pair & (I == 0))
            assert np.any(pair & ((I == A - 2) | (J == A - 2))) and np.any(pair & (J == A - 1))
            ties_exact = 0
            for c in np.flatnonzero(pair):
                N = z["N"][c]
                s = _reference(z["P"][c], N, z["Q"][c], math.sqrt(int(N.sum())) or 1, regime)
                ties_exact += s[I[c]] == s[J[c]] and z["out_vl"][c] == I[c]
            assert ties_exact >= 10, (A, regime, ties_exact)
            rows = np.flatnonzero(r)
            assert np.any(z["out_vl"][rows] == -1) and np.any(z["N"][rows].max(axis=1) == 0) and np.any(z["N"][rows].max(axis=1) > 2000)
            ex = z["EX"][rows] > 0
            P, Q = z["P"][rows], z["Q"][rows]
            assert np.any(ex & (P == 0)) and np.any(ex & (P > 0) & (P < tiny))
            assert np.any(ex & (Q == 1)) and np.any(ex & (Q == -1)) and np.any(ex & (Q == 0) & np.signbit(Q))
