"""No GPU: what the cases of tests/conv_epilogue_cases.py (run on the device by tests/test_gpu_conv_epilogue.py) can catch and reach.

 * power: every fault of conv_epilogue_model.FAULTS changes the expected bits of at least one element of every case group it
   applies to (APPLIES); the number of detecting elements is printed;
 * the cases do not depend on the order of accumulation: the model with every sum taken in reversed order gives identical bits,
   and every accumulator is exact in fp32;
 * coverage: over the launches of a group every case class (conv_epilogue_cases.CLASSES_OF: all ten, but the add-order
   discriminator where there is no skip tensor to reorder) occurs at every pixel-in-tile index 0..255 and in every output
   channel 0..255 -- the strong members of two classes, a finite f in (65504, 65520] and a -0 in bias or skip, in their own right;
 * every rounding class really rounds: no element counted as a tie or a tie's neighbour is representable before the conversion;
 * the rounding helpers and a few guard vectors by hand."""
import numpy as np
import pytest

from tests import conv_epilogue_cases as C
from tests import conv_epilogue_model as M

CONV_GROUPS = M.GROUPS[:4]
M_E = 2.0 ** -10                    # the fp16 step at 1


def _detecting(group, fault):
    return [int((~M.same_bits(C.expected(L), C.expected(L, fault))).sum()) for L in C.launches(group)]


@pytest.mark.parametrize("fault", M.FAULTS)
def test_every_fault_changes_expected_bits_in_every_group_it_applies_to(fault):
    assert set(M.APPLIES) == set(M.FAULTS) and len(M.FAULTS) == 11
    for group in M.GROUPS:
        per = _detecting(group, fault)
        if group in M.APPLIES[fault]:
            print("%-26s %-13s detected by %7d elements in %2d of %2d launches" % (fault, group, sum(per), sum(1 for v in per if v), len(per)))
            assert sum(per) > 0, (fault, group)


@pytest.mark.parametrize("group", CONV_GROUPS)
def test_reversed_accumulation_order_gives_identical_bits(group):
    for L in C.launches(group):
        assert M.exact_in_fp32(C.acc_of(L)), L
        assert np.array_equal(C.expected(L), C.expected(L, reverse=True)), L


@pytest.mark.parametrize("group", CONV_GROUPS)
def test_every_class_at_every_pixel_index_and_in_every_channel(group):
    px = {c: np.zeros(256, bool) for c in C.CLASSES_OF[group]}
    ch = {c: np.zeros(256, bool) for c in C.CLASSES_OF[group]}
    count = {c: 0 for c in C.CLASSES_OF[group]}
    for L in C.launches(group):
        cl = C.classify(L)
        q = np.arange(L.M) % 256
        for c in px:
            m = cl[c]
            count[c] += int(m.sum())
            np.logical_or.at(px[c], q, m.any(axis=1))
            ch[c] |= m.any(axis=0)
    print("%s: elements per class %s" % (group, count))
    for c in px:
        assert px[c].all(), (group, c, "pixel-in-tile indices never reached", np.flatnonzero(~px[c])[:8])
        assert ch[c].all(), (group, c, "output channels never reached", np.flatnonzero(~ch[c])[:8])


@pytest.mark.parametrize("group", CONV_GROUPS)
def test_rounding_classes_really_round(group):
    n = 0
    for L in C.launches(group):
        cl = C.classify(L)
        o, f = C.body(L, want_f=True)
        for c in C.ROUNDING_CLASSES:
            m = cl[c]
            with np.errstate(over="ignore"):
                back = f[m].astype(np.float16).astype(np.float32)
            assert (back != f[m]).all(), (L, c)                         # not representable: the conversion has to choose
            n += int(m.sum())
        # and both directions of a tie occur: to even is down for some, up for others
        t = cl["tie"]
        if t.any() and L.M >= 256:
            up = o[t].view(np.float16).astype(np.float64) > f[t].astype(np.float64)
            assert up.any() and (~up).any(), L
    assert n > 1000


def test_tracers_sit_on_corners_and_an_edge_of_the_middle_sample():
    for group in ("tower_skip", "tower_noskip"):
        tr = [L for L in C.launches(group) if L.clean is not None]
        assert [(L.n, L.h, L.w) for L in tr] == [(3, 7, 7), (2, 19, 19), (11, 5, 5), (3, 11, 11)] and all(L.M % 256 for L in tr)
        for L in tr:
            assert L.n >= 2 and all(i == L.n // 2 for i, _, _ in L.marks)
            assert {(0, 0), (0, L.w - 1), (L.h - 1, 0), (L.h - 1, L.w - 1), (L.h // 2, 0)} == set((y, x) for _, y, x in L.marks)
            nb = C.neighbourhood(L).reshape(L.n, -1)
            other = [i for i in range(L.n) if i != L.n // 2]
            assert nb[L.n // 2].any() and not nb[other].any()
            # outside the neighbourhoods the tracer changes nothing (but skip's last pixel), inside it shows
            a = C.expected(L)[C.Y_FRONT:C.Y_FRONT + L.M]
            b = C.expected(L.clean)[C.Y_FRONT:C.Y_FRONT + L.M]
            out = ~C.neighbourhood(L)
            if L.skip is not None:
                assert not np.isfinite(L.skip[L.M - 1].astype(np.float64)).all() and not M.same_bits(a[L.M - 1], b[L.M - 1]).all()
                out[L.M - 1] = False
            assert M.same_bits(a[out], b[out]).all() and not M.same_bits(a[~out], b[~out]).all()


def test_every_board_size_has_its_launches():
    """the tower shapes of board sizes 5, 7, 13 and 19 (S - 2) in both tower groups, k_stem and the packed stem at the boards
    themselves: each at least once, and at 3x3, 5x5 and 11x11 with more than one tile"""
    for group in ("tower_skip", "tower_noskip"):
        shapes = set((L.h, L.w) for L in C.launches(group))
        assert {(3, 3), (5, 5), (11, 11), (17, 17)} <= shapes, (group, shapes)
        assert all(any(L.h == t and L.M > 256 and L.M % 256 for L in C.launches(group)) for t in (3, 5, 11)), group
    assert {(5, 5), (7, 7), (13, 13), (19, 19)} <= set((L.h, L.w) for L in C.launches("stem"))
    assert {(S, k) for S in (5, 7, 13, 19) for k in (0, 5)} <= set((L.S, L.sym) for L in C.launches("packed"))


def test_rounding_helpers_by_hand():
    f = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -23, 65519.99, 65520.0, 70000.0,
                  2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, np.inf, 0.0, 2.0 ** -26])
    want = {"rne": [1, 1 + 2 * M_E, 1 + M_E, 1, 65504, np.inf, np.inf, 0, 2.0 ** -23, 2.0 ** -14, np.inf, 0, 0],
            "rtz": [1, 1 + M_E, 1, 1, 65504, 65504, 65504, 0, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, np.inf, 0, 0],
            "half_up": [1 + M_E, 1 + 2 * M_E, 1 + M_E, 1, 65504, np.inf, np.inf, 2.0 ** -24, 2.0 ** -23, 2.0 ** -14, np.inf, 0, 0]}
    for mode, w in want.items():
        assert M.round_half(f, mode).astype(np.float64).tolist() == w, mode
    lo, hi = M.fp16_neighbours(np.array([1 + 2.0 ** -11, 1.0, 65519.0, 65536.0, 2.0 ** -25]))
    assert lo.tolist() == [1, 1, 65504, 65536, 0] and hi.tolist() == [1 + M_E, 1, 65536, 65536, 2.0 ** -24]


def test_epilogue_by_hand():
    """the issue's own examples, one element each"""
    def one(acc, bias, skip=None, fault=None, col=None):
        o, _ = M.epilogue(np.array([[acc]], np.float64), M.h([bias]), None if skip is None else M.h([[skip]]),
                          None if col is None else np.array([[col]], np.float32), fault)
        return int(o[0, 0])

    hb = lambda v: int(M.bits(M.h([v]))[0])                                           # noqa: E731
    assert one(1.0, 2.0 ** -11, 0.0) == hb(1.0) and one(1.0, 2.0 ** -11, 0.0, "half_up") == hb(1 + M_E)
    assert one(1 + M_E, 2.0 ** -11, 0.0) == hb(1 + 2 * M_E) and one(1 + M_E, 2.0 ** -11, 0.0, "rtz") == hb(1 + M_E)
    a = (1 + M_E) ** 2
    assert one(a, 0.0, -(1 + 2 * M_E)) == hb(2.0 ** -20) and one(a, 0.0, -(1 + 2 * M_E), "acc_to_fp16_first") == 0
    assert one(32768.0, -32768.0, 2.0 ** -9) == 0 and one(32768.0, -32768.0, 2.0 ** -9, "bias_before_skip") == hb(2.0 ** -9)
    assert one(1.0, 0.0, float("nan")) == M.QNAN and one(1.0, 0.0, float("nan"), "nan_to_zero") == 0
    assert one(65504.0, 0.0, 16.0) == 0x7C00 and one(65504.0, 0.0, 16.0, "inf_saturates") == 0x7BFF
    assert one(65504.0, 0.0, 15.0) == 0x7BFF and one(1.0, 0.0, float("-inf")) == 0 and one(1.0, float("inf"), 1.0) == 0x7C00
    assert one(2.0 ** -20, 0.0) == hb(2.0 ** -20) and one(2.0 ** -20, 0.0, None, "flush_subnormal_out") == 0
    assert one(0.0, -0.0, -0.0) == 0 and one(0.0, -0.0, -0.0, "neg_zero_kept") == 0          # f is +0: the conv kernels cannot tell
    assert one(0.0, 1.0, None, None, 2.0 ** -11 + 2.0 ** -23) == hb(1 + M_E)                    # the colour term's low bits decide
    # k_bias_act: two rounded fp16 adds, bias first; -0 + -0 = -0 becomes +0
    ba = lambda x, b, s, fault=None: int(M.bias_act(M.h([[x]]), M.h([b]), None if s is None else M.h([[s]]), fault)[0, 0])   # noqa: E731
    assert ba(1.0, 2.0 ** -11, 2.0 ** -11) == hb(1.0) and ba(1.0, 2.0 ** -11, 2.0 ** -11, "bias_act_single_rounding") == hb(1 + M_E)
    assert ba(1.0, 2.0 ** -11, -2.0 ** -11) == hb(1 - 2.0 ** -11) and ba(1.0, 2.0 ** -11, -2.0 ** -11, "bias_before_skip") == hb(1.0)
    assert ba(-0.0, -0.0, None) == 0 and ba(-0.0, -0.0, None, "neg_zero_kept") == 0x8000
    assert ba(65504.0, 16.0, None) == 0x7C00 and ba(float("nan"), 1.0, 1.0) == M.QNAN and ba(float("inf"), 1.0, float("-inf")) == M.QNAN


def test_conv_model_by_hand():
    """0 * inf is NaN, the padding is +0 times the weight, a neighbouring sample is never read"""
    x = np.zeros((2, 2, 2, 2), np.float16)
    x[0, 1, 1, 0] = np.inf                                                     # last pixel of sample 0
    w = np.zeros((2, 3, 3, 2), np.float16)
    w[0, 1, 1, 0], w[1, 0, 0, 1] = 1.0, 2.0
    acc = M.conv_acc(x, w, 1)
    assert np.isposinf(acc[3, 0]) and np.isnan(acc[:4, 1]).all() and np.isnan(acc[:3, 0]).all()
    assert (acc[4:] == 0).all()                                                # sample 1: adjacent in memory, untouched
    assert np.isnan(M.conv_acc(x, w, 1, fault="edge_multiplied")[4:]).any()
    w[1, 0, 0, 1] = np.inf                                                     # inf weight on a tap that is off the board: 0 * inf
    acc = M.conv_acc(np.ones((1, 1, 1, 2), np.float16), w, 1)
    assert acc[0, 0] == 1.0 and np.isnan(acc[0, 1])


GUARD = [("tower_skip", 0, [(0, 0), (17, 3), (288, 255)]), ("tower_noskip", 3, [(0, 0), (100, 100)]),
         ("stem", 0, [(0, 0), (260, 255)]), ("packed", 0, [(0, 0), (130, 7)])]


def test_guard_vectors():
    """(group, launch, elements) and their expected bits as literals: a change to the builders is noticed"""
    got = [[int(C.body(C.launches(g)[i])[p, k]) for p, k in el] for g, i, el in GUARD]
    print("guard vectors:", got)
    assert got == GUARD_BITS


GUARD_BITS = [[15360, 32256, 1025], [0, 15362], [31744, 15360], [15362, 32256]]
