"""The constructed rule positions (tests/golden/rule_shapes_S*.npz): the CPU oracle equals everything the reference recorded
on them, the fixture reaches the code it was built for, and a restated kernel with a fault switched on loses cases on it.
CPU only; tests/test_gpu_rule_shapes.py runs the kernels on the same files."""
import functools

import numpy as np
import pytest

from oracle import oracle as ora
from tests import rule_shapes as rs
from tests.helpers import sha8


@pytest.mark.parametrize("S", rs.SIZES)
def test_oracle_equals_reference_on_shapes(S):
    f = rs.load_shapes(S)
    for p in range(f.P):
        b = f.boards[p:p + 1]
        assert np.array_equal(ora.legal_moves(b), f.legal[p]), f.names[p]
        w = f.winner[p]
        assert ora.get_winner(b, f.komi) == (int(w[0]), int(w[1]), float(w[2])), f.names[p]
    for k in range(f.K):
        p, a, colour = int(f.play_pos[k]), int(f.play_a[k]), int(f.play_colour[k])
        b = f.boards[p:p + 1].copy()
        _, mover = ora.make_play(a % S, a // S, b, colour or None)
        assert mover == f.play_mover[k], (f.names[p], a, colour)
        assert np.array_equal(sha8(b), f.play_hash[k]), (f.names[p], a, colour)
        assert np.array_equal(sha8(ora.legal_moves(b))[:4], f.play_legal_hash[k]), (f.names[p], a, colour)


def test_fixture_is_valid_and_mirrored():
    """What the generator asserts, once more on the stored planes: the history plane of the side to move is its stones plus
    vanished ones on empty points (0, 1 and 2 of them occur), and every board is there for both sides to move."""
    for S in rs.SIZES:
        f = rs.load_shapes(S)
        own, opp, prev = f.boards[..., 0] != 0, f.boards[..., 1] != 0, f.boards[..., 2] != 0
        assert not (own & opp).any()
        gone = prev & ~own
        assert not (own & ~prev).any() and not (gone & opp).any()
        assert set(gone.reshape(f.P, -1).sum(axis=1)) == {0, 1, 2}
        absolute = {}
        for p in range(f.P):
            if not gone[p].any():
                black = own[p] if f.colour[p] == 1 else opp[p]
                white = opp[p] if f.colour[p] == 1 else own[p]
                absolute.setdefault((black.tobytes(), white.tobytes()), set()).add(int(f.colour[p]))
        assert all(v == {1, -1} for v in absolute.values())


@functools.lru_cache(maxsize=None)
def _measured(S):
    """The played-out goldens set the cap of the fill_capped fault: the deepest flood they need, stones or empty points."""
    g_fails, g_st = rs.run_goldens(S, None)
    cap = max(g_st.get("stone", 0), g_st.get("empty", 0))
    s_fails, s_st = rs.run_shapes(S, cap)
    return cap, g_fails, g_st, s_fails, s_st


@pytest.mark.parametrize("S", rs.SIZES)
def test_fixture_reach(S):
    """The restated kernel equals the reference on every case, and on the way its row-Jacobi fill needs at least
    S*S/2 - S trips for one stone group and for one empty region (the column serpentine needs (S*S + 1)/2 from one end; the
    shapes here seed the fill a few points further in).  That is a condition on the fixture, not a tolerance."""
    cap, g_fails, g_st, fails, st = _measured(S)
    assert fails["none"] == 0 and g_fails["none"] == 0
    print("S=%d deepest fill, trips: shapes %d (stones) / %d (empty); played-out goldens %d / %d" % (
        S, st["stone"], st["empty"], g_st["stone"], g_st["empty"]))
    assert st["stone"] >= S * S / 2 - S and st["empty"] >= S * S / 2 - S
    assert st["remaining_ge2"] >= 1          # two or more groups left to the loop after the single-stone path
    assert st["two_lib_c"] >= 1              # a group with exactly two liberties, both without an empty neighbour


@pytest.mark.parametrize("S", rs.SIZES)
def test_faults_lose_cases(S):
    """Proof that the fixture can fail.  Five of the six faults lose cases at every size.  The capped fill passes every
    played-out golden by construction of the cap and fails here.  no_suicide_after_capture cannot differ on any board: a
    move that captures has the captured point as a liberty, so the own-group test it skips never fires (0 and 0 below)."""
    cap, g_fails, g_st, fails, st = _measured(S)
    for k in rs.FAULTS:
        print("S=%d %-26s fails %4d of %d cases here, %4d of %d in the played-out goldens" % (
            S, k, fails[k], st["cases"], g_fails[k], g_st["cases"]))
    assert g_fails["fill_capped"] == 0 and fails["fill_capped"] > 0
    for k in ("nl_ge1", "while_if", "single_ge1", "ko_ge1"):
        assert fails[k] > 0, k
    assert fails["no_suicide_after_capture"] == 0 and g_fails["no_suicide_after_capture"] == 0
