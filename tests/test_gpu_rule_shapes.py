"""The rules kernels on the constructed positions of tests/golden/rule_shapes_S*.npz (flood fills of ~S*S/2 trips, the
legal-set shortcuts on dense boards, half-board captures and suicides, ko histories), through the C ABI:
 * every kernel form behind sgo_advance_legal_dev, sgo_legal_dev and sgo_score_dev against what the reference recorded;
 * the same cases in other batch orders and next to plies that leave at once: a result must not depend on the wave's other half;
 * index lists on every entry point that takes one, with sentinels around the named records;
 * the host calls for groups, territory, take_stones and the score at all five sizes against the oracle."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

from tests import rule_shapes as rs

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
FORMS = ("mode0", "mode1", "mode2", "fused_in_place", "fused_in_idx")


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


class Cases(object):
    pass


@functools.lru_cache(maxsize=None)
def _cases(S):
    """The recorded plays of one size plus moves on occupied points and outside the board, an odd number in all; the positions
    packed on the device, followed by one empty board (the record the filler plies of the batch tests play on)."""
    import torch
    from sejonggo_amd import _lib as L
    lib = L.load()
    f = rs.load_shapes(S)
    c = Cases()
    c.f, c.S, c.N, c.A = f, S, f.N, f.A
    c.NW, c.RW = lib.sgo_plane_words(S), lib.sgo_packed_words(S)
    pos, a, col, want = list(f.play_pos), list(f.play_a), list(f.play_colour), list(f.play_mover)
    stones = (f.boards[..., 0] != 0) | (f.boards[..., 1] != 0)
    with_stones = [p for p in range(f.P) if stones[p].any()]
    for j, p in enumerate(with_stones[::max(1, len(with_stones) // 12)]):
        occ = np.flatnonzero(stones[p].reshape(-1))
        for pt, cl in ((occ[0], 0), (occ[-1], -int(f.colour[p])), (occ[len(occ) // 2], int(f.colour[p]))):
            pos.append(p); a.append(int(pt)); col.append(cl); want.append(-101)
        for bad in (-1, f.A, f.A + 3)[j % 3:j % 3 + 1]:
            pos.append(p); a.append(bad); col.append(0); want.append(-102)
    if len(pos) % 2 == 0:
        pos.append(0); a.append(-7); col.append(0); want.append(-102)
    c.n, c.K = len(pos), f.K
    c.pos, c.a, c.col, c.want = (np.array(v, dtype=np.int32) for v in (pos, a, col, want))
    c.ok = np.arange(c.n) < f.K
    c.occupied = (int(with_stones[0]), int(np.flatnonzero(stones[with_stones[0]].reshape(-1))[0]))
    boards = np.concatenate([f.boards, np.zeros((1, S, S, 17), dtype=np.int32)])
    boards[-1, :, :, 16] = 1
    d_boards = torch.from_numpy(boards).cuda()
    c.table = torch.zeros((f.P + 1, c.RW), dtype=torch.int32, device="cuda")
    L.check(lib.sgo_pack_dev(S, f.P + 1, L.ptr(d_boards), L.ptr(c.table), L.stream_ptr()))
    back = torch.zeros_like(d_boards)
    L.check(lib.sgo_unpack_dev(S, f.P + 1, L.ptr(c.table), L.ptr(back), L.stream_ptr()))
    assert torch.equal(back[:, :, :, :4], d_boards[:, :, :, :4]) and torch.equal(back[..., 16], d_boards[..., 16])
    return c


def _run(L, c, form, rows, a, col, out=None, in_idx=True, out_idx=None):
    """One sgo_advance_legal_dev call of n plies on the table rows `rows`.  Returns (records, legal, status); records is `out`
    when given (then out_idx says where)."""
    import torch
    lib = L.load()
    n = len(rows)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).cuda()
    d_rows, d_a, d_col = dev(rows), dev(a), dev(col)
    legal = torch.full((n, c.NW), SENTINEL, dtype=torch.int32, device="cuda")
    status = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    st = L.stream_ptr()
    old = lib.sgo_advance_mode(-1)
    try:
        if form == "fused_in_idx":
            assert in_idx
            d_in, p_in_idx = c.table, L.ptr(d_rows)
        else:
            d_in, p_in_idx = c.table.index_select(0, d_rows.long()).contiguous(), None
        if form == "fused_in_place":
            assert out is None
            out = d_in
        elif out is None:
            out = torch.full((n, c.RW), SENTINEL, dtype=torch.int32, device="cuda")
        if form.startswith("mode"):
            assert out_idx is None
            lib.sgo_advance_mode(int(form[4]))
        d_out_idx = dev(out_idx) if out_idx is not None else None
        L.check(lib.sgo_advance_legal_dev(c.S, n, L.ptr(d_in), p_in_idx, L.ptr(d_a), L.ptr(d_col), L.ptr(out), L.ptr(d_out_idx),
                                          L.ptr(legal), L.ptr(status), st))
        torch.cuda.synchronize()
    finally:
        lib.sgo_advance_mode(old)
    return out, legal, status


def _masks(legal, A):
    """legal words [n][NW] (device) -> uint8 [n][A] in the reference's convention: 1 = illegal"""
    w = legal.cpu().numpy().view(np.uint8)
    return (1 - np.unpackbits(w, axis=1, bitorder="little")[:, :A]).astype(np.uint8)


def _verify(L, c, records, legal, status, sel=None):
    """records / legal / status of the cases `sel` (default: all, in order) against the reference's recorded values."""
    import torch
    lib = L.load()
    sel = np.arange(c.n) if sel is None else sel
    assert np.array_equal(status.cpu().numpy(), c.want[sel]), "status / mover"
    ok = np.flatnonzero(c.ok[sel])
    d_ok = torch.from_numpy(ok).cuda()
    boards = torch.zeros((len(ok), c.S, c.S, 17), dtype=torch.int32, device="cuda")
    picked = records.index_select(0, d_ok).contiguous()
    L.check(lib.sgo_unpack_dev(c.S, len(ok), L.ptr(picked), L.ptr(boards), L.stream_ptr()))
    boards = boards.cpu().numpy()
    masks = _masks(legal.index_select(0, d_ok), c.A)
    f = c.f
    for j, i in enumerate(sel[ok]):
        what = (f.names[f.play_pos[i]], int(f.play_a[i]), int(f.play_colour[i]))
        assert hashlib.sha1(boards[j:j + 1].tobytes()).digest()[:8] == f.play_hash[i].tobytes(), ("board",) + what
        assert hashlib.sha1(masks[j].tobytes()).digest()[:4] == f.play_legal_hash[i].tobytes(), ("legal",) + what


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("S", rs.SIZES)
def test_advance_against_recorded(L, S, form):
    """Each kernel form on its own: the three dense forms (sgo_advance_mode), the fused kernel in place and through an input
    index list.  Mover / status, the board after the ply (sha8 of the unpacked tensor) and the legal set of the new position
    against the reference; a move on an occupied point or outside the board leaves its record as it was."""
    import torch
    c = _cases(S)
    records, legal, status = _run(L, c, form, c.pos, c.a, c.col)
    _verify(L, c, records, legal, status)
    if form == "fused_in_place":
        bad = torch.from_numpy(np.flatnonzero(~c.ok)).cuda()
        assert torch.equal(records.index_select(0, bad), c.table.index_select(0, torch.from_numpy(c.pos[~c.ok]).cuda().long()))
    if form == "fused_in_idx":
        bad = torch.from_numpy(np.flatnonzero(~c.ok)).cuda()
        assert bool((records.index_select(0, bad) == SENTINEL).all())


@pytest.mark.parametrize("S", rs.SIZES)
def test_legal_and_score_against_recorded(L, S):
    """sgo_legal_dev and sgo_score_dev on the positions themselves, dense and through a shuffled index list with repeats; the
    words behind the last result keep their sentinel."""
    import torch
    lib = L.load()
    c = _cases(S)
    f = c.f
    rng = np.random.RandomState(31 + S)
    for idx in (None, np.concatenate([rng.permutation(f.P), rng.randint(0, f.P, size=7)]).astype(np.int32)):
        n = f.P if idx is None else len(idx)
        which = np.arange(f.P) if idx is None else idx
        d_idx = None if idx is None else torch.from_numpy(idx).cuda()
        legal = torch.full((n + 4, c.NW), SENTINEL, dtype=torch.int32, device="cuda")
        res = torch.full((n + 4, 3), SENTINEL, dtype=torch.int32, device="cuda")
        L.check(lib.sgo_legal_dev(S, n, L.ptr(c.table), L.ptr(d_idx), L.ptr(legal), L.stream_ptr()))
        L.check(lib.sgo_score_dev(S, n, L.ptr(c.table), L.ptr(d_idx), C.c_double(f.komi), L.ptr(res), L.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((legal[n:] == SENTINEL).all()) and bool((res[n:] == SENTINEL).all())
        masks = _masks(legal[:n], c.A)
        res = res[:n].cpu().numpy()
        for i, p in enumerate(which):
            assert np.array_equal(masks[i], f.legal[p]), (f.names[p], "legal")
            assert (res[i, 0], res[i, 1], res[i, 2] + f.komi) == tuple(f.winner[p]), (f.names[p], "score")


@pytest.mark.parametrize("S", rs.SIZES)
def test_batch_composition(L, S):
    """The same cases reversed, in a seeded permutation, and interleaved one for one with passes on the empty board and with
    moves on an occupied point (both leave the kernel at once), the cases in the first and in the second half of each wave;
    every batch has an odd length.  All four kernels must give, case for case, the records of the plain order."""
    import torch
    c = _cases(S)
    n = c.n
    assert n % 2 == 1
    records, legal, status = _run(L, c, "mode2", c.pos, c.a, c.col)
    _verify(L, c, records, legal, status)
    rng = np.random.RandomState(17 + S)
    empty_row, (occ_row, occ_pt) = c.f.P, c.occupied
    orders = [("reversed", np.arange(n)[::-1].copy(), None), ("permuted", rng.permutation(n), None)]
    for name, row, pt, st in (("pass", empty_row, c.N, 1), ("occupied", occ_row, occ_pt, -101)):
        for first in (0, 1):
            m = 2 * n - 1 if first == 0 else 2 * n + 1
            case_at = np.arange(n) * 2 + first
            orders.append(("%s_%d" % (name, first), np.arange(n), (m, case_at, row, pt, st)))
    for name, order, fill in orders:
        rows, a, col = c.pos[order], c.a[order], c.col[order]
        at = np.arange(n)
        if fill is not None:
            m, at, row, pt, st = fill
            is_fill = np.ones(m, dtype=bool)
            is_fill[at] = False
            rows2, a2, col2 = np.full(m, row, dtype=np.int32), np.full(m, pt, dtype=np.int32), np.zeros(m, dtype=np.int32)
            rows2[at], a2[at], col2[at] = rows, a, col
            rows, a, col = rows2, a2, col2
        d_at = torch.from_numpy(at).cuda()
        d_order_ok = torch.from_numpy(np.flatnonzero(c.ok[order])).cuda()
        for form in ("mode0", "mode1", "mode2", "fused_in_place"):
            r2, l2, s2 = _run(L, c, form, rows, a, col)
            s2 = s2.cpu().numpy()
            assert np.array_equal(s2[at], c.want[order]), (name, form, "status")
            if fill is not None:
                assert (s2[is_fill] == st).all(), (name, form, "filler status")
            got_r = r2.index_select(0, d_at).index_select(0, d_order_ok)
            got_l = l2.index_select(0, d_at).index_select(0, d_order_ok)
            d_src = torch.from_numpy(order[np.flatnonzero(c.ok[order])]).cuda()
            assert torch.equal(got_r, records.index_select(0, d_src)), (name, form, "record")
            assert torch.equal(got_l, legal.index_select(0, d_src)), (name, form, "legal")


@pytest.mark.parametrize("S", rs.SIZES)
def test_index_lists(L, S):
    """d_in_idx shuffled, d_out_idx shuffled over a larger buffer, and both: the fused kernel writes the named records only
    (a refused ply writes nothing), everything else keeps its sentinel."""
    import torch
    c = _cases(S)
    n = c.n
    rng = np.random.RandomState(5 + S)
    for use_in, use_out in ((True, False), (False, True), (True, True)):
        order = rng.permutation(n)
        rows, a, col = c.pos[order], c.a[order], c.col[order]
        form = "fused_in_idx" if use_in else "fused_in_place"
        if not use_out:
            records, legal, status = _run(L, c, form, rows, a, col)
            _verify(L, c, records, legal, status, order)
            continue
        m = 2 * n + 3
        out = torch.full((m, c.RW), SENTINEL, dtype=torch.int32, device="cuda")
        out_idx = rng.permutation(m)[:n].astype(np.int32)
        if use_in:
            _, legal, status = _run(L, c, form, rows, a, col, out=out, out_idx=out_idx)
        else:
            # dense input, listed output: a fresh dense copy of the input records as d_in
            records_in = c.table.index_select(0, torch.from_numpy(rows).cuda().long()).contiguous()
            legal, status = _run_dense_in_listed_out(L, c, records_in, a, col, out, out_idx)
        untouched = np.ones(m, dtype=bool)
        untouched[out_idx[c.ok[order]]] = False
        assert bool((out[torch.from_numpy(np.flatnonzero(untouched)).cuda()] == SENTINEL).all()), "sentinel"
        _verify(L, c, out.index_select(0, torch.from_numpy(out_idx).cuda().long()), legal, status, order)


def _run_dense_in_listed_out(L, c, records_in, a, col, out, out_idx):
    import torch
    lib = L.load()
    n = len(a)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).cuda()
    d_a, d_col, d_out_idx = dev(a), dev(col), dev(out_idx)
    legal = torch.full((n, c.NW), SENTINEL, dtype=torch.int32, device="cuda")
    status = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    L.check(lib.sgo_advance_legal_dev(c.S, n, L.ptr(records_in), None, L.ptr(d_a), L.ptr(d_col), L.ptr(out), L.ptr(d_out_idx),
                                      L.ptr(legal), L.ptr(status), L.stream_ptr()))
    torch.cuda.synchronize()
    return legal, status


@pytest.mark.parametrize("S", rs.SIZES)
def test_host_calls_on_serpentines(L, S):
    """sgo_board_query modes 0 and 1, sgo_take_stones and sgo_get_winner on the serpentine, ringed and corridor boards against
    the oracle's capture_group, color_board, make_play and get_winner (the goldens reach these calls at 9x9 only)."""
    from oracle import oracle as ora
    lib = L.load()
    f = rs.load_shapes(S)
    sel = [p for p in range(f.P) if f.names[p].split("_")[0] in ("serp", "ring", "corr") and "_ko" not in f.names[p]]
    assert len(sel) >= 20
    n = len(sel)
    boards = np.ascontiguousarray(f.boards[sel])
    real = ((boards[..., 0] - boards[..., 1]) * f.colour[sel][:, None, None]).astype(np.int8)
    # the score
    w, bl, wh = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    L.check(lib.sgo_get_winner(S, n, L.ptr(boards), C.c_double(f.komi), L.ptr(w), L.ptr(bl), L.ptr(wh)))
    for i in range(n):
        assert (w[i], bl[i], wh[i]) == ora.get_winner(boards[i:i + 1], f.komi), f.names[sel[i]]
    # territory fill of both colours
    for colour in (1, -1):
        member, lib_ = np.zeros((n, S, S), np.uint8), np.ones((n, S, S), np.uint8)
        zeros, cols = np.zeros(n, np.int32), np.full(n, colour, np.int32)
        L.check(lib.sgo_board_query(S, n, 1, L.ptr(real), L.ptr(zeros), L.ptr(zeros), L.ptr(cols), L.ptr(member), L.ptr(lib_)))
        assert not lib_.any()
        for i in range(n):
            want = ora.color_board(real[i], colour)
            assert np.array_equal(np.where(member[i] != 0, colour, real[i]), want), (f.names[sel[i]], colour)
    # groups: seeded at the first and at the last stone of each colour.  With the empty points turned into
    # walls the group has no liberty and the oracle lists it; on the board itself it lives exactly when the kernel finds liberties
    for walled in (True, False):
        cells = np.where(real == 0, 2, real).astype(np.int8) if walled else real
        xs, ys, cols, keep = [], [], [], []
        for i in range(n):
            for colour in (1, -1):
                pts = np.flatnonzero(real[i].reshape(-1) == colour)
                for pt in (pts[:1].tolist() + pts[-1:].tolist()):
                    xs.append(pt % S); ys.append(pt // S); cols.append(colour); keep.append(i)
        m = len(xs)
        member, lib_ = np.zeros((m, S, S), np.uint8), np.zeros((m, S, S), np.uint8)
        q_cells = np.ascontiguousarray(cells[keep])       # kept in names: the call reads them through bare pointers
        q_xs, q_ys, q_cols = np.array(xs, np.int32), np.array(ys, np.int32), np.array(cols, np.int32)
        L.check(lib.sgo_board_query(S, m, 0, L.ptr(q_cells), L.ptr(q_xs), L.ptr(q_ys), L.ptr(q_cols), L.ptr(member), L.ptr(lib_)))
        for j in range(m):
            grp = ora.capture_group(xs[j], ys[j], cells[keep[j]])
            if walled:
                got = sorted((int(x), int(y)) for y, x in zip(*np.nonzero(member[j])))
                assert grp is not None and got == sorted(grp) and not lib_[j].any(), (f.names[sel[keep[j]]], xs[j], ys[j])
            else:
                assert np.array_equal(member[j], walled_member[j]), (f.names[sel[keep[j]]], xs[j], ys[j])
                mem = member[j] != 0
                near = np.zeros_like(mem)
                near[1:] |= mem[:-1]; near[:-1] |= mem[1:]; near[:, 1:] |= mem[:, :-1]; near[:, :-1] |= mem[:, 1:]
                assert np.array_equal(lib_[j] != 0, near & (real[keep[j]] == 0)), (f.names[sel[keep[j]]], xs[j], ys[j])
                assert (grp is None) == bool(lib_[j].any())
        walled_member = member
    # take_stones: the recorded plays of these positions, the stone put down by hand
    sel_set = {p: i for i, p in enumerate(sel)}
    plays = [k for k in range(f.K) if int(f.play_pos[k]) in sel_set and f.play_colour[k] == 0]
    tb = np.ascontiguousarray(f.boards[f.play_pos[plays]])
    xs, ys = (f.play_a[plays] % S).astype(np.int32), (f.play_a[plays] // S).astype(np.int32)
    tb[np.arange(len(plays)), ys, xs, 0] = 1
    before = tb.copy()
    L.check(lib.sgo_take_stones(S, len(plays), L.ptr(tb), L.ptr(xs), L.ptr(ys)))
    assert np.array_equal(tb[..., 2:], before[..., 2:])
    for j, k in enumerate(plays):
        b = f.boards[f.play_pos[k]][None].copy()
        ora.make_play(int(xs[j]), int(ys[j]), b)
        assert np.array_equal(tb[j, :, :, 0], b[0, :, :, 1]) and np.array_equal(tb[j, :, :, 1], b[0, :, :, 0]), (f.names[f.play_pos[k]], k)
