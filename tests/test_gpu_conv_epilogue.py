"""The epilogues of the convolution kernels and of k_bias_act, bit for bit against tests/conv_epilogue_model.py on the constructed
cases of tests/conv_epilogue_cases.py (tests/test_conv_epilogue_power.py shows on CPU what these cases catch and reach).

 * raw 16-bit views are compared, a NaN as "is NaN"; y is a view into a buffer of canaries and the WHOLE buffer is compared; x and
   skip are views into buffers whose guard rows are NaN, so a read past either end shows in the output;
 * tower cases on every tower route: k_conv4w and k_conv8w behind sgo_conv3x3_tower_dev, k_conv4r behind
   sgo_conv3x3_tower_packed_dev, and the dispatching sgo_conv3x3_bias_act_dev; stem cases through sgo_conv3x3_stem_dev (and the
   dispatcher) and sgo_stem_packed_dev on records sgo_pack_dev wrote; k_bias_act in place and out of place;
 * tracers: with non-finite values planted on the corners and an edge of the middle sample, every output outside their 3x3
   neighbourhoods is bit-identical to the launch without them;
 * k_heads: a NaN at one pixel of one row of the tower output makes that row's policy and value NaN and leaves every other row's
   bits alone;
 * the whole 9x9 4-block calibrated net with one bias of a middle block set to NaN: policy and value are NaN in every row and
   netcal.logit_error is inf, on each tower kernel and both head routes -- which is what makes the isfinite assert of
   tests/test_gpu_net_parity.py mean what its comment says; with the bias restored the launch is back within LOGIT_TOL."""
import numpy as np
import pytest

from tests import conv_epilogue_cases as C
from tests import conv_epilogue_model as M
from tests import netcal

pytestmark = pytest.mark.gpu

TOWER_ROUTES = ("k_conv4w", "k_conv8w", "k_conv4r", "dispatch")


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(rows2d):
    """(buffer, view): rows2d [M, C] fp16 inside C.GUARD_ROWS rows of NaN on either side"""
    import torch
    m, c = rows2d.shape
    buf = torch.full((m + 2 * C.GUARD_ROWS, c), float("nan"), dtype=torch.float16, device="cuda")
    view = buf[C.GUARD_ROWS:C.GUARD_ROWS + m]
    view.copy_(_dev(rows2d))
    assert view.data_ptr() % 16 == 0
    return buf, view


def _ybuf(m):
    import torch
    buf = torch.full((C.Y_FRONT + m + C.Y_BACK, 256), M.CANARY, dtype=torch.int16, device="cuda")
    return buf, buf[C.Y_FRONT:C.Y_FRONT + m]


def _check(buf, want, what):
    import torch
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint16)
    assert got.shape == want.shape, what
    bad = ~M.same_bits(got, want)
    if bad.any():
        r, k = np.argwhere(bad)[0]
        raise AssertionError("%s: %d elements differ, first at buffer row %d (pixel %d) channel %d: got 0x%04x want 0x%04x"
                             % (what, int(bad.sum()), r, r - C.Y_FRONT, k, got[r, k], want[r, k]))
    return got


def _run_tower(L, route, launch, bank_cache):
    import torch
    lib, st = L.load(), L.stream_ptr()
    xb, x = _guarded(launch.x.reshape(launch.M, 256))
    sb, skip = _guarded(launch.skip) if launch.skip is not None else (None, None)
    w, b = _dev(launch.wt), _dev(launch.bias)
    ybuf, y = _ybuf(launch.M)
    sp = None if skip is None else skip.data_ptr()
    n, h, wd = launch.n, launch.h, launch.w
    if route == "k_conv4r":
        key = launch.wt.tobytes()
        if key not in bank_cache:
            bank = torch.empty(lib.sgo_conv3x3_tower_packed_bytes(), dtype=torch.uint8, device="cuda")
            L.check(lib.sgo_conv3x3_tower_prepack_dev(w.data_ptr(), bank.data_ptr(), st), "prepack")
            bank_cache.clear()
            bank_cache[key] = bank
        L.check(lib.sgo_conv3x3_tower_packed_dev(n, h, wd, x.data_ptr(), bank_cache[key].data_ptr(), b.data_ptr(), sp, y.data_ptr(), st), route)
    elif route == "dispatch":
        L.check(lib.sgo_conv3x3_bias_act_dev(n, h, wd, 256, 256, 1, x.data_ptr(), w.data_ptr(), b.data_ptr(), sp, y.data_ptr(), st), route)
    else:
        old = lib.sgo_conv_tower_kernel(0 if route == "k_conv8w" else 1)
        try:
            L.check(lib.sgo_conv3x3_tower_dev(n, h, wd, x.data_ptr(), w.data_ptr(), b.data_ptr(), sp, y.data_ptr(), st), route)
        finally:
            lib.sgo_conv_tower_kernel(old)
    return _check(ybuf, C.expected(launch), "%s %r" % (route, launch))


@pytest.mark.parametrize("group", ["tower_skip", "tower_noskip"])
@pytest.mark.parametrize("route", TOWER_ROUTES)
def test_tower_epilogue_bits(L, route, group):
    banks = {}
    for launch in C.launches(group):
        got = _run_tower(L, route, launch, banks)
        front, back = got[:C.Y_FRONT], got[C.Y_FRONT + launch.M:]
        assert (front == M.CANARY).all() and (back == M.CANARY).all(), (route, launch, "canaries")
        if launch.clean is not None:
            # the tracer: outside the 3x3 neighbourhoods of the planted values (and skip's last pixel) nothing moved
            clean = _run_tower(L, route, launch.clean, banks)
            out = ~C.neighbourhood(launch)
            if launch.skip is not None:
                out[launch.M - 1] = False
            a, b = got[C.Y_FRONT:C.Y_FRONT + launch.M], clean[C.Y_FRONT:C.Y_FRONT + launch.M]
            assert np.array_equal(a[out], b[out]), (route, launch, "a planted value reached beyond its neighbourhood")
            assert not M.same_bits(a[~out], b[~out]).all()


def test_stem_epilogue_bits(L):
    lib, st = L.load(), L.stream_ptr()
    for launch in C.launches("stem"):
        xb, x = _guarded(launch.x.reshape(-1, 32))
        w, b = _dev(launch.wt), _dev(launch.bias)
        for route in ("sgo_conv3x3_stem_dev", "dispatch"):
            ybuf, y = _ybuf(launch.M)
            if route == "dispatch":
                L.check(lib.sgo_conv3x3_bias_act_dev(launch.n, launch.h, launch.w, 32, 256, 0, x.data_ptr(), w.data_ptr(), b.data_ptr(),
                                                     None, y.data_ptr(), st), route)
            else:
                L.check(lib.sgo_conv3x3_stem_dev(launch.n, launch.h, launch.w, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), st), route)
            _check(ybuf, C.expected(launch), "%s %r" % (route, launch))


def test_packed_stem_epilogue_bits(L):
    import torch
    lib, st = L.load(), L.stream_ptr()
    for launch in C.launches("packed"):
        S, n = launch.S, launch.n
        boards = _dev(launch.boards)
        recs = torch.zeros((n, lib.sgo_packed_words(S)), dtype=torch.int32, device="cuda")
        # (these two entry points declare no argument types: pointers go through L.ptr, a bare int would be cut to 32 bits)
        L.check(lib.sgo_pack_dev(S, n, L.ptr(boards), L.ptr(recs), st), "sgo_pack_dev")
        # the planes the model convolves are the planes the device makes of these records under this symmetry
        x = torch.zeros((n, S, S, 17), dtype=torch.float32, device="cuda")
        L.check(lib.sgo_nn_pack_dev(S, n, L.ptr(recs), None, launch.sym, 0, 1, L.ptr(x), st), "sgo_nn_pack_dev")
        torch.cuda.synchronize()
        xn = x.cpu().numpy()
        assert np.array_equal(xn[..., :16], C.packed_planes(launch).astype(np.float32)), launch
        assert np.array_equal(xn[..., 16], np.broadcast_to(launch.colour[:, None, None], (n, S, S)).astype(np.float32)), launch
        w10, b, wcol = _dev(launch.w10), _dev(launch.bias), _dev(launch.wcol)
        ybuf, y = _ybuf(launch.M)
        L.check(lib.sgo_stem_packed_dev(S, n, recs.data_ptr(), None, launch.sym, None, w10.data_ptr(), b.data_ptr(), wcol.data_ptr(),
                                        y.data_ptr(), st), "sgo_stem_packed_dev")
        _check(ybuf, C.expected(launch), repr(launch))


def test_bias_act_bits(L):
    import torch
    lib, st = L.load(), L.stream_ptr()
    for launch in C.launches("bias_act"):
        x, b = _dev(launch.x), _dev(launch.bias)
        skip = None if launch.skip is None else _dev(launch.skip)
        sp = None if skip is None else skip.data_ptr()
        want = C.expected(launch)
        out = torch.full(x.shape, M.CANARY, dtype=torch.int16, device="cuda")
        L.check(lib.sgo_bias_act_dev(x.numel(), launch.C, x.data_ptr(), b.data_ptr(), sp, out.data_ptr(), st), "sgo_bias_act_dev")
        _check(out, want, "%r out of place" % (launch,))
        y = x.clone()
        L.check(lib.sgo_bias_act_dev(y.numel(), launch.C, y.data_ptr(), b.data_ptr(), sp, y.data_ptr(), st), "sgo_bias_act_dev")
        _check(y.view(torch.int16), want, "%r in place" % (launch,))


def test_heads_pass_a_nan_to_its_own_row_only(L):
    import torch
    from tests import test_gpu_heads as th
    S, n, row = 9, 33, 17
    c = th.int_case(L, S)
    args = (c.head_w, c.head_b, c.bank, c.p_fc_b, c.v_fc1_b, c.v_fc2_w, c.v_fc2_b)
    pol0, val0 = th.run_heads(L, S, n, c.y, *args)
    y = c.y.clone()
    y[row, 3, 4, 100] = float("nan")
    pol1, val1 = th.run_heads(L, S, n, y, *args)
    assert bool(torch.isnan(pol1[row]).all()) and bool(torch.isnan(val1[row])), "the row with the NaN"
    others = [r for r in range(n + 2) if r != row]                          # the guard rows behind the outputs included
    assert torch.equal(pol1[others].view(torch.int32), pol0[others].view(torch.int32))
    assert torch.equal(val1[others].view(torch.int32), val0[others].view(torch.int32))
    assert bool(torch.isfinite(pol0[:n]).all()) and bool(torch.isfinite(val0[:n]).all())


@pytest.mark.parametrize("heads", ["torch_heads", "k_heads"])
@pytest.mark.parametrize("kernel", ["k_conv4w", "k_conv8w", "k_conv4r"])
def test_whole_net_with_a_nan_bias_is_not_finite(L, kernel, heads):
    import torch
    from tests import test_gpu_net_parity as tp
    S, blocks, ply, rows = 9, 4, 30, 8
    case = tp.shared_case(L, S, blocks)
    fnet, recs = case.fnet, case.recs[ply]
    ref = case.ref(ply, 0)[0][:rows]
    tol = netcal.LOGIT_TOL[(S, blocks)]
    mid = len(fnet.blocks) // 2
    saved = fnet.blocks[mid]
    assert fnet.use_fused_heads(heads == "k_heads") == (heads == "k_heads")
    try:
        with tp._Tower(case, kernel):
            b1 = saved[1].clone()
            b1[5] = float("nan")
            try:
                fnet.blocks[mid] = (saved[0], b1, saved[2], saved[3])
                p, v = fnet.predict_packed(recs.data_ptr(), None, rows, 0)
            finally:
                fnet.blocks[mid] = saved
            assert bool(torch.isnan(p).all()) and bool(torch.isnan(v).all()), "a NaN bias in block %d left finite outputs" % mid
            assert netcal.logit_error(torch.log(p.double()), ref) == float("inf")
            p, v = fnet.predict_packed(recs.data_ptr(), None, rows, 0)
            assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all())
            restored = netcal.logit_error(torch.log(p.double()), ref)
            assert restored <= tol, restored
    finally:
        fnet.use_fused_heads(False)

