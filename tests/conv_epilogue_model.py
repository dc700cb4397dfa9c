"""The epilogue contract of the 3x3 convolution kernels (k_conv4w, k_conv8w, k_conv4r, k_stem, k_stem_packed) and of k_bias_act,
in NumPy, without a GPU ("Epilogue contract").

Convolution: an explicit sum over taps and channels in float64 with plain IEEE arithmetic -- every product is formed, 0 * inf is
NaN, nothing is skipped (np.einsum without `optimize` is a plain loop of multiply-adds, no BLAS).  The accumulator starts at +0, as
the kernels' registers do.  A tap off the board contributes the PADDING, +0, times its weight (what the tile code's zero area
holds and what a zero-padded convolution computes); the pixel that lies there in memory -- a neighbouring sample's -- is not read.
The cases of tests/conv_epilogue_cases.py keep every accumulator exact in fp32 in any summation order (one fp16 x fp16 product
per output, or two whose sum is representable), which `exact_in_fp32` asserts, so the model assumes nothing about the MFMA order.

Epilogue of the conv kernels:   f = fp32(fp32(acc + skip) + bias)        (stems: no skip; packed stem: fp32(. + col * wcol) last)
                                out = NaN if f is NaN, else fp16(max(f, +0)) to nearest, ties to even:
                                +inf stays +inf, finite f >= 65520 becomes +inf, -0 becomes +0, results below 2^-14 are subnormal.
Why f cannot be -0 in those kernels: acc starts at +0 and x + (-x) = +0 under round-to-nearest, so acc is never -0; (+0) + (-0) =
+0 for skip and bias.  `neg_zero_kept` therefore applies to k_bias_act only, whose fp16 sum (-0) + (-0) is -0.

k_bias_act: r = fp16(x + bias); r = fp16(r + skip): two correctly rounded fp16 adds (bias first), then the same ReLU rule.

FAULTS are mutations of this model that the case set must catch (tests/test_conv_epilogue_power.py); APPLIES names, per fault,
the case groups in which it can change a result at all.
"""
import numpy as np

QNAN = 0x7E00           # how a NaN is written in expected bits (compared as "is NaN")
CANARY = 0x5A5A         # fp16 bits of the guard rows around y
GROUPS = ("tower_skip", "tower_noskip", "stem", "packed", "bias_act")
FAULTS = ("rtz", "half_up", "acc_to_fp16_first", "bias_before_skip", "nan_to_zero", "inf_saturates", "flush_subnormal_out",
          "neg_zero_kept", "edge_multiplied", "tail_skip_unclamped", "bias_act_single_rounding")
APPLIES = {
    "rtz": GROUPS,                                        # conversion truncates
    "half_up": GROUPS,                                    # ties round away from zero
    "acc_to_fp16_first": GROUPS[:4],                      # the accumulator is rounded to fp16 before the adds
    "bias_before_skip": ("tower_skip", "packed", "bias_act"),   # the adds in the other order (packed: colour term before bias)
    "nan_to_zero": GROUPS,                                # f > 0 ? f : 0
    "inf_saturates": GROUPS,                              # +inf / overflow clamped to 65504
    "flush_subnormal_out": GROUPS,                        # subnormal fp16 results become 0
    "neg_zero_kept": ("bias_act",),                       # f < 0 ? 0 : f keeps -0 (see above why only there)
    "edge_multiplied": ("tower_skip", "tower_noskip"),    # off-board taps: the neighbour in memory times zero
    "tail_skip_unclamped": ("tower_skip", "tower_noskip"),   # rows past M of a ragged tile are computed from what lies there and stored
    "bias_act_single_rounding": ("bias_act",),            # k_bias_act adding in fp32 and rounding once, as the conv kernels do
}


def h(v):
    """fp16 array of values that must be exact in fp16"""
    a = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):
        r = a.astype(np.float16)
    ok = (r.astype(np.float64) == a) | (np.isnan(a) & np.isnan(r))
    assert ok.all(), "not exact in fp16: %r" % (a[~ok][:4],)
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def same_bits(a, b):
    """element-wise: identical fp16 bits, or both NaN"""
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    nan_a, nan_b = (a & 0x7FFF) > 0x7C00, (b & 0x7FFF) > 0x7C00
    return (a == b) | (nan_a & nan_b)


def _grid(mag):
    """value of an fp16 magnitude pattern, with 0x7C00 read as 65536: the next step of the grid beyond 65504"""
    mag = np.asarray(mag, np.uint16)
    with np.errstate(invalid="ignore"):
        v = mag.view(np.float16).astype(np.float64)
    return np.where(mag == 0x7C00, 65536.0, v)


def round_half(f, mode="rne"):
    """float64 values (NaN-free) -> fp16.  rne: IEEE nearest-even (NumPy's conversion: overflow to inf from 65520, gradual
    underflow); rtz: toward zero; half_up: nearest, ties away from zero."""
    f = np.asarray(f, np.float64)
    with np.errstate(over="ignore"):
        r = f.astype(np.float16)
    if mode == "rne":
        return r
    rb = r.view(np.uint16)
    sign, mag = rb & 0x8000, (rb & 0x7FFF).astype(np.uint16)
    a, fin = np.abs(f), np.isfinite(f)
    rv = _grid(mag)
    if mode == "rtz":
        mag = np.where(fin & ((rv > a) | (mag == 0x7C00)), np.minimum(mag - 1, 0x7BFF), mag)
    else:
        assert mode == "half_up", mode
        nxt = _grid(np.minimum(mag + 1, 0x7C00).astype(np.uint16))
        mag = np.where(fin & (rv < a) & ((nxt - a) == (a - rv)), mag + 1, mag)
    return (sign | mag).astype(np.uint16).view(np.float16)


def fp16_neighbours(f):
    """(lo, hi): the fp16 grid values (65536 = the step beyond 65504) with lo <= |f| <= hi, lo == hi when |f| is on the grid"""
    a = np.abs(np.asarray(f, np.float64))
    a = np.where(np.isfinite(a), a, 0.0)
    lo_bits = (round_half(np.minimum(a, 65536.0), "rtz").view(np.uint16) & 0x7FFF).astype(np.uint16)
    lo_bits = np.where(a >= 65536.0, 0x7C00, lo_bits).astype(np.uint16)
    lo = _grid(lo_bits)
    hi = np.where(lo == a, lo, _grid(np.minimum(lo_bits + 1, 0x7C00).astype(np.uint16)))
    return lo, hi


def exact_in_fp32(acc):
    fin = np.isfinite(acc)
    with np.errstate(over="ignore", invalid="ignore"):
        return bool((acc.astype(np.float32).astype(np.float64)[fin] == acc[fin]).all())


def conv_acc(x, w, pad, reverse=False, fault=None, rows=None):
    """acc [rows, K] float64 of x [n, h, w, C] with filters w [K, 3, 3, C] (cross-correlation, tap = dy * 3 + dx), pad 0 or 1.
    rows: how many output pixels to compute (default all; more than that -- `tail_skip_unclamped` -- have no tap on the board).
    reverse: the terms are added in the opposite order (taps 8..0, channels C-1..0)."""
    n, hh, ww, C = x.shape
    K = w.shape[0]
    ho, wo = (hh, ww) if pad else (hh - 2, ww - 2)
    M = n * ho * wo
    rows = M if rows is None else rows
    flat = np.asarray(x, np.float64).reshape(n * hh * ww, C)
    w64 = np.asarray(w, np.float64)
    p = np.arange(rows)
    s, r = p // (ho * wo), p % (ho * wo)
    oy, ox = r // wo, r % wo
    acc = np.zeros((rows, K), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in (range(8, -1, -1) if reverse else range(9)):
            dy, dx = divmod(t, 3)
            iy, ix = oy + dy - pad, ox + dx - pad
            on = (iy >= 0) & (iy < hh) & (ix >= 0) & (ix < ww) & (p < M)
            src = np.clip((s * hh + iy) * ww + ix, 0, n * hh * ww - 1)        # off the board: the neighbour in memory
            px = flat[src]
            if fault == "edge_multiplied":
                px = np.where(on[:, None], px, px * 0.0)
            else:
                px = np.where(on[:, None], px, 0.0)
            wt = w64[:, dy, dx, :]
            if reverse:
                px, wt = px[:, ::-1], wt[:, ::-1]
            acc += np.einsum("mc,kc->mk", px, wt)
    return acc


def _relu_round(f, fault):
    """f float32 -> fp16 bits by the contract (or a fault's version of it)"""
    nan = np.isnan(f)
    f64 = np.where(nan, 0.0, f.astype(np.float64))
    g = np.where(f64 < 0, 0.0, f64) if fault == "neg_zero_kept" else np.where(f64 > 0, f64, 0.0)
    o = round_half(g, fault if fault in ("rtz", "half_up") else "rne")
    if fault == "inf_saturates":
        o = np.where(np.isinf(o), np.float16(65504.0), o)
    if fault == "flush_subnormal_out":
        o = np.where(np.abs(o.astype(np.float64)) < 2.0 ** -14, np.float16(0.0), o)
    b = bits(o).copy()
    if fault != "nan_to_zero":
        b[nan] = QNAN
    return b


def epilogue(acc, bias, skip=None, colterm=None, fault=None):
    """(fp16 bits [M, K], f float32 [M, K]) of acc float64 [M, K], bias fp16 [K], skip fp16 [M, K] or None, colterm float32
    [M, K] or None (the packed stem's col * wcol, exact because col is +-1)."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = acc.astype(np.float32)
        if fault == "acc_to_fp16_first":
            a = a.astype(np.float16).astype(np.float32)
        terms = ([np.asarray(skip, np.float16).astype(np.float32)] if skip is not None else []) + \
                [np.asarray(bias, np.float16).astype(np.float32)[None, :]] + \
                ([np.asarray(colterm, np.float32)] if colterm is not None else [])
        if fault == "bias_before_skip":
            terms = terms[::-1]
        f = a
        for t in terms:
            f = (f + t).astype(np.float32)                   # one correctly rounded fp32 add each
    return _relu_round(f, fault), f


def bias_act(x, bias, skip=None, fault=None):
    """fp16 bits of k_bias_act: x [rows, C], bias [C], skip [rows, C] or None, all fp16.  The sum of two fp16 numbers is exact
    in float64, so each add is one rounding of an exact value."""
    mode = fault if fault in ("rtz", "half_up") else "rne"

    def add(a, b):
        with np.errstate(invalid="ignore", over="ignore"):
            s = a.astype(np.float64) + b.astype(np.float64)
        nan = np.isnan(s)
        r = round_half(np.where(nan, 0.0, s), mode).copy()
        r[nan] = np.float16(np.nan)
        return r

    x, bias = np.asarray(x, np.float16), np.asarray(bias, np.float16)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        if fault == "bias_act_single_rounding":
            f = (x.astype(np.float32) + bias.astype(np.float32)).astype(np.float32)
            if skip is not None:
                f = (f + np.asarray(skip, np.float16).astype(np.float32)).astype(np.float32)
            return _relu_round(f, None)
        if skip is None:
            r = add(x, bias)
        elif fault == "bias_before_skip":
            r = add(add(x, np.asarray(skip, np.float16)), bias)
        else:
            r = add(add(x, bias), np.asarray(skip, np.float16))
        return _relu_round(r.astype(np.float32), fault)
