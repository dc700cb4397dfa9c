"""Constructed inputs for the epilogues of the convolution kernels, with accumulators that are exact by construction, and their
expected output bits from tests/conv_epilogue_model.py.  Run on the device by tests/test_gpu_conv_epilogue.py; what they can
catch is shown without a GPU by tests/test_conv_epilogue_power.py.

Weights are one-hot: w[k][tap(k)][c(k)] = s_k, zero elsewhere, c = PERM a fixed non-identity permutation (a channel mix-up
shows), so acc[p][k] is ONE exact fp16 x fp16 product (the packed stem: up to two 0/1 x fp16 products whose sum is representable)
and exact in fp32 in any order.  In the tower x[.][c(k)] and skip[.][k] are free per element, bias and s per channel: a channel has
a KIND (s, bias), rotated over the launches, and walks the kind's list of (x, skip) VARIANTS over the pixels.  The classes an
element belongs to are not labels but properties computed from the model (`classify`): ties, neighbours of ties, overflow (and
its edge, 65504 < f <= 65520), subnormals, zeros and signs (and a -0 among the addends), the two discriminators, non-finite inputs.

Layouts: x, skip and y are views into larger buffers (`GUARD_ROWS` pixel rows of NaN before and after x and skip, `Y_FRONT` /
`Y_BACK` rows of CANARY around y); the expected output covers y's whole buffer.  Tracer launches put non-finite values on the four
corners and an edge of the middle sample and into skip at pixel M - 1 of a ragged launch; their twin without the tracer is `clean`.

Shapes: the tower at 17x17, 7x7, 19x19 and 1x1 and at the tower shapes of board sizes 5, 7 and 13 (3x3, 5x5, 11x11); k_stem and the
packed stem at board sizes 5, 7, 13 and 19.
"""
import functools

import numpy as np

from tests import conv_epilogue_model as M

E = 2.0 ** -10
NAN, INF = float("nan"), float("inf")
GUARD_ROWS = 64                  # NaN rows before / after x and skip
Y_FRONT, Y_BACK = 8, 256         # canary rows around y (the back one holds a whole tile: `tail_skip_unclamped`)
PERM = (np.arange(256) * 77 + 13) % 256

# ---- tower / k_stem kinds: (s, bias) and the (x, skip) variants walked over the pixels (skip is ignored without a skip tensor)
KINDS = [
    (1.0, 2.0 ** -11, [
        (1.0, 0.0), (1.0 + E, -0.0),                                   # exact ties: 1 + 2^-11 (down), 1 + 3 * 2^-11 (up)
        (1.0, 2.0 ** -23), (1.0, -2.0 ** -23),                         # their fp32 neighbours
        (1.0 + E, 2.0 ** -23), (1.0 + E, -2.0 ** -23),
        (-2.0 ** -11, 0.0), (-1.0, 0.5), (0.0, -0.0),                  # 0 by cancellation, negative, -0 in skip
        (65504.0, 0.0), (65504.0, 16.0 - 2.0 ** -7), (65504.0, 16.0),  # 65504, just below 65520, 65520
        (65504.0, 32.0), (65504.0, 65504.0), (-65504.0, -65504.0),     # above, far above, far below
        (1.0, NAN), (1.0, INF), (1.0, -INF), (2.0, -1.0)]),
    (1.0 + E, -(1.0 + 2 * E), [
        (1.0 + E, 0.0),                                                # acc_to_fp16_first: 2^-20 against 0
        (1.0 + 3 * E, 0.0), (1.0 + 2 * E, 0.0), (1.0 + E, 1.0),        # a tie at 2^-9, exact, 1 + 2^-20
        (1.0 + E, 2.0 ** -24), (1.0 + E, 1.0 + 2 * E), (1.0, 0.0), (2.0, -0.5), (1.0 + E, NAN), (1.0 + E, INF), (1.0 + E, -INF),
        (3.0 + 2 * E, -1.0)]),
    (256.0, -32768.0, [
        (128.0, 2.0 ** -9),                                            # bias_before_skip: fp32(32768 + 2^-9) = 32768
        (128.0, 3 * 2.0 ** -9), (128.0, 2.0 ** -8), (128.0, -0.0), (127.9375, 0.0), (128.125, 0.0),
        (384.0, 0.0), (383.75, 0.0), (383.75, 32.0), (383.75, 48.0), (383.75, 48.0 - 2.0 ** -5),
        (128.0, NAN), (128.0, INF), (128.0, -INF), (128.0, 1.0 + E)]),
    (2.0 ** -14, -0.0, [
        (1.0, 0.0), (1.0 - 2.0 ** -11, 0.0), (1.0 - E, 0.0),           # smallest normal, the tie below it, largest subnormal
        (0.5 + 2.0 ** -11, 0.0), (0.5 + 3 * 2.0 ** -11, 0.0),          # subnormal ties, down and up
        (0.25 + 2.0 ** -12, 0.0), (0.25 + 3 * 2.0 ** -12, 0.0),        # a quarter / three quarters of a subnormal step
        (E, 0.0), (2.0 ** -11, 0.0), (3 * 2.0 ** -11, 0.0), (2.0 ** -12, 0.0),   # 2^-24, the ties around it, below half of it
        (0.0, -0.0), (-0.0, -0.0), (-1.0, 0.0), (1.0, 2.0 ** -14), (1.0, -2.0 ** -14), (1.0, 2.0 ** -24),
        (1.0, NAN), (1.0, INF), (1.0, -INF), (65504.0, 0.0), (65504.0, 65504.0)]),
    (1.0 + E, 2.0 ** -11, [
        (1.0 + E, 0.0), (1.0, 0.0), (1.0 - 2.0 ** -11, 0.0), (1.0 - 2.0 ** -11, -2.0 ** -11), (1.0 + 2 * E, 0.0),
        (65504.0, 0.0), (-1.0, 0.0), (32.0, 0.0), (1.0, NAN), (1.0, INF), (1.0, -INF), (1.0 + E, -2.0 ** -11)]),
    (1.0 + 2 * E, 0.0, [
        (1.0 - 2.0 ** -11, 0.0), (1.0 - 2.0 ** -11, 2.0 ** -20), (1.0 - 2.0 ** -11, 2.0 ** -19),   # below a tie, the tie, above
        (1.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-1.0, 1.0 + 2 * E), (65504.0, 0.0), (0.5 + 2.0 ** -11, 0.0),
        (1.0, NAN), (1.0, INF), (1.0, -INF)]),
    (1.5, -0.0, [
        (43680.0, 0.0), (43680.0, -1.0), (43680.0, -0.0),              # 65520 from one product (the only way without a skip), 65519
        (43648.0, 48.0), (43648.0, 32.0), (43680.0, 16.0),             # 65520 and 65504 through the skip, 65536
        (1.0, 0.0), (-1.0, 0.0), (0.0, -0.0), (43680.0, NAN), (43680.0, INF), (43680.0, -INF), (43680.0, -16.0 + 2.0 ** -7)]),
]
NK = len(KINDS)

# ---- packed stem kinds (s1, s2, bias, wcol): acc is 0, s1, s2 or s1 + s2 by the stones; f = fp32(fp32(acc + bias) +- wcol).  Their
#      classes come round with period 8, so 8 rotations show each channel every class.
PKINDS = [
    (0, 0, 1.0 + E, 2.0 ** -11),                      # ties both ways: 1 + 3 * 2^-11 (up), 1 + 2^-11 (down)
    (0, 0, 1.0 + E, 2.0 ** -11 + 2.0 ** -23),         # their neighbours: wcol's low mantissa bits reach the rounding
    (16.0, 8.0, 65504.0, 0.0),                        # 65504, 65512, 65520, 65528 by the stones
    (0, 0, 2.0 ** -15, 2.0 ** -25),                   # subnormal ties
    (0, 0, -0.0, 0.5),                                # -0 in the bias; negative under colour -
    (1.0, 2.0 ** -11, -1.0, 0.0),                     # acc_to_fp16_first: acc = 1 + 2^-11 where both stones lie
    (49152.0, -49152.0, 2.0 ** -9, 49152.0),          # bias_before_skip: fp32(+-49152 + 2^-9) = +-49152, then the colour term cancels
    (0, 0, 1.0, NAN),
    (0, 0, 1.0 + 3 * E, 2.0 ** -11),
    (0, 0, 1.0 + E, 2.0 ** -11 - 2.0 ** -23),
    (16.0, 0, 65504.0, 0.0),                          # 65520 under a stone: inf
    (0, 0, 2.0 ** -16, 3 * 2.0 ** -26),               # a quarter / three quarters of a subnormal step
    (0, 0, -0.0, 0.0),                                # zeros with signs
    (1.0 + E, 2.0 ** -11, -(1.0 + E), 2.0 ** -24),
    (49152.0, -49152.0, 3 * 2.0 ** -9, 49152.0),
    (INF, 0, 1.0, 0.0),                               # 0 * inf where no stone lies
    (1.0, 0, 2.0 ** -11, 0.0),                        # a tie through the accumulator
    (0, 0, 1.0 + 3 * E, 2.0 ** -11 + 2.0 ** -22),
    (16.0, 32.0, 65504.0, 2.0 ** -30),                # 65504, 65520, above
    (2.0 ** -15, 2.0 ** -24, 2.0 ** -16, 2.0 ** -27),
    (1.0, -1.0, -0.0, 0.0),                           # 0 by cancellation under both stones, -1 under one, -0 in the bias
    (1.0, 2.0 ** -11, -1.0, 2.0 ** -30),
    (40960.0, -40960.0, 2.0 ** -9, 40960.0),
    (0, 0, -INF, 1.0),
    (0, 0, 65472.0, 16.0),                            # ties at 65488 and 65456
    (0, 0, 2.0 + 2 * E, 2.0 ** -10 + 2.0 ** -22),
    (8.0, 8.0, 65504.0, 0.0),                         # 65512 (below 65520), 65520
    (0, 0, 3 * 2.0 ** -24, 2.0 ** -25),
    (-1.0, 0, -0.0, 0.0),
    (2.0, 2.0 ** -10, -2.0, 0.0),
    (49152.0, -49152.0, 2.0 ** -9, 49152.0),
    (0, 0, 1.0, -INF),
]
NPK = len(PKINDS)


def _poison(how, r, bias, wt):
    """non-finite biases and weights: on six channels (how = True), or on every channel, the six sorts rotated (how = "all")"""
    for i, k in enumerate(range(256) if how == "all" else [(31 + 97 * r + 40 * j) % 256 for j in range(6)]):
        which = (i + r) % 6 if how == "all" else i
        if which < 3:
            bias[k] = np.float16((NAN, INF, -INF)[which])
        else:
            wt[k][wt[k] != 0] = np.float16((NAN, INF, -INF)[which - 3])


class Launch(object):
    """One launch: group, name, shape and tensors (NumPy, fp16 unless noted).  M output pixel rows, K = 256 output channels."""
    clean = None

    def __init__(self, group, name, **kw):
        self.group, self.name = group, name
        self.__dict__.update(kw)

    def __repr__(self):
        return "%s:%s" % (self.group, self.name)


def _arr(vals):
    return M.h(np.array(vals, dtype=np.float64))


_VX = [_arr([v[0] for v in k[2]]) for k in KINDS]
_VS = [_arr([v[1] for v in k[2]]) for k in KINDS]


def tower_launch(n, h, w, r, with_skip, mixed_taps=False, poison=False, tracer=False):
    Mx = n * h * w
    kind = (np.arange(256) + r) % NK
    tap = ((np.arange(256) * 5 + r) % 9) if mixed_taps else np.full(256, 4)
    s = _arr([KINDS[g][0] for g in kind])
    bias = _arr([KINDS[g][1] for g in kind])
    x = np.full((Mx, 256), 0.5, dtype=np.float16)
    skip = np.zeros((Mx, 256), dtype=np.float16)
    wt = np.zeros((256, 3, 3, 256), dtype=np.float16)
    p = np.arange(Mx)
    rr = p % (h * w)
    oy, ox = rr // w, rr % w
    for k in range(256):
        g = kind[k]
        vi = (p + k // NK + r) % len(_VX[g])
        dy, dx = divmod(int(tap[k]), 3)
        iy, ix = oy + dy - 1, ox + dx - 1
        on = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
        x[(p + (dy - 1) * w + dx - 1)[on], PERM[k]] = _VX[g][vi][on]
        skip[:, k] = _VS[g][vi]
        wt[k, dy, dx, PERM[k]] = s[k]
    if poison:
        _poison(poison, r, bias, wt)
    name = "%dx%dx%d r%d %s%s%s%s" % (n, h, w, r, "skip" if with_skip else "noskip", " mixed-taps" if mixed_taps else "",
                                      (" poison-all" if poison == "all" else " poison") if poison else "", " tracer" if tracer else "")
    L = Launch("tower_skip" if with_skip else "tower_noskip", name, n=n, h=h, w=w, pad=1, M=Mx, x=x.reshape(n, h, w, 256), wt=wt,
               bias=bias, skip=skip if with_skip else None, marks=[])
    if tracer:
        L.clean = tower_launch(n, h, w, r, with_skip, mixed_taps, poison)
        i = n // 2
        xs = L.x
        for (yy, xx, ch, v) in ((0, 0, 5, NAN), (0, w - 1, 200, INF), (h - 1, 0, 77, -INF), (h - 1, w - 1, 255, NAN), (h // 2, 0, 0, INF)):
            xs[i, yy, xx, ch] = np.float16(v)
            L.marks.append((i, yy, xx))
        if with_skip:
            L.skip[Mx - 1, 0::3], L.skip[Mx - 1, 1::3] = np.float16(NAN), np.float16(INF)
    return L


def stem_launch(n, h, w, r, poison=False):
    """k_stem: x [n, h, w, 32], 'valid'.  The 8 output channels that read input channel c share its plane, so the kind belongs
    to the input channel and the variants walk over the INPUT pixels."""
    cin = PERM % 32
    kind_c = (np.arange(32) + r) % NK
    kind = kind_c[cin]
    tap = (np.arange(256) * 5 + r) % 9
    bias = _arr([KINDS[g][1] for g in kind])
    pin = np.arange(n * h * w)
    x = np.zeros((n * h * w, 32), dtype=np.float16)
    for c in range(32):
        x[:, c] = _VX[kind_c[c]][(pin + c + r) % len(_VX[kind_c[c]])]
    wt = np.zeros((256, 3, 3, 32), dtype=np.float16)
    for k in range(256):
        wt[k, tap[k] // 3, tap[k] % 3, cin[k]] = np.float16(KINDS[kind[k]][0])
    if poison:
        _poison(poison, r, bias, wt)
        xs = x.reshape(n, h, w, 32)
        xs[n // 2, h // 2, w // 2, 3] = np.float16(NAN)              # reaches the 3x3 outputs around it in that sample, nothing else
        xs[n // 2, 0, 0, 9] = np.float16(INF)
    return Launch("stem", "%dx%dx%d r%d%s" % (n, h, w, r, (" poison-all" if poison == "all" else " poison") if poison else ""), n=n, h=h, w=w, pad=0,
                  M=n * (h - 2) * (w - 2), x=x.reshape(n, h, w, 32), wt=wt, bias=bias, skip=None)


def packed_launch(S, n, r, sym, first_colour):
    """k_stem_packed: boards [n, S, S, 17] int32 as sgo_pack_dev reads them (16 stone planes of 0 / 1, plane 16 the colour to move,
    +1 or -1, alternating over the samples), w10 [256][10][16] fp16 two-hot, bias fp16, wcol float32."""
    boards = np.zeros((n, S, S, 17), dtype=np.int32)
    boards[..., :16] = np.random.RandomState(100 * S + r).random_sample((n, S, S, 16)) < 0.4
    colour = np.where((np.arange(n) % 2 == 0) == (first_colour > 0), 1, -1).astype(np.int32)
    boards[..., 16] = colour[:, None, None]
    kind = (np.arange(256) + r) % NPK
    w10 = np.zeros((256, 10, 16), dtype=np.float16)
    tap1, pl1 = (np.arange(256) * 5 + r) % 9, PERM % 16
    tap2, pl2 = (tap1 + 4) % 9, (pl1 + 7) % 16
    for k in range(256):
        s1, s2 = PKINDS[kind[k]][:2]
        w10[k, tap1[k], pl1[k]] = M.h(s1)
        w10[k, tap2[k], pl2[k]] = M.h(s2)
    bias = _arr([PKINDS[g][2] for g in kind])
    wcol = np.array([PKINDS[g][3] for g in kind], dtype=np.float64).astype(np.float32)
    assert (np.isnan(wcol) | (wcol.astype(np.float64) == np.array([PKINDS[g][3] for g in kind]))).all()
    return Launch("packed", "S%d n%d r%d sym%d colour%+d" % (S, n, r, sym, first_colour), S=S, n=n, h=S, w=S, pad=0, sym=sym,
                  M=n * (S - 2) * (S - 2), boards=boards, colour=colour, w10=w10, bias=bias, wcol=wcol, skip=None)


def packed_planes(L):
    """the 16 stone planes the kernel convolves: boards under symmetry L.sym (0: identity, 5: rotation by 180 degrees --
    transformed[i][j] = source[S-1-i][S-1-j])"""
    assert L.sym in (0, 5)
    b = L.boards[..., :16]
    return (b if L.sym == 0 else b[:, ::-1, ::-1, :]).astype(np.float16)


# ---- k_bias_act: an element-wise table, rows x C
_BA = [  # (x, bias, skip)
    (1.0, 2.0 ** -11, 2.0 ** -11),               # two ties to even: 1; one rounding would give 1 + 2^-10
    (1.0, 2.0 ** -11, -2.0 ** -11),              # (x + b) + s = 1 - 2^-11, (x + s) + b = 1
    (1.0 + E, 2.0 ** -11, 0.0), (1.0 + E, 2.0 ** -11, 2.0 ** -11),
    (-0.0, -0.0, -0.0), (0.0, -0.0, -0.0), (-1.0, 1.0, -0.0), (-1.0, 0.5, 0.25),
    (65504.0, 16.0, 0.0), (65504.0, 8.0, 8.0), (65504.0, 15.0, 0.0), (65504.0, 16.0, -INF), (65504.0, 65504.0, -65504.0),
    (2.0 ** -14, -2.0 ** -15, 0.0), (2.0 ** -14, -2.0 ** -24, 0.0), (2.0 ** -24, 2.0 ** -24, -2.0 ** -24), (3 * 2.0 ** -24, 0.0, 2.0 ** -14),
    (NAN, 1.0, 1.0), (1.0, NAN, 1.0), (1.0, 1.0, NAN), (INF, 1.0, -INF), (INF, -1.0, 1.0), (-INF, 1.0, 1.0), (1.0, INF, 1.0),
    (2048.0, 1.0, 1.0), (2048.0, 3.0, 0.0), (1024.0, 0.5, 0.0), (1024.0, 1.5, 0.0), (-3.0, 1.0, 2.0), (-3.0, 1.0, 2.0 + 2 * E),
]


def bias_act_launch(C, rows=37, with_skip=True):
    """bias is per channel: channel c has the bias of entry c (mod the table), its rows walk the entries with that bias and
    take x and skip from them"""
    x, skip, bias = np.zeros((rows, C), np.float16), np.zeros((rows, C), np.float16), np.zeros(C, np.float16)
    for c in range(C):
        b = _BA[c % len(_BA)][1]
        mine = [e for e in _BA if M.bits(M.h(e[1])) == M.bits(M.h(b))]
        bias[c] = M.h(b)
        for rw in range(rows):
            e = mine[(rw + c // len(_BA)) % len(mine)]
            x[rw, c], skip[rw, c] = M.h(e[0]), M.h(e[2])
    return Launch("bias_act", "C%d rows%d %s" % (C, rows, "skip" if with_skip else "noskip"), C=C, rows=rows, x=x, bias=bias,
                  skip=skip if with_skip else None)


# ---------------------------------------------------------------------------------------------------- the sets
@functools.lru_cache(maxsize=None)
def launches(group):
    out = []
    if group in ("tower_skip", "tower_noskip"):
        sk = group == "tower_skip"
        for r in range(NK):                                       # every channel meets every kind; two tiles, the second of 33 pixels
            out.append(tower_launch(1, 17, 17, r, sk, mixed_taps=r % 2 == 1))
        out.append(tower_launch(3, 7, 7, 1, sk, mixed_taps=True, poison=True))          # one ragged tile
        out.append(tower_launch(3, 7, 7, 2, sk, tracer=True))
        out.append(tower_launch(2, 19, 19, 3, sk, mixed_taps=True))                     # three tiles at the widest board
        out.append(tower_launch(2, 19, 19, 4, sk, mixed_taps=True, tracer=True))
        out.append(tower_launch(9, 1, 1, 4, sk, poison=True))
        out.append(tower_launch(1, 17, 17, 5, sk, mixed_taps=True, poison="all"))       # a non-finite bias or weight in every channel
        # the tower shapes of board sizes 5, 7 and 13: 28.4, 10.2 and 2.1 samples per tile, one tile and 5 / 19 / 107 pixels
        out.append(tower_launch(29, 3, 3, 6, sk, mixed_taps=True))
        out.append(tower_launch(11, 5, 5, 0, sk, tracer=True))
        out.append(tower_launch(3, 11, 11, 1, sk, mixed_taps=True, tracer=True))
    elif group == "stem":
        for r in range(NK):
            out.append(stem_launch(29, 5, 5, r) if r % 2 == 0 else stem_launch(1, 19, 19, r))
        out += [stem_launch(29, 5, 5, 1, poison=True), stem_launch(1, 19, 19, 2, poison=True), stem_launch(29, 5, 5, 3, poison="all")]
        out += [stem_launch(11, 7, 7, 4), stem_launch(5, 13, 13, 5)]                    # board sizes 7 and 13: 275 and 605 outputs
    elif group == "packed":
        for r in range(8):
            S, n = ((5, 29), (19, 1))[r % 2]
            out.append(packed_launch(S, n, r, (0, 5)[(r // 2) % 2], (1, -1)[(r // 4) % 2]))
        out += [packed_launch(19, 1, 9, 5, 1), packed_launch(19, 1, 20, 0, -1), packed_launch(5, 29, 17, 5, -1)]
        out += [packed_launch(7, 13, 3, 0, 1), packed_launch(7, 13, 12, 5, -1),         # board sizes 7 and 13, each under both symmetries
                packed_launch(13, 3, 6, 5, 1), packed_launch(13, 3, 21, 0, -1)]
    else:
        assert group == "bias_act", group
        out = [bias_act_launch(C, 37, sk) for C in (8, 256) for sk in (True, False)]
    return tuple(out)


def acc_of(L, reverse=False, fault=None, rows=None):
    if L.group == "packed":
        w = L.w10[:, :9, :].reshape(256, 3, 3, 16)
        return M.conv_acc(packed_planes(L), w, 0, reverse=reverse, fault=fault, rows=rows)
    return M.conv_acc(L.x, L.wt, L.pad, reverse=reverse, fault=fault, rows=rows)


_ACC = {}


def _acc_cached(L):
    if id(L) not in _ACC:
        _ACC[id(L)] = acc_of(L)
        assert M.exact_in_fp32(_ACC[id(L)]), L
    return _ACC[id(L)]


def colterm(L):
    if L.group != "packed":
        return None
    col = np.repeat(L.colour, (L.S - 2) ** 2).astype(np.float32)[:, None]
    with np.errstate(invalid="ignore"):
        return col * L.wcol[None, :]


def body(L, fault=None, reverse=False, want_f=False):
    """expected fp16 bits [M, K] of the launch's own rows (bias_act: [rows, C])"""
    if L.group == "bias_act":
        return M.bias_act(L.x, L.bias, L.skip, fault)
    acc = _acc_cached(L) if (not reverse and fault != "edge_multiplied") else acc_of(L, reverse, fault)
    o, f = M.epilogue(acc, L.bias, L.skip, colterm(L), fault)
    return (o, f) if want_f else o


def expected(L, fault=None, reverse=False):
    """expected bits of y's whole buffer: [Y_FRONT + M + Y_BACK, 256] for the conv kernels, [rows, C] for k_bias_act"""
    if L.group == "bias_act":
        return body(L, fault)
    buf = np.full((Y_FRONT + L.M + Y_BACK, 256), M.CANARY, dtype=np.uint16)
    buf[Y_FRONT:Y_FRONT + L.M] = body(L, fault, reverse)
    if fault == "tail_skip_unclamped" and L.group.startswith("tower") and L.M % 256:
        end = (L.M + 255) // 256 * 256
        acc = acc_of(L, rows=end)[L.M:]                           # no tap of such a row lies on the board: +0
        skip = None if L.skip is None else np.full((end - L.M, 256), np.nan, dtype=np.float16)      # what lies behind skip
        buf[Y_FRONT + L.M:Y_FRONT + end] = M.epilogue(acc, L.bias, skip)[0]
    return buf


# ---------------------------------------------------------------------------------------------------- classes
# overflow_edge and neg_zero_in are the strong members of overflow and zero_sign, covered in their own right: a finite f in
# (65504, 65520] -- just below 65520 and 65520 itself, the tie that becomes inf -- and a -0 in the bias or the skip.
CLASSES = ("tie", "near_tie", "overflow", "overflow_edge", "subnormal", "zero_sign", "neg_zero_in", "acc16", "non_finite", "add_order")
_NO_ORDER = CLASSES[:-1]        # add_order needs two addends after the accumulator: it does not exist without a skip tensor
CLASSES_OF = {"tower_skip": CLASSES, "tower_noskip": _NO_ORDER, "stem": _NO_ORDER, "packed": CLASSES}
ROUNDING_CLASSES = ("tie", "near_tie")


def classify(L):
    """{class: bool [M, K]} from the model's own values of launch L (conv groups)"""
    o, f = body(L, want_f=True)
    f64 = f.astype(np.float64)
    fin = np.isfinite(f64)
    lo, hi = M.fp16_neighbours(f64)
    a = np.abs(f64)
    pos = fin & (f64 > 0)
    off_grid = pos & (lo != hi)
    tie = off_grid & ((hi - a) == (a - lo))
    # a tie's neighbour: off the tie by at most 1/512 of the fp16 step -- with a skip that is the fp32 neighbour itself (2^-23 at
    # 1), without one the nearest a single product gets (2^-20, 2^-21): either way 2^-9 of what a tolerance test can see
    with np.errstate(invalid="ignore"):
        near = off_grid & ~tie & (np.abs(a - (lo + hi) / 2) <= (hi - lo) / 512)
    acc = _acc_cached(L)
    srcs_nonfinite = ~np.isfinite(acc) | ~np.isfinite(L.bias.astype(np.float64))[None, :]
    neg0 = np.broadcast_to((M.bits(L.bias) == 0x8000)[None, :], f.shape).copy()
    if L.skip is not None:
        srcs_nonfinite |= ~np.isfinite(L.skip.astype(np.float64))
        neg0 |= M.bits(L.skip) == 0x8000
    if L.group == "packed":
        srcs_nonfinite |= ~np.isfinite(L.wcol)[None, :]
    return {"tie": tie, "near_tie": near,
            "overflow": (fin & (f64 >= 65504.0)) | (np.isposinf(f64) & ~srcs_nonfinite),
            "overflow_edge": fin & (f64 > 65504.0) & (f64 <= 65520.0),
            "subnormal": pos & (f64 <= 2.0 ** -14),
            "zero_sign": (fin & (f64 <= 0)) | (neg0 & fin),
            "neg_zero_in": neg0 & fin,
            "acc16": ~M.same_bits(o, body(L, "acc_to_fp16_first")),
            "add_order": ~M.same_bits(o, body(L, "bias_before_skip")) if L.group in M.APPLIES["bias_before_skip"] else np.zeros(f.shape, bool),
            "non_finite": srcs_nonfinite}


def neighbourhood(L):
    """bool [M]: output pixels within the 3x3 neighbourhood of a tracer mark of launch L (tower)"""
    m = np.zeros((L.n, L.h, L.w), dtype=bool)
    for (i, yy, xx) in L.marks:
        m[i, max(0, yy - 1):yy + 2, max(0, xx - 1):xx + 2] = True
    return m.reshape(-1)
