"""GPU: the game-records kernels (include/sgo.h "game records", csrc/sgo_records.hip) and records.RecordSet on top of them.

k_records_replay against the reference's five 19x19 records ply by ply (tests/golden/sgf_S19.npz) and, word for word over the
WHOLE record and legal arrays, against the model (tests/records_model.py) on constructed sets at 5, 7, 9 and 13;
k_records_score against the model bit for bit; RecordSet.score and write_samples end to end with stub nets."""
import os

import numpy as np
import pytest

from tests import records_model as M
from tests.helpers import GOLDEN, load, read_sample, sha8, unpack_mask

pytestmark = pytest.mark.gpu

SGO_ERR_ARG, SGO_ERR_OCCUPIED, SGO_ERR_RANGE = -1, -101, -102


def _device(S, max_games, max_entries):
    from sejonggo_amd.records import DeviceRecords
    return DeviceRecords(S, max_games, max_entries)


def _arrays(be):
    """(records uint32 [cap, RW], legal uint32 [cap, NW]) as they are on the device now"""
    return be.records.cpu().numpy().view(np.uint32), be.legal.cpu().numpy().view(np.uint32)


def _fill(be, seed):
    """a random pattern in every word of both arrays; returns it"""
    import torch
    rng = np.random.RandomState(seed)
    pr = rng.randint(0, 1 << 32, size=tuple(be.records.shape), dtype=np.uint64).astype(np.uint32)
    pl = rng.randint(0, 1 << 32, size=tuple(be.legal.shape), dtype=np.uint64).astype(np.uint32)
    be.records.copy_(torch.from_numpy(pr.view(np.int32)))
    be.legal.copy_(torch.from_numpy(pl.view(np.int32)))
    torch.cuda.synchronize()
    return pr, pl


def _check_set(be, S, games, seed):
    """replays `games` over a random pattern and compares both WHOLE arrays, status and fail_at with the model"""
    pr, pl = _fill(be, seed)
    n, off, acts, cols = M.lists_of(games)
    status, fail_at = be.replay(n, off, acts, cols)
    want = M.replay(S, games)
    assert status.tolist() == want["status"].tolist() and fail_at.tolist() == want["fail_at"].tolist()
    R = len(want["written"])
    exp_r, exp_l = pr.copy(), pl.copy()
    exp_r[:R][want["written"]] = want["records"][want["written"]]
    exp_l[:R][want["written"]] = want["legal"][want["written"]]
    got_r, got_l = _arrays(be)
    bad = np.flatnonzero((got_r != exp_r).any(axis=1))
    assert len(bad) == 0, ("records differ", bad[:8], R)
    bad = np.flatnonzero((got_l != exp_l).any(axis=1))
    assert len(bad) == 0, ("legal words differ", bad[:8], R)
    return want, got_r, got_l


# ------------------------------------------------------------------------------------------------ the reference's records
def _golden_games(z, S):
    out = []
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        acts = [S * S if y >= S else int(y) * S + int(x) for x, y, _ in mv]
        out.append((acts, [int(c) for _, _, c in mv]))
    return out


def test_five_golden_records_in_one_call():
    """About 1 650 positions: 310-351 plies per game, an odd game count, unequal lengths in the two halves of a wave.  After
    sgo_unpack_dev every record's board hash and legal mask equal the reference's at every ply."""
    z = load("sgf_S19.npz")
    S = int(z["size"])
    A = S * S + 1
    games = _golden_games(z, S)
    total = sum(len(a) for a, _ in games)
    be = _device(S, 5, total)
    try:
        n, off, acts, cols = M.lists_of(games)
        status, fail_at = be.replay(n, off, acts, cols)
        assert not status.any() and (fail_at == -1).all()
        boards = be.boards(np.arange(total + 5))
        legal = be.legal.cpu().numpy().view(np.uint32)
        bits = np.unpackbits(legal.view(np.uint8), axis=1, bitorder="little")[:, :A]
        for g in range(5):
            base = int(off[g]) + g
            hashes, masks = z["g%02d_hashes" % g], z["g%02d_masks" % g]
            assert len(hashes) == n[g] + 1
            for k in range(n[g] + 1):
                assert np.array_equal(sha8(boards[base + k:base + k + 1]), hashes[k]), (g, k)
                # the golden holds play.legal_moves' vector, which flags the ILLEGAL points
                assert np.array_equal(bits[base + k], 1 - unpack_mask(masks[k], A)), (g, k)
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------ constructed sets
@pytest.mark.parametrize("S", [5, 7, 9, 13])
def test_constructed_sets_word_for_word(S):
    """1, 2, 3 and 65 games; lengths 0, 1, 7, 8, 9 and the maximum; a zero-length game beside a long one and the reverse; passes,
    a capture, a ko recapture that the legal set refuses, a suicide, handicap and white set-up stones, one colour twice; refusals
    at entry 0, in the middle and at the last entry in either half of a wave; positions of rule_shapes_S*.npz as prefixes."""
    N = S * S
    G = M.constructed_games(S)
    shapes = M.shape_prefix_games(S)
    assert len(shapes) >= 2
    be = _device(S, 65, 4 * N + 64 * 3 * N)
    try:
        _check_set(be, S, [G["one"]], 1)
        _check_set(be, S, [G["empty"]], 2)
        _check_set(be, S, [G["empty"], G["long"]], 3)
        _check_set(be, S, [G["long"], G["empty"]], 4)
        _check_set(be, S, [G["seven"], G["eight"], G["nine"]], 5)
        _check_set(be, S, [G["max_length"]], 6)
        # the ko recapture is refused by the legal set of the record before it, and played all the same
        want, _, got_l = _check_set(be, S, [G["ko_retake"], G["passes"]], 7)
        t = G["ko_retake"][0][-1]
        assert not (got_l[len(G["ko_retake"][0]) - 1][t >> 5] >> np.uint32(t & 31)) & 1
        assert want["status"][0] == 0
        # a refusal in either half: the partner equals its run beside the same list with the refused entry made a pass
        for name in ("refuse_first", "refuse_middle", "refuse_last", "refuse_negative"):
            acts, cols = G[name]
            for order in (0, 1):
                pair = [(acts, cols), G["long"]] if order == 0 else [G["long"], (acts, cols)]
                want, got_r, got_l = _check_set(be, S, pair, 8)
                j = int(want["fail_at"][order])
                assert want["status"][order] in (SGO_ERR_OCCUPIED, SGO_ERR_RANGE) and want["status"][1 - order] == 0
                fixed = list(acts)
                fixed[j] = N
                pair2 = [(fixed, cols), G["long"]] if order == 0 else [G["long"], (fixed, cols)]
                _, ok_r, ok_l = _check_set(be, S, pair2, 8)
                lo = 0 if order == 1 else len(acts) + 1
                hi = lo + len(G["long"][0]) + 1
                assert np.array_equal(got_r[lo:hi], ok_r[lo:hi]) and np.array_equal(got_l[lo:hi], ok_l[lo:hi])
        # 65 games: everything at once, an odd count, refusals on even and on odd places
        names = [k for k in sorted(G) if k != "max_length"]
        many = [G[names[i % len(names)]] for i in range(40)] + [g for _, g in shapes]
        many += [G["refuse_middle"], G["capture"], G["suicide"], G["refuse_last"], G["refuse_first"]]
        while len(many) < 65:
            many.append(G[names[(3 * len(many)) % len(names)]])
        assert len(many) == 65
        want, _, _ = _check_set(be, S, many, 9)
        refused = np.flatnonzero(want["status"])
        assert (refused % 2 == 0).any() and (refused % 2 == 1).any()
    finally:
        be.close()


def test_bad_arguments_run_nothing():
    from sejonggo_amd import _lib
    S = 5
    N = S * S
    be = _device(S, 4, 60)
    try:
        pr, pl = _fill(be, 21)

        def call(n_entries, off, acts):
            n_entries, off = np.asarray(n_entries, np.int32), np.asarray(off, np.int32)
            acts = np.asarray(acts, np.int32)
            cols = np.zeros(len(acts), np.int32)
            status, fail_at = np.full(len(n_entries), 77, np.int32), np.full(len(n_entries), 77, np.int32)
            rc = be.lib.sgo_records_replay(be.h, len(n_entries), _lib.ptr(n_entries), _lib.ptr(off), _lib.ptr(acts), _lib.ptr(cols),
                                           _lib.ptr(status), _lib.ptr(fail_at), _lib.stream_ptr())
            return rc, status, fail_at

        cases = [([-1], [0], [0]),                                   # a negative length
                 ([4 * N + 1], [0], [N] * (4 * N + 1)),              # longer than SGO_SETUP_MAX_MOVES
                 ([1] * 5, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]),        # more games than max_games
                 ([30, 31], [0, 30], [N] * 61),                      # more entries than max_entries
                 ([2, 2], [0, 3], [0, 1, 2, 3, 4])]                  # lists that are not back to back
        for n_entries, off, acts in cases:
            rc, status, fail_at = call(n_entries, off, acts)
            assert rc == SGO_ERR_ARG, (n_entries, rc)
            assert (status == 77).all() and (fail_at == 77).all()
            got_r, got_l = _arrays(be)
            assert np.array_equal(got_r, pr) and np.array_equal(got_l, pl)
        rc, status, fail_at = call([60], [0], [N] * 60)              # the capacity itself is served
        assert rc == 0 and status.tolist() == [0]
        assert be.lib.sgo_records_replay(be.h, 0, None, None, None, None, None, None, _lib.stream_ptr()) == 0
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------ the score kernel
SPECIALS = np.array([np.nan, 0.0, -0.0, -0.25, -1.0, np.inf, 1e-45, 3e-39, 0.125, 0.25, 0.5], dtype=np.float32)


def _score_case(S, seed, n, n_buckets, one_bucket=None):
    """(game list, rows) for the score tests: an asymmetric position sequence with a capture, and n rows over its records with
    policies drawn from a few values (ties on both sides of the target) and the special floats."""
    N, A = S * S, S * S + 1
    rng = np.random.RandomState(seed)
    G = M.constructed_games(S)
    games = [G["ko_retake"], G["long"], G["handicap"]]
    R = sum(len(a) for a, _ in games) + len(games)
    index = rng.randint(0, R, size=n).astype(np.int32)
    target = rng.randint(0, A, size=n).astype(np.int32)
    target[rng.rand(n) < 0.15] = N                                    # the pass as target
    policy = rng.choice(np.array([0.0625, 0.125, 0.25], np.float32), size=(n, A)).astype(np.float32)
    mode = rng.randint(0, 6, size=n)
    for i in range(n):
        if mode[i] == 0:                                              # the special floats all over the row
            policy[i] = rng.choice(SPECIALS, size=A)
        elif mode[i] == 1:                                            # the target first
            policy[i, :] = rng.choice(np.array([0.0625, 0.125], np.float32), size=A)
        elif mode[i] == 2:                                            # the target last: everything else above it
            policy[i, :] = rng.choice(np.array([0.5, 0.75], np.float32), size=A)
        elif mode[i] == 3:                                            # full-mantissa values, no ties
            policy[i] = rng.random_sample(A).astype(np.float32)
    value = rng.choice(np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, np.nan, 1e-45, -1e-45], np.float32), size=n)
    z = rng.randint(-1, 2, size=n).astype(np.int32)
    bucket = rng.randint(0, n_buckets, size=n).astype(np.int32) if one_bucket is None else np.full(n, one_bucket, np.int32)
    if one_bucket is None and n >= 2:
        bucket[0], bucket[-1] = 0, n_buckets - 1
    return games, index, target, z, bucket, policy, value


def _run_score(be, S, index, target, z, bucket, n_buckets, policy_k, value, k):
    import torch
    n = len(index)
    dev = be.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    d_rank, d_best = torch.full((n,), 99, dtype=torch.int32, device=dev), torch.full((n,), 99, dtype=torch.int32, device=dev)
    d_pt, d_flags = torch.full((n,), 9.0, dtype=torch.float32, device=dev), torch.full((n,), 99, dtype=torch.int32, device=dev)
    counters = torch.zeros((n_buckets, 8), dtype=torch.int64, device=dev)
    be.score(n, t(index), t(target), t(z), t(bucket), n_buckets, t(policy_k), t(value), k, d_rank, d_best, d_pt, d_flags, counters)
    torch.cuda.synchronize()
    return {"rank": d_rank.cpu().numpy(), "best": d_best.cpu().numpy(), "p_target": d_pt.cpu().numpy(),
            "flags": d_flags.cpu().numpy(), "counters": counters.cpu().numpy()}


def _same_score(got, want):
    for key in ("rank", "best", "flags"):
        assert np.array_equal(got[key], want[key]), (key, np.flatnonzero(got[key] != want[key])[:8])
    assert np.array_equal(got["p_target"].view(np.uint32), want["p_target"].view(np.uint32))
    assert np.array_equal(got["counters"], want["counters"])


@pytest.fixture(scope="module")
def score_env():
    S = 5
    games = _score_case(S, 0, 1, 1)[0]
    be = _device(S, 4, sum(len(a) for a, _ in games))
    n, off, acts, cols = M.lists_of(games)
    status, _ = be.replay(n, off, acts, cols)
    assert not status.any()
    legal = be.legal.cpu().numpy().view(np.uint32).copy()
    assert np.array_equal(legal[:len(M.replay(S, games)["legal"])], M.replay(S, games)["legal"])
    yield S, be, legal
    be.close()


@pytest.mark.parametrize("n,k", [(1, 0), (2, 3), (3, 5), (300, 0), (300, 1), (300, 2), (300, 3), (300, 4), (300, 5), (300, 6), (300, 7)])
def test_score_rows_bit_for_bit(score_env, n, k):
    """ranks, best, flags, counters and the raw bits of p_target against the model: the target first, last and in the middle, ties
    at its value on both sides, illegal targets (occupied points included), the pass, NaN / +-0 / negatives / +inf / denormals,
    z = 0 rows, values of exactly 0, bucket ids at both ends, all eight symmetries on asymmetric positions."""
    S, be, legal = score_env
    NB = 7
    _, index, target, z, bucket, policy, value = _score_case(S, 100 + n + k, n, NB)
    got = _run_score(be, S, index, target, z, bucket, NB, policy, value, k)
    want = M.score(S, legal, index, target, z, bucket, NB, policy, value, k)
    _same_score(got, want)
    if n == 300:
        assert (want["flags"] == 0).any() and (want["rank"] == 0).any() and want["counters"][:, 3].sum() > 0


def test_score_4096_rows_into_one_bucket(score_env):
    S, be, legal = score_env
    _, index, target, z, bucket, policy, value = _score_case(S, 7, 4096, 3, one_bucket=2)
    got = _run_score(be, S, index, target, z, bucket, 3, policy, value, 6)
    want = M.score(S, legal, index, target, z, bucket, 3, policy, value, 6)
    _same_score(got, want)
    assert got["counters"][2, 0] == 4096 and not got["counters"][:2].any()


def test_score_skips_rows_out_of_range_and_n_zero(score_env):
    S, be, legal = score_env
    A = S * S + 1
    _, index, target, z, bucket, policy, value = _score_case(S, 8, 6, 2)
    index[1], target[2], bucket[3], target[4] = len(legal), A, 2, -1
    got = _run_score(be, S, index, target, z, bucket, 2, policy, value, 0)
    want = M.score(S, legal, index, target, z, bucket, 2, policy, value, 0)
    _same_score(got, want)
    assert got["flags"][1:5].tolist() == [2, 2, 2, 2] and got["counters"][:, 0].sum() == 2
    from sejonggo_amd import _lib
    assert be.lib.sgo_records_score_dev(be.h, 0, *([None] * 4), 1, None, None, 0, *([None] * 5), _lib.stream_ptr()) == 0
    assert be.lib.sgo_records_score_dev(be.h, 1, *([None] * 4), 1, None, None, 8, *([None] * 5), _lib.stream_ptr()) == SGO_ERR_ARG


# ------------------------------------------------------------------------------------------------ end to end
def _golden_record(z, gi, S, winner):
    from sejonggo_amd.records import Record
    mv = z["g%02d_moves" % gi]
    entries = [(S * S if y >= S else int(y) * S + int(x), int(c)) for x, y, c in mv]
    return Record("golden%d" % gi, S, entries, [False] * len(entries), list(range(1, len(entries) + 1)), winner)


@pytest.mark.parametrize("kind,symmetry", [("hash", "identity"), ("table", 3)])
def test_record_set_score_end_to_end(kind, symmetry):
    """RecordSet.score with a stub net on tests/golden/review_S19.sgf and two of the golden records: buckets and totals equal the
    model's, fed with the policy and value arrays fetched from the device; the float64 sums with ==."""
    from sejonggo_amd import records as R
    from sejonggo_amd.stub_nets import make_stub
    z = load("sgf_S19.npz")
    S = 19
    with open(os.path.join(GOLDEN, "review_S19.sgf")) as f:
        recs = [R.parse_record(f.read(), "review")]
    recs += [_golden_record(z, 0, S, 1), _golden_record(z, 2, S, None)]
    rs = R.RecordSet(recs, S)
    try:
        res = rs.score(make_stub(kind, S), batch=256, symmetry=symmetry, bucket=20, keep_policy=True)
        rows = res["rows"]
        n = len(rows["action"])
        assert n == sum(1 for r in recs for s in r.setup if not s) and not rs.refused
        legal = rs.backend.legal.cpu().numpy().view(np.uint32)
        NB = len(res["buckets"])
        k = 0 if symmetry == "identity" else symmetry
        want = M.score(S, legal, rows["index"], rows["action"], rows["z"], rows["bucket"], NB, rows["policy"], rows["value"], k)
        got = {key: rows[key] for key in ("rank", "best", "flags", "p_target")}
        got["counters"] = np.array([[d[c] for c in R.COUNTERS] + [0, 0] for d in res["buckets"]], np.int64)
        _same_score(got, want)
        ce, se = M.float_sums(rows["p_target"], rows["value"], rows["z"], rows["bucket"], NB)
        assert [d["ce_sum"] for d in res["buckets"]] == ce.tolist() and [d["se_sum"] for d in res["buckets"]] == se.tolist()
        tot = res["total"]
        assert tot["rows"] == n and tot["top1"] == int((want["rank"] == 0).sum()) and tot["top5"] == int((want["rank"] < 5).sum())
        assert tot["value_rows"] == int((rows["z"] != 0).sum()) and tot["illegal"] == int((want["flags"] == 0).sum())
        assert (rows["z"][rows["game"] == 2] == 0).all() and (rows["z"][rows["game"] == 1] != 0).all()
        t_ce = 0.0
        for b in range(NB):
            t_ce += float(ce[b])
        assert tot["ce_sum"] == t_ce and tot["cross_entropy"] == t_ce / n
    finally:
        rs.close()


def test_write_samples_of_a_short_record(tmp_path):
    """boards equal the oracle's replay, one-hot policy targets (the pass last), value targets +1 for the winner's moves"""
    from oracle import oracle
    from sejonggo_amd import records as R
    S = 5
    N = S * S
    text = "(;FF[4]SZ[5]RE[W+3.5]AB[bb]AW[dd];B[cc];W[];B[ab];W[cb])"
    rec = R.parse_record(text, "short")
    rs = R.RecordSet([rec], S)
    try:
        out = rs.write_samples(str(tmp_path))
        assert out["games"] == 1 and out["samples"] == 4 and not out["existing"]
        board, _ = oracle.game_init(S)
        oracle.make_play(1, 1, board, 1)
        oracle.make_play(3, 3, board, -1)
        for node, (a, colour) in zip((1, 2, 3, 4), ((2 * S + 2, 1), (N, -1), (1 * S + 0, 1), (1 * S + 2, -1))):
            b, p, v = read_sample(str(tmp_path / "KGS" / "short" / ("move_%03d" % node) / "sample.h5"))
            assert b.shape == (1, S, S, 17) and b.dtype == np.float32 and np.array_equal(b, board.astype(np.float32)), node
            assert p.shape == (N + 1,) and p[a] == 1.0 and p.sum() == 1.0
            assert float(v) == (1.0 if colour == -1 else -1.0)
            oracle.make_play(a % S if a < N else 0, a // S if a < N else S, board, colour)
        again = rs.write_samples(str(tmp_path))
        assert again["existing"] == ["short"] and again["samples"] == 0
    finally:
        rs.close()
