"""After the weights of a resident net are replaced IN PLACE, every evaluation route reads the new weights -- the copies derived
from them included.

The only in-place writer is distributed.broadcast_net (the first step of dist_selfplay.run_rank and of bench.py --gpus N): it
overwrites the tensors distributed.net_tensors lists and calls net.refresh().  transplant() below is what it does to a receiving
rank.  The routes read more than those tensors: the packed stem's own form of the stem (stem_w10, stem_wcol), the k_conv4r
filter banks (_banks), the k_heads bank (_heads_bank) and NativeNet's library copy of every weight.

a. transplant(A, B) + A.refresh(): every route of A gives the bits of the same route of a B that was built fresh;
b. the negative control in the same test: before the transplant every route differs in every row, and between the transplant and
   refresh() the routes that read a derived copy still do (a test that passes without the refresh would prove nothing);
c. refresh() packs into the same buffers (captured engine rounds hold their addresses);
d. every device tensor a net object holds is either broadcast (net_tensors) or named in FusedInferenceNet.DERIVED;
e. an engine with captured rounds plays, after transplant + refresh, the game of a fresh engine on the other net.

Every comparison is torch.equal on float32 bits: no tolerance anywhere.  tests/dist_net_worker.py runs routes() on two ranks.
"""
import numpy as np
import pytest

from tests.test_gpu_baseline_nets import _playout_records

pytestmark = pytest.mark.gpu

# the smallest shapes on which the packed stem, k_conv4r, k_heads and NativeNet all exist, with two heads-bank geometries
# (K = 2 * t * t padded 18 -> 32 at 5x5, 98 -> 128 at 9x9)
CASES = [(5, 1), (9, 2)]
IDS = ["5x5_1block", "9x9_2block"]
N_DENSE, N_LIST, SYMS = 48, 17, (0, 5)
# routes that read a copy refresh() has to rewrite: _banks, _heads_bank, the library's own weights
NEED_REFRESH = ("packed+tower", "packed+heads", "native", "native+tower")


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


class Rows(object):
    """48 packed records (16 each after 0, S*S/4 and S*S/2 plies) and the four evaluations every route runs on them: all 48 in
    record order and 17 through a shuffled index list, under symmetry 0 and 5; for the tensor route the channel-padded fp16
    tensor of the same rows (k_nn_pack layout 2).  Built once per board size, never written afterwards."""

    def __init__(self, L, S, seed=4100):
        import torch
        lib = L.load()
        self.S = S
        self.recs = torch.cat([_playout_records(L, S, N_DENSE // 3, ply, seed=seed + ply) for ply in (0, S * S // 4, S * S // 2)])
        assert self.recs.shape == (N_DENSE, lib.sgo_packed_words(S)) and self.recs.is_contiguous()
        g = torch.Generator().manual_seed(seed)
        self.idx = torch.randperm(N_DENSE, generator=g)[:N_LIST].to(torch.int32).cuda()
        self.calls = [(n, idx, k) for k in SYMS for (n, idx) in ((N_DENSE, None), (N_LIST, self.idx))]
        self.n_rows = sum(c[0] for c in self.calls)
        self.x = []
        for n, idx, k in self.calls:
            x = torch.zeros((n, S, S, 32), dtype=torch.float16, device="cuda")
            L.check(lib.sgo_nn_pack_dev(S, n, L.ptr(self.recs), None if idx is None else L.ptr(idx), k, 2, 0, L.ptr(x), L.stream_ptr()))
            self.x.append(x)
        torch.cuda.synchronize()


_ROWS = {}


def rows_for(L, S):
    if S not in _ROWS:
        _ROWS[S] = Rows(L, S)
    return _ROWS[S]


def transplant(dst, src):
    """What broadcast_net does to a receiving rank: the listed tensors are overwritten in place, nothing else is touched."""
    from sejonggo_amd.distributed import net_tensors
    a, b = net_tensors(dst), net_tensors(src)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x.copy_(y)


def _evaluate(net, rows, tensor_route):
    import torch
    ps, vs = [], []
    for (n, idx, k), x in zip(rows.calls, rows.x):
        if tensor_route:
            p, v = net.predict_on_batch(x)
        else:
            p, v = net.predict_packed(rows.recs.data_ptr(), None if idx is None else idx.data_ptr(), n, k)
        assert p.shape == (n, net.A) and p.dtype == torch.float32 and v.dtype == torch.float32
        ps.append(p)
        vs.append(v.reshape(n, 1))
    torch.cuda.synchronize()
    return torch.cat(ps), torch.cat(vs)


def routes(net, rows):
    """(name, policy [130, A] f32, value [130, 1] f32) of every evaluation route of `net` on the rows.  The net's route switches
    are left as they were found."""
    from sejonggo_amd.net import NativeNet
    was = (net.packed_tower, net.fused_heads)
    try:
        if isinstance(net, NativeNet):
            # the library's net, through its slice loop where max_batch < 48
            for name, tower in (("native", False), ("native+tower", True)):
                assert net.use_packed_tower(tower) == tower
                yield (name,) + _evaluate(net, rows, False)
            return
        for name, tensor, tower, heads in (("tensor", True, False, False), ("packed", False, False, False),
                                           ("packed+tower", False, True, False), ("packed+heads", False, False, True),
                                           ("packed+both", False, True, True)):
            assert net.use_packed_tower(tower) == tower and net.use_fused_heads(heads) == heads
            yield (name,) + _evaluate(net, rows, tensor)
    finally:
        net.use_packed_tower(was[0])
        net.use_fused_heads(was[1])


def outputs(net, rows):
    return {name: (p, v) for name, p, v in routes(net, rows)}


def rows_that_differ(a, b):
    """How many rows of two route outputs differ in any bit of policy or value."""
    return int(((a[0] != b[0]).any(dim=1) | (a[1] != b[1]).any(dim=1)).sum().item())


def same_bits(a, b):
    import torch
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def make_net(S, blocks, seed, native):
    """A resident net of the given seed with every optional route switched on (all banks exist)."""
    from sejonggo_amd.net import NativeNet, build_fused_net
    fnet, module = build_fused_net(S, blocks, seed=seed)
    net = NativeNet(module, max_batch=16) if native else fnet
    assert net.use_packed_tower(True) and net.use_fused_heads(True)
    assert len(net._banks) == 2 * blocks and net._heads_bank is not None
    return net


def bank_addresses(net):
    return sorted(b.data_ptr() for b in net._banks.values()) + [net._heads_bank.data_ptr()]


# ------------------------------------------------------------------------------------------- a, b, c: transplant equals fresh
@pytest.mark.parametrize("native", [False, True], ids=["fused", "native"])
@pytest.mark.parametrize("S,blocks", CASES, ids=IDS)
def test_transplant_then_refresh_equals_a_fresh_net(L, S, blocks, native):
    rows = rows_for(L, S)
    A, B = make_net(S, blocks, 1, native), make_net(S, blocks, 2, native)
    want = outputs(B, rows)
    assert set(want) == ({"native", "native+tower"} if native else {"tensor", "packed", "packed+tower", "packed+heads", "packed+both"})
    all_rows = rows.n_rows
    assert all_rows == 2 * (N_DENSE + N_LIST) == want[next(iter(want))][0].shape[0]

    # two seeds: two different nets, on every route and in every row
    bad = []
    for name, out in outputs(A, rows).items():
        d = rows_that_differ(out, want[name])
        if d != all_rows:
            bad.append("before the transplant %s differs from the other net in %d of %d rows only" % (name, d, all_rows))
    assert not bad, "\n".join(bad)

    banks = bank_addresses(A)
    transplant(A, B)
    # b. between the transplant and refresh(): a route that reads only the listed tensors is B's already; one that reads a derived
    # copy is still not B's in any row (the tower, the heads or all of the library's net are the old model's)
    for name, out in outputs(A, rows).items():
        d = rows_that_differ(out, want[name])
        if name in NEED_REFRESH:
            if d != all_rows:
                bad.append("without refresh() %s already agrees with the other net in %d of %d rows: the control proves nothing"
                           % (name, all_rows - d, all_rows))
        elif name != "packed+both" and d:
            bad.append("%s reads only the listed tensors, yet differs in %d of %d rows after the transplant" % (name, d, all_rows))
    assert not bad, "\n".join(bad)

    A.refresh()
    # a. every route of A gives the bits of the same route of B
    for name, out in outputs(A, rows).items():
        if not same_bits(out, want[name]):
            bad.append("after transplant + refresh() %s differs in %d of %d rows" % (name, rows_that_differ(out, want[name]), all_rows))
    assert not bad, "\n".join(bad)
    # c. into the same buffers
    assert bank_addresses(A) == banks
    # and B itself was only read
    assert all(same_bits(out, want[name]) for name, out in outputs(B, rows).items())
    if native:
        A.close()
        B.close()


@pytest.mark.parametrize("native", [False, True], ids=["fused", "native"])
def test_refresh_keeps_every_bank_where_it_is(L, native):
    """c. on its own, the addresses by layer: captured engine rounds hold them."""
    net = make_net(9, 2, 3, native)
    by_layer = dict((w, b.data_ptr()) for w, b in net._banks.items())
    heads = net._heads_bank.data_ptr()
    weights = [t.data_ptr() for blk in net.blocks for t in blk]
    for _ in range(2):
        net.refresh()
    assert dict((w, b.data_ptr()) for w, b in net._banks.items()) == by_layer and net._heads_bank.data_ptr() == heads
    assert [t.data_ptr() for blk in net.blocks for t in blk] == weights
    # a net without banks gets none from refresh()
    from sejonggo_amd.net import build_fused_net
    plain = build_fused_net(5, 1, seed=3)[0]
    plain.refresh()
    assert plain._banks == {} and plain._heads_bank is None and not plain.packed_tower and not plain.fused_heads
    if native:
        net.close()


# ------------------------------------------------------------------------------------------- d. nothing read is forgotten
def _tensors_in(value):
    import torch
    if torch.is_tensor(value):
        yield value
    elif isinstance(value, (list, tuple)):
        for x in value:
            for t in _tensors_in(x):
                yield t
    elif isinstance(value, dict):
        for x in value.values():
            for t in _tensors_in(x):
                yield t


@pytest.mark.parametrize("native", [False, True], ids=["fused", "native"])
def test_every_device_tensor_is_broadcast_or_derived(L, native):
    """A device tensor of the net object that is neither in net_tensors (so: broadcast and checksummed) nor under an attribute
    named in DERIVED (so: rewritten by refresh()) is state a weight change leaves stale -- how stem_w10 slipped through."""
    from sejonggo_amd.distributed import net_tensors
    from sejonggo_amd.net import FusedInferenceNet
    net = make_net(9, 2, 4, native)
    rows = rows_for(L, 9)
    outputs(net, rows)                                   # whatever a route creates lazily exists now
    listed = set(t.data_ptr() for t in net_tensors(net))
    derived = getattr(FusedInferenceNet, "DERIVED", ())   # without the attribute every bank is reported below, by name
    seen = {}
    for attr, value in vars(net).items():
        for t in _tensors_in(value):
            if t.is_cuda:
                seen.setdefault(attr, []).append(t)
    forgotten = [attr for attr, ts in seen.items() if attr not in derived and any(t.data_ptr() not in listed for t in ts)]
    assert not forgotten, "device tensors neither broadcast nor derived: %s" % ", ".join(sorted(forgotten))
    assert FusedInferenceNet.DERIVED == ("_banks", "_heads_bank")
    for attr in FusedInferenceNet.DERIVED:
        assert seen.get(attr), "%s holds no device tensor: DERIVED names nothing" % attr
    # and the other way round: everything listed is an attribute of the object (nothing is broadcast into a temporary)
    held = set(t.data_ptr() for ts in seen.values() for t in ts)
    assert listed <= held
    assert len(listed) == len(net_tensors(net)) == 4 + 4 * 2 + 8          # stem (two forms), two blocks, heads: no tensor twice
    if native:
        net.close()


# ------------------------------------------------------------------------------------------- e. captured rounds
G_E, SIMS_E, E_E, NM_E, K_E = 4, 16, 4, 6, 3


def engine_for(net, S, graph, num_moves=NM_E):
    """The engine of test_gpu_native_net.py section 5, at any board size."""
    from sejonggo_amd.engine import SelfPlayEngine
    return SelfPlayEngine(net, size=S, n_games=G_E, sims=SIMS_E, energy=E_E, stop_exploration=3, num_moves=num_moves, komi=5.5,
                          symmetry=K_E, graph=graph)


def play(eng, S, num_moves=NM_E):
    """Steps an engine through one set of games on fixed noise and uniforms; per step the tree bytes of every slot, at the end
    the move records per slot."""
    rng = np.random.RandomState(21)
    noises, uni = rng.dirichlet([0.03] * (S * S + 1), size=G_E), rng.random_sample((G_E, num_moves))
    eng.start_games(np.arange(G_E), noises=noises, uniforms=uni)
    trees = []
    while True:
        st = eng.step()
        eng.drain()
        trees.append(tuple(eng.tree_serialize(s)[0].tobytes() for s in range(G_E)))
        if st.n_active == 0:
            break
        assert len(trees) < 400
    moves = {s: [(m["action"], m["player"], np.float32(m["value"]).tobytes(), m["policy"].tobytes(), m["packed"].tobytes())
                 for m in eng.records[s]] for s in range(G_E)}
    return trees, moves


def test_captured_rounds_survive_a_weight_change(L):
    S, blocks = 9, 2
    net, other = make_net(S, blocks, 1, False), make_net(S, blocks, 2, False)
    eng = engine_for(net, S, True)
    assert eng.packed and eng.graph
    first_trees, first_moves = play(eng, S)
    replays, graphs = eng.n_graph_replays, dict(eng._graphs)
    assert replays > 0 and graphs
    transplant(net, other)
    net.refresh()
    trees, moves = play(eng, S)
    # the rounds captured for the first games were replayed, not captured again
    assert eng.n_graph_replays > replays
    assert set(eng._graphs) == set(graphs) and all(eng._graphs[nb] is g for nb, g in graphs.items())
    fresh = engine_for(other, S, True)
    want_trees, want_moves = play(fresh, S)
    assert fresh.n_graph_replays > 0
    assert all(len(want_moves[s]) == NM_E for s in range(G_E))
    assert len(trees) == len(want_trees)
    for i, (x, y) in enumerate(zip(trees, want_trees)):
        assert x == y, "trees differ after step %d" % i
    assert moves == want_moves
    assert moves != first_moves and trees != first_trees
    eng.close()
    fresh.close()
