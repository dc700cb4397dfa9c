"""The net as an object of libsgo_hip.so (sgo_net_*, net.NativeNet).

4. composition is bit-exact: NativeNet.predict_packed == sgo_heads_dev on the tower output computed through FusedInferenceNet's
   own sgo_stem_packed_dev + _conv calls, with an index list and a device-side symmetry word, through the slice loop
   (max_batch = 16), on the packed tower route, and again after a weight change + refresh();
5. the engine on it: SelfPlayEngine(NativeNet) and SelfPlayEngine(FusedInferenceNet with fused heads) play identical games
   (moves, values, policy targets, tree bytes after every step), eagerly and with captured rounds, and a ctypes-only loop
   (sgo_eval_list -> sgo_net_predict_packed_dev -> sgo_step) on a net filled from HOST arrays reproduces the same game;
6. arguments.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_heads import tower_output

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from sejonggo_amd import _lib
    _lib.require_gpu()
    return _lib


def _seeded_module(S, blocks, seed=5):
    from sejonggo_amd.net import build_fused_net
    return build_fused_net(S, blocks, seed=seed)[1]


def _expected(L, nn, recs, idx, n, kdev):
    """sgo_heads_dev on the tower output of FusedInferenceNet's own calls (nn is a NativeNet, hence a FusedInferenceNet)."""
    y = tower_output(L, nn, recs.data_ptr(), idx.data_ptr(), n, 0, kdev.data_ptr())
    assert nn.use_fused_heads(True)
    return nn._heads_kernel(y)


# ---------------------------------------------------------------------------------------------------------- 4. composition
@pytest.mark.parametrize("S,blocks,ply", [(19, 2, 120), (9, 4, 30), (5, 4, 8), (7, 4, 16), (13, 4, 60)],
                         ids=["19x19_2block", "9x9_4block", "5x5_4block", "7x7_4block", "13x13_4block"])
def test_composition_is_bit_exact(L, S, blocks, ply):
    import torch
    from sejonggo_amd.net import NativeNet
    from tests.test_gpu_baseline_nets import _playout_records
    module = _seeded_module(S, blocks)
    big, small = NativeNet(module, max_batch=4096), NativeNet(module, max_batch=16)
    recs = _playout_records(L, S, 64, ply, seed=77 + S)
    g = torch.Generator().manual_seed(S)
    kdev = torch.tensor([6], dtype=torch.int32, device="cuda")            # overrides the sym_k argument (0) when the kernels run

    def check(what):
        outs = []
        for n in (1, 37, 64):
            idx = torch.randperm(64, generator=g)[:n].to(torch.int32).cuda()
            want_p, want_v = _expected(L, big, recs, idx, n, kdev)
            for nn in (big, small):
                p, v = nn.predict_packed(recs.data_ptr(), idx.data_ptr(), n, 0, kdev.data_ptr())
                assert p.shape == (n, S * S + 1) and v.shape == (n, 1) and p.dtype == v.dtype == torch.float32
                assert torch.equal(p, want_p) and torch.equal(v, want_v), (what, n, nn.max_batch)
            outs.append(want_p.clone())
        # without an index list the slices start at their own records
        want_p, want_v = _expected(L, big, recs, torch.arange(64, dtype=torch.int32, device="cuda"), 64, kdev)
        p, v = small.predict_packed(recs.data_ptr(), None, 64, 0, kdev.data_ptr())
        assert torch.equal(p, want_p) and torch.equal(v, want_v), what
        # and the symmetry word is honoured: another k gives other bits
        p0, _ = big.predict_packed(recs.data_ptr(), None, 64, 0, None)
        assert not torch.equal(p0, want_p)
        return outs

    before = check("initial")
    # the k_conv4r route of the library's net: same bits
    assert big.use_packed_tower(True)
    check("packed tower")
    big.use_packed_tower(False)
    # a weight change reaches the library's copy through refresh() only
    for nn in (big, small):
        nn.p_fc_w[3:40, 5:60] *= -1.5
        nn.blocks[0][0][7:90, :, 1, :] *= 0.5
    stale, _ = big.predict_packed(recs.data_ptr(), None, 64, 0, kdev.data_ptr())
    for nn in (big, small):
        nn.refresh()
    g.manual_seed(S)
    after = check("refreshed")
    assert not any(torch.equal(a, b) for a, b in zip(before, after))
    fresh, _ = big.predict_packed(recs.data_ptr(), None, 64, 0, kdev.data_ptr())
    assert not torch.equal(stale, fresh)
    assert big.packed_ok and big.name == module.name and big.flops_per_eval() == module.flops_per_eval()
    big.close()
    small.close()


# ---------------------------------------------------------------------------------------------------------- 5. the engine
S5, G5, SIMS5, E5, NM5, K5 = 9, 4, 16, 4, 6, 3


def _draws():
    rng = np.random.RandomState(21)
    return rng.dirichlet([0.03] * (S5 * S5 + 1), size=G5), rng.random_sample((G5, NM5))


def _play(eng):
    """Steps an engine to the end; per step the tree bytes of every slot, at the end the move records per slot."""
    noises, uni = _draws()
    eng.start_games(np.arange(G5), noises=noises, uniforms=uni)
    trees = []
    while True:
        st = eng.step()
        eng.drain()
        trees.append(tuple(eng.tree_serialize(s)[0].tobytes() for s in range(G5)))
        if st.n_active == 0:
            break
        assert len(trees) < 400
    moves = {s: [(m["action"], m["player"], np.float32(m["value"]).tobytes(), m["policy"].tobytes(), m["packed"].tobytes())
                 for m in eng.records[s]] for s in range(G5)}
    return trees, moves


def _engine(net, graph):
    from sejonggo_amd.engine import SelfPlayEngine
    return SelfPlayEngine(net, size=S5, n_games=G5, sims=SIMS5, energy=E5, stop_exploration=3, num_moves=NM5, komi=5.5,
                          symmetry=K5, graph=graph)


@pytest.fixture(scope="module")
def nets5():
    from sejonggo_amd.net import FusedInferenceNet, NativeNet
    import torch
    module = _seeded_module(S5, 4, seed=9)
    fnet = FusedInferenceNet(module, torch.float16, "cuda")
    assert fnet.use_fused_heads(True)
    return module, fnet, NativeNet(module, max_batch=64)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_engine_on_native_net_plays_the_same_game(L, nets5, graph):
    module, fnet, nnet = nets5
    a, b = _engine(nnet, graph), _engine(fnet, graph)
    assert a.packed and b.packed and a.graph == graph
    ta, ma = _play(a)
    tb, mb = _play(b)
    if graph:
        assert a.n_graph_replays > 0 and b.n_graph_replays > 0
    assert all(len(ma[s]) == NM5 for s in range(G5))
    assert len(ta) == len(tb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert x == y, "trees differ after step %d" % i
    assert ma == mb
    a.close()
    b.close()


def test_ctypes_only_loop_reproduces_the_game(L, nets5):
    """The loop of INTEGRATION.md against include/sgo.h alone; the net is filled from host (numpy) arrays."""
    import torch
    module, fnet, nnet = nets5
    lib = L.load()
    eng = _engine(nnet, False)
    want_trees, want_moves = _play(eng)
    eng.close()

    A, RW = S5 * S5 + 1, lib.sgo_packed_words(S5)
    host = {k: getattr(fnet, k).detach().cpu().numpy() for k in ("stem_w10", "stem_b", "stem_wcol", "head_w", "head_b", "p_fc_w", "p_fc_b",
                                                        "v_fc1_w", "v_fc1_b", "v_fc2_w", "v_fc2_b")}
    blocks = [[(t.detach().permute(0, 2, 3, 1) if t.dim() == 4 else t.detach()).contiguous().cpu().numpy() for t in b] for b in fnet.blocks]
    assert blocks[0][0].shape == (256, 3, 3, 256)                                    # OHWI
    arr = [(C.c_void_p * len(blocks))(*[b[i].ctypes.data for b in blocks]) for i in range(4)]
    w = L.NetWeights(block_w1=arr[0], block_b1=arr[1], block_w2=arr[2], block_b2=arr[3],
                     **{k: v.ctypes.data for k, v in host.items()})
    net = C.c_void_p(lib.sgo_net_create(S5, len(blocks), 8, 0))                      # max_batch 8 < G * E: the slice loop
    assert net, lib.sgo_last_error()
    L.check(lib.sgo_net_set_weights(net, C.byref(w), None), "sgo_net_set_weights")

    cfg = L.Config(size=S5, n_games=G5, sims=SIMS5, energy=E5, stop_exploration=3, num_moves=NM5, blocks_per_game=0, self_play=1,
                   komi=5.5, dirichlet_epsilon=eng_epsilon(), device_id=0, two_model=0, shared_blocks=0)
    ctx = C.c_void_p(lib.sgo_ctx_create(C.byref(cfg)))
    assert ctx, lib.sgo_last_error()
    noises, uni = _draws()
    slots = np.arange(G5, dtype=np.int32)
    L.check(lib.sgo_start_games(ctx, G5, L.ptr(slots), L.ptr(np.ascontiguousarray(noises)), L.ptr(np.ascontiguousarray(uni)),
                                C.c_int(NM5), None, None), "sgo_start_games")
    rec, idx = C.c_void_p(), C.c_void_p()
    L.check(lib.sgo_eval_list(ctx, C.byref(rec), C.byref(idx), None), "sgo_eval_list")
    pol = torch.zeros((G5 * E5, A), dtype=torch.float32, device="cuda")             # the two output allocations
    val = torch.zeros((G5 * E5,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = L.Status()
    pp = vp = None
    trees, recs_out = [], {s: [] for s in range(G5)}
    cap = 2 * G5 + 16
    while True:
        L.check(lib.sgo_step(ctx, pp, vp, C.c_int(K5), None, C.byref(st)), "sgo_step")
        assert st.error == 0
        if st.n_records:
            r = np.zeros(cap, dtype=L.MOVE_RECORD_DTYPE)
            packed = np.zeros((cap, RW), dtype=np.uint32)
            policy = np.zeros((cap, A), dtype=np.float64)
            m = L.check(lib.sgo_drain_records(ctx, C.c_int(cap), L.ptr(r), L.ptr(packed), L.ptr(policy)), "sgo_drain_records")
            for i in np.lexsort((r["move_n"][:m], r["game"][:m])):
                recs_out[int(r["game"][i])].append((int(r["action"][i]), int(r["player"][i]), r["value"][i].tobytes(),
                                                    policy[i].tobytes(), packed[i].tobytes()))
        step_trees = []
        for s in range(G5):
            nn_, ne_ = C.c_int64(0), C.c_int64(0)
            sz = L.check(lib.sgo_tree_serialize(ctx, C.c_int(s), None, C.c_int64(0), C.byref(nn_), C.byref(ne_)))
            buf = np.zeros(max(1, sz), dtype=np.uint8)
            L.check(lib.sgo_tree_serialize(ctx, C.c_int(s), L.ptr(buf), C.c_int64(sz), C.byref(nn_), C.byref(ne_)))
            step_trees.append(buf[:sz].tobytes())
        trees.append(tuple(step_trees))
        if st.n_active == 0:
            break
        assert len(trees) < 400
        L.check(lib.sgo_net_predict_packed_dev(net, st.n_eval, rec, idx, K5, None, pol.data_ptr(), val.data_ptr(), None),
                "sgo_net_predict_packed_dev")
        pp, vp = C.c_void_p(pol.data_ptr()), C.c_void_p(val.data_ptr())
    lib.sgo_ctx_destroy(ctx)
    lib.sgo_net_destroy(net)
    assert len(trees) == len(want_trees)
    for i, (x, y) in enumerate(zip(trees, want_trees)):
        assert x == y, "trees differ after step %d" % i
    assert recs_out == want_moves


def test_resident_form_returns_a_native_net_only_when_asked(L, nets5):
    """conf['NATIVE_NET'] (default 0, read with .get) switches predicting_queue_worker.resident_form; the name is kept."""
    from sejonggo_amd import predicting_queue_worker as pq
    from sejonggo_amd.conf import conf
    from sejonggo_amd.net import FusedInferenceNet, NativeNet
    module = nets5[0]
    assert not conf.get('NATIVE_NET', 0)
    default = pq.resident_form(module, 0)
    assert type(default) is FusedInferenceNet and not default.fused_heads
    conf['NATIVE_NET'] = 1
    try:
        native = pq.resident_form(module, 0)
    finally:
        del conf['NATIVE_NET']
    assert type(native) is NativeNet and native.name == module.name and native.packed_ok
    native.close()


def eng_epsilon():
    from sejonggo_amd.conf import conf
    return conf['DIRICHLET_EPSILON']


# ---------------------------------------------------------------------------------------------------------- 6. arguments
def test_arguments(L):
    import torch
    lib = L.load()
    ERR_ARG = -1
    for S, nb, mb in ((8, 4, 64), (9, 0, 64), (9, 4, 0), (21, 2, 8)):
        assert not lib.sgo_net_create(S, nb, mb, 0)
        assert b"sgo_net_create" in lib.sgo_last_error()
    assert lib.sgo_heads_packed_bytes(8) < 0
    S, n = 9, 3
    A, t = S * S + 1, S - 2
    f16 = dict(dtype=torch.float16, device="cuda")
    y = torch.zeros((n, t, t, 256), **f16)
    hw, hb = torch.zeros((4, 256), **f16), torch.zeros(4, **f16)
    pw, pb = torch.zeros((A, 2 * t * t), **f16), torch.zeros(A, **f16)
    vw, vb = torch.zeros((256, 2 * t * t), **f16), torch.zeros(256, **f16)
    w2, b2 = torch.zeros(256, **f16), torch.zeros(1, **f16)
    bank = torch.empty(lib.sgo_heads_packed_bytes(S), dtype=torch.uint8, device="cuda")
    pol = torch.full((n, A), -7.0, dtype=torch.float32, device="cuda")
    val = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    st = L.stream_ptr()
    assert lib.sgo_heads_prepack_dev(8, pw.data_ptr(), vw.data_ptr(), bank.data_ptr(), st) == ERR_ARG
    assert lib.sgo_heads_prepack_dev(S, None, vw.data_ptr(), bank.data_ptr(), st) == ERR_ARG
    assert lib.sgo_heads_prepack_dev(S, pw.data_ptr(), vw.data_ptr(), None, st) == ERR_ARG
    assert lib.sgo_heads_prepack_dev(S, pw.data_ptr(), vw.data_ptr(), bank.data_ptr(), st) == 0
    args = [y, hw, hb, bank, pb, vb, w2, b2, pol, val]
    ptrs = [a.data_ptr() for a in args]
    assert lib.sgo_heads_dev(8, n, *ptrs, st) == ERR_ARG
    assert lib.sgo_heads_dev(S, -1, *ptrs, st) == ERR_ARG
    for i in range(len(ptrs)):
        bad = list(ptrs)
        bad[i] = None
        assert lib.sgo_heads_dev(S, n, *bad, st) == ERR_ARG, i
        assert lib.sgo_last_error()
    assert lib.sgo_heads_dev(S, 0, *ptrs, st) == 0                                   # n = 0: nothing is launched
    torch.cuda.synchronize()
    assert bool((pol == -7.0).all()) and bool((val == -7.0).all())
    assert lib.sgo_heads_dev(S, n, *ptrs, st) == 0                                   # zeros in: uniform policy, value 0
    torch.cuda.synchronize()
    assert torch.allclose(pol, torch.full_like(pol, 1.0 / A), rtol=1e-6) and bool((val == 0).all())

    net = C.c_void_p(lib.sgo_net_create(S, 1, 4, 0))
    assert net
    recs = torch.zeros((4, lib.sgo_packed_words(S)), dtype=torch.int32, device="cuda")
    assert lib.sgo_net_predict_packed_dev(net, 1, recs.data_ptr(), None, 0, None, pol.data_ptr(), val.data_ptr(), st) < 0   # no weights yet
    assert lib.sgo_net_set_weights(net, None, st) == ERR_ARG
    assert lib.sgo_net_set_weights(None, None, st) == ERR_ARG
    assert lib.sgo_net_set_weights(net, C.byref(L.NetWeights()), st) == ERR_ARG       # null fields
    assert lib.sgo_net_predict_packed_dev(None, 1, recs.data_ptr(), None, 0, None, pol.data_ptr(), val.data_ptr(), st) == ERR_ARG
    assert lib.sgo_net_predict_packed_dev(net, 1, None, None, 0, None, pol.data_ptr(), val.data_ptr(), st) == ERR_ARG
    assert lib.sgo_net_predict_packed_dev(net, 1, recs.data_ptr(), None, 8, None, pol.data_ptr(), val.data_ptr(), st) == ERR_ARG
    assert lib.sgo_net_predict_packed_dev(net, 1, recs.data_ptr(), None, 0, None, None, val.data_ptr(), st) == ERR_ARG
    assert lib.sgo_net_packed_tower(None, 1, st) == ERR_ARG and lib.sgo_net_packed_tower(net, 2, st) == ERR_ARG
    assert lib.sgo_net_packed_tower(net, 1, st) == 0 and lib.sgo_net_packed_tower(net, 1, st) == 0      # before any weights: banks only
    assert lib.sgo_net_packed_tower(net, 0, st) == 0
    lib.sgo_net_destroy(net)
    lib.sgo_net_destroy(None)
