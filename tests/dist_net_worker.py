"""One rank of the replica tests (started by sejonggo_amd.distributed.launch_ranks): the weight broadcast into a resident net,
and what the net evaluates afterwards.
usage: dist_net_worker.py standin <out_dir>      CPU: broadcast_net into an object with FusedInferenceNet's tensor attributes
       dist_net_worker.py device <out_dir> [moves]   GPU, gloo, ranks share the device: FusedInferenceNet and NativeNet, every route
A failed check prints its line and the rank leaves with exit code 1."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class StandIn(object):
    """FusedInferenceNet's weight attributes as small CPU tensors (same names, dtypes and memory formats), filled from `seed`;
    refresh() records how often it ran and the checksum of the tensors it found."""

    def __init__(self, seed, blocks=2, ch=8, S=5):
        import torch
        g = torch.Generator().manual_seed(seed)
        t2, A = (S - 2) * (S - 2), S * S + 1

        def r(*shape, **kw):
            return torch.randn(*shape, generator=g).to(kw.get("dtype", torch.float16))

        def cl(w):
            return w.contiguous(memory_format=torch.channels_last)

        self.stem_w, self.stem_b = cl(r(ch, 32, 3, 3)), r(ch)
        self.stem_w10, self.stem_wcol = r(ch, 10, 16), r(ch, dtype=torch.float32)
        self.blocks = [(cl(r(ch, ch, 3, 3)), r(ch), cl(r(ch, ch, 3, 3)), r(ch)) for _ in range(blocks)]
        self.head_w, self.head_b = r(4, ch), r(4)
        self.p_fc_w, self.p_fc_b = r(A, 2 * t2), r(A)
        self.v_fc1_w, self.v_fc1_b = r(256, 2 * t2), r(256)
        self.v_fc2_w, self.v_fc2_b = r(1, 256), r(1)
        self.refreshed = []

    def refresh(self):
        from sejonggo_amd.distributed import _checksum, net_tensors
        self.refreshed.append(_checksum(net_tensors(self)))


class _Checks(object):
    def __init__(self, rank):
        self.rank, self.failed = rank, []

    def __call__(self, ok, what):
        if not ok:
            self.failed.append(what)
            print("rank %d: FAILED: %s" % (self.rank, what), file=sys.stderr)


def standin(out_dir):
    import torch
    import torch.distributed as dist
    from sejonggo_amd.distributed import _checksum, broadcast_net, init_from_env, net_tensors
    from sejonggo_amd.net import PolicyValueNet
    rank, world, _ = init_from_env("gloo")
    check = _Checks(rank)
    net, src = StandIn(100 + rank), StandIn(100)
    names = [n for n in ("stem_w", "stem_b", "stem_w10", "stem_wcol") if any(getattr(net, n) is t for t in net_tensors(net))]
    check(names == ["stem_w", "stem_b", "stem_w10", "stem_wcol"], "net_tensors lists %r of the stem" % (names,))
    differed = not torch.equal(net.stem_w10, src.stem_w10) and not torch.equal(net.stem_wcol, src.stem_wcol)
    check(differed == (rank != 0), "the ranks start from different weights")
    info = broadcast_net(net)
    check(info["identical"], "identical")
    check(torch.equal(net.stem_w10, src.stem_w10) and torch.equal(net.stem_wcol, src.stem_wcol), "stem_w10 and stem_wcol arrive")
    check(all(torch.equal(a, b) for a, b in zip(net_tensors(net), net_tensors(src))), "every listed tensor is rank 0's")
    check(all(a.stride() == b.stride() for a, b in zip(net_tensors(net), net_tensors(src))), "memory formats are kept")
    check(len(net.refreshed) == 1, "refresh() ran %d times" % len(net.refreshed))
    check(net.refreshed == [info["checksum"]] and info["checksum"] == _checksum(net_tensors(src)),
          "refresh() ran before the last tensor had arrived")
    n_old = 2 + 4 * len(net.blocks) + 8
    check(info["tensors"] == n_old + 2 == len(net_tensors(net)), "info['tensors'] = %d" % info["tensors"])
    check(info["bytes"] == sum(t.numel() * t.element_size() for t in net_tensors(src)), "info['bytes']")
    # a torch module has no refresh(): its path is what it was (tests/dist_worker.py)
    torch.manual_seed(100 + rank)
    mod = PolicyValueNet(5, 1, 8, name="r%d" % rank)
    minfo = broadcast_net(mod)
    torch.manual_seed(100)
    want = PolicyValueNet(5, 1, 8)
    check(minfo["identical"] and minfo["tensors"] == len(list(mod.parameters())) + len(list(mod.buffers())), "module: info")
    check(all(torch.equal(a, b) for a, b in zip(net_tensors(mod), net_tensors(want))), "module: weights are rank 0's")
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump({"failed": check.failed, "refreshed": net.refreshed, "checksum": info["checksum"], "tensors": info["tensors"],
                   "module_checksum": minfo["checksum"]}, f)
    dist.barrier()
    dist.destroy_process_group()
    return 1 if check.failed else 0


def device(out_dir, moves):
    import torch
    import torch.distributed as dist
    from sejonggo_amd import _lib as L
    from sejonggo_amd.distributed import broadcast_net, init_from_env
    from tests.test_gpu_net_replicas import (Rows, engine_for, make_net, outputs, play, rows_that_differ, same_bits)
    rank, world, dev = init_from_env("gloo")
    L.require_gpu()
    check = _Checks(rank)
    S, blocks = 5, 1
    rows = Rows(L, S, seed=4100)
    mine = [make_net(S, blocks, 100 + rank, native) for native in (False, True)]
    ref = [make_net(S, blocks, 100, native) for native in (False, True)]
    want, before = {}, {}
    for a, b in zip(mine, ref):
        want.update(outputs(b, rows))
        before.update(outputs(a, rows))
    for net in mine:
        info = broadcast_net(net)
        check(info["identical"], "identical (%s)" % type(net).__name__)
        check(info["tensors"] == 4 + 4 * blocks + 8, "info['tensors'] = %d" % info["tensors"])
    after = {}
    for net in mine:
        after.update(outputs(net, rows))
    check(set(after) == set(want) and len(want) == 7, "routes: %r" % sorted(after))
    for name in sorted(want):
        d0, d1 = rows_that_differ(before[name], want[name]), rows_that_differ(after[name], want[name])
        check(same_bits(after[name], want[name]), "%s: %d of %d rows differ from rank 0's net after the broadcast" % (name, d1, rows.n_rows))
        if rank == 0:
            check(same_bits(before[name], want[name]) and same_bits(before[name], after[name]), "%s: rank 0's own net changed" % name)
        else:
            check(d0 == rows.n_rows, "%s: only %d of %d rows differed before the broadcast" % (name, d0, rows.n_rows))
    # replicas with equal seeds play equal games
    fnet = mine[0]
    assert fnet.packed_tower and fnet.fused_heads
    eng = engine_for(fnet, S, False, num_moves=moves)
    trees, played = play(eng, S, num_moves=moves)
    eng.close()
    h = hashlib.sha256()
    for s in sorted(played):
        for m in played[s]:
            h.update(repr(m[:2]).encode())
            for b in m[2:]:
                h.update(b)
    n_moves = sum(len(v) for v in played.values())
    check(n_moves > 0, "no move was played")
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump({"failed": check.failed, "game": h.hexdigest(), "n_moves": n_moves, "n_steps": len(trees)}, f)
    for net in mine[1:] + ref[1:]:
        net.close()
    dist.barrier()
    dist.destroy_process_group()
    return 1 if check.failed else 0


def main():
    mode, out_dir = sys.argv[1], sys.argv[2]
    if mode == "standin":
        return standin(out_dir)
    return device(out_dir, int(sys.argv[3]) if len(sys.argv) > 3 else 6)


if __name__ == "__main__":
    sys.exit(main())
