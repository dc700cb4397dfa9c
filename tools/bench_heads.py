"""A/B of the heads alone: A = the framework route of net.FusedInferenceNet._tower_and_heads (eight small launches: a GEMM for the two
1x1 convolutions, three F.linear, softmax, tanh and their glue), B = sgo_heads_dev (k_heads, csrc/sgo_heads.hpp: one launch).

Both arms run on the SAME real tower output: the post-ReLU activations of a seeded net's own stem and tower on played positions, not
random data.  Arms are interleaved launch by launch in one process after a warm-up, each launch bracketed by HIP events; the report
has the median and the spread (min, 10th / 90th percentile) per arm, the number of kernels an arm launches (torch profiler), and B's
share of its floor: the n * t^2 * 512 bytes of activations it must read over the rate a 1.2-GB table swept in order reaches on this
chip (6.0 TB/s; the spec peak is 8.0).

    python tools/bench_heads.py [--reps 30] [--out profiles/heads_ab.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.0e12      # bytes / s, an in-order sweep of 1.2 GB
SHAPES = [("headline", 19, 8192, 2, 120), ("config2", 9, 2048, 2, 30)]     # name, board size (tower 17x17 / 7x7), positions, blocks, ply


def played_records(L, S, n, ply, seed):
    """n packed records after `ply` seeded random legal moves each, played on the device by board_advance."""
    import torch
    lib = L.load()
    A, NW, RW = S * S + 1, lib.sgo_plane_words(S), lib.sgo_packed_words(S)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    cur = torch.zeros((n, RW), dtype=torch.int32, device="cuda")
    nxt = torch.zeros_like(cur)
    legal = torch.full((n, NW), -1, dtype=torch.int32, device="cuda")
    legal[:, NW - 1] = (1 << ((A - 1) % 32 + 1)) - 1
    shifts = torch.arange(32, device="cuda", dtype=torch.int32)
    for _ in range(ply):
        bits = ((legal.unsqueeze(-1) >> shifts) & 1).reshape(n, NW * 32)[:, :A].float()
        bits[:, A - 1] = 0.01
        mv = torch.multinomial(bits, 1, generator=g).reshape(-1).to(torch.int32)
        L.check(lib.sgo_advance_legal_dev(S, n, L.ptr(cur), None, L.ptr(mv), None, L.ptr(nxt), None, L.ptr(legal), None, L.stream_ptr()))
        cur, nxt = nxt, cur
    return cur


def tower_output(L, fnet, recs, n):
    import torch
    y = torch.empty((n, fnet.channels, fnet.t, fnet.t), dtype=torch.float16, device=fnet.device, memory_format=torch.channels_last)
    L.check(fnet.lib.sgo_stem_packed_dev(fnet.size, n, recs.data_ptr(), None, 0, None, fnet.stem_w10.data_ptr(), fnet.stem_b.data_ptr(),
                                         fnet.stem_wcol.data_ptr(), y.data_ptr(), L.stream_ptr()), "sgo_stem_packed_dev")
    for (w1, b1, w2, b2) in fnet.blocks:
        z = fnet._conv(y, w1, b1, 1)
        y = fnet._conv(z, w2, b2, 1, skip=y)
    return y


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]
    return {"median_us": 1e3 * q(0.5), "min_us": 1e3 * s[0], "p10_us": 1e3 * q(0.1), "p90_us": 1e3 * q(0.9), "reps": len(s)}


def count_kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(names), sorted(set(names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "heads_ab.json"))
    ap.add_argument("--no-kernel-count", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repetitions"
    import torch
    from sejonggo_amd import _lib as L
    from sejonggo_amd.net import build_fused_net
    L.require_gpu()
    result = {"device": torch.cuda.get_device_name(0), "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "shapes": {}}
    for name, S, n, blocks, ply in SHAPES:
        fnet, _ = build_fused_net(S, blocks, seed=3)
        y = tower_output(L, fnet, played_records(L, S, n, ply, seed=41), n)
        assert fnet.use_fused_heads(True)
        fnet.fused_heads = False
        saved = fnet.blocks
        fnet.blocks = []                                  # _tower_and_heads without the tower: the heads as the product runs them

        def arm_a():
            return fnet._tower_and_heads(y)

        def arm_b():
            return fnet._heads_kernel(y)

        with torch.no_grad():
            pa, va = arm_a()
            pb, vb = arm_b()
            dp = float((pa.double() - pb.double()).abs().max())
            dv = float((va.double() - vb.double()).abs().max())
            for _ in range(args.warmup):
                arm_a()
                arm_b()
            torch.cuda.synchronize()
            times = {"A": [], "B": []}
            for _ in range(args.reps):
                for key, fn in (("A", arm_a), ("B", arm_b)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[key].append(e0.elapsed_time(e1))
            launches = {}
            if not args.no_kernel_count:
                try:
                    for key, fn in (("A", arm_a), ("B", arm_b)):
                        launches[key], _ = count_kernels(fn)
                except Exception as e:                        # the timings stand without the count
                    print("kernel count unavailable: %r" % (e,), file=sys.stderr)
        fnet.blocks = saved
        t2 = fnet.t * fnet.t
        floor_us = 1e6 * n * t2 * 512 / HBM_ACHIEVABLE
        a, b = stats(times["A"]), stats(times["B"])
        result["shapes"][name] = {
            "positions": n, "tower": "%dx%d" % (fnet.t, fnet.t), "activation_bytes": n * t2 * 512,
            "A_torch_route": dict(a, launches=launches.get("A")), "B_sgo_heads_dev": dict(b, launches=launches.get("B")),
            "B_floor_us": floor_us, "B_fraction_of_floor": floor_us / b["median_us"], "speedup_B_over_A": a["median_us"] / b["median_us"],
            "max_abs_dp_A_vs_B": dp, "max_abs_dv_A_vs_B": dv,
        }
        print("HEADS_AB %s n=%d %s: A %.1f us (p10 %.1f p90 %.1f, %s launches)  B %.1f us (p10 %.1f p90 %.1f, %s launches)  "
              "floor %.1f us = %.2f of B  |dp| %.1e |dv| %.1e" % (name, n, result["shapes"][name]["tower"], a["median_us"], a["p10_us"],
                                                                a["p90_us"], launches.get("A"), b["median_us"], b["p10_us"], b["p90_us"],
                                                                launches.get("B"), floor_us, floor_us / b["median_us"], dp, dv), flush=True)
        del y, fnet
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
