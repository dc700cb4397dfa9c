"""What the per-analysis bench tools (bench_keys, _tactics, _life, _shapes, _moves, _influence) share: the percentile summary,
the HIP-event bracket, the golden 19x19 games as replay lists, and the compiler's resource figures of a kernel."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 19


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]          # noqa: E731
    return {"median_us": 1e3 * q(0.5), "min_us": 1e3 * s[0], "p10_us": 1e3 * q(0.1), "p90_us": 1e3 * q(0.9), "reps": len(s)}


def timed(fn):
    """milliseconds of fn() between two HIP events on the current stream"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def load_games(copies):
    """(n_entries, off, actions, colours, first): the five records of tests/golden/sgf_S19.npz repeated `copies` times as the int32
    lists of sgo_records_replay, and the number of records of the first copy."""
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "sgf_S19.npz"))
    games = []
    for gi in range(5):
        mv = z["g%02d_moves" % gi]
        games.append(([S * S if y >= S else int(y) * S + int(x) for x, y, _ in mv], [int(c) for _, _, c in mv]))
    first = sum(len(g[0]) + 1 for g in games)
    games = games * copies
    n_entries = np.array([len(g[0]) for g in games], np.int32)
    off = np.concatenate([[0], np.cumsum(n_entries)[:-1]]).astype(np.int32)
    acts = np.concatenate([g[0] for g in games]).astype(np.int32)
    cols = np.concatenate([g[1] for g in games]).astype(np.int32)
    return n_entries, off, acts, cols, first


def resources(source, kernel):
    """{"vgprs" / "sgprs" / "lds_bytes" / "scratch": {size: value}} of sgo::<kernel><S> from the device listing of csrc/<source>;
    None without hipcc"""
    import vmcnt_isa_check
    asm = vmcnt_isa_check.device_asm(source=source)
    if asm is None:
        return None
    out = {"vgprs": {}, "sgprs": {}, "lds_bytes": {}, "scratch": {}}
    head = r"^\s*\.amdhsa_kernel\s+_ZN3sgo%d%sILi(\d+)EE\S*\n(.*?)^\s*\.end_amdhsa_kernel" % (len(kernel), kernel)
    for m in re.finditer(head, asm, re.M | re.S):
        d = dict(re.findall(r"^\s*(\.amdhsa_\w+)\s+(\S+)", m.group(2), re.M))
        size = m.group(1)
        out["vgprs"][size] = int(d[".amdhsa_next_free_vgpr"])
        out["sgprs"][size] = int(d[".amdhsa_next_free_sgpr"])
        out["lds_bytes"][size] = int(d[".amdhsa_group_segment_fixed_size"])
        out["scratch"][size] = int(d[".amdhsa_private_segment_fixed_size"])
    return out
