"""A scripted stand-in for engine.SelfPlayEngine, and the driver runs recorded in tests/golden/slot_loop_traces.json.

FakeEngine has the surface the three worker bodies drive (start_games / start_eval_games / step / drain / results / records /
status / game_data / close) and no GPU: it inherits game_data from the real class and replaces everything that touches the
library.  A script maps game number -> (plies, outcome): every step an active slot records one ply until it has `plies` of
them, then ends with `outcome` (1 = done, negative = engine error code); a zero-ply game ends on its first step.  The result
fields of a game are fixed functions of its number.  Every call is appended, with its arguments, to a trace.

    python tests/fake_engine.py        # rewrites the golden file from the code that is checked out

The golden file was written by this command on the commit BEFORE the three loops became one (see its "recorded_on" entry);
tests/test_slot_loop.py requires the drivers to reproduce it element for element."""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sejonggo_amd import _lib                                   # noqa: E402
from sejonggo_amd.engine import MoveRecord, SelfPlayEngine      # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "slot_loop_traces.json")


class FakeEngine(SelfPlayEngine):
    script = {}          # game number -> (plies, outcome); games not listed play DEFAULT
    DEFAULT = (2, 1)
    unnamed = None       # iterator of game numbers for start_games calls without ids (the ranks pass none)
    trace = None         # the list every instance of a run appends to

    def __init__(self, net, n_games=None, size=None, net2=None, **kw):
        self.net, self.net2, self.two_model = net, net2, net2 is not None
        self.G, self.S = n_games, size
        self.A = size * size + 1
        self.RW = 16 * ((size * size + 31) // 32)
        self.status = _lib.Status()
        self.records, self.game_ids = {}, {}
        self.n_steps = self.n_net_calls = self.n_net_positions = 0
        self.ctx = None
        self._slots = {}       # slot -> {"game", "plies", "outcome", "played", "done", "fresh": undrained records}
        self.trace.append(["init", {"n_games": n_games, "size": size, "two_model": self.two_model,
                                    "kw": {k: kw[k] for k in sorted(kw) if isinstance(kw[k], (int, float, str, bool, type(None)))}}])

    def close(self):
        if self.trace is not None and getattr(self, "_slots", None) is not None:
            self.trace.append(["close"])
            self._slots = None

    def _start(self, slots, ids):
        for i, s in enumerate(slots):
            g = ids[i] if ids is not None else next(self.unnamed)
            plies, outcome = self.script.get(g, self.DEFAULT)
            self._slots[int(s)] = {"game": g, "plies": plies, "outcome": outcome, "played": 0, "done": 0, "fresh": []}
            self.records[int(s)] = []
            self.game_ids[int(s)] = None if ids is None else ids[i]

    def start_games(self, slots, noises=None, uniforms=None, resign=None, ids=None):
        self.trace.append(["start_games", [int(s) for s in slots], None if resign is None else [_plain(r) for r in resign],
                           None if ids is None else list(ids)])
        self._start(slots, ids)

    def start_eval_games(self, slots, first_model=None, uniforms=None, resign_model1=None, resign_model2=None, ids=None):
        self.trace.append(["start_eval_games", [int(s) for s in slots], None, None if ids is None else list(ids)])
        self._start(slots, ids)

    def step(self):
        st = self.status
        st.error = st.error_game = 0
        for s in sorted(self._slots):
            sl = self._slots[s]
            if sl["done"]:
                continue
            if sl["played"] < sl["plies"]:
                sl["fresh"].append(sl["played"])
                sl["played"] += 1
            if sl["played"] == sl["plies"]:
                sl["done"] = sl["outcome"]
                if sl["outcome"] < 0 and not st.error:
                    st.error, st.error_game = sl["outcome"], s
        st.n_records = sum(len(sl["fresh"]) for sl in self._slots.values())
        st.n_done = sum(1 for sl in self._slots.values() if sl["done"])
        st.n_active = len(self._slots) - st.n_done
        self.n_steps += 1
        self.n_net_calls += 1
        self.n_net_positions += st.n_active
        self.trace.append(["step", {k: int(getattr(st, k)) for k in ("n_records", "n_active", "n_done", "error", "error_game")}])
        return st

    def drain(self):
        n = 0
        for s in sorted(self._slots):
            sl = self._slots[s]
            for move_n in sl["fresh"]:
                a = (7 * sl["game"] + 3 * move_n) % self.A
                packed = np.zeros(self.RW, dtype=np.uint32)
                packed[0] = np.uint32(sl["game"] * 64 + move_n)
                policy = np.zeros(self.A, dtype=np.float64)
                policy[a] = 1.0
                rec = MoveRecord(policy=policy, value=np.float32(((5 * sl["game"] + 3 * move_n) % 11 - 5) / 8.0),
                                 move=(a % self.S, a // self.S), move_n=move_n, player=1 if move_n % 2 == 0 else -1, packed=packed,
                                 action=a, game_seq=0)
                rec.size = self.S
                self.records.setdefault(s, []).append(rec)
                n += 1
            sl["fresh"] = []
        self.status.n_records = 0
        self.trace.append(["drain", n])
        return n

    def results(self, slots=None):
        out = np.zeros(self.G, dtype=_lib.GAME_RESULT_DTYPE)
        for s, sl in self._slots.items():
            g = sl["game"]
            r = out[s]
            r["done"], r["n_moves"] = sl["done"], sl["played"]
            r["winner"], r["end_reason"] = (1, -1, 0)[g % 3], (2, 1, 0)[(g // 2) % 3]
            r["black"], r["white"] = 10 + g, 7.5 + 3 * (g % 4)
            r["last_player"] = 1 if sl["played"] % 2 else -1
            r["first_model"], r["blocks_high_water"] = g % 2, 100 + g
        self.trace.append(["results", [int(d) for d in out["done"]]])
        return out


def _plain(v):
    """JSON form of a value the drivers hand around (numpy scalars become Python numbers)."""
    return v.item() if isinstance(v, np.generic) else v


class _Net(object):
    def __init__(self, name):
        self.name = name


@contextlib.contextmanager
def _patched(*triples):
    """(object, attribute, value) triples set for the duration of the block."""
    old = [(o, a, getattr(o, a)) for o, a, _ in triples]
    for o, a, v in triples:
        setattr(o, a, v)
    try:
        yield
    finally:
        for o, a, v in old:
            setattr(o, a, v)


@contextlib.contextmanager
def _conf(**kw):
    from sejonggo_amd.conf import conf
    old = dict(conf)
    conf.update(kw)
    try:
        yield
    finally:
        conf.clear()
        conf.update(old)


def _listing(root):
    """Sorted directories under root, relative, two levels below the model directory (game and move directories)."""
    out = []
    for d, subs, files in os.walk(root):
        subs.sort()
        rel = os.path.relpath(d, root)
        if rel != ".":
            out.append(rel.replace(os.sep, "/") + ("/" + "+".join(sorted(f for f in files if not f.endswith(".npz"))) if files else ""))
    return sorted(out)


def _saved(g, gd):
    return [g, len(gd['moves']), gd['winner_model'], gd['result'], _plain(gd['resign_model1'])]


def _run(case, tmp, body):
    """One driver run against FakeEngine: conf, the engine and the model loaders replaced; trace, return value, directory
    listings, saver sequence and the slot-failure messages collected."""
    from sejonggo_amd import engine, predicting_queue_worker as pq
    trace, saved = [], []
    names = {"BEST_SYM": "best", "BEST": "best", "BEST_NAME": "best", "LATEST_NAME": "latest"}
    fake = type("FakeEngine", (FakeEngine,), {"script": case.get("script", {}), "trace": trace,
                                              "unnamed": iter(case.get("unnamed", []))})
    dirs = {k: os.path.join(tmp, k.lower()) for k in ("SELF_PLAY_DIR", "EVAL_DIR", "GAMES_DIR")}
    for rel in case.get("existing", []):
        os.makedirs(os.path.join(tmp, rel))
    err = io.StringIO()
    settings = dict(dirs, SIZE=5, ENGINE_HALVES=1, ENGINE_GRAPH=False, WRITER_THREADS=1, WRITER_PROCESSES=0, SGF_ENABLED=False,
                    RESIGNATION_PERCENT=0.0, RESIGNATION_ALLOWED_ERROR=0.5, WRITE_NPZ_TWIN=False)
    settings.update(case.get("conf", {}))
    with _conf(**settings), contextlib.redirect_stderr(err), _patched(
            (engine, "SelfPlayEngine", fake), (pq, "get_model", lambda ind, gpu=None: _Net("best" if ind.startswith("BEST") else "latest")),
            (pq, "put_name_request", lambda ind: names[ind])):
        ret = body(saved)
    return {"trace": trace, "returned": ret, "saved": saved,
            "dirs": {k.lower(): _listing(v) for k, v in dirs.items() if os.path.isdir(v)},
            "messages": [l for l in err.getvalue().splitlines() if "failed with engine error" in l]}


# ------------------------------------------------------------------------------------------------ the three drivers
def run_selfplay_case(case, tmp):
    from sejonggo_amd.selfplay_worker import run_selfplay

    def body(saved):
        stats = {}
        played = run_selfplay(0, "BEST_SYM", on_game=lambda g, gd: saved.append(_saved(g, gd)), stats=stats, **case["args"])
        return {"played": played, "stats_keys": sorted(stats), "steps": stats["steps"], "moves": stats["moves"],
                "games": stats["games"], "files": stats["files"], "net_calls": stats["net_calls"]}
    return _run(case, tmp, body)


def run_evaluation_case(case, tmp):
    from sejonggo_amd import evaluator, sgfsave
    from sejonggo_amd.evaluate_worker import run_evaluation

    def body(saved):
        real_data, real_eval = sgfsave.save_game_data, evaluator.save_eval_game

        def data(model_name, g, gd, game_name="game"):
            saved.append(_saved(g, gd) + [model_name, game_name, gd['first_model']])
            return real_data(model_name, g, gd, game_name=game_name)

        def result(model_name, g, winner_model):
            saved.append(["eval", model_name, g, winner_model])
            return real_eval(model_name, g, winner_model)

        with _patched((sgfsave, "save_game_data", data), (evaluator, "save_eval_game", result)):
            return list(run_evaluation(0, **case["args"]))
    return _run(case, tmp, body)


def run_rank_case(case, tmp):
    """World 1 on gloo: the real process group, the real TupleGather, the real writer of rank 0."""
    import torch.distributed as dist
    from sejonggo_amd import dist_selfplay, distributed

    def body(saved):
        real_init, real_tuples = distributed.init_from_env, dist_selfplay._tuples_of

        def init(backend):
            rank, world, local = real_init(backend)
            return rank, world, 0 if local is None else local

        def tuples(g, gd, rank, size):
            saved.append(_saved(g, gd))
            return real_tuples(g, gd, rank, size)

        env = {k: os.environ.pop(k, None) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SGO_CONF_JSON", "SGO_RDZV_PORT")}
        try:
            with _patched((distributed, "init_from_env", init), (dist_selfplay, "_tuples_of", tuples),
                          (distributed, "broadcast_net", lambda net, src=0: {"identical": True})):
                return list(dist_selfplay.run_rank("gloo", **case["args"]))
        finally:
            if dist.is_initialized():
                dist.destroy_process_group()
            os.environ.update({k: v for k, v in env.items() if v is not None})
    return _run(case, tmp, body)


# Together the scripts hold: a failed slot that is refilled and one that cannot be; a zero-move game; steps where the per-step
# drain fires without turnover; steps with n_done <= idle and idle slots; more slots than games; only_game; max_steps cutting
# run_selfplay and run_rank short; sync_every not dividing the step count; a pre-existing game directory in every driver.
CASES = {
    # 7 reservable games on 3 slots: game 1 fails early (slot refilled), game 3 has no moves, game 7 fails when no number is
    # left (slot stays idle while games 5 and 6 go on: n_done == idle steps), game_00002 exists
    "selfplay_turnover": (run_selfplay_case, {
        "args": {"n_games": 8, "games_per_gpu": 3},
        "script": {0: (3, 1), 1: (1, -201), 3: (0, 1), 4: (2, 1), 5: (4, 1), 6: (6, 1), 7: (1, -201)},
        "existing": ["self_play_dir/best/game_00002"]}),
    "selfplay_more_slots_than_games": (run_selfplay_case, {
        "args": {"n_games": 2, "games_per_gpu": 5}, "script": {0: (3, 1), 1: (2, 1)}}),
    "selfplay_only_game": (run_selfplay_case, {
        "args": {"n_games": 6, "games_per_gpu": 4, "only_game": 3}, "script": {3: (3, 1)}}),
    "selfplay_only_game_taken": (run_selfplay_case, {
        "args": {"n_games": 6, "games_per_gpu": 4, "only_game": 3}, "existing": ["self_play_dir/best/game_00003"]}),
    "selfplay_max_steps": (run_selfplay_case, {
        "args": {"n_games": 6, "games_per_gpu": 2, "max_steps": 3}, "script": {0: (2, 1), 1: (5, 1), 2: (5, 1)}}),
    "evaluation_turnover": (run_evaluation_case, {
        "args": {"n_games": 7, "games_per_gpu": 3},
        "script": {0: (2, 1), 2: (1, -201), 3: (4, 1), 4: (0, 1), 5: (6, 1), 6: (2, -202)},
        "existing": ["eval_dir/latest/game_001"]}),
    "evaluation_more_slots_than_games": (run_evaluation_case, {
        "args": {"n_games": 2, "games_per_gpu": 4}, "script": {0: (1, 1), 1: (3, 1)}, "conf": {"COMPAT_WINNER_MODEL": False}}),
    "rank_turnover": (run_rank_case, {
        "args": {"sync_every": 3}, "conf": {"N_GAMES": 8, "GAMES_PER_GPU": 3},
        "script": {0: (3, 1), 1: (1, -201), 3: (0, 1), 4: (2, 1), 5: (4, 1), 6: (5, 1), 7: (1, -201)},
        "existing": ["self_play_dir/best/game_00002"], "unnamed": [0, 1, 3, 4, 5, 6, 7]}),
    "rank_max_steps": (run_rank_case, {
        "args": {"sync_every": 3, "max_steps": 4}, "conf": {"N_GAMES": 6, "GAMES_PER_GPU": 2},
        "script": {0: (2, 1), 1: (6, 1), 2: (6, 1)}, "unnamed": [0, 1, 2, 3, 4, 5]}),
    "rank_more_slots_than_games": (run_rank_case, {
        "args": {"sync_every": 4}, "conf": {"N_GAMES": 2, "GAMES_PER_GPU": 5}, "script": {0: (3, 1), 1: (2, 1)},
        "unnamed": [0, 1]}),
}


def run_case(name, tmp):
    runner, case = CASES[name]
    return json.loads(json.dumps(runner(case, tmp)))       # the form the golden file holds (tuples are lists, keys strings)


if __name__ == "__main__":
    import subprocess
    import tempfile
    out = {"recorded_on": subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"]).decode().strip(), "cases": {}}
    for name in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            out["cases"][name] = run_case(name, tmp)
        print(name, "steps:", sum(1 for t in out["cases"][name]["trace"] if t[0] == "step"), "returned:", out["cases"][name]["returned"])
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
