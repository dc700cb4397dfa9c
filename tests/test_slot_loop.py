"""The slot-turnover loop (sejonggo_amd/_slot_loop.py) under its three drivers, on CPU: run_selfplay, run_evaluation and
run_rank against the scripted engine of tests/fake_engine.py must reproduce tests/golden/slot_loop_traces.json -- every engine
call with its arguments, the return values, the directories on disk, the games handed to the savers and the failure messages --
as recorded from the three separate loops these drivers had before (the file's "recorded_on" commit).  And the one builder of
the game-result fields against what the three earlier builders returned."""
import json

import numpy as np
import pytest

from tests import fake_engine

with open(fake_engine.GOLDEN) as _f:
    TRACES = json.load(_f)["cases"]


def test_the_fixture_holds_every_required_situation():
    """What review asks of the scripts, checked on the recorded traces themselves."""
    assert sorted(TRACES) == sorted(fake_engine.CASES)

    def steps_of(trace):
        """(status, slots without a game before the step, did results() follow before the next step) for every step"""
        out, owned, G = [], set(), trace[0][1]["n_games"]
        for i, t in enumerate(trace):
            if t[0].startswith("start"):
                owned |= set(t[1])
            elif t[0] == "step":
                after = [u[0] for u in trace[i + 1:]]
                after = after[:after.index("step")] if "step" in after else after
                out.append((t[1], G - len(owned), "results" in after))
            elif t[0] == "results":
                owned -= {s for s, d in enumerate(t[1]) if d != 0}
        return out

    for driver in ("selfplay", "evaluation", "rank"):
        main = TRACES[driver + "_turnover"]
        msgs, tr = main["messages"], main["trace"]
        assert len(msgs) == 2                                                      # two failed slots ...
        starts = [t for t in tr if t[0].startswith("start")]
        assert len(starts) == 3                                                    # ... the first refilled, the last not
        steps = steps_of(tr)
        assert any(st["n_records"] >= tr[0][1]["n_games"] and not turned for st, idle, turned in steps)   # drain alone
        assert any(idle > 0 and 0 < st["n_done"] <= idle and not turned for st, idle, turned in steps)    # idle, no turnover
        assert any(d.endswith("game_00002") or d.endswith("game_001") for v in main["dirs"].values() for d in v)  # pre-existing
        small = TRACES[driver + "_more_slots_than_games"]["trace"]
        assert small[0][1]["n_games"] == 2                                         # G clamped to the games there are
    assert [s[1] for s in TRACES["selfplay_turnover"]["saved"]].count(0) == 0      # the zero-move game is not saved ...
    assert "best/game_00003" not in TRACES["selfplay_turnover"]["dirs"]["self_play_dir"]       # ... and gives its directory back
    assert TRACES["selfplay_only_game"]["trace"][1][3] == [3] and TRACES["selfplay_only_game"]["trace"][0][1]["n_games"] == 1
    assert TRACES["selfplay_max_steps"]["returned"]["steps"] == 3 and TRACES["selfplay_max_steps"]["trace"][-2][0] != "results"
    n_steps = sum(1 for t in TRACES["rank_max_steps"]["trace"] if t[0] == "step")
    assert n_steps == 4 and n_steps % fake_engine.CASES["rank_max_steps"][1]["args"]["sync_every"] != 0
    assert sum(1 for t in TRACES["rank_turnover"]["trace"] if t[0] == "step") % 3 != 0


@pytest.mark.parametrize("name", sorted(fake_engine.CASES))
def test_driver_reproduces_the_recorded_run(name, tmp_path):
    got, want = fake_engine.run_case(name, str(tmp_path)), TRACES[name]
    assert sorted(got) == sorted(want)
    for key in ("returned", "saved", "dirs", "messages"):
        assert got[key] == want[key], key
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, "call %d" % i
    assert len(got["trace"]) == len(want["trace"])


# ------------------------------------------------------------------------------------------------ the game-result fields
# (winner, end reason, last player, black points, white points, nameB, nameW, black is model 1, COMPAT_WINNER_MODEL) -> what the
# builders before _game_loop.game_result_fields returned for it: SelfPlayEngine.game_data for one name, the two-model
# SelfPlayEngine._eval_game_data (the reference's asynchronous winner rule) for two.  With the rule switched off that is
# `nameB if black won else nameW`, which is also what play_loop's tail computed for the synchronous path.
RESULT_FIELDS = [
    ((1, 'PLAYED ALL MOVES', -1, 12, 7.5, 'a', 'a', True, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((1, 'PLAYED ALL MOVES', -1, 12, 7.5, 'a', 'a', True, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((1, 'PLAYED ALL MOVES', -1, 12, 7.5, 'a', 'a', False, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((1, 'PLAYED ALL MOVES', -1, 12, 7.5, 'a', 'a', False, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((1, 'resign', 1, 12, 7.5, 'a', 'a', True, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((1, 'resign', 1, 12, 7.5, 'a', 'a', True, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((1, 'resign', 1, 12, 7.5, 'a', 'a', False, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((1, 'resign', 1, 12, 7.5, 'a', 'a', False, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((1, 'BOTH_PASSED', -1, 12, 7.5, 'a', 'a', True, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'BOTH_PASSED'}),
    ((1, 'BOTH_PASSED', -1, 12, 7.5, 'a', 'a', True, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'BOTH_PASSED'}),
    ((1, 'BOTH_PASSED', -1, 12, 7.5, 'a', 'a', False, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'BOTH_PASSED'}),
    ((1, 'BOTH_PASSED', -1, 12, 7.5, 'a', 'a', False, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'BOTH_PASSED'}),
    ((0, 'PLAYED ALL MOVES', 1, 5, 5.0, 'a', 'a', True, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'PLAYED ALL MOVES'}),
    ((0, 'PLAYED ALL MOVES', 1, 5, 5.0, 'a', 'a', True, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'PLAYED ALL MOVES'}),
    ((0, 'PLAYED ALL MOVES', 1, 5, 5.0, 'a', 'a', False, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'PLAYED ALL MOVES'}),
    ((0, 'PLAYED ALL MOVES', 1, 5, 5.0, 'a', 'a', False, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'PLAYED ALL MOVES'}),
    ((0, 'resign', -1, 5, 5.0, 'a', 'a', True, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'W+R', 'end_reason': 'resign'}),
    ((0, 'resign', -1, 5, 5.0, 'a', 'a', True, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'W+R', 'end_reason': 'resign'}),
    ((0, 'resign', -1, 5, 5.0, 'a', 'a', False, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'W+R', 'end_reason': 'resign'}),
    ((0, 'resign', -1, 5, 5.0, 'a', 'a', False, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'W+R', 'end_reason': 'resign'}),
    ((0, 'BOTH_PASSED', 1, 5, 5.0, 'a', 'a', True, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'BOTH_PASSED'}),
    ((0, 'BOTH_PASSED', 1, 5, 5.0, 'a', 'a', True, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'BOTH_PASSED'}),
    ((0, 'BOTH_PASSED', 1, 5, 5.0, 'a', 'a', False, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'BOTH_PASSED'}),
    ((0, 'BOTH_PASSED', 1, 5, 5.0, 'a', 'a', False, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'BOTH_PASSED'}),
    ((-1, 'PLAYED ALL MOVES', -1, 3, 9.5, 'a', 'a', True, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((-1, 'PLAYED ALL MOVES', -1, 3, 9.5, 'a', 'a', True, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((-1, 'PLAYED ALL MOVES', -1, 3, 9.5, 'a', 'a', False, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((-1, 'PLAYED ALL MOVES', -1, 3, 9.5, 'a', 'a', False, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((-1, 'resign', 1, 3, 9.5, 'a', 'a', True, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((-1, 'resign', 1, 3, 9.5, 'a', 'a', True, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((-1, 'resign', 1, 3, 9.5, 'a', 'a', False, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((-1, 'resign', 1, 3, 9.5, 'a', 'a', False, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((-1, 'BOTH_PASSED', -1, 3, 9.5, 'a', 'a', True, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'BOTH_PASSED'}),
    ((-1, 'BOTH_PASSED', -1, 3, 9.5, 'a', 'a', True, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'BOTH_PASSED'}),
    ((-1, 'BOTH_PASSED', -1, 3, 9.5, 'a', 'a', False, True), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'BOTH_PASSED'}),
    ((-1, 'BOTH_PASSED', -1, 3, 9.5, 'a', 'a', False, False), {'modelB_name': 'a', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'BOTH_PASSED'}),
    ((1, 'PLAYED ALL MOVES', -1, 12, 7.5, 'a', 'b', True, True), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((1, 'PLAYED ALL MOVES', -1, 12, 7.5, 'a', 'b', True, False), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((1, 'PLAYED ALL MOVES', -1, 12, 7.5, 'b', 'a', False, True), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((1, 'PLAYED ALL MOVES', -1, 12, 7.5, 'b', 'a', False, False), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'b', 'result': 'B+4.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((1, 'resign', 1, 12, 7.5, 'a', 'b', True, True), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 1, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((1, 'resign', 1, 12, 7.5, 'a', 'b', True, False), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 1, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((1, 'resign', 1, 12, 7.5, 'b', 'a', False, True), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((1, 'resign', 1, 12, 7.5, 'b', 'a', False, False), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'b', 'result': 'B+R', 'end_reason': 'resign'}),
    ((1, 'BOTH_PASSED', -1, 12, 7.5, 'a', 'b', True, True), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'BOTH_PASSED'}),
    ((1, 'BOTH_PASSED', -1, 12, 7.5, 'a', 'b', True, False), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'BOTH_PASSED'}),
    ((1, 'BOTH_PASSED', -1, 12, 7.5, 'b', 'a', False, True), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'a', 'result': 'B+4.5', 'end_reason': 'BOTH_PASSED'}),
    ((1, 'BOTH_PASSED', -1, 12, 7.5, 'b', 'a', False, False), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 1, 'winner_model': 'b', 'result': 'B+4.5', 'end_reason': 'BOTH_PASSED'}),
    ((0, 'PLAYED ALL MOVES', 1, 5, 5.0, 'a', 'b', True, True), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'PLAYED ALL MOVES'}),
    ((0, 'PLAYED ALL MOVES', 1, 5, 5.0, 'a', 'b', True, False), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'PLAYED ALL MOVES'}),
    ((0, 'PLAYED ALL MOVES', 1, 5, 5.0, 'b', 'a', False, True), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'PLAYED ALL MOVES'}),
    ((0, 'PLAYED ALL MOVES', 1, 5, 5.0, 'b', 'a', False, False), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'PLAYED ALL MOVES'}),
    ((0, 'resign', -1, 5, 5.0, 'a', 'b', True, True), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': None, 'winner_model': None, 'result': 'W+R', 'end_reason': 'resign'}),
    ((0, 'resign', -1, 5, 5.0, 'a', 'b', True, False), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': None, 'winner_model': None, 'result': 'W+R', 'end_reason': 'resign'}),
    ((0, 'resign', -1, 5, 5.0, 'b', 'a', False, True), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'W+R', 'end_reason': 'resign'}),
    ((0, 'resign', -1, 5, 5.0, 'b', 'a', False, False), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'W+R', 'end_reason': 'resign'}),
    ((0, 'BOTH_PASSED', 1, 5, 5.0, 'a', 'b', True, True), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'BOTH_PASSED'}),
    ((0, 'BOTH_PASSED', 1, 5, 5.0, 'a', 'b', True, False), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'BOTH_PASSED'}),
    ((0, 'BOTH_PASSED', 1, 5, 5.0, 'b', 'a', False, True), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'BOTH_PASSED'}),
    ((0, 'BOTH_PASSED', 1, 5, 5.0, 'b', 'a', False, False), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': None, 'winner_model': None, 'result': 'D+0.0', 'end_reason': 'BOTH_PASSED'}),
    ((-1, 'PLAYED ALL MOVES', -1, 3, 9.5, 'a', 'b', True, True), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 0, 'winner_model': 'b', 'result': 'W+6.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((-1, 'PLAYED ALL MOVES', -1, 3, 9.5, 'a', 'b', True, False), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 0, 'winner_model': 'b', 'result': 'W+6.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((-1, 'PLAYED ALL MOVES', -1, 3, 9.5, 'b', 'a', False, True), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'b', 'result': 'W+6.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((-1, 'PLAYED ALL MOVES', -1, 3, 9.5, 'b', 'a', False, False), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'PLAYED ALL MOVES'}),
    ((-1, 'resign', 1, 3, 9.5, 'a', 'b', True, True), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 0, 'winner_model': 'b', 'result': 'B+R', 'end_reason': 'resign'}),
    ((-1, 'resign', 1, 3, 9.5, 'a', 'b', True, False), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 0, 'winner_model': 'b', 'result': 'B+R', 'end_reason': 'resign'}),
    ((-1, 'resign', 1, 3, 9.5, 'b', 'a', False, True), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'b', 'result': 'B+R', 'end_reason': 'resign'}),
    ((-1, 'resign', 1, 3, 9.5, 'b', 'a', False, False), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'B+R', 'end_reason': 'resign'}),
    ((-1, 'BOTH_PASSED', -1, 3, 9.5, 'a', 'b', True, True), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 0, 'winner_model': 'b', 'result': 'W+6.5', 'end_reason': 'BOTH_PASSED'}),
    ((-1, 'BOTH_PASSED', -1, 3, 9.5, 'a', 'b', True, False), {'modelB_name': 'a', 'modelW_name': 'b', 'winner': 0, 'winner_model': 'b', 'result': 'W+6.5', 'end_reason': 'BOTH_PASSED'}),
    ((-1, 'BOTH_PASSED', -1, 3, 9.5, 'b', 'a', False, True), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'b', 'result': 'W+6.5', 'end_reason': 'BOTH_PASSED'}),
    ((-1, 'BOTH_PASSED', -1, 3, 9.5, 'b', 'a', False, False), {'modelB_name': 'b', 'modelW_name': 'a', 'winner': 0, 'winner_model': 'a', 'result': 'W+6.5', 'end_reason': 'BOTH_PASSED'}),
]


@pytest.mark.parametrize("async_rule", [True, False])
def test_game_result_fields_are_what_the_three_builders_returned(async_rule):
    from sejonggo_amd._game_loop import game_result_fields
    from sejonggo_amd.conf import conf
    assert len(RESULT_FIELDS) == 3 * 3 * 2 * 2 * 2
    old = conf.get('COMPAT_WINNER_MODEL', True)
    try:
        for args, want in RESULT_FIELDS:
            conf['COMPAT_WINNER_MODEL'] = args[-1]
            if not async_rule:         # the synchronous rule never looks at COMPAT_WINNER_MODEL: the entry with it switched off
                want = dict(RESULT_FIELDS)[args[:-1] + (False,)]
            got = game_result_fields(*args[:-1], async_winner_rule=async_rule)
            assert got == want and list(got) == list(want), args
            assert [type(v) for v in got.values()] == [type(v) for v in want.values()], args
    finally:
        conf['COMPAT_WINNER_MODEL'] = old


def _engine(two_model):
    eng = type("FakeEngine", (fake_engine.FakeEngine,), {"trace": []})(
        fake_engine._Net("a"), n_games=1, size=5, net2=fake_engine._Net("a") if two_model else None)
    eng.records[0], eng.game_ids[0] = [], 7
    return eng


def test_engine_game_data_key_sets_and_one_model_equals_two_equal_names():
    """SelfPlayEngine.game_data: the common fields and each form's extras, with today's types; for every result a self-play
    engine can produce, the one-model form and the two-model form with equal names agree on the common keys."""
    from sejonggo_amd import _lib
    from sejonggo_amd.engine import END_REASONS
    common = ['moves', 'modelB_name', 'modelW_name', 'winner', 'winner_model', 'result', 'end_reason', 'resign_model1', 'resign_model2',
              'black_points', 'white_points', 'slot', 'id']
    one, two = _engine(False), _engine(True)
    for winner, (black, white) in ((1, (12, 7.5)), (0, (5, 5.0)), (-1, (3, 9.5))):
        for reason in END_REASONS:
            for last in (1, -1):
                r = np.zeros(1, dtype=_lib.GAME_RESULT_DTYPE)[0]
                r["winner"], r["end_reason"], r["last_player"], r["black"], r["white"] = winner, reason, last, black, white
                r["done"], r["first_model"], r["blocks_high_water"] = 1, 0, 33        # a self-play engine has no first_model
                g1, g2 = one.game_data(0, r, "a"), two.game_data(0, r)
                assert sorted(g1) == sorted(common + ['blocks_high_water']) and sorted(g2) == sorted(common + ['first_model'])
                assert {k: g1[k] for k in common} == {k: g2[k] for k in common}
                assert g1['moves'] is one.records[0] and g1['resign_model1'] is None and g1['resign_model2'] is None
                assert (type(g1['black_points']), type(g1['white_points']), type(g1['slot']), g1['id']) == (int, float, int, 7)
                assert (g1['blocks_high_water'], type(g1['blocks_high_water']), g2['first_model'], type(g2['first_model'])) == (33, int, 0, int)
                assert g1['result'] == ("%s+R" % "BDW"[1 - last] if reason == 1 else "%s+%s" % ("BDW"[1 - winner], abs(black - white)))


# ------------------------------------------------------------------------------------------------ the reservation rule
def test_game_scheduler_root_pattern_candidates_and_skip_only(tmp_path):
    """What evaluation and the ranks need of GameScheduler beyond test_host_logic's two tests: another directory pattern, an
    explicit sequence of candidates, and the ranks' resume rule -- skip what exists, create nothing."""
    import os
    from sejonggo_amd.selfplay_worker import GameScheduler
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "latest", "game_001"))
    ev = GameScheduler(root, "latest", 3, None, None, pattern="game_%03d")
    assert [ev.reserve() for _ in range(3)] == [0, 2, None]
    assert sorted(os.listdir(os.path.join(root, "latest"))) == ["game_000", "game_001", "game_002"]
    ev.discard(2)
    assert sorted(os.listdir(os.path.join(root, "latest"))) == ["game_000", "game_001"]
    os.makedirs(os.path.join(root, "m", "game_00005"))
    rk = GameScheduler(root, "m", 12, 0.1, 0.05, candidates=[1, 5, 9], create=False)
    assert [rk.reserve() for _ in range(3)] == [1, 9, None]
    assert os.listdir(os.path.join(root, "m")) == ["game_00005"]
