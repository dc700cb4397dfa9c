"""The one loop that keeps an engine's game slots filled, behind selfplay_worker.run_selfplay, evaluate_worker.run_evaluation
and dist_selfplay.run_rank: step the engine, drain its move records, and whenever slots have finished or failed hand each to
the driver and restart the freed slots with the next game numbers in ONE batched start.  The engine is anything with
step / drain / results / records (engine.SelfPlayEngine, engine.DualEngine); what differs between the drivers comes in as
callables."""


class SlotLoop(object):
    def __init__(self, eng, n_slots, reserve, start, finished, failed, max_steps=None):
        """reserve() -> next game number or None (GameScheduler.reserve); start(slots, games): one batched engine start;
        finished(slot, game, result) / failed(slot, game, error): what the driver does with a slot whose game ended, before
        the slot's records are dropped."""
        self.eng, self.G, self.max_steps = eng, n_slots, max_steps
        self.reserve, self.start, self.finished, self.failed = reserve, start, finished, failed
        self.slot_game = {}      # slot -> game number of the game it plays
        self.steps = 0
        self.active = self._fill(range(n_slots))
        self.idle = n_slots - self.active      # finished slots that could not be refilled (no game numbers left)
        self.playing = self.active > 0

    def _fill(self, slots):
        start, games = [], []
        for s in slots:
            g = self.reserve()
            if g is None:
                continue
            self.slot_game[s] = g
            start.append(s)
            games.append(g)
        if start:
            self.start(start, games)
        return len(start)

    def advance(self):
        """One engine step; the records are drained once there is a slot's worth of them."""
        st = self.eng.step()
        self.steps += 1
        if st.n_records >= self.G:
            self.eng.drain()
        return st

    def turn_over(self, st):
        """After advance(): ended slots to the driver, freed slots restarted.  Returns whether any slot had ended."""
        eng = self.eng
        turned = st.n_done > self.idle or bool(st.error and st.error_game in self.slot_game)
        if turned:
            eng.drain()
            res = eng.results()
            free = []
            for s in list(self.slot_game):
                done = res[s]["done"]
                if done == 0:
                    continue
                g = self.slot_game.pop(s)
                if done < 0:
                    self.failed(s, g, done)
                else:
                    self.finished(s, g, res[s])
                eng.records[s] = []        # the finished game owns its move list now
                free.append(s)
            refilled = self._fill(free)
            self.active += refilled - len(free)
            self.idle += len(free) - refilled
        self.playing = self.active > 0 and (self.max_steps is None or self.steps < self.max_steps)
        return turned

    def step(self):
        return self.turn_over(self.advance())

    def run(self):
        while self.playing:
            self.step()
