"""GTP front-end with the reference's engine classes (sejonggo_nomodel.py:20-185): SejongGoEngine (play / genmove
on a persistent MCTS tree) and GTPEngine (name, version, protocol_version, list_commands, boardsize, komi, play,
genmove, clear_board, parse_command).  Single-game latency mode of the same path: the tree is a host dict tree
searched by nomodel_self_play.select_play (leaves of a round are evaluated in one batched forward pass), rules and
net run on the MI355X.  Parity: the move-coordinate text mapping is pinned by the tests; search results follow the
host async path, which is pinned by the reference's goldens."""
import string
import sys

import numpy as np

from . import __version__
from .conf import conf
from .nomodel_self_play import select_play
from .play import coord2index, game_init, index2coord, make_play, new_tree
from .predicting_queue_worker import destroy_predicting_workers, get_model, init_predicting_workers, put_predict_request

COLOR_TO_PLAYER = {'B': 1, 'W': -1, 'b': 1, 'w': -1, 'black': 1, 'white': -1}


class SejongGoEngine(object):
    def __init__(self, mcts_simulations, board, resign=None, temperature=0, add_noise=False, process_id=0):
        self.mcts_simulations = mcts_simulations
        self.resign = resign
        self.temperature = temperature
        self.board = board
        self.add_noise = add_noise
        self.mcts_tree = None
        self.move = 1
        self.process_id = process_id
        self.player = board[0, 0, 0, -1]
        self.model_indicator = "BEST"
        init_predicting_workers(conf['GPUs'][:1])

    @property
    def model(self):
        return get_model(self.model_indicator)

    def close(self):
        destroy_predicting_workers(conf['GPUs'][:1])

    def set_temperature(self, temperature):
        self.temperature = temperature

    def play(self, color, x, y, update_tree=True):
        size = self.board.shape[-2]
        index = coord2index(x, y, size)
        if update_tree:
            if self.mcts_tree and index in self.mcts_tree['subtree']:
                self.mcts_tree = self.mcts_tree['subtree'][index]
                self.mcts_tree['parent'] = None
            else:
                self.mcts_tree = None
        self.board, self.player = make_play(x, y, self.board, color)
        self.move += 1
        return self.board, self.player

    def genmove(self, color):
        size = self.board.shape[-2]
        policy, value = put_predict_request(self.model_indicator, self.board, response_now=True)
        if self.resign and value <= self.resign:
            return 0, size + 1, policy, value, self.board, self.player
        if not self.mcts_tree or not self.mcts_tree['subtree']:
            self.mcts_tree = new_tree(policy, self.board, add_noise=self.add_noise)
        keep = conf['MCTS_SIMULATIONS']
        conf['MCTS_SIMULATIONS'] = self.mcts_simulations
        try:
            index = select_play(self.board, conf['ENERGY'], self.mcts_tree, self.temperature, self.model_indicator, self.process_id)
        finally:
            conf['MCTS_SIMULATIONS'] = keep
        x, y = index2coord(index, size)
        policy_target = np.zeros(size * size + 1)
        for a, child in self.mcts_tree['subtree'].items():
            policy_target[a] = child['p']
        self.board, self.player = self.play(color, x, y)
        return x, y, policy_target, value, self.board, self.player

    def analyze(self, sims=None):
        """Search without moving, the comparator of the device engine's sgo_session_analyze: genmove's root prediction
        (:60), no resign test, new_tree when there is no tree (:63-64), select_play's simulation loop for `sims` simulations
        (None: mcts_simulations) with the chosen move discarded.  Board and move stay; the searched tree is kept.  Returns
        (policy, value) of the root prediction."""
        policy, value = put_predict_request(self.model_indicator, self.board, response_now=True)
        if not self.mcts_tree or not self.mcts_tree['subtree']:
            self.mcts_tree = new_tree(policy, self.board, add_noise=self.add_noise)
        keep = conf['MCTS_SIMULATIONS']
        conf['MCTS_SIMULATIONS'] = sims or self.mcts_simulations
        try:
            select_play(self.board, conf['ENERGY'], self.mcts_tree, 0, self.model_indicator, self.process_id)
        finally:
            conf['MCTS_SIMULATIONS'] = keep
        return policy, value


class DeviceSejongGoEngine(object):
    """SejongGoEngine on the device engine: the game is a session slot of an engine.SessionEngine (tree, rules and search on
    the GPU), with the attribute surface GTPEngine drives -- play, genmove, board, player (who moved last, as make_play returns
    it), move, mcts_tree, model, close.
    `engine` / `slot` put it on a slot of an existing SessionEngine (many games in one context); otherwise it owns a context
    of one game (engine_kw go to SessionEngine).  Temperature 0 and no noise only: the host engine remains for the rest.
    One deviation from the reference: a `play` with an out-of-turn colour drops the tree (include/sgo.h).
    `moves` is the list of (action, colour) since clear_board -- external plays and generated moves, not resigns -- from which
    `undo` and `load` set the slot up again in one launch (engine.SessionEngine.setup); `analyze` searches without moving."""

    def __init__(self, mcts_simulations, board=None, resign=None, temperature=0, add_noise=False, net=None, engine=None, slot=0,
                 **engine_kw):
        if temperature != 0 or add_noise:
            raise ValueError("DeviceSejongGoEngine plays at temperature 0 without noise; use SejongGoEngine for the rest")
        if board is not None and np.any(np.asarray(board)[..., :16]):
            raise ValueError("DeviceSejongGoEngine starts from the empty board")
        self.mcts_simulations = mcts_simulations
        self.resign = resign
        self.temperature = 0
        self.add_noise = False
        self.move = 1
        self.player = 1                     # as the reference keeps it: the board's colour plane at first, then who moved last
        self.slot = int(slot)
        self._own = engine is None
        self._workers = False
        if engine is None:
            from .engine import SessionEngine
            if net is None:
                init_predicting_workers(conf['GPUs'][:1])
                self._workers = True
                net = get_model("BEST")
            engine_kw.setdefault("n_games", 1)
            engine = SessionEngine(net, sims=mcts_simulations, **engine_kw)
        self.engine = engine
        self.size = engine.S
        self.moves = []
        self.n_setup = 0                    # leading entries of `moves` that are set-up stones of a loaded record: undo stops there
        self.engine.open([self.slot], resign=resign)

    @property
    def model(self):
        return self.engine.net

    @property
    def board(self):
        return self.engine.board(self.slot)

    @board.setter
    def board(self, board):
        # GTPEngine.clear_board assigns the empty board, then mcts_tree = None and move = 1
        if np.any(np.asarray(board)[..., :16]):
            raise ValueError("a session starts from the empty board")
        self.engine.open([self.slot], resign=self.resign)
        self.player = 1
        self.moves, self.n_setup = [], 0

    @property
    def mcts_tree(self):
        """The device tree as the reference's nested dicts (engine.tree_dict); its subtree is empty while the root is unexpanded."""
        return self.engine.tree_dict(self.slot)

    @mcts_tree.setter
    def mcts_tree(self, tree):
        if tree is not None or self.engine.tree_dict(self.slot)['subtree']:
            raise ValueError("the device tree is dropped by clear_board only")

    def close(self):
        if getattr(self, "_game_records", None) is not None:
            self._game_records.close()
            self._game_records = None
        if self._own and self.engine is not None:
            self.engine.close()
            if self._workers:
                destroy_predicting_workers(conf['GPUs'][:1])
        self.engine = None

    def set_temperature(self, temperature):
        if temperature != 0:
            raise ValueError("DeviceSejongGoEngine plays at temperature 0")

    def play(self, color, x, y, update_tree=True):
        index = coord2index(x, y, self.size)
        status = int(self.engine.play([self.slot], [index], [color or 0])[0])
        if status:
            raise ValueError("play %s at (%d, %d) refused: %d (%s)" % (color, x, y, status, {
                -101: "the point is occupied", -102: "outside the board", -203: "the slot is not a holding session"}.get(status, "?")))
        self.move += 1
        self.moves.append((index, int(color or 0)))
        board = self.board
        self.player = -int(board[0, 0, 0, -1])           # make_play returns the player who moved (play.py:226-242)
        return board, self.player

    def genmove(self, color):
        board = self.board
        if color and color != int(board[0, 0, 0, -1]):
            raise ValueError("genmove for the side that is not to move: play the missing move (or a pass) first")
        action, value, policy = self.engine.genmove([self.slot])[0]
        if action < 0:
            return 0, self.size + 1, policy, value, board, self.player
        x, y = index2coord(action, self.size)
        self.move += 1
        self.moves.append((int(action), 0))
        self.player = int(board[0, 0, 0, -1])
        return x, y, policy, value, self.board, self.player

    def load(self, moves, colors=None, n_setup=0):
        """The slot is set to the empty board followed by `moves` (actions y * S + x, pass = S * S; colors: 0 / None = the side to
        move, +1 / -1 explicit -- an out-of-turn colour places set-up and handicap stones) in one launch; the tree is dropped.
        A refused list (an occupied point, an action off the board) raises ValueError and leaves the game as it was.
        n_setup: the first n_setup entries are set-up stones (AB / AW of a record), which `undo` does not take back."""
        moves = [int(a) for a in moves]
        colors = [0] * len(moves) if colors is None else [int(c or 0) for c in colors]
        status, fail_at = self.engine.setup([self.slot], [moves], [colors])
        if int(status[0]):
            raise ValueError("move list refused at index %d: %d" % (int(fail_at[0]), int(status[0])))
        self.moves, self.n_setup = list(zip(moves, colors)), int(n_setup)
        self.move = 1 + len(moves)
        board = self.board
        self.player = -int(board[0, 0, 0, -1]) if moves else 1
        return board, self.player

    def undo(self):
        """GTP undo: a set-up of the move list without its last entry (a resign is no entry).  ValueError when the list is empty."""
        if len(self.moves) <= self.n_setup:
            raise ValueError("cannot undo")
        return self.load([a for a, _ in self.moves[:-1]], [c for _, c in self.moves[:-1]], n_setup=self.n_setup)

    def analyze(self, sims=None):
        """Search without moving (engine.SessionEngine.analyze): the tree is kept, a second call deepens it.  Returns (policy,
        value): the root's prior row as a genmove would record it and the net's value; `report` reads the search."""
        _, value, policy = self.engine.analyze([self.slot], sims)[0]
        return policy, value

    def report(self, top=5, depth=8):
        """engine.SessionEngine.report for this game: a dict of arrays with one row."""
        return self.engine.report([self.slot], top=top, depth=depth)

    @staticmethod
    def _held(v):
        """v, the one-row result of a session analysis (or its status array), where the slot is a holding session"""
        if int(getattr(v, "status", v)[0]):
            raise ValueError("the slot is not a holding session")
        return v

    def keys(self):
        """(canon, mask) of the position on the board (engine.SessionEngine.keys): what records.Book.moves takes."""
        k = self.engine.keys([self.slot])
        self._held(k["status"])
        return int(k["canon"][0]), int(k["mask"][0])

    def tactics(self):
        """The chains with one or two liberties of the position on the board, read out (engine.SessionEngine.tactics): a list of
        tactics.Chain in ascending anchor order."""
        return self._held(self.engine.tactics([self.slot])).chains_of(0)

    def life(self):
        """Unconditional life of the position on the board (engine.SessionEngine.life): a life.Life with one row."""
        return self._held(self.engine.life([self.slot]))

    def influence(self, dead="life", **params):
        """Bouzy's influence map of the position on the board (engine.SessionEngine.influence): (an influence.Influence with one
        row, the stones int8 [S * S], +1 black).  dead "life": proved-dead stones are lifted first; None: none are."""
        from .rollout import real_board
        v = self._held(self.engine.influence([self.slot], dead=dead, **params))
        return v, np.asarray(real_board(self.board), dtype=np.int8).reshape(-1)

    def shapes(self, shape):
        """Where a shapes.Shape occurs in the position on the board (engine.SessionEngine.shapes): a shapes.Shapes with one row."""
        return self._held(self.engine.shapes([self.slot], shape))

    def move_outcomes(self, side=0):
        """What one ply on every point of the position on the board would do (engine.SessionEngine.moves): a moves.Moves with one
        row.  side 0: the side to move, 1: the other colour.  (`moves` is this engine's move list.)"""
        return self._held(self.engine.moves([self.slot], side))

    def secure(self, side=0):
        """What one more stone on every empty point of the position on the board makes pass-alive (engine.SessionEngine.secure):
        (a secure.Secure with one row, the stones int8 [S * S], +1 black).  side 0: the side to move, 1: the other colour."""
        from .rollout import real_board
        v = self._held(self.engine.secure([self.slot], side))
        return v, np.asarray(real_board(self.board), dtype=np.int8).reshape(-1)

    def solve(self, ask=None, region=None, rules=1, max_nodes=4096, max_region=12):
        """Life and death in the position on the board (engine.SessionEngine.solve): (a solve.Solve with one row, the stones int8
        [S * S], +1 black).  ask None: every enclosed chain; else the chain on that point, read in `region` (a list of points)
        when given."""
        from .rollout import real_board
        from .solve import region_words
        v = self._held(self.engine.solve([self.slot], None if ask is None else [ask], None if region is None else region_words(self.size, region)[None],
                                         rules=rules, max_region=max_region, max_nodes=max_nodes))
        return v, np.asarray(real_board(self.board), dtype=np.int8).reshape(-1)

    def race(self, ask=None, rules=1, max_libs=4, max_nodes=1024, max_region=8):
        """Capturing races in the position on the board (engine.SessionEngine.race): a race.Race with one row.  ask None: every
        pair in contact; else the pair on those two points."""
        return self._held(self.engine.race([self.slot], None if ask is None else [ask], None, rules=rules, max_libs=max_libs,
                                           max_region=max_region, max_nodes=max_nodes))

    def connect(self, ask=None, rules=1, cut_libs=1, max_nodes=1024, max_region=8):
        """Connections in the position on the board (engine.SessionEngine.connect): (a connect.Connect with one row, the stones int8
        [S * S], +1 black).  ask None: every near pair; else the pair on those two points."""
        from .rollout import real_board
        v = self._held(self.engine.connect([self.slot], None if ask is None else [ask], None, rules=rules, cut_libs=cut_libs,
                                           max_region=max_region, max_nodes=max_nodes))
        return v, np.asarray(real_board(self.board), dtype=np.int8).reshape(-1)

    def superko(self, rule=0):
        """Which moves of the side to move would repeat an earlier position of THIS game (include/sgo.h "superko"): a
        superko.Superko with one row.  A session slot holds seven positions of history, not the game, so the move list is replayed
        into a records object of one game (created at the first call, sgo_records_replay) and the analysis runs on its last record
        with the whole game as history.  rule 0 / "positional", 1 / "situational"."""
        from .records import DeviceRecords, max_entries_of
        from .superko import Superko, rule_of
        rule = rule_of(rule)
        if getattr(self, "_game_records", None) is None:
            self._game_records = DeviceRecords(self.size, 1, max_entries_of(self.size), self.engine.device.index or 0)
        rec, n = self._game_records, len(self.moves)
        status, fail_at = rec.replay([n], [0], [a for a, _ in self.moves], [c for _, c in self.moves])
        if int(status[0]):
            raise ValueError("the move list does not replay: entry %d refused (%d)" % (int(fail_at[0]), int(status[0])))
        sets, back, counts = rec.superko([n], [0], rule, n + 1)
        return Superko(self.size, sets.cpu().numpy().view(np.uint32), back.cpu().numpy(), counts.cpu().numpy())

    def playouts(self, per_row=None, rules=1, seed=0):
        """How the game ends from here by light playouts (engine.SessionEngine.playouts; include/sgo.h "light playouts"): the
        position played out per_row times (None: playout.DEFAULT_PER_ROW) with uniformly random moves that spare the mover's eyes
        -- no net is asked.  Returns (a playout.Playouts with one row, the stones int8 [S, S], +1 black); board, tree and move
        number stay.  The answer is kept until the position changes.  An ESTIMATE, not a proof."""
        from .playout import DEFAULT_PER_ROW
        from .rollout import real_board
        key = (tuple(self.moves), per_row, rules, seed)
        if getattr(self, "_playout_cache", (None,))[0] != key:
            board = self.board
            v = self._held(self.engine.playouts([self.slot], per_row=int(per_row or DEFAULT_PER_ROW), seed=seed, rules=rules))
            v.white_to_play = np.array([int(board[0, 0, 0, -1]) == -1])
            self._playout_cache = (key, v, real_board(board))
        return self._playout_cache[1], self._playout_cache[2]

    def uct(self, trees=None, sims=None, komi=0.0, seed=0, rules=1):
        """Which move, by playout tree search (engine.SessionEngine.uct; include/sgo.h "playout tree search"): `trees` searches of
        `sims` simulations each from the position on the board (None: the untuned defaults of uct.py) -- no net is asked.  Returns a
        uct.Search with one row; board, tree and move number stay.  An ESTIMATE, not a proof."""
        v = self._held(self.engine.uct([self.slot], trees=trees, sims=sims, seed=seed, rules=rules, komi=komi))
        v.white_to_play = np.array([int(self.board[0, 0, 0, -1]) == -1])
        return v

    def legal(self):
        """bool [S * S + 1]: the legal set of the position on the board (play.legal_moves flags the illegal ones)."""
        from .play import legal_moves
        return np.asarray(legal_moves(self.board)).reshape(-1) == 0

    def rollouts(self, per_src=None, seed=0):
        """How the game ends from here: the position played out per_src times (None: conf['ROLLOUTS']) with the net's policy
        (engine.SessionEngine.rollouts).  Returns this game's row of counts (rollout.result_row) and the stones on the board
        (int8 [S, S], +1 black); board, tree and move number stay.  The answer is kept until the position changes."""
        from .rollout import real_board, result_row
        key = (tuple(self.moves), per_src, seed)
        if getattr(self, "_rollout_cache", (None,))[0] != key:
            row = result_row(self.engine.rollouts([self.slot], per_src=per_src, seed=seed), 0)
            self._rollout_cache = (key, row, real_board(self.board))
        return self._rollout_cache[1], self._rollout_cache[2]


class GTPFailure(Exception):
    """A command that GTP answers with `? message` (undo on an empty game, a command the engine behind cannot serve)."""


class GTPEngine(object):
    def __init__(self, engine=None, book=None, book_min=1, superko=None, score=None, player="net", uct_trees=None, uct_sims=None):
        """player: "net" (default: genmove is the net's tree search, as ever) or "uct": genmove plays the best move of the playout
        tree search (include/sgo.h "playout tree search"; uct_trees / uct_sims, None: the untuned defaults of uct.py), which asks
        no net -- the device engine may stand on a stub net then, `score` defaults to "playouts", and every command that would call
        the net answers a failure that says so; device engine only.
        score: "rollouts" (default: final_score, final_status_list and sgo-ownership stand on policy rollouts, as ever) or
        "playouts" (they stand on light playouts, which ask no net); device engine only.
        book: a records.Book (or the path of its .npz) genmove answers from while it holds a legal move played at least
        book_min times; it needs the device engine (position keys come from the session slot).
        superko: None, or "positional" / "situational" (0 / 1): `play` refuses a move that repeats an earlier position of the game
        and genmove never makes one; it needs the device engine too (the move list is replayed on the device)."""
        self._komi = 0
        if player not in ("net", "uct"):
            raise ValueError("player is 'net' or 'uct'")
        if player == "uct" and (engine is None or not hasattr(engine, "uct")):
            raise ValueError("--player uct needs the device engine (gtp --device)")
        self.player_kind, self.uct_trees, self.uct_sims = player, uct_trees, uct_sims
        if score is None:
            score = "playouts" if player == "uct" else "rollouts"
        if score not in ("rollouts", "playouts"):
            raise ValueError("score is 'rollouts' or 'playouts'")
        if score == "playouts" and (engine is None or not hasattr(engine, "playouts")):
            raise ValueError("--score playouts needs the device engine (gtp --device)")
        self.score = score
        self.superko_rule = None
        if superko is not None:
            from .superko import rule_of
            if engine is None or not hasattr(engine, "superko"):
                raise ValueError("superko needs the device engine (gtp --device)")
            self.superko_rule = rule_of(superko)
        self.book, self.book_min = None, int(book_min)
        if book is not None:
            if engine is None or not hasattr(engine, "keys"):
                raise ValueError("an opening book needs the device engine (gtp --device)")
            from .records import Book
            self.book = book if isinstance(book, Book) else Book.load(book)
            if self.book.size != conf['SIZE']:
                raise ValueError("the book is {0}x{0}, the configuration {1}x{1}".format(self.book.size, conf['SIZE']))
        self.size = conf['SIZE']
        self.board, self.player = game_init(self.size)
        self.sejong_engine = engine or SejongGoEngine(conf['MCTS_SIMULATIONS'], self.board)

    def name(self):
        return "SejongGo - {} - {} simulations".format(self.sejong_engine.model.name, conf['MCTS_SIMULATIONS'])

    def version(self):
        return __version__

    def protocol_version(self):
        return "2"

    def list_commands(self):
        return "\n".join(["name", "version", "protocol_version", "list_commands", "known_command", "boardsize", "komi", "play",
                          "genmove", "undo", "loadsgf", "clear_board", "final_score", "final_status_list", "sgo-analyze",
                          "sgo-ownership", "sgo-book", "sgo-ladders", "sgo-life", "sgo-find", "sgo-moves", "sgo-influence",
                          "sgo-estimate", "sgo-secure", "sgo-solve", "sgo-race", "sgo-connect", "sgo-groups", "sgo-superko", "sgo-playouts",
                          "sgo-playout-moves", "sgo-uct", "quit"])

    def known_command(self, name=""):
        # the method name behind a hyphenated private command is accepted by parse_command too, so it is known as well
        return "true" if name in self.list_commands().split("\n") or name in self.ALIASES.values() else "false"

    def boardsize(self, size):
        if int(size) != self.size:
            raise Exception("The board size in configuration is {0}x{0} but GTP asked to play {1}x{1}".format(self.size, int(size)))
        return ""

    def komi(self, komi):
        self._komi = komi
        return ""

    def parse_move(self, move):
        """GTP vertex -> (x, y): letters skip 'I', rows count from the bottom (sejonggo_nomodel.py:104-120)."""
        if move.lower() == 'pass':
            return 0, self.size
        x = string.ascii_uppercase.index(move[0].upper())
        if x >= 9:
            x -= 1
        y = int(move[1:]) - 1
        return x, self.size - y - 1

    def print_move(self, x, y):
        if y >= self.size:
            return "pass" if y == self.size else "resign"
        row = self.size - y - 1
        if x >= 8:
            x += 1
        return string.ascii_uppercase[x] + str(row + 1)

    def _to_move(self):
        return int(np.asarray(self.sejong_engine.board)[0, 0, 0, -1])

    def play(self, color, move):
        x, y = self.parse_move(move)
        if self.superko_rule is not None and y < self.size and COLOR_TO_PLAYER[color] == self._to_move():
            # the table is the side to move's; a stone placed out of turn is set-up, as everywhere else
            if self.sejong_engine.superko(self.superko_rule).played(0, y * self.size + x)[0]:
                raise GTPFailure("illegal move")
        self.board, self.player = self.sejong_engine.play(COLOR_TO_PLAYER[color], x, y)
        return ""

    def _superko_move(self, player, extra):
        """genmove while superko forbids what the inherited rule allows: the search runs without moving, and the child with the
        largest (visits, mean, higher index) that is not forbidden is played as an external move; a pass when there is none"""
        self.sejong_engine.analyze()
        r = self.sejong_engine.report(top=1, depth=1)
        N, Q = np.asarray(r["N"][0]), np.asarray(r["Q"][0])
        best = None
        for a in range(len(N)):
            if N[a] >= 0 and a not in extra and (best is None or (int(N[a]), float(Q[a]), a) > (int(N[best]), float(Q[best]), best)):
                best = a
        points = self.size * self.size
        x, y = (best % self.size, best // self.size) if best is not None and best < points else (0, self.size)
        self.board, self.player = self.sejong_engine.play(player, x, y)
        return self.print_move(x, y)

    def _book_moves(self):
        """[(action, count, wins, losses)] of the book for the position on the board, most played first; [] without a book"""
        if self.book is None:
            return []
        return self.book.moves(*self.sejong_engine.keys())

    def _no_net(self, what):
        """a command that would call the net, on an engine that was started without one"""
        if self.player_kind == "uct":
            raise GTPFailure("%s asks the net, and this engine was started with --player uct, without a model" % what)

    def _uct_move(self, player, extra):
        """genmove of --player uct: the most visited child of the playout tree search (ties: the larger wins2, the lower point) that
        superko does not forbid, played as an external move through the slot's play; a pass when there is none"""
        if player != self._to_move():
            raise GTPFailure("genmove for the side that is not to move: play the missing move (or a pass) first")
        v = self.sejong_engine.uct(self.uct_trees, self.uct_sims, float(self._komi))
        points = self.size * self.size
        ranked = v.ranked(0, lambda a: a not in extra)
        best = ranked[0] if ranked else points
        x, y = (best % self.size, best // self.size) if best < points else (0, self.size)
        self.board, self.player = self.sejong_engine.play(player, x, y)
        return self.print_move(x, y)

    def genmove(self, color):
        player = COLOR_TO_PLAYER[color]
        extra = set()
        if self.superko_rule is not None and player == self._to_move():
            extra = {a for a, _ in self.sejong_engine.superko(self.superko_rule).extra(0)}
        if self.book is not None and player == self._to_move():
            rows = [r for r in self._book_moves() if r[1] >= self.book_min]
            legal = self.sejong_engine.legal() if rows else None
            for a, _, _, _ in rows:
                if legal[a] and a not in extra:
                    # an external move as far as the session is concerned: its tree follows as for any play
                    x, y = (a % self.size, a // self.size) if a < self.size * self.size else (0, self.size)
                    self.board, self.player = self.sejong_engine.play(player, x, y)
                    return self.print_move(x, y)
        if self.player_kind == "uct":
            return self._uct_move(player, extra)
        if extra:
            return self._superko_move(player, extra)
        x, y, _, _, self.board, self.player = self.sejong_engine.genmove(player)
        return self.print_move(x, y)

    def sgo_book(self):
        """Private extension `sgo-book`: the book's moves for the position on the board, one line `vertex count wins losses`
        each, most played first; empty when there are none (or no book)."""
        self._engine_method("keys")
        return "\n".join("%s %d %d %d" % (self._vertex(a), c, w, l) for a, c, w, l in self._book_moves())

    def clear_board(self):
        self.board, self.player = game_init(self.size)
        self.sejong_engine.board = self.board
        self.sejong_engine.mcts_tree = None
        self.sejong_engine.move = 1
        return ""

    def _engine_method(self, name):
        """undo / load / analyze / report exist on the device engine only"""
        method = getattr(self.sejong_engine, name, None)
        if method is None or not hasattr(self.sejong_engine, "load"):
            raise GTPFailure("not supported")
        return method

    def undo(self):
        undo = self._engine_method("undo")
        try:
            self.board, self.player = undo()
        except ValueError:
            raise GTPFailure("cannot undo")
        return ""

    def loadsgf(self, filename, move_number=None):
        """GTP loadsgf: the main line of the record up to, not including, move `move_number` (all of it when absent); set-up
        stones (AB / AW) are placed first and count as no move."""
        load = self._engine_method("load")
        from .sgfload import load_file
        try:
            game = load_file(filename)
            last = None if move_number is None else int(move_number)
        except (IOError, OSError, ValueError) as e:
            raise GTPFailure("cannot load file" + (": %s" % e if isinstance(e, ValueError) else ""))
        if game.size != self.size:
            raise GTPFailure("cannot load file: the record is {0}x{0}, the configuration {1}x{1}".format(game.size, self.size))
        moves = game.prefix(last - 1) if last is not None else game.moves
        try:
            n_setup = 0
            while n_setup < len(moves) and game.setup[n_setup]:
                n_setup += 1                          # the leading AB / AW stones: `undo` leaves them on the board
            self.board, self.player = load([a for a, _ in moves], [c for _, c in moves], n_setup=n_setup)
        except ValueError as e:
            raise GTPFailure("cannot load file: %s" % e)
        if game.komi is not None:
            self._komi = game.komi
        return ""

    def _vertex(self, action):
        return self.print_move(action % self.size, action // self.size)

    def sgo_analyze(self, sims=None, top=5, depth=8):
        """Private extension `sgo-analyze [sims]`: searches the position without moving and replies one line per top child --
        vertex, visits, mean, prior, pv vertices."""
        self._no_net("sgo-analyze")
        analyze, report = self._engine_method("analyze"), self._engine_method("report")
        try:
            analyze(int(sims) if sims is not None else None)
        except ValueError:
            raise GTPFailure("syntax error")
        r = report(top=int(top), depth=int(depth))
        lines = []
        for k, a in enumerate(r["top_action"][0]):
            if a < 0:
                break
            pv = " ".join(self._vertex(int(m)) for m in r["pv"][0][k] if m >= 0)
            lines.append("%s visits %d mean %.4f prior %.4f pv %s" % (self._vertex(int(a)), int(r["N"][0][a]), float(r["Q"][0][a]),
                                                                      float(r["P"][0][a]), pv))
        return "\n".join(lines)

    def _score_source(self):
        """the callable behind final_score, final_status_list and sgo-ownership: () -> (a row shaped like rollout.result_row, the
        stones); policy rollouts unless the engine was started with score = playouts"""
        if self.score == "playouts":
            playouts = self._engine_method("playouts")

            def source():
                v, stones = playouts()
                return v.row(0), stones
            return source
        self._no_net("scoring by policy rollouts (--score rollouts)")
        return self._engine_method("rollouts")

    def final_score(self):
        """GTP final_score from policy rollouts: the points two thirds of the rollouts give one colour, minus komi."""
        from .rollout import final_score
        row, _ = self._score_source()()
        return final_score(row, float(self._komi))

    def final_status_list(self, status=""):
        """GTP final_status_list alive|dead|seki: the stones whose point the rollouts give to their own colour / to the
        opponent / to neither."""
        from .rollout import stone_status
        rollouts = self._score_source()
        if status not in ("alive", "dead", "seki"):
            raise GTPFailure("syntax error")
        row, stones = rollouts()
        return " ".join(self._vertex(a) for a in sorted(stone_status(row, stones)[status]))

    def sgo_ownership(self):
        """Private extension `sgo-ownership`: S lines of S signed per-mille values from the top row down, black positive:
        (black_own - white_own) * 1000 / rollouts, rounded towards zero."""
        row, _ = self._score_source()()
        R = max(1, int(row["rollouts"]))
        d = (np.asarray(row["black_own"], dtype=np.int64) - np.asarray(row["white_own"], dtype=np.int64)).reshape(self.size, self.size)
        return "\n".join(" ".join("%d" % (int(np.sign(v)) * (1000 * abs(int(v)) // R)) for v in line) for line in d)

    def quit(self):
        return ""

    def sgo_ladders(self):
        """Private extension `sgo-ladders`: one line per chain with one or two liberties that the reader catches (include/sgo.h
        "chains and ladders") -- the anchor vertex, colour, size, liberties, `capturable` (caught when the attacker moves first) or
        `dead` (caught even when the defender moves first), then `attack V` and `defend V` (none: no such move)."""
        from .tactics import format_chain
        chains = self._engine_method("tactics")()
        return "\n".join(format_chain(c, self._vertex) for c in chains if c.capturable or c.dead)

    def sgo_life(self):
        """Private extension `sgo-life`: unconditional life of the position (include/sgo.h "unconditional life") -- S lines of S
        characters from the top row down: B / W an alive stone, b / w a point of black / white territory (empty, or a dead stone of
        the other colour), . anything else; then one line `settled P/N black SB white SW`."""
        from .life import format_board
        return format_board(self._engine_method("life")(), 0)

    def sgo_find(self, *rows):
        """Private extension `sgo-find ROW/ROW/...`: where the shape drawn by the rows (shapes.Shape.parse: X O . * ?, `|` and lines
        of `-` for the edges; rows joined by `/`) occurs in the position (include/sgo.h "shape search") -- S lines of S characters
        from the top row down: # a point under a cared cell of a match, . anything else; then one line `hits H variants V cover K`."""
        from .shapes import Shape, format_cover
        if not rows:
            raise GTPFailure("syntax error")
        try:
            shape = Shape.parse("/".join(rows))
        except ValueError as e:
            raise GTPFailure("bad shape: %s" % e)
        return format_cover(self._engine_method("shapes")(shape), 0)

    def sgo_moves(self, *words):
        """Private extension `sgo-moves [capture|atari|escape|selfatari|forbidden|all] [opponent]`: what one ply on a point would do
        (include/sgo.h "move outcomes") -- one line per point of the kind in ascending point order (default all: every empty
        point), `V captures C size Z liberties L joins J ataris A`, then `ko` / `suicide` / `forbidden` where they hold.  The
        mover is the side to move; with `opponent` the other colour, so `opponent capture` lists the stones en prise.  capture,
        atari, escape (a chain with one liberty gets two or more) and selfatari list allowed moves only; forbidden lists the
        points the legal-move rule forbids although the stone would stand."""
        from .moves import KINDS, format_kind
        kind, side = "all", 0
        for w in words:
            if w == "opponent" and side == 0:
                side = 1
            elif w in KINDS and kind == "all":
                kind = w
            else:
                raise GTPFailure("syntax error")
        return format_kind(self._engine_method("move_outcomes")(side), 0, kind, self._vertex)

    def sgo_superko(self, *words):
        """Private extension `sgo-superko [situational]`: the moves of the side to move that would repeat an earlier position of
        the game (include/sgo.h "superko") -- one line `V K` per point in ascending point order, K plies back (1: a ko
        recapture), with `forbidden` appended where the inherited ko rule would allow the move.  Positional (equal stones) by
        default; `situational` asks for the same side to move as well.  Empty when nothing repeats."""
        from .superko import format_repeat
        if len(words) > 1 or (words and words[0] not in ("positional", "situational")):
            raise GTPFailure("syntax error")
        return format_repeat(self._engine_method("superko")(words[0] if words else "positional"), 0, self._vertex)

    def _playout_words(self, words, default):
        """(the number, rules) of `[N] [inherited]`"""
        n, rules = default, 1
        for w in words:
            if w == "inherited" and rules == 1:
                rules = 0
            elif w.isdigit() and n == default and int(w) >= 1:
                n = int(w)
            else:
                raise GTPFailure("syntax error")
        return n, rules

    def sgo_playouts(self, *words):
        """Private extension `sgo-playouts [N] [inherited]`: N light playouts from the position (include/sgo.h "light playouts";
        default playout.DEFAULT_PER_ROW) -- one line `score M +- SD  capped C%  playouts N` (black - white, komi-free), then S lines
        of S signed per-mille values from the top row down, black positive: who holds the point at the end.  Uniformly random moves
        that spare the mover's eyes; no net is asked.  `inherited` plays under the inherited legal set, where a ko can never be
        connected and the ply cap ends what does not end.  An ESTIMATE, not a proof."""
        from .playout import DEFAULT_PER_ROW, MAX_PER_ROW, format_summary
        n, rules = self._playout_words(words, DEFAULT_PER_ROW)
        if n > MAX_PER_ROW:
            raise GTPFailure("at most %d playouts" % MAX_PER_ROW)
        v, _ = self._engine_method("playouts")(n, rules)
        return format_summary(v, 0) + "\n" + v.format_board(0)

    def sgo_uct(self, *words):
        """Private extension `sgo-uct [trees T] [sims K]`: the playout tree search from the position (include/sgo.h "playout tree
        search"; default: the engine's --uct-trees / --uct-sims, else the untuned defaults of uct.py) at the GTP komi -- a head line
        `best V winrate W simulations N nodes M depth D`, then one line `V visits winrate rave-visits rave-winrate` per move, the
        ten most visited first; win rates are the side to move's.  No net is asked.  An ESTIMATE, not a proof."""
        from .uct import MAX_SIMS, MAX_TREES, format_moves
        opt = {"trees": self.uct_trees, "sims": self.uct_sims}
        if len(words) % 2:
            raise GTPFailure("syntax error")
        for key, val in zip(words[::2], words[1::2]):
            if key not in opt or not val.isdigit() or not 1 <= int(val) <= (MAX_TREES if key == "trees" else MAX_SIMS):
                raise GTPFailure("syntax error")
            opt[key] = int(val)
        v = self._engine_method("uct")(opt["trees"], opt["sims"], float(self._komi))
        return format_moves(v, 0, 10, self._vertex)

    def sgo_playout_moves(self, *words):
        """Private extension `sgo-playout-moves [K] [inherited]`: the K (default 10) best first moves of the side to move by the
        all-moves-as-first table of the light playouts -- one line `V count mean` per move: in how many playouts the side to move
        was the first to play V, and the mean final score of those from its view.  Moves seen in fewer than 1 % of the playouts are
        left out.  An ESTIMATE, not a proof."""
        from .playout import format_moves
        k, rules = self._playout_words(words, 10)
        v, _ = self._engine_method("playouts")(None, rules)
        return format_moves(v, 0, k, self._vertex, min_count=max(1, v.count(0, "playouts") // 100))

    def sgo_secure(self, *words):
        """Private extension `sgo-secure [opponent] [min K]`: what one more stone makes pass-alive (include/sgo.h "securing moves")
        -- the board from the top row down, one cell per point: X / O a stone, the gain (stones and points that become safe beyond
        those that are) on every allowed point whose gain is at least K (default 2: a stone that merely extends a living chain
        gains 1), - on an allowed point that loses some, . anything else; then `base B allowed A securing N harmful H` and `best V
        gain G secures ...` with the points the best move makes safe, or `best none`.  The mover is the side to move; with
        `opponent` the other colour.  A proof about one ply: the opponent's answer is not read."""
        from .secure import MIN_GAIN, format_board
        side, k, words = 0, None, list(words)
        while words:
            w = words.pop(0)
            if w == "opponent" and side == 0:
                side = 1
            elif w == "min" and k is None and words and words[0].lstrip("-").isdigit():
                k = int(words.pop(0))
            else:
                raise GTPFailure("syntax error")
        v, stones = self._engine_method("secure")(side)
        return format_board(v, 0, stones, self._vertex, MIN_GAIN if k is None else k)

    def sgo_solve(self, *words):
        """Private extension `sgo-solve [VERTEX [REGION-VERTEX ...]] [nodes K] [inherited]`: can the chain on VERTEX be killed when
        both sides play (include/sgo.h "life and death")?  One line `V colour empty E verdict kill K live L nodes A D` -- verdict
        alive / unsettled / dead / unknown / open, kill the attacker's first killing move, live the defender's first saving move
        (`pass`: it need not answer), the node counts of the two queries -- then the board from the top row down: X / O a stone, * an
        empty point of the region M the reader is confined to, K / L the kill / live move (! where they are one point), . anything
        else.  Further vertices give M explicitly; `nodes K` sets the budget per query (default 4096); `inherited` reads under the
        legal-move rule as inherited (rules = 0) instead of the sound one.  Without a vertex: one line per enclosed chain.  The
        verdict of a bounded reader inside M, not a proof about the game."""
        from .solve import MAX_NODES, format_board, format_target
        pts, nodes, rules, words = [], None, 1, list(words)
        while words:
            w = words.pop(0)
            if w == "inherited" and rules == 1:
                rules = 0
            elif w == "nodes" and nodes is None and words and words[0].isdigit() and 1 <= int(words[0]) <= MAX_NODES:
                nodes = int(words.pop(0))
            else:
                try:
                    x, y = self.parse_move(w)
                except Exception:
                    raise GTPFailure("syntax error")
                if not (0 <= x < self.size and 0 <= y < self.size):
                    raise GTPFailure("syntax error")
                pts.append(y * self.size + x)
        N = self.size * self.size
        v, stones = self._engine_method("solve")(pts[0] if pts else None, pts[1:] or None, rules=rules, max_nodes=nodes or 4096)
        targets = v.targets_of(0)
        if not pts:
            return "\n".join(format_target(t, self._vertex, N) for t in targets)
        if targets[0].verdict is None:
            raise GTPFailure("no stone on %s" % self._vertex(pts[0]))
        return format_target(targets[0], self._vertex, N) + "\n" + format_board(self.size, stones, v.region(0, 0), targets[0])

    def sgo_race(self, *words):
        """Private extension `sgo-race [VERTEX VERTEX] [libs K] [nodes K] [inherited]`: which of two chains in contact falls first
        (include/sgo.h "capturing races")?  One line per pair `B W libs b w shared s empty E outcome black catch C save S white
        catch C save S nodes Ab Db Aw Dw` -- B / W the lowest point of the black / white chain, outcome `black wins`, `white wins`,
        `first to move wins`, `standoff`, `open` or the two racer words (safe / unsettled / caught / unknown), catch the other
        side's first catching move (`wait`: it waits out a ko ban), save the racer's own first saving move (`pass`: it need not
        answer).  With two vertices: that pair only; without: every pair in contact whose chains have at most `libs K` liberties
        (default 4).  `nodes K` sets the budget per query (default 1024); `inherited` reads under the legal-move rule as inherited
        (rules = 0).  The verdict of a bounded reader inside the pair's region, not a proof about the game."""
        from .race import MAX_LIBS, MAX_NODES, format_pair
        pts, nodes, libs, rules, words = [], None, None, 1, list(words)
        while words:
            w = words.pop(0)
            if w == "inherited" and rules == 1:
                rules = 0
            elif w == "nodes" and nodes is None and words and words[0].isdigit() and 1 <= int(words[0]) <= MAX_NODES:
                nodes = int(words.pop(0))
            elif w == "libs" and libs is None and words and words[0].isdigit() and 1 <= int(words[0]) <= MAX_LIBS:
                libs = int(words.pop(0))
            else:
                try:
                    x, y = self.parse_move(w)
                except Exception:
                    raise GTPFailure("syntax error")
                if not (0 <= x < self.size and 0 <= y < self.size):
                    raise GTPFailure("syntax error")
                pts.append(y * self.size + x)
        if len(pts) not in (0, 2):
            raise GTPFailure("syntax error")
        N = self.size * self.size
        v = self._engine_method("race")(tuple(pts) if pts else None, rules=rules, max_libs=libs or 4, max_nodes=nodes or 1024)
        pairs = v.pairs_of(0)
        if pts and pairs[0].no_pair:
            raise GTPFailure("no pair on %s %s" % (self._vertex(pts[0]), self._vertex(pts[1])))
        return "\n".join(format_pair(p, self._vertex, N) for p in pairs)

    def _connect_words(self, words, vertices):
        """(points, keyword arguments) of `sgo-connect` / `sgo-groups` words"""
        from .connect import MAX_CUT_LIBS, MAX_NODES
        pts, nodes, libs, rules, words = [], None, None, 1, list(words)
        while words:
            w = words.pop(0)
            if w == "inherited" and rules == 1:
                rules = 0
            elif w == "nodes" and nodes is None and words and words[0].isdigit() and 1 <= int(words[0]) <= MAX_NODES:
                nodes = int(words.pop(0))
            elif w == "cutlibs" and libs is None and words and words[0].isdigit() and int(words[0]) <= MAX_CUT_LIBS:
                libs = int(words.pop(0))
            else:
                try:
                    x, y = self.parse_move(w)
                except Exception:
                    raise GTPFailure("syntax error")
                if not (vertices and 0 <= x < self.size and 0 <= y < self.size):
                    raise GTPFailure("syntax error")
                pts.append(y * self.size + x)
        if len(pts) not in (0, 2):
            raise GTPFailure("syntax error")
        return pts, dict(rules=rules, cut_libs=1 if libs is None else libs, max_nodes=nodes or 1024)

    def sgo_connect(self, *words):
        """Private extension `sgo-connect [VERTEX VERTEX] [cutlibs K] [nodes K] [inherited]`: can two chains of one colour be cut
        apart (include/sgo.h "connections")?  One line per pair `X Y colour shared s links k empty E cutting c verdict cut C join J
        nodes A D` -- X / Y the lowest points of the two chains, verdict connected / unsettled / cut / unknown / open, cut the other
        side's first cutting move (`pass`: it cuts by playing elsewhere), join the first joining move.  With two vertices: that pair
        only; without: every near pair.  `cutlibs K` lets opposing chains with up to K liberties between the two count as
        capturable cutting chains (default 1); `nodes K` sets the budget per query (default 1024); `inherited` reads under the
        legal-move rule as inherited (rules = 0).  The verdict of a bounded reader inside the pair's region, not a proof about the
        game."""
        from .connect import format_pair
        pts, kw = self._connect_words(words, True)
        v, _ = self._engine_method("connect")(tuple(pts) if pts else None, **kw)
        pairs = v.pairs_of(0)
        if pts and pairs[0].no_pair:
            raise GTPFailure("no pair on %s %s" % (self._vertex(pts[0]), self._vertex(pts[1])))
        return "\n".join(format_pair(p, self._vertex, self.size * self.size) for p in pairs)

    def sgo_groups(self, *words):
        """Private extension `sgo-groups [cutlibs K] [nodes K] [inherited]`: the board with one letter per GROUP -- the chains that
        `sgo-connect` reads as connected, tied together -- upper case for black and lower case for white, then `chains C groups G
        connected P` and, where it applies, `table cut` (more near pairs than the table holds: the partition may be too fine) and
        `undecided` (some pair is unknown or open and ties nothing)."""
        from .connect import FLAG_CUT_TABLE, FLAG_UNDECIDED, format_groups
        _, kw = self._connect_words(words, False)
        v, stones = self._engine_method("connect")(None, **kw)
        c = v.group_counts[0]
        tail = "chains %d groups %d connected %d" % (c[0], c[1], c[2])
        tail += " table cut" if c[3] & FLAG_CUT_TABLE else ""
        tail += " undecided" if c[3] & FLAG_UNDECIDED else ""
        return format_groups(self.size, v.groups[0], set(np.flatnonzero(stones > 0).tolist())) + "\n" + tail

    def _influence(self, words):
        from .influence import PRESETS
        preset, dead = None, "life"
        for w in words:
            if w == "nodead" and dead is not None:
                dead = None
            elif w in PRESETS and preset is None:
                preset = w
            else:
                raise GTPFailure("syntax error")
        return self._engine_method("influence")(dead=dead, **PRESETS[preset or "territory"])

    def sgo_influence(self, *words):
        """Private extension `sgo-influence [territory|area] [nodead]`: Bouzy's influence map of the position (include/sgo.h
        "influence"; an estimate, not a proof) -- S lines of S characters from the top row down: X / O a live stone, b / w a point of
        black / white territory, + / - black / white moyo beyond the territory, . neutral; then `estimate B+x.x black P white Q
        neutral R komi K`.  territory (default) is the triple (5, 10, 21), area (4, 0, 0).  The stones unconditional life proves
        dead are lifted first unless `nodead` is given."""
        from .influence import format_board
        v, stones = self._influence(words)
        return format_board(v, stones, 0, float(self._komi))

    def sgo_estimate(self, *words):
        """Private extension `sgo-estimate [territory|area] [nodead]`: the score of `sgo-influence`'s estimate line alone, `B+x.x` /
        `W+x.x` / `0` (live stones + territory, minus komi)."""
        from .influence import score_text
        v, _ = self._influence(words)
        return score_text(v.estimate(0, float(self._komi)))

    ALIASES = {"sgo-analyze": "sgo_analyze", "sgo-ownership": "sgo_ownership", "sgo-book": "sgo_book", "sgo-ladders": "sgo_ladders",
               "sgo-life": "sgo_life", "sgo-find": "sgo_find", "sgo-moves": "sgo_moves", "sgo-influence": "sgo_influence",
               "sgo-estimate": "sgo_estimate", "sgo-secure": "sgo_secure", "sgo-solve": "sgo_solve", "sgo-race": "sgo_race",
               "sgo-connect": "sgo_connect", "sgo-groups": "sgo_groups", "sgo-superko": "sgo_superko",
               "sgo-playouts": "sgo_playouts", "sgo-playout-moves": "sgo_playout_moves", "sgo-uct": "sgo_uct"}      # GTP private extensions carry a hyphen; methods cannot

    def parse_command(self, line):
        tokens = line.strip().split(" ")
        if not tokens or not tokens[0]:
            return ""
        name = self.ALIASES.get(tokens[0], tokens[0])
        method = getattr(self, name, None)
        if method is None or name.startswith("_"):
            return "? unknown command\n\n"
        try:
            result = method(*tokens[1:])
        except GTPFailure as e:
            return "? %s\n\n" % e
        return "=\n\n" if not result.strip() else "= " + result + "\n\n"


def main(inp=sys.stdin, out=sys.stdout, device=False, book=None, book_min=1, superko=None, score=None, player="net", uct_trees=None,
         uct_sims=None):
    """device=True (`python -m sejonggo_amd.gtp --device`): the game lives on the device engine (DeviceSejongGoEngine).
    book (`--book FILE [--book-min N]`, device only): genmove plays from the opening book records.py wrote while it has a move.
    superko (`--superko positional|situational`, device only): `play` refuses and genmove avoids a move that repeats an earlier
    position of the game.
    player "uct" (`--player uct [--uct-trees T --uct-sims K]`, device only): genmove plays the playout tree search's best move and the
    engine starts WITHOUT loading a model: the session stands on the uniform stub net, which nothing asks."""
    if player != "net" and not device:
        sys.stderr.write("--player uct needs the device engine: run with --device\n")
        return 2
    if book is not None and not device:
        sys.stderr.write("--book needs the device engine: run with --device\n")
        return 2
    if superko is not None and not device:
        sys.stderr.write("--superko needs the device engine: run with --device\n")
        return 2
    if score not in (None, "rollouts") and not device:
        sys.stderr.write("--score playouts needs the device engine: run with --device\n")
        return 2
    net = None
    if player == "uct":
        from .stub_nets import make_stub
        net = make_stub("uniform", conf['SIZE'])                     # a given net: no predicting worker starts, no model file is read
    engine = GTPEngine(engine=DeviceSejongGoEngine(conf['MCTS_SIMULATIONS'], size=conf['SIZE'], net=net) if device else None, book=book,
                       book_min=book_min, superko=superko, score=score, player=player, uct_trees=uct_trees, uct_sims=uct_sims)
    for line in inp:
        for cmd in line.split("\n"):
            res = engine.parse_command(cmd)
            if res.strip():
                out.write(res)
                out.flush()
            if cmd.strip() == "quit":
                engine.sejong_engine.close()
                return


def _cli(argv):
    import argparse
    ap = argparse.ArgumentParser(description="GTP on stdin / stdout")
    ap.add_argument("--device", action="store_true", help="the game lives on the device engine")
    ap.add_argument("--book", default=None, help="an opening book (.npz of `python -m sejonggo_amd.records --book`); needs --device")
    ap.add_argument("--book-min", type=int, default=1, help="play a book move only when it was played at least N times (default 1)")
    ap.add_argument("--superko", default=None, choices=("positional", "situational"),
                    help="refuse and avoid moves that repeat an earlier position of the game; needs --device")
    ap.add_argument("--score", default=None, choices=("rollouts", "playouts"),
                    help="what final_score, final_status_list and sgo-ownership stand on: policy rollouts (default) or light playouts, "
                         "which ask no net (the default with --player uct); needs --device")
    ap.add_argument("--player", default="net", choices=("net", "uct"),
                    help="who answers genmove: the net's tree search (default) or the playout tree search, which asks no net -- the "
                         "engine then starts without loading a model; needs --device")
    ap.add_argument("--uct-trees", type=int, default=None, help="independent searches per genmove of --player uct (default: uct.TREES)")
    ap.add_argument("--uct-sims", type=int, default=None, help="simulations per search of --player uct (default: uct.SIMS)")
    a = ap.parse_args(argv)
    return main(device=a.device, book=a.book, book_min=a.book_min, superko=a.superko, score=a.score, player=a.player, uct_trees=a.uct_trees,
                uct_sims=a.uct_sims)


if __name__ == "__main__":
    sys.exit(_cli(sys.argv[1:]))
