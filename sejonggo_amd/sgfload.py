"""A minimal reader of the main line of an SGF game record, written from the FF[4] property grammar:

    Collection = GameTree+      GameTree = "(" Sequence GameTree* ")"      Sequence = Node+      Node = ";" Property*
    Property = PropIdent PropValue+      PropIdent = UcLetter+      PropValue = "[" CValueType "]"

inside a value "\\" escapes the next character (so "\\]" does not close it; an escaped line break is removed).  The main line is
the first game tree's sequence followed, at every fork, by its FIRST child: later children (variations) are ignored.
Read: SZ (one number; "19:19" for square boards), KM, the set-up stones AB / AW (point lists, compressed "aa:cc" rectangles
included), the moves B / W, a pass as "[]" or, on boards up to 19x19, "[tt]" (and, outside the grammar, as a point one row below the
board, which is how engines that keep (x, y = size) for the pass have written it).  Everything else is skipped.

    game = loads(text)      # or load_file(path)
    game.size, game.komi    # komi None when the record has none
    game.moves              # [(action, colour)]: action = y * size + x, pass = size * size; colour +1 black, -1 white
    game.setup              # [bool] per entry: True for an AB / AW stone, False for a B / W move
    game.prefix(k)          # the entries up to and including the k-th B / W move (set-up stones count as no move)

The (action, colour) list is what engine.SessionEngine.setup takes: set-up stones are played as stones of an explicit colour.

For collections of records (records.py): root_properties(text) gives the root node's properties ({ident: [values]}: RE, PB, ...),
node_indices(text) the index on the main line (root = 0) of the node every entry of loads(text).moves comes from, and
result_winner(values) reads RE."""
import collections


class SgfGame(collections.namedtuple("SgfGame", "size komi moves setup")):
    def prefix(self, k):
        out, seen = [], 0
        for entry, is_setup in zip(self.moves, self.setup):
            if not is_setup:
                if seen >= k:
                    break
                seen += 1
            out.append(entry)
        return out

    @property
    def n_moves(self):
        return sum(1 for s in self.setup if not s)


def _main_line(text):
    """[{ident: [values]}] for the nodes of the main line."""
    nodes, i, n = [], 0, len(text)
    depth = 0          # open game trees on the main line
    skip = 0           # > 0: inside a variation that is ignored (its nesting depth)
    closed = set()     # depths at which the main line has already taken its first child
    node = None
    while i < n:
        ch = text[i]
        if ch == "(":
            if skip:
                skip += 1
            elif depth in closed:
                skip = 1
            else:
                closed.add(depth)
                depth += 1
            i += 1
        elif ch == ")":
            if skip:
                skip -= 1
            else:
                depth -= 1
                if depth == 0:
                    break                   # the first game tree of the collection is the record
            i += 1
        elif ch == ";":
            if not skip:
                if depth == 0:
                    raise ValueError("SGF: a node outside a game tree")
                node = {}
                nodes.append(node)
            i += 1
        elif ch.isupper():
            j = i
            while j < n and (text[j].isupper() or text[j].islower()):       # FF[3] allowed lower-case letters in identifiers
                j += 1
            ident = "".join(c for c in text[i:j] if c.isupper())
            values = []
            while True:
                while j < n and text[j].isspace():
                    j += 1
                if j >= n or text[j] != "[":
                    break
                j += 1
                buf = []
                while j < n and text[j] != "]":
                    if text[j] == "\\" and j + 1 < n:
                        j += 1
                        if text[j] == "\r" and j + 1 < n and text[j + 1] == "\n":
                            j += 1
                        if text[j] not in "\r\n":
                            buf.append(text[j])
                    else:
                        buf.append(text[j])
                    j += 1
                if j >= n:
                    raise ValueError("SGF: a property value is not closed")
                j += 1
                values.append("".join(buf))
            if not values:
                raise ValueError("SGF: property %s has no value" % ident)
            if not skip:
                if node is None:
                    raise ValueError("SGF: a property outside a node")
                node.setdefault(ident, []).extend(values)
            i = j
        elif ch.isspace() or skip or depth == 0:     # text in front of the collection is skipped
            i += 1
        else:
            raise ValueError("SGF: unexpected %r at offset %d" % (ch, i))
    if not nodes:
        raise ValueError("SGF: no game tree")
    return nodes


def _point(v, size):
    if len(v) != 2 or not all("a" <= c <= "z" for c in v):
        raise ValueError("SGF: bad point %r" % v)
    x, y = ord(v[0]) - 97, ord(v[1]) - 97
    if x >= size or y >= size:
        raise ValueError("SGF: point %r is off the %dx%d board" % (v, size, size))
    return y * size + x


def _row_below_board(v, size):
    """Outside FF[4]: records written from (x, y) engine coordinates spell the pass (x, size) as a point one row below the board
    ("at" on 19x19); it is read as the pass it stands for."""
    return len(v) == 2 and 0 <= ord(v[0]) - 97 < size and ord(v[1]) - 97 == size


def _points(values, size):
    out = []
    for v in values:
        if ":" in v:
            a, b = v.split(":", 1)
            pa, pb = _point(a, size), _point(b, size)
            for y in range(pa // size, pb // size + 1):
                for x in range(pa % size, pb % size + 1):
                    out.append(y * size + x)
        else:
            out.append(_point(v, size))
    return out


def loads(text):
    nodes = _main_line(text)
    root = nodes[0]
    size = 19
    if "SZ" in root:
        sz = root["SZ"][0].strip()
        cols, _, rows = sz.partition(":")
        try:
            size = int(cols)
            if rows and int(rows) != size:
                raise ValueError
        except ValueError:
            raise ValueError("SGF: SZ[%s] is no square board size" % sz)
        if not 1 <= size <= 26:
            raise ValueError("SGF: SZ[%s] is outside 1..26" % sz)
    komi = None
    if "KM" in root and root["KM"][0].strip():
        try:
            komi = float(root["KM"][0])
        except ValueError:
            raise ValueError("SGF: KM[%s] is no number" % root["KM"][0])
    moves, setup = [], []
    for node in nodes:
        for ident, colour in (("AB", 1), ("AW", -1)):
            for a in _points(node.get(ident, []), size):
                moves.append((a, colour))
                setup.append(True)
        for ident, colour in (("B", 1), ("W", -1)):
            for v in node.get(ident, []):
                v = v.strip()
                is_pass = v == "" or (v == "tt" and size <= 19) or _row_below_board(v, size)
                moves.append((size * size if is_pass else _point(v, size), colour))
                setup.append(False)
    return SgfGame(size, komi, moves, setup)


def root_properties(text):
    """{ident: [values]} of the root node of the record's main line."""
    return dict(_main_line(text)[0])


def node_indices(text):
    """One int per entry of loads(text).moves, in its order: the index of the entry's node on the main line, root = 0.  For a
    B / W move this is the position of its node in the main sequence, whether or not the root carries a move itself."""
    out = []
    for i, node in enumerate(_main_line(text)):
        for ident in ("AB", "AW"):
            for v in node.get(ident, []):
                if ":" in v:
                    a, b = v.split(":", 1)
                    out.extend([i] * ((ord(b[0]) - ord(a[0]) + 1) * (ord(b[1]) - ord(a[1]) + 1)))
                else:
                    out.append(i)
        out.extend([i] * (len(node.get("B", [])) + len(node.get("W", []))))
    return out


def result_winner(root):
    """+1 / -1 from the RE of root_properties: "B+..." / "W+..." (any case, leading blanks skipped); None for everything else
    ("0", "Draw", "Void", "?", no RE at all)."""
    re = (root.get("RE") or [""])[0].strip().upper()
    if re.startswith("B+"):
        return 1
    if re.startswith("W+"):
        return -1
    return None


def load_file(path):
    with open(path, "r") as f:
        return loads(f.read())
