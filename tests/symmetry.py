"""The two board symmetries under which the whole specification is invariant, for
tests/test_symmetry.py (the CPU oracle and the host code) and tests/test_gpu_symmetry.py (the GPU).
The maps and comparisons are pure Python: they ask neither the oracle nor the library anything
(only `input_fens`, the shared inputs, has the library's host code print canonical FENs).

Colour flip F: ranks 1 <-> 8, piece colours swapped, the side to move swapped, the castling rights'
case swapped, the en-passant rank flipped; rule50 and fullmove stay.  The evaluation is relative to
the side to move and HalfKAv2_hm to the perspective, so every field of a record is unchanged, and
the move tree maps by from ^ 56, to ^ 56.

File mirror M: files a <-> h, for positions without castling rights (castling is not mirror
symmetric: the king ends on the c or g file either way).  The "_hm" of HalfKAv2_hm is this
symmetry.  Moves map by from ^ 7, to ^ 7.

Ranked lines break ties of equal values by the 16-bit move encoding, which neither map preserves:
`compare_lines` compares what is invariant whatever the ties, and whole lines where no tie decides.
"""
FLIP_MASK = 0x0E38    # 56 | 56 << 6: the rank bits of `to` and `from`
MIRROR_MASK = 0x01C7  # 7 | 7 << 6: the file bits
FLAG_NO_SCORE = 64    # an empty line (include/gpu_nnue.h at gn_line)
FLAG_IN_CHECK, FLAG_SEARCHED, FLAG_NO_MOVES, FLAG_DRAW = 1, 128, 256, 512


# ---- FENs ----------------------------------------------------------------------------------------

def _castling_white_first(field):
    return "".join(c for c in field if c.isupper()) + "".join(c for c in field if c.islower())


def flip_fen(fen):
    """F of a FEN with all six fields.  The castling field (KQkq or Shredder file letters) comes out
    with white's letters first, each colour's in the order they had."""
    placement, stm, castling, ep, rule50, fullmove = fen.split()
    placement = "/".join(r.swapcase() for r in reversed(placement.split("/")))
    stm = {"w": "b", "b": "w"}[stm]
    if castling != "-":
        castling = _castling_white_first(castling.swapcase())
    if ep != "-":
        ep = ep[0] + str(9 - int(ep[1]))
    return " ".join((placement, stm, castling, ep, rule50, fullmove))


def without_fullmove(fen):
    """The first five fields.  F keeps a position's fullmove number, but the number counts black's
    moves: below a position and its image it differs by one at every other ply, so positions
    reached by moves are compared under F without it.  Nothing evaluated reads it."""
    return fen.rsplit(" ", 1)[0]


def mirror_fen(fen):
    """M of a FEN with all six fields; ValueError for a position with castling rights."""
    placement, stm, castling, ep, rule50, fullmove = fen.split()
    if castling != "-":
        raise ValueError(f"the file mirror needs a position without castling rights: {fen}")
    placement = "/".join(r[::-1] for r in placement.split("/"))
    if ep != "-":
        ep = "abcdefgh"[7 - "abcdefgh".index(ep[0])] + ep[1]
    return " ".join((placement, stm, castling, ep, rule50, fullmove))


# ---- moves ---------------------------------------------------------------------------------------

def flip_move(m):
    """F of a move in the 16-bit Stockfish encoding (promotion and type bits stay); 0, the absent
    move of best_move / reply / an empty line, stays 0."""
    m = int(m)
    return m ^ FLIP_MASK if m else 0


def mirror_move(m):
    m = int(m)
    return m ^ MIRROR_MASK if m else 0


def flip_uci(u):
    """F of a UCI move: e2e4 -> e7e5, e1g1 -> e8g8, a7a8q -> a2a1q."""
    return u[0] + str(9 - int(u[1])) + u[2] + str(9 - int(u[3])) + u[4:]


def mirror_uci(u):
    f = lambda c: "abcdefgh"[7 - "abcdefgh".index(c)]
    return f(u[0]) + u[1] + f(u[2]) + u[3] + u[4:]


def flip_game(game):
    """F of (root_fen, moves, skip); moves a string of UCI moves or a sequence of them."""
    root, moves, skip = game
    if isinstance(moves, str):
        moves = " ".join(flip_uci(u) for u in moves.split())
    else:
        moves = [flip_uci(u) for u in moves]
    return flip_fen(root), moves, skip


def best_move_tie(child_a, child_b):
    """True when two replies of a searched position may stand for one another as its best_move:
    the move encoding alone decides between them, and neither map preserves its order.  child_a,
    child_b: the gn_eval records of the two replies' children in the position's mode.  Both
    checkmates, both stalemates, or both out of check with equal final_v (a child in check with a
    legal move is searched one level down: no record of the child itself shows a tie there)."""
    fa, fb = int(child_a["flags"]), int(child_b["flags"])
    none_a, none_b, check_a, check_b = fa & FLAG_NO_MOVES, fb & FLAG_NO_MOVES, fa & FLAG_IN_CHECK, fb & FLAG_IN_CHECK
    if none_a and none_b:
        return check_a == check_b
    if none_a or none_b or check_a or check_b:
        return False
    return int(child_a["final_v"]) == int(child_b["final_v"])


# ---- ranked lines --------------------------------------------------------------------------------

def compare_lines(a, b, map_move, compared=None, reply_tie=None):
    """One position's K lines `a` (gn_line or gn_line2 records, ranked) against the transformed
    position's `b`.  Asserted whatever the ties: equal value sequences, equal score sequences, equal
    numbers of non-empty lines.  Asserted for every non-empty line whose value no other non-empty
    line of the K has: the whole line, move (and reply) through map_move, flags (and plies).  When
    all K lines are non-empty a line with line K's value is left out of that: the cut may split a
    group of equal values that goes on below it.

    A gn_line2's reply is the child's best reply, ties again to the smaller encoding: where the two
    replies differ, reply_tie(move, reply of a, reply of b mapped back, flags), all in a's frame,
    must show that they tie (`replies_tie` on the two grandchildren's records); without a
    reply_tie a different reply fails.

    compared: a list that receives the indices of the lines compared in full.  Returns (lines
    compared in full, non-empty lines)."""
    names = a.dtype.names
    assert b.dtype == a.dtype and len(a) == len(b)
    va, vb = [int(v) for v in a["value"]], [int(v) for v in b["value"]]
    assert va == vb, (va, vb)
    assert a["score"].tolist() == b["score"].tolist(), (a["score"].tolist(), b["score"].tolist())
    live_a = [not (int(f) & FLAG_NO_SCORE) for f in a["flags"]]
    live_b = [not (int(f) & FLAG_NO_SCORE) for f in b["flags"]]
    n = sum(live_a)
    assert n == sum(live_b), (n, sum(live_b))
    assert live_a == [j < n for j in range(len(a))] == live_b  # the non-empty lines come first
    values = va[:n]
    full = 0
    for j in range(n):
        if values.count(va[j]) != 1 or (n == len(a) and va[j] == va[-1]):
            continue
        assert map_move(a["move"][j]) == int(b["move"][j]), (j, a[j], b[j])
        assert int(a["flags"][j]) == int(b["flags"][j]), (j, a[j], b[j])
        if "reply" in names:
            assert int(a["plies"][j]) == int(b["plies"][j]), (j, a[j], b[j])
            if map_move(a["reply"][j]) != int(b["reply"][j]):
                assert int(a["reply"][j]) and int(b["reply"][j]), (j, a[j], b[j])
                assert reply_tie is not None and reply_tie(int(a["move"][j]), int(a["reply"][j]),
                                                           map_move(b["reply"][j]), int(a["flags"][j])), (j, a[j], b[j])
        if compared is not None:
            compared.append(j)
        full += 1
    return full, n


def replies_tie(grandchild_a, grandchild_b, line_flags):
    """True when two replies of a gn_line2 certainly tie.  grandchild_a, grandchild_b: the gn_eval
    records, in the lines' mode, of the positions after either reply; line_flags: the line's flags
    (equal in both lines).  A drawn reply (GN_FLAG_DRAW on a line of two plies) ties with another
    drawn reply; a check-extended one (GN_FLAG_SEARCHED) has no record that shows its value: no tie
    is accepted there.  Otherwise both replies mate, both stalemate, or both leave positions with
    a legal move and equal final_v."""
    if line_flags & FLAG_DRAW:
        return True
    if line_flags & FLAG_SEARCHED:
        return False
    fa, fb = int(grandchild_a["flags"]), int(grandchild_b["flags"])
    if (fa | fb) & FLAG_NO_MOVES:
        return (fa & (FLAG_NO_MOVES | FLAG_IN_CHECK)) == (fb & (FLAG_NO_MOVES | FLAG_IN_CHECK))
    return int(grandchild_a["final_v"]) == int(grandchild_b["final_v"])


def compare_line_tables(ta, tb, map_move, where=None, reply_tie=None):
    """compare_lines over lines[positions, K] tables: (lines compared in full, non-empty lines,
    [(position, line index)] compared in full).  reply_tie(position, move, reply, reply, flags)."""
    assert ta.shape == tb.shape
    full = live = 0
    at = []
    for i in range(len(ta)):
        js = []
        tie = None if reply_tie is None else (lambda *args, i=i: reply_tie(i, *args))
        try:
            f, n = compare_lines(ta[i], tb[i], map_move, js, tie)
        except AssertionError as e:
            raise AssertionError(f"position {i}{'' if where is None else ' (' + str(where[i]) + ')'}: {e}") from e
        full, live = full + f, live + n
        at += [(i, j) for j in js]
    return full, live, at


# ---- the inputs of both test files ---------------------------------------------------------------

def input_fens():
    """About 300 positions as canonical FENs (gn_board_to_fen of gn_pack_fens; host code only):
    tests/golden/special_fens.txt, the FENs of perft.json and score_fens.json, the fixtures of the
    ranked-lines rules and 96 seeded random positions.  Returns (raw FENs, canonical FENs); the
    random positions are their own raw form."""
    import json
    import os

    import lines_extended_rule as X
    import lines_rule as R
    from fishnet_amd import gpu_nnue as G
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "special_fens.txt")) as f:
        raw = [l.strip() for l in f if l.strip() and not l.startswith("#")]
    with open(os.path.join(golden, "perft.json")) as f:
        raw += [c["fen"] for c in json.load(f)["cases"]]
    with open(os.path.join(golden, "score_fens.json")) as f:
        raw += [r[0] for r in json.load(f)["results"]["full"]]
    raw += R.fixture_fens() + X.fixture_fens()
    boards, ok = G.pack_fens(raw)
    assert ok.all()
    raw += G.boards_to_fens(G.random_positions(0x5EED5A11, 0, 96, 160))
    return raw, G.boards_to_fens(boards) + raw[len(boards):]


def mirror_subset(fens):
    """The indices of the canonical FENs without castling rights: where M applies."""
    return [i for i, f in enumerate(fens) if f.split()[2] == "-"]
