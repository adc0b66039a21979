"""The three-ply ranked lines with game-history draws (include/gpu_nnue.h at gn_line3, "game history")
restated in Python from the CPU oracle alone, for tests/test_lines3_history.py and
tests/test_gpu_lines3_history.py.

Composed from the restatements it extends, static leaves only.  For position k of a game and a legal
move m with child c: a child without a legal move is tests/lines3_rule.py's line; a move
tests/history_rule.py draws (`drawn_moves`) is a drawn line that ends at the child; otherwise
(R3(c), reply, reply2, flags) is line 1 of tests/lines2_history_rule.py's two-ply history lines of c,
taken as position k + 1 of the game fens[:k + 1] + [c] -- the grandchildren and great-grandchildren are
counted against positions 0..=k, c itself being no occurrence for either.
"""
import numpy as np

import history_rule as H
import lines2_history_rule as H2
import lines3_rule as L3
import lines_rule as R

FLAG_DRAW = H.FLAG_DRAW
LINE3_DTYPE = L3.LINE3_DTYPE
EMPTY3 = L3.EMPTY3
FIXTURE = "lines3_history_games.txt"


def fixture_games():
    """[(root_fen, uci_moves, skip)] of tests/golden/lines3_history_games.txt."""
    return H.fixture_games(FIXTURE)


def plain_lines3(O, big, small, fens, k, mode):
    """Position k's three-ply lines without history (tests/lines3_rule.py, static leaves)."""
    return L3.all_lines3(O, big, small, fens[k], L3.LEAF_STATIC, 0, mode)


_child_lines = {}


def child_line(O, big, small, fens, k, c, mode):
    """L of the rule: line 1 (value, score, move, reply, flags, plies) of the two-ply history ranking with
    child c of position k as the parent, c's game so far being positions 0..=k followed by c; None when
    c has no legal move.  Computed once per (game so far, child, mode)."""
    key = (id(big), id(small), tuple(fens[:k + 1]), c, mode, bytes(O.eval_params()))
    if key not in _child_lines:
        ls = H2.all_lines2(O, big, small, list(fens[:k + 1]) + [c], k + 1, mode)
        _child_lines[key] = ls[0] if ls else None
    return _child_lines[key]


def all_lines3(O, big, small, fens, k, mode):
    """Every three-ply line of position k of the game `fens` (every position, skipped ones included),
    ranked: [((value, score, move, reply, reply2, flags, plies, 0), PV)]."""
    plain = {l[0][2]: l for l in plain_lines3(O, big, small, fens, k, mode)}
    if not plain:
        return []
    P = O.eval_params()
    material = R.wdl_material(fens[k], P)
    drawn = H.drawn_moves(O, fens, k)
    out = []
    for m, c, alive in H._children(O, fens[k]):
        check = plain[m][0][5] & R.FLAG_IN_CHECK
        if not alive:
            out.append(plain[m])
            continue
        if m in drawn:
            out.append(((0, 0, m, 0, 0, FLAG_DRAW | check, 1, 0), [m]))
            continue
        r3, _, reply, reply2, lfl, lplies = child_line(O, big, small, fens, k, c, mode)
        v = R.negate_ply(r3)
        score, mate = R.rule_score(v, material, P)
        fl = check | mate | (lfl & (R.FLAG_NO_MOVES | L3.FLAG_SEARCHED | FLAG_DRAW))
        out.append(((v, score, m, reply, reply2, fl, 1 + lplies, 0), [m, reply, reply2][:1 + lplies]))
    out.sort(key=lambda l: (-l[0][0], l[0][2]))
    return out


def draw_depths(O, fens, k):
    """The plies (1: child, 2: grandchild, 3: great-grandchild) at which the rule draws some position
    below position k, as {ply: "fifty" and / or "threefold" kinds}, whichever line is chosen."""
    out = {}
    level = [list(fens[:k + 1])]
    for ply in (1, 2, 3):
        nxt = []
        for g in level:
            at = len(g) - 1
            # (the positions after k are no occurrences: drawn_moves counts g[:at + 1], of which those
            # beyond k have the other side to move or lie two plies back)
            drawn = H.drawn_moves(O, g, at)
            for kind in drawn.values():
                out.setdefault(ply, set()).add(kind)
            for m, c, alive in H._children(O, g[at]):
                if alive and m not in drawn:
                    nxt.append(g + [c])
        level = nxt
    return out


def game_lines3(O, big, small, fens, skip, mode, K, only=None):
    """(lines[len(fens), K] as LINE3_DTYPE, pvs[len(fens), K] as PV_DTYPE) of one game; a skipped
    position has only empty lines.  only: the positions to compute (the others stay zero)."""
    rows = []
    for k in range(len(fens)):
        rows.append([] if k in skip or (only is not None and k not in only) else all_lines3(O, big, small, fens, k, mode))
    lines, pvs = L3.table(rows, K)
    if only is not None:
        for k in range(len(fens)):
            if k not in only:
                lines[k] = np.zeros(K, dtype=LINE3_DTYPE)
    return lines, pvs


# the positions of each fixture game that the tests compute (the rule enumerates three plies per
# position): {game: positions}
CHOSEN = {0: (4, 5, 6, 7), 1: (3,), 2: (3,), 3: (4, 5, 6, 7), 4: (0,), 5: (0,), 6: (0,), 7: (4, 5, 6, 7)}
