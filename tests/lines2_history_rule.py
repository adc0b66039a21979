"""The two-ply ranked lines with game-history draws (include/gpu_nnue.h at gn_line2) restated in
Python from the CPU oracle alone, for tests/test_lines2_history.py and
tests/test_gpu_lines2_history.py.

Composed from the two restatements it extends.  For position k of a game and a legal move m with
child c: a move tests/history_rule.py draws (`drawn_moves`) is a drawn line that ends at the child;
a child without a legal move is tests/lines2_rule.py's; otherwise (R(c), reply, draw) is line 1 of
history_rule's depth-1 lines of c, taken as position k + 1 of the game fens[:k + 1] + [c] -- the
grandchildren are counted against positions 0..=k, c itself having the other side to move.
"""
import numpy as np

import history_rule as H
import lines2_rule as R2
import lines_rule as R

FLAG_DRAW = H.FLAG_DRAW
LINE2_DTYPE = R2.LINE2_DTYPE
EMPTY2 = R2.EMPTY2


def fixture_games():
    """[(root_fen, uci_moves, skip)] of tests/golden/lines2_history_games.txt."""
    return H.fixture_games("lines2_history_games.txt")


def both_fixtures():
    """history_games.txt's games, then lines2_history_games.txt's."""
    return H.fixture_games() + fixture_games()


def all_lines2(O, big, small, fens, k, mode):
    """Every two-ply line of position k of the game `fens` (every position, skipped ones included),
    ranked: [(value, score, move, reply, flags, plies)]."""
    kids = R2.child_replies(O, big, small, fens[k], mode)
    if not kids:
        return []
    P = O.eval_params()
    material = R.wdl_material(fens[k], P)
    drawn = H.drawn_moves(O, fens, k)
    out = []
    for m, check, replies in kids:
        fl = R.FLAG_IN_CHECK if check else 0
        if m in drawn:
            out.append((0, 0, m, 0, FLAG_DRAW | fl, 1))
            continue
        if replies:
            c = O.child_fen(fens[k], m)
            r_c, _, reply, rfl = H.all_lines(O, big, small, list(fens[:k + 1]) + [c], k + 1, mode)[0]
            fl |= rfl & FLAG_DRAW
            plies = 2
        else:
            r_c, reply, plies = (-R.VALUE_MATE if check else 0), 0, 1
            fl |= R.FLAG_NO_MOVES
        v = R.negate_ply(r_c)
        score, mate = R.rule_score(v, material, P)
        out.append((v, score, m, reply, mate | fl, plies))
    out.sort(key=lambda l: (-l[0], l[2]))
    return out


def draws_nothing(O, big, small, fens, k, mode):
    """True when the rule draws nothing at either level at position k: no child and no grandchild of
    it with a legal move is drawn (whichever reply is chosen)."""
    if H.drawn_moves(O, fens, k):
        return False
    for m, _, alive in H._children(O, fens[k]):
        if alive and H.drawn_moves(O, list(fens[:k + 1]) + [O.child_fen(fens[k], m)], k + 1):
            return False
    return True


def game_lines2(O, big, small, fens, skip, mode, K, only=None):
    """lines[len(fens), K] of one game as LINE2_DTYPE; a skipped position has only empty lines.
    only: the positions to compute (the others stay zero)."""
    out = np.zeros((len(fens), K), dtype=LINE2_DTYPE)
    for k in range(len(fens)):
        if only is not None and k not in only:
            continue
        ls = [] if k in skip else all_lines2(O, big, small, fens, k, mode)[:K]
        for j in range(K):
            out[k, j] = ls[j] if j < len(ls) else EMPTY2
    return out
