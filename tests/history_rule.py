"""The game-history draws of the ranked lines (include/gpu_nnue.h at gn_history) restated in
Python from the CPU oracle alone, on top of tests/lines_rule.py, for tests/test_history.py and
tests/test_gpu_history.py.

From the oracle: `replay_game` gives a game's positions as FENs, `legal_moves` / `child_fen` a
position's children.  Restated here: a position's identity is the first four fields of its
normalised FEN; a child with a legal move is drawn by rule when its half-move clock is at least
100 or when its identity equals that of at least two of the game's positions up to and including
the parent -- counted over the whole game so far, without the kernel's bounded walk.
"""
import functools
import os

import numpy as np

import lines_rule as R

HERE = os.path.dirname(os.path.abspath(__file__))
FLAG_DRAW = 512


def fixture_games(name="history_games.txt"):
    """[(root_fen, uci_moves, skip)] of tests/golden/<name>, a `root | moves | skip` line per game."""
    out = []
    with open(os.path.join(HERE, "golden", name)) as f:
        for l in f:
            if not l.strip() or l.startswith("#"):
                continue
            root, moves, skip = (x.strip() for x in l.split("|"))
            out.append((root, moves, tuple(int(x) for x in skip.split())))
    return out


def identity(fen):
    return tuple(fen.split()[:4])


@functools.lru_cache(maxsize=None)
def _children(O, fen):
    """((move, child FEN, the child has a legal move), ...) of fen."""
    out = []
    for m in O.legal_moves(fen):
        c = O.child_fen(fen, m)
        out.append((m, c, bool(O.legal_moves(c))))
    return tuple(out)


def drawn_moves(O, fens, k):
    """The moves of position k of the game `fens` whose child is drawn by rule, as
    {move: "fifty" or "threefold"}; fens: every position of the game, skipped ones included."""
    seen = [identity(f) for f in fens[:k + 1]]
    out = {}
    for m, c, alive in _children(O, fens[k]):
        if not alive:
            continue  # mate, or stalemate: GN_FLAG_NO_MOVES without GN_FLAG_DRAW
        if int(c.split()[4]) >= 100:
            out[m] = "fifty"
        elif seen.count(identity(c)) >= 2:
            out[m] = "threefold"
    return out


def occurrences(O, fens, k):
    """{move: how many of positions 0..=k have the child's identity} for position k's legal moves."""
    seen = [identity(f) for f in fens[:k + 1]]
    return {m: seen.count(identity(c)) for m, c, _ in _children(O, fens[k])}


def all_lines(O, big, small, fens, k, mode):
    """Every line of position k of the game, ranked, with the drawn moves valued 0."""
    drawn = drawn_moves(O, fens, k)
    out = []
    for v, score, m, flags in R.all_lines(O, big, small, fens[k], mode):
        if m in drawn:
            v, score, flags = 0, 0, (flags & R.FLAG_IN_CHECK) | FLAG_DRAW
        out.append((v, score, m, flags))
    out.sort(key=lambda l: (-l[0], l[2]))
    return out


def game_lines(O, big, small, fens, skip, mode, K, only=None):
    """lines[len(fens), K] of one game as LINE_DTYPE; a skipped position has only empty lines.
    only: the positions to compute (the others stay zero)."""
    out = np.zeros((len(fens), K), dtype=R.LINE_DTYPE)
    for k in range(len(fens)):
        if only is not None and k not in only:
            continue
        ls = [] if k in skip else all_lines(O, big, small, fens, k, mode)[:K]
        for j in range(K):
            out[k, j] = ls[j] if j < len(ls) else R.EMPTY
    return out
