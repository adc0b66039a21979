"""The ranked-lines rule (include/gpu_nnue.h at gn_line) restated in Python from the CPU oracle
alone, for tests/test_lines.py and tests/test_gpu_lines.py.

From the oracle: `expand_eval` gives a position's legal moves and child records (final_v, the
in-check flag) in a mode; `legal_moves(child_fen(fen, move))` tells whether a child has a move.
Restated here, not taken from any record: `negate_ply`, `rule_score` and the `to_cp` arithmetic
(UCIEngine::to_cp with the win-rate parameters the oracle reports as its defaults, in Python's
doubles, which neither fuse nor reorder; rounded half away from zero).
"""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
VALUE_MATE = 32000
VALUE_MATE_IN_MAX_PLY = VALUE_MATE - 246
FLAG_IN_CHECK, FLAG_MATE, FLAG_NO_SCORE, FLAG_NO_MOVES = 1, 32, 64, 256
LINE_DTYPE = np.dtype([("value", "<i4"), ("score", "<i4"), ("move", "<u2"), ("flags", "<u2")])
EMPTY = (0, 0, 0, FLAG_NO_SCORE)
SEED, N_RANDOM = 0x5EED11E5, 512  # the seeded random set of the GPU tests
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


def fixture_fens():
    with open(os.path.join(HERE, "golden", "lines_fens.txt")) as f:
        return [l.strip() for l in f if l.strip() and not l.startswith("#")]


def negate_ply(v):
    v = -v
    return v - 1 if v >= VALUE_MATE_IN_MAX_PLY else v + 1 if v <= -VALUE_MATE_IN_MAX_PLY else v


def round_half_away(x):
    r = int(x)  # toward zero; x - r is exact
    if abs(x - r) >= 0.5:
        r += 1 if x > 0 else -1
    return r


def wdl_material(fen, P):
    board = fen.split()[0].lower()
    return sum(w * board.count(c) for w, c in zip(P.wdl_piece_weight, "pnbrq"))


def to_cp(v, material, P):
    mc = min(max(material, P.wdl_material_min), P.wdl_material_max)
    m = mc / P.wdl_material_anchor
    a = ((P.wdl_a[0] * m + P.wdl_a[1]) * m + P.wdl_a[2]) * m + P.wdl_a[3]
    return round_half_away((100 * v) / a)


def rule_score(v, material, P):
    """(score, GN_FLAG_MATE or 0) of a rule value."""
    if abs(v) >= VALUE_MATE_IN_MAX_PLY:
        ply = VALUE_MATE - abs(v)
        return ((ply + 1) // 2 if v > 0 else -(ply // 2)), FLAG_MATE
    return to_cp(v, material, P), 0


@functools.lru_cache(maxsize=None)
def _no_move_children(O, fen):
    """The moves of fen whose child has no legal move (mode-independent)."""
    return frozenset(m for m in O.legal_moves(fen) if not O.legal_moves(O.child_fen(fen, m)))


def all_lines(O, big, small, fen, mode):
    """Every line of fen, ranked: [(value, score, move, flags)]; [] for a bad position or one
    without a legal move."""
    try:
        _, moves, kids = O.expand_eval(big, small, fen, mode)
    except ValueError:
        return []
    P = O.eval_params()
    material = wdl_material(fen, P)
    dead = _no_move_children(O, fen) if moves else frozenset()
    out = []
    for m, k in zip(moves, kids):
        check = bool(int(k["flags"]) & FLAG_IN_CHECK)
        none = m in dead
        v = negate_ply((-VALUE_MATE if check else 0) if none else int(k["final_v"]))
        score, mate = rule_score(v, material, P)
        out.append((v, score, m, mate | (FLAG_IN_CHECK if check else 0) | (FLAG_NO_MOVES if none else 0)))
    out.sort(key=lambda l: (-l[0], l[2]))
    return out


def lines(O, big, small, fens, mode, K):
    """lines[len(fens), K] as LINE_DTYPE: the first K lines of each position, then empty lines."""
    out = np.zeros((len(fens), K), dtype=LINE_DTYPE)
    for i, fen in enumerate(fens):
        ls = all_lines(O, big, small, fen, mode)[:K]
        for k in range(K):
            out[i, k] = ls[k] if k < len(ls) else EMPTY
    return out


def reply_in_check_with_move(O, big, small, fen, mode=0):
    """True when some legal reply of fen leaves the opponent in check with a legal move: where the
    score rule goes one level deeper than the lines."""
    return any((l[3] & FLAG_IN_CHECK) and not (l[3] & FLAG_NO_MOVES) for l in all_lines(O, big, small, fen, mode))
