"""The check-extended ranked lines (include/gpu_nnue.h at gn_line, "check-extended") restated in
Python from the CPU oracle alone, for tests/test_lines_extended.py and
tests/test_gpu_lines_extended.py.

It reuses the four restatements it extends (tests/lines_rule.py, lines2_rule.py, history_rule.py,
lines2_history_rule.py) for `negate_ply`, `rule_score`, the material and the drawn moves.  Restated
here: `value(fen, d)`, the in-check part of the gn_eval.score rule, as a recursion over the
oracle's `expand_eval` / `child_fen` / `legal_moves`; and the leaf value E(x) with its precedence:
no legal move, then (history forms) drawn by rule, then in check with a legal move -> value(x, 2)
with GN_FLAG_SEARCHED, else the static final_v.
"""
import os

import numpy as np

import history_rule as H
import lines2_rule as R2
import lines_rule as R

FLAG_SEARCHED = 128
FLAG_DRAW = H.FLAG_DRAW
NOT_EXTENDED = -(2 ** 31)
SEED1, N_RANDOM1 = 0x5EED33E5, 128  # the seeded random sets of the tests: one ply ...
SEED2, N_RANDOM2 = 0x5EED44E5, 48   # ... and two plies

# the fixtures of tests/golden/lines_extended_fens.txt, in the file's order
MATING_REPLY = "7R/3k3p/8/1R1b3Q/P2pr2P/3BP3/6K1/2R1B3 b - - 7 76"          # e4e7+ allows a mating reply
MATE_IN_2 = "3k3B/N1n1q2r/4r3/p2p1K2/1PBpp1P1/P4p2/4R2P/2b3NR b - - 3 47"   # e7f7+ / e7f8+ mate in 2
TWO_PLY_A = "8/1b6/2kp4/Q3R3/5P1r/7P/1B4K1/8 b - - 0 75"
TWO_PLY_B = "8/7N/1Pr4B/8/3PP1k1/p7/P4K1R/8 b - - 8 67"
TWO_PLY_MATE = "3Q4/3bp3/4P3/p1k5/P3p3/1K4R1/1R6/8 b - - 1 74"              # d7b5 b2c2: mate -2
FIFTY = "7k/8/8/8/8/8/8/R3K3 w - - 99 80"                                   # a1a8+ reaches rule50 100


def fixture_fens():
    with open(os.path.join(R.HERE, "golden", "lines_extended_fens.txt")) as f:
        return [l.strip() for l in f if l.strip() and not l.startswith("#")]


_value = {}


def value(O, big, small, fen, d, mode):
    """(value(fen, d), best reply) of the gn_eval.score rule for a position in check with a legal
    move: the maximum over the legal replies of negate_ply, a reply in check with a legal move going
    one level down while d > 1, any other taking its static final_v; ties to the smaller move."""
    key = (id(big), id(small), fen, d, mode, bytes(O.eval_params()))  # (the values follow the oracle's parameters)
    if key not in _value:
        _, moves, kids = O.expand_eval(big, small, fen, mode)
        best, bm = None, None
        for m, k in zip(moves, kids):
            c = O.child_fen(fen, m)
            check = bool(int(k["flags"]) & R.FLAG_IN_CHECK)
            if not O.legal_moves(c):
                v = -R.VALUE_MATE if check else 0
            elif check and d > 1:
                v = value(O, big, small, c, d - 1, mode)[0]
            else:
                v = int(k["final_v"])
            v = R.negate_ply(v)
            if best is None or v > best or (v == best and m < bm):
                best, bm = v, m
        _value[key] = (best, bm)
    return _value[key]


def leaves(O, big, small, fen, mode):
    """Per legal move of fen, in the oracle's order: (move, leaf FEN, in check, has a legal move,
    static final_v); None for a bad position."""
    try:
        _, moves, kids = O.expand_eval(big, small, fen, mode)
    except ValueError:
        return None
    out = []
    for m, k in zip(moves, kids):
        c = O.child_fen(fen, m)
        out.append((m, c, bool(int(k["flags"]) & R.FLAG_IN_CHECK), bool(O.legal_moves(c)), int(k["final_v"])))
    return out


def extensions(O, big, small, fen, mode):
    """d_ext of fen's leaves, in the oracle's order: value(leaf, 2) where the leaf is in check with a
    legal move, NOT_EXTENDED elsewhere."""
    return [value(O, big, small, c, 2, mode)[0] if check and alive else NOT_EXTENDED
            for _, c, check, alive, _ in leaves(O, big, small, fen, mode) or []]


def all_lines(O, big, small, fen, mode, drawn=()):
    """Every extended line of fen, ranked: [(value, score, move, flags)].  drawn: the moves whose
    child is drawn by rule (the history forms)."""
    P = O.eval_params()
    material = R.wdl_material(fen, P)
    out = []
    for m, c, check, alive, final_v in leaves(O, big, small, fen, mode) or []:
        fl = R.FLAG_IN_CHECK if check else 0
        if not alive:
            v, fl = (-R.VALUE_MATE if check else 0), fl | R.FLAG_NO_MOVES
        elif m in drawn:
            v, fl = 0, fl | FLAG_DRAW
        elif check:
            v, fl = value(O, big, small, c, 2, mode)[0], fl | FLAG_SEARCHED
        else:
            v = final_v
        v = R.negate_ply(v)
        score, mate = R.rule_score(v, material, P)
        out.append((v, score, m, fl | mate))
    out.sort(key=lambda l: (-l[0], l[2]))
    return out


def all_lines2(O, big, small, fen, mode, fens=None, k=None):
    """Every extended two-ply line of fen, ranked: [(value, score, move, reply, flags, plies)].  With
    fens / k (the history forms): fen is position k of the game fens, and the draws apply at both
    levels, before the extension."""
    kids = leaves(O, big, small, fen, mode)
    if not kids:
        return []
    P = O.eval_params()
    material = R.wdl_material(fen, P)
    history = fens is not None
    drawn = H.drawn_moves(O, fens, k) if history else {}
    out = []
    for m, c, check, alive, _ in kids:
        fl = R.FLAG_IN_CHECK if check else 0
        if not alive:
            r_c, reply, plies, fl = (-R.VALUE_MATE if check else 0), 0, 1, fl | R.FLAG_NO_MOVES
        elif m in drawn:
            out.append((0, 0, m, 0, FLAG_DRAW | fl, 1))
            continue
        else:  # the child stays an interior node: line 1 of its extended depth-1 lines
            gdrawn = H.drawn_moves(O, list(fens[:k + 1]) + [c], k + 1) if history else ()
            r_c, _, reply, rfl = all_lines(O, big, small, c, mode, gdrawn)[0]
            fl |= rfl & (FLAG_DRAW | FLAG_SEARCHED)
            plies = 2
        v = R.negate_ply(r_c)
        score, mate = R.rule_score(v, material, P)
        out.append((v, score, m, reply, mate | fl, plies))
    out.sort(key=lambda l: (-l[0], l[2]))
    return out


def _table(rows, K, dtype, empty):
    out = np.zeros((len(rows), K), dtype=dtype)
    for i, ls in enumerate(rows):
        for j in range(K):
            out[i, j] = ls[j] if j < len(ls) else empty
    return out


def lines(O, big, small, fens, mode, K):
    """lines[len(fens), K] as LINE_DTYPE (no history)."""
    return _table([all_lines(O, big, small, f, mode)[:K] for f in fens], K, R.LINE_DTYPE, R.EMPTY)


def lines2(O, big, small, fens, mode, K):
    """lines[len(fens), K] as LINE2_DTYPE (no history)."""
    return _table([all_lines2(O, big, small, f, mode)[:K] for f in fens], K, R2.LINE2_DTYPE, R2.EMPTY2)


def game_lines(O, big, small, fens, skip, mode, K, history):
    """One game's lines[len(fens), K]; a skipped position has only empty lines."""
    rows = []
    for k in range(len(fens)):
        drawn = H.drawn_moves(O, fens, k) if history and k not in skip else ()
        rows.append([] if k in skip else all_lines(O, big, small, fens[k], mode, drawn)[:K])
    return _table(rows, K, R.LINE_DTYPE, R.EMPTY)


def game_lines2(O, big, small, fens, skip, mode, K, history):
    """One game's two-ply lines[len(fens), K]; a skipped position has only empty lines."""
    rows = []
    for k in range(len(fens)):
        if k in skip:
            rows.append([])
        elif history:
            rows.append(all_lines2(O, big, small, fens[k], mode, fens, k)[:K])
        else:
            rows.append(all_lines2(O, big, small, fens[k], mode)[:K])
    return _table(rows, K, R2.LINE2_DTYPE, R2.EMPTY2)
