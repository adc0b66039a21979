"""The two-ply ranked-lines rule (include/gpu_nnue.h at gn_line2) restated in Python from the CPU
oracle alone, for tests/test_lines2.py and tests/test_gpu_lines2.py.

It reuses the depth-1 restatement (tests/lines_rule.py): for a child c with a legal move, R(c) and
the reply are line 1 of `all_lines(child_fen(p, m))`, the header's "relation to gn_line"; a child
without a legal move is mated (-VALUE_MATE) or stalemated (0) by its in-check flag.  `negate_ply`,
`rule_score` and the material are lines_rule's.
"""
import os

import numpy as np

import lines_rule as R

LINE2_DTYPE = np.dtype([("value", "<i4"), ("score", "<i4"), ("move", "<u2"), ("reply", "<u2"), ("flags", "<u2"),
                        ("plies", "<u2")])
EMPTY2 = (0, 0, 0, 0, R.FLAG_NO_SCORE, 0)
SEED, N_RANDOM, N_WIDE = 0x5EED22E5, 48, 512  # the seeded random sets of the GPU tests
MATE_IN_ONE = "rnbqkbnr/pppp1ppp/8/4p3/8/5P2/PPPPP1PP/RNBQKBNR w KQkq - 0 2"  # g2g4 allows d8h4 mate
TWO_MATES = "rr6/6k1/8/2P5/8/8/6PP/7K w - - 0 1"  # after c5c6 both a8a1 and b8b1 mate


def fixture_fens():
    with open(os.path.join(R.HERE, "golden", "lines2_fens.txt")) as f:
        return [l.strip() for l in f if l.strip() and not l.startswith("#")]


def uci_move(uci):
    """A plain (non-castling, non-promoting) UCI move in the 16-bit Stockfish encoding."""
    sq = lambda s: "abcdefgh".index(s[0]) + 8 * (int(s[1]) - 1)
    return sq(uci[0:2]) << 6 | sq(uci[2:4])


def child_replies(O, big, small, fen, mode):
    """Per legal move m of fen, in the oracle's order: (m, the child in check?, the child's ranked
    depth-1 lines); None for a bad position."""
    try:
        _, moves, kids = O.expand_eval(big, small, fen, mode)
    except ValueError:
        return None
    return [(m, bool(int(k["flags"]) & R.FLAG_IN_CHECK), R.all_lines(O, big, small, O.child_fen(fen, m), mode))
            for m, k in zip(moves, kids)]


def all_lines2(O, big, small, fen, mode):
    """Every two-ply line of fen, ranked: [(value, score, move, reply, flags, plies)]; [] for a bad
    position or one without a legal move."""
    kids = child_replies(O, big, small, fen, mode)
    if not kids:
        return []
    P = O.eval_params()
    material = R.wdl_material(fen, P)
    out = []
    for m, check, replies in kids:
        if replies:  # R(c) = the child's line 1
            r_c, reply, none, plies = replies[0][0], replies[0][2], 0, 2
        else:
            r_c, reply, none, plies = (-R.VALUE_MATE if check else 0), 0, R.FLAG_NO_MOVES, 1
        v = R.negate_ply(r_c)
        score, mate = R.rule_score(v, material, P)
        out.append((v, score, m, reply, mate | (R.FLAG_IN_CHECK if check else 0) | none, plies))
    out.sort(key=lambda l: (-l[0], l[2]))
    return out


def lines2(O, big, small, fens, mode, K):
    """lines[len(fens), K] as LINE2_DTYPE: the first K lines of each position, then empty lines."""
    out = np.zeros((len(fens), K), dtype=LINE2_DTYPE)
    for i, fen in enumerate(fens):
        ls = all_lines2(O, big, small, fen, mode)[:K]
        for k in range(K):
            out[i, k] = ls[k] if k < len(ls) else EMPTY2
    return out
