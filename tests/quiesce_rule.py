"""The quiescent ranked lines (include/gpu_nnue.h at gn_line, "quiescent") restated in Python from the
CPU oracle alone, for tests/test_quiesce.py and tests/test_gpu_quiesce.py.

It reuses the restatements it extends (tests/lines_rule.py, lines2_rule.py, history_rule.py) for
`negate_ply`, `rule_score`, the material and the drawn moves.  Restated here: the noisy moves, Q(x, d)
as a recursion over the oracle's `expand_eval` / `child_fen` / `legal_moves` (one `expand_eval` per
node, then the filter on its moves), "searched", d_ext with the counts gn_quiesce_device reports, and
the leaf value with its precedence: no legal move, then (history forms) drawn by rule, then searched
-> Q(x, depth) with GN_FLAG_SEARCHED, else the static final_v.
"""
import os

import numpy as np

import history_rule as H
import lines2_rule as R2
import lines_rule as R

FLAG_SEARCHED = 128
FLAG_DRAW = H.FLAG_DRAW
NOT_EXTENDED = -(2 ** 31)
MAX_DEPTH = 4
SEED, N_RANDOM, N_RANDOM3 = 0x5EED55E5, 64, 16  # the seeded random sets of the tests: depth 1 / 2, and depth 3
SEED2, N_RANDOM2 = 0x5EED66E5, 3                # ... and two plies

# the fixtures of tests/golden/quiesce_fens.txt, in the file's order: (name, FEN, the move to the leaf)
FIXTURES = (
    ("en_passant_only", "4k3/8/8/8/3p4/8/4P3/4K3 w - - 0 1", "e2e4"),
    ("quiet_promotions", "8/4P3/8/8/8/k7/8/4K3 b - - 0 1", "a3a2"),
    ("capturing_underpromotion", "3r4/4P3/8/8/8/k7/8/4K3 b - - 0 1", "a3a2"),
    ("capture_gives_check", "n3k3/8/8/8/8/7p/8/R3K3 b - - 0 1", "h3h2"),
    ("capture_mates", "4n2k/6pp/7P/8/8/p7/8/4R1K1 b - - 0 1", "a3a2"),
    ("capture_stalemates", "k7/8/1K6/5n2/8/8/7B/8 b - - 0 1", "f5d6"),
    ("one_evasion", "7k/6p1/8/8/8/8/8/4R1K1 w - - 0 1", "e1e8"),
    ("double_check", "4k3/8/8/8/4N3/8/8/4R1K1 w - - 0 1", "e4d6"),
    ("pinned_capture", "4r2k/8/8/8/3p4/8/4N3/4K3 b - - 0 1", "h8h7"),
    ("defended_piece", "7k/8/8/8/8/2p5/3n4/4K3 b - - 0 1", "h8h7"),
    ("chess960_castling", "4k3/7p/8/8/8/8/8/1RK5 b Q - 0 1", "h7h6"),
    ("fifty_before_searched", "8/8/8/7p/6kP/8/8/K7 w - - 99 80", "a1a2"),
)


def fixture_fens():
    with open(os.path.join(R.HERE, "golden", "quiesce_fens.txt")) as f:
        return [l.strip() for l in f if l.strip() and not l.startswith("#")]


def noisy(O, fen, m):
    """A move of fen's side is noisy: a capture (castling, king takes own rook, is none), an en-passant
    capture, or a promotion to a queen."""
    typ = m >> 14
    if typ == 3:
        return False
    if typ == 2 or (m & 63) in O._placement(fen):
        return True
    return typ == 1 and (m >> 12) & 3 == 3


_node, _alive, _q = {}, {}, {}


def _key(O, big, small, mode):
    return (id(big), id(small), mode, bytes(O.eval_params()))  # (the values follow the oracle's parameters)


def node(O, big, small, fen, mode):
    """fen's legal moves, in the oracle's order: ((move, child FEN, the child is in check, its static
    final_v, the move is noisy), ...); one expand_eval.  ValueError for a bad position."""
    key = _key(O, big, small, mode) + (fen,)
    if key not in _node:
        _, moves, kids = O.expand_eval(big, small, fen, mode)
        _node[key] = tuple((m, O.child_fen(fen, m), bool(int(k["flags"]) & R.FLAG_IN_CHECK), int(k["final_v"]),
                            noisy(O, fen, m)) for m, k in zip(moves, kids))
    return _node[key]


def alive(O, fen):
    if fen not in _alive:
        _alive[fen] = bool(O.legal_moves(fen))
    return _alive[fen]


def searched_moves(O, big, small, fen, mode, check):
    """The entries of node(fen) the quiescence searches: all in check, the noisy ones otherwise."""
    return [k for k in node(O, big, small, fen, mode) if check or k[4]]


def Q(O, big, small, fen, d, mode, check, static):
    """(Q(fen, d), the positions evaluated below fen); check / static: fen's own in-check bit and
    static final_v, which its parent's expand_eval gave."""
    if not alive(O, fen):
        return (-R.VALUE_MATE if check else 0), 0
    if d == 0:
        return static, 0
    key = _key(O, big, small, mode) + (fen, d)
    if key not in _q:
        best, below = (None if check else static), 0
        for _, c, kcheck, kstatic, _ in searched_moves(O, big, small, fen, mode, check):
            v, n = Q(O, big, small, c, d - 1, mode, kcheck, kstatic)
            v = R.negate_ply(v)
            best = v if best is None or v > best else best
            below += 1 + n
        _q[key] = (best, below)
    return _q[key]


def is_searched(O, big, small, fen, mode, check):
    """A leaf is searched: it has a legal move and is in check, or it has a noisy legal move."""
    return alive(O, fen) and (check or any(k[4] for k in node(O, big, small, fen, mode)))


def leaves(O, big, small, fen, mode):
    """Per legal move of fen, in the oracle's order: (move, leaf FEN, in check, has a legal move, static
    final_v, searched); None for a bad position."""
    try:
        kids = node(O, big, small, fen, mode)
    except ValueError:
        return None
    return [(m, c, check, alive(O, c), static, is_searched(O, big, small, c, mode, check))
            for m, c, check, static, _ in kids]


def extensions(O, big, small, fen, depth, mode):
    """(d_ext of fen's leaves in the oracle's order, searched leaves, nodes evaluated below them)."""
    ext, ns, nn = [], 0, 0
    for _, c, check, _, static, srch in leaves(O, big, small, fen, mode) or []:
        if srch:
            v, n = Q(O, big, small, c, depth, mode, check, static)
            ext.append(v)
            ns, nn = ns + 1, nn + n
        else:
            ext.append(NOT_EXTENDED)
    return ext, ns, nn


def all_lines(O, big, small, fen, depth, mode, drawn=()):
    """Every quiescent line of fen, ranked: [(value, score, move, flags)].  drawn: the moves whose
    child is drawn by rule (the history forms)."""
    P = O.eval_params()
    material = R.wdl_material(fen, P)
    out = []
    for m, c, check, live, static, srch in leaves(O, big, small, fen, mode) or []:
        fl = R.FLAG_IN_CHECK if check else 0
        if not live:
            v, fl = (-R.VALUE_MATE if check else 0), fl | R.FLAG_NO_MOVES
        elif m in drawn:
            v, fl = 0, fl | FLAG_DRAW
        elif srch:
            v, fl = Q(O, big, small, c, depth, mode, check, static)[0], fl | FLAG_SEARCHED
        else:
            v = static
        v = R.negate_ply(v)
        score, mate = R.rule_score(v, material, P)
        out.append((v, score, m, fl | mate))
    out.sort(key=lambda l: (-l[0], l[2]))
    return out


def all_lines2(O, big, small, fen, depth, mode, fens=None, k=None):
    """Every quiescent two-ply line of fen, ranked: [(value, score, move, reply, flags, plies)].  With
    fens / k (the history forms): fen is position k of the game fens, and the draws apply at both
    levels, before the quiescence."""
    kids = leaves(O, big, small, fen, mode)
    if not kids:
        return []
    P = O.eval_params()
    material = R.wdl_material(fen, P)
    history = fens is not None
    drawn = H.drawn_moves(O, fens, k) if history else {}
    out = []
    for m, c, check, live, _, _ in kids:
        fl = R.FLAG_IN_CHECK if check else 0
        if not live:
            r_c, reply, plies, fl = (-R.VALUE_MATE if check else 0), 0, 1, fl | R.FLAG_NO_MOVES
        elif m in drawn:
            out.append((0, 0, m, 0, FLAG_DRAW | fl, 1))
            continue
        else:  # the child stays an interior node: line 1 of its quiescent depth-1 lines
            gdrawn = H.drawn_moves(O, list(fens[:k + 1]) + [c], k + 1) if history else ()
            r_c, _, reply, rfl = all_lines(O, big, small, c, depth, mode, gdrawn)[0]
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


def lines(O, big, small, fens, depth, mode, K):
    """lines[len(fens), K] as LINE_DTYPE (no history)."""
    return _table([all_lines(O, big, small, f, depth, mode)[:K] for f in fens], K, R.LINE_DTYPE, R.EMPTY)


def lines2(O, big, small, fens, depth, mode, K):
    """lines[len(fens), K] as LINE2_DTYPE (no history)."""
    return _table([all_lines2(O, big, small, f, depth, mode)[:K] for f in fens], K, R2.LINE2_DTYPE, R2.EMPTY2)


def game_lines(O, big, small, fens, skip, depth, mode, K, history):
    """One game's lines[len(fens), K]; a skipped position has only empty lines."""
    rows = []
    for k in range(len(fens)):
        drawn = H.drawn_moves(O, fens, k) if history and k not in skip else ()
        rows.append([] if k in skip else all_lines(O, big, small, fens[k], depth, mode, drawn)[:K])
    return _table(rows, K, R.LINE_DTYPE, R.EMPTY)


def game_lines2(O, big, small, fens, skip, depth, mode, K, history):
    """One game's two-ply lines[len(fens), K]; a skipped position has only empty lines."""
    rows = []
    for k in range(len(fens)):
        if k in skip:
            rows.append([])
        elif history:
            rows.append(all_lines2(O, big, small, fens[k], depth, mode, fens, k)[:K])
        else:
            rows.append(all_lines2(O, big, small, fens[k], depth, mode)[:K])
    return _table(rows, K, R2.LINE2_DTYPE, R2.EMPTY2)
