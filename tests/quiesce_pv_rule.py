"""The quiescence's own variation (include/gpu_nnue.h at gn_line, "the quiescence's own moves", and at
gn_pv) restated in Python over tests/quiesce_rule.py, for tests/test_quiesce_pv.py and
tests/test_gpu_quiesce_pv.py.

Restated here: PVQ(x, d) with its two tie rules (among moves the smaller 16-bit encoding; stand pat
wins a tie with a move), the d_tail rows gn_quiesce_pv_device writes, the gn_pv of a gn_line and of a
gn_line2, and the replay identity: negate_ply applied len(PVQ) times to the end position's own value
is Q(x, d).  Q, the noisy moves, the searched set and negate_ply are quiesce_rule's.

How ties are counted (`Counts`): on the nodes PVQ visits from a searched leaf -- the leaf, then the
child of each move it plays, down to the node where it stops -- and per move, from the final values,
not from a scan in some move order.  Where a move is played, every other searched move of the node
whose negate_ply(Q(child, d - 1)) equals the played move's is one *move tie*: the smaller encoding
decided.  Where the node stands pat, every searched move whose value equals the node's static
final_v is one *stand-pat tie*: a move as good as standing pat was not played.
"""
import numpy as np

import lines_rule as R
import quiesce_rule as Q

MAX_PV = 2 + Q.MAX_DEPTH
PV_DTYPE = np.dtype([("len", "<u2"), ("moves", "<u2", (MAX_PV,)), ("reserved", "<u2")])


class Counts:
    def __init__(self):
        self.move_ties = self.stand_pat_ties = self.nodes = 0


def _choice(O, big, small, fen, d, mode, check, static):
    """The node's searched entries with their values [(value, move, entry)], the chosen one or None
    (stand pat, or nothing to search)."""
    vals = []
    for k in Q.searched_moves(O, big, small, fen, mode, check):
        m, c, kcheck, kstatic, _ = k
        vals.append((R.negate_ply(Q.Q(O, big, small, c, d - 1, mode, kcheck, kstatic)[0]), m, k))
    if not vals:
        return vals, None
    best = min(vals, key=lambda t: (-t[0], t[1]))
    if not check and best[0] <= static:
        return vals, None
    return vals, best


def pvq(O, big, small, fen, d, mode, check, static):
    """PVQ(fen, d) as a tuple of moves; check / static as for quiesce_rule.Q."""
    out = []
    while d > 0 and Q.alive(O, fen):
        _, best = _choice(O, big, small, fen, d, mode, check, static)
        if best is None:
            break
        _, m, (_, fen, check, static, _) = best
        out.append(m)
        d -= 1
    return tuple(out)


def count_ties(O, big, small, fen, d, mode, check, static, counts):
    """Adds the ties on the nodes PVQ(fen, d) visits (the module's docstring)."""
    while d > 0 and Q.alive(O, fen):
        vals, best = _choice(O, big, small, fen, d, mode, check, static)
        if not vals:
            return
        counts.nodes += 1
        if best is None:
            counts.stand_pat_ties += sum(1 for v, _, _ in vals if v == static)
            return
        counts.move_ties += sum(1 for v, _, _ in vals if v == best[0]) - 1
        _, _, (_, fen, check, static, _) = best
        d -= 1


def end_value(O, big, small, fen, moves, mode, check, static):
    """The value of the position after `moves` from fen, by itself: -VALUE_MATE (in check) or 0
    without a legal move, else its static final_v; every move must be a searched move where it is
    played (legal, and noisy unless the mover is in check)."""
    for m in moves:
        k = next((k for k in Q.searched_moves(O, big, small, fen, mode, check) if k[0] == m), None)
        assert k is not None, (fen, m)
        _, fen, check, static, _ = k
    if not Q.alive(O, fen):
        return -R.VALUE_MATE if check else 0
    return static


def replayed(O, big, small, fen, moves, mode, check, static):
    """negate_ply applied len(moves) times to the end position's own value."""
    v = end_value(O, big, small, fen, moves, mode, check, static)
    for _ in moves:
        v = R.negate_ply(v)
    return v


def tails(O, big, small, fen, depth, mode):
    """The d_tail rows of fen's leaves in the oracle's order: {move: PVQ(leaf, depth)}; () for an
    unsearched leaf."""
    return {m: (pvq(O, big, small, c, depth, mode, check, static) if srch else ())
            for m, c, check, _, static, srch in Q.leaves(O, big, small, fen, mode) or []}


def tail_row(moves):
    return list(moves) + [0] * (Q.MAX_DEPTH - len(moves))


def _pv(moves):
    out = np.zeros((), dtype=PV_DTYPE)
    out["len"] = len(moves)
    out["moves"][:len(moves)] = moves
    return out


def line_pvs(O, big, small, fens, lines, depth, mode, with_tails=True):
    """The gn_pv of each gn_line of lines[len(fens), K] (LINE_DTYPE): [move] + PVQ(child, depth) where
    the line is searched."""
    out = np.zeros(lines.shape, dtype=PV_DTYPE)
    for i, fen in enumerate(fens):
        t = None
        for j, ln in enumerate(lines[i]):
            if int(ln["flags"]) & R.FLAG_NO_SCORE:
                continue
            mv = [int(ln["move"])]
            if with_tails and int(ln["flags"]) & Q.FLAG_SEARCHED:
                t = t if t is not None else tails(O, big, small, fen, depth, mode)
                mv += t[mv[0]]
            out[i, j] = _pv(mv)
    return out


def line2_pvs(O, big, small, fens, lines, depth, mode, with_tails=True):
    """The gn_pv of each gn_line2 of lines[len(fens), K] (LINE2_DTYPE): [move] or [move, reply], then
    PVQ(grandchild, depth) where plies == 2 and the line is searched."""
    out = np.zeros(lines.shape, dtype=PV_DTYPE)
    for i, fen in enumerate(fens):
        for j, ln in enumerate(lines[i]):
            if int(ln["flags"]) & R.FLAG_NO_SCORE:
                continue
            mv = [int(ln["move"])]
            if int(ln["plies"]) == 2:
                mv.append(int(ln["reply"]))
                if with_tails and int(ln["flags"]) & Q.FLAG_SEARCHED:
                    mv += tails(O, big, small, O.child_fen(fen, mv[0]), depth, mode)[mv[1]]
            out[i, j] = _pv(mv)
    return out
