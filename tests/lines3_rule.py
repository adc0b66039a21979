"""The three-ply ranked lines (include/gpu_nnue.h at gn_line3) restated in Python from the CPU oracle
alone, for tests/test_lines3.py and tests/test_gpu_lines3.py.

A three-ply line of p is a two-ply line of a child of p, negated, so the rule is built on the two-ply
restatements, one per leaf rule: tests/lines2_rule.py (GN_LEAF_STATIC), tests/lines_extended_rule.py
(GN_LEAF_CHECKS), tests/quiesce_rule.py with tests/quiesce_pv_rule.py for the tails (GN_LEAF_QUIESCE),
and tests/see_rule.py's `pruned()` for GN_OPT_QUIESCE_SEE -- each over `oracle.child_fen(p, m)`.
`negate_ply`, `rule_score` and the material are tests/lines_rule.py's.

`root_step` is the root level alone, from arrays: what gn_rank_lines3_device computes from an
expansion's offsets, moves and child flags and each child's line 1 (and its gn_pv).  It reads nothing
of the oracle but the evaluation parameters for `rule_score`.
"""
import os

import numpy as np

import lines2_rule as R2
import lines_extended_rule as X
import lines_rule as R
import quiesce_pv_rule as PV
import quiesce_rule as Q
import see_rule as S

LEAF_STATIC, LEAF_CHECKS, LEAF_QUIESCE = 0, 1, 2
MAX_DEPTH3 = PV.MAX_PV - 3
FLAG_SEARCHED = Q.FLAG_SEARCHED
LINE3_DTYPE = np.dtype([("value", "<i4"), ("score", "<i4"), ("move", "<u2"), ("reply", "<u2"), ("reply2", "<u2"),
                        ("flags", "<u2"), ("plies", "<u2"), ("reserved", "<u2")])
EMPTY3 = (0, 0, 0, 0, 0, R.FLAG_NO_SCORE, 0, 0)
PV_DTYPE = PV.PV_DTYPE
SEED, N_WIDE = 0x5EED77E5, 48  # the seeded random set of the library-against-library test

# the fixtures of tests/golden/lines3_fens.txt
MATE_IN_2 = "4k3/8/R7/1R6/8/8/8/4K3 w - - 0 1"     # b5b7 e8d8 a6a8 and a6a7 e8d8 b5b8: mate 2
MATED_IN_2 = "4k3/1R6/R7/8/8/8/8/4K3 b - - 0 1"    # both moves are answered by a6a8: mate -1, plies 2
PLY1_ENDS = "k7/8/1K6/8/8/8/7Q/8 w - - 0 1"        # one mating move and six stalemating ones: plies 1
MOVES_218 = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"
BAD_FEN = "not a fen"
MATED = "rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3"


def _section(name):
    """The FENs of one `[name]` section of tests/golden/lines3_fens.txt, in the file's order."""
    out, on = [], False
    with open(os.path.join(R.HERE, "golden", "lines3_fens.txt")) as f:
        for l in f:
            l = l.strip()
            if l.startswith("["):
                on = l == f"[{name}]"
            elif on and l and not l.startswith("#"):
                out.append(l)
    return out


def static_fens():
    """The set of the static and the check-extended rule."""
    return _section("static")


def quiesce_fens(depth=1):
    """The low-material sets of the quiescent rule: depth 1, and the smaller one of depth 2 and of the
    pruned rule."""
    return _section("quiesce1" if depth == 1 else "quiesce2")


def all_lines2(O, big, small, fen, leaf, depth, mode):
    """The two-ply ranking of fen under the leaf rule (the caller enters see_rule.pruned() for Qs)."""
    if leaf == LEAF_STATIC:
        return R2.all_lines2(O, big, small, fen, mode)
    if leaf == LEAF_CHECKS:
        return X.all_lines2(O, big, small, fen, mode)
    return Q.all_lines2(O, big, small, fen, depth, mode)


def line2_pv(O, big, small, fen, line, leaf, depth, mode):
    """The gn_pv of a two-ply line (value, score, move, reply, flags, plies) of fen, as a list of moves."""
    mv = [line[2]]
    if line[5] == 2:
        mv.append(line[3])
        if leaf == LEAF_QUIESCE and line[4] & FLAG_SEARCHED:
            mv += PV.tails(O, big, small, O.child_fen(fen, line[2]), depth, mode)[line[3]]
    return mv


_lines3 = {}


def all_lines3(O, big, small, fen, leaf=LEAF_STATIC, depth=0, mode=0, pruned=False):
    """Every three-ply line of fen, ranked: [((value, score, move, reply, reply2, flags, plies, 0), PV)];
    [] for a bad position or one without a legal move."""
    key = (id(big), id(small), fen, leaf, depth, mode, pruned, bytes(O.eval_params()))
    if key in _lines3:
        return _lines3[key]
    try:
        _, moves, kids = O.expand_eval(big, small, fen, mode)
    except ValueError:
        moves, kids = [], []
    P = O.eval_params()
    material = R.wdl_material(fen, P) if moves else 0
    out = []
    for m, k in zip(moves, kids):
        check = bool(int(k["flags"]) & R.FLAG_IN_CHECK)
        c = O.child_fen(fen, m)
        if pruned:
            with S.pruned():
                l2 = all_lines2(O, big, small, c, leaf, depth, mode)
                pv = line2_pv(O, big, small, c, l2[0], leaf, depth, mode) if l2 else []
        else:
            l2 = all_lines2(O, big, small, c, leaf, depth, mode)
            pv = line2_pv(O, big, small, c, l2[0], leaf, depth, mode) if l2 else []
        fl = R.FLAG_IN_CHECK if check else 0
        if l2:
            L = l2[0]
            r3, reply, reply2, plies = L[0], L[2], L[3], 1 + L[5]
            fl |= L[4] & (R.FLAG_NO_MOVES | FLAG_SEARCHED)
        else:
            r3, reply, reply2, plies, fl = (-R.VALUE_MATE if check else 0), 0, 0, 1, fl | R.FLAG_NO_MOVES
        v = R.negate_ply(r3)
        score, mate = R.rule_score(v, material, P)
        out.append(((v, score, m, reply, reply2, fl | mate, plies, 0), [m] + pv))
    out.sort(key=lambda l: (-l[0][0], l[0][2]))
    _lines3[key] = out
    return out


def _pv(moves):
    out = np.zeros((), dtype=PV_DTYPE)
    out["len"] = len(moves)
    out["moves"][:len(moves)] = moves
    return out


def table(rows, K):
    """(lines[len(rows), K] as LINE3_DTYPE, pvs[len(rows), K] as PV_DTYPE) of ranked [(line, PV)] rows:
    the first K of each, then empty lines."""
    lines = np.zeros((len(rows), K), dtype=LINE3_DTYPE)
    pvs = np.zeros((len(rows), K), dtype=PV_DTYPE)
    for i, ls in enumerate(rows):
        for j in range(K):
            lines[i, j] = ls[j][0] if j < len(ls) else EMPTY3
            if j < len(ls):
                pvs[i, j] = _pv(ls[j][1])
    return lines, pvs


def lines3(O, big, small, fens, leaf, depth, mode, K, pruned=False, skip=()):
    """(lines, pvs) of the positions; the indices in skip have only empty lines (the games call)."""
    return table([[] if i in skip else all_lines3(O, big, small, f, leaf, depth, mode, pruned)
                  for i, f in enumerate(fens)], K)


def root_step(P, materials, offsets, moves, child_flags, child_lines, child_pvs, K, total=None):
    """gn_rank_lines3_device on arrays: materials[n] (the roots' win-rate material), offsets[n + 1],
    moves / child_flags over the children, child_lines (LINE2_DTYPE) and child_pvs (PV_DTYPE, or None)
    their line 1 and its PV; every range clamped to total and cut to its first 256 children (the
    header at gn_rank_lines3_device).  Returns (lines[n, K], pvs[n, K] or None)."""
    n = len(offsets) - 1
    total = len(child_lines) if total is None else total
    rows = []
    for i in range(n):
        b = min(int(offsets[i + 1]), total)
        a = min(int(offsets[i]), b)
        b = min(b, a + 256)
        row = []
        for j in range(a, b):
            L = child_lines[j]
            check = bool(int(child_flags[j]) & R.FLAG_IN_CHECK)
            none = bool(int(L["flags"]) & R.FLAG_NO_SCORE)
            fl = R.FLAG_IN_CHECK if check else 0
            if none:
                r3, reply, reply2, plies, fl, tail = (-R.VALUE_MATE if check else 0), 0, 0, 1, fl | R.FLAG_NO_MOVES, []
            else:
                r3, reply, reply2, plies = int(L["value"]), int(L["move"]), int(L["reply"]), 1 + int(L["plies"])
                fl |= int(L["flags"]) & (R.FLAG_NO_MOVES | FLAG_SEARCHED)
                tail = [] if child_pvs is None else child_pvs[j]["moves"][:int(child_pvs[j]["len"])].tolist()
            v = R.negate_ply(r3)
            score, mate = R.rule_score(v, materials[i], P)
            m = int(moves[j])
            row.append(((v, score, m, reply, reply2, fl | mate, plies, 0), [m] + tail[:PV.MAX_PV - 1]))
        row.sort(key=lambda l: (-l[0][0], l[0][2]))
        rows.append(row)
    lines, pvs = table(rows, K)
    return lines, (None if child_pvs is None else pvs)
