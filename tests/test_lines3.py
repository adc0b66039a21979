"""The three-ply ranked lines on the CPU: the rule's known answers (include/gpu_nnue.h at gn_line3,
restated in tests/lines3_rule.py from the oracle alone), the struct and dtype sizes, the rule's
consequences checked on the restatement itself, the numpy root step against it, and the conditions
the inputs of tests/test_gpu_lines3.py must meet so that none of its tests passes vacuously."""
import os
import re

import numpy as np
import pytest

import lines2_rule as R2
import lines3_rule as L3
import lines_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mv = R2.uci_move


@pytest.fixture(scope="module")
def rule(oracle_lib, oracle_nets):
    big, small = oracle_nets
    return lambda fen, leaf=L3.LEAF_STATIC, depth=0, mode=0, pruned=False: \
        L3.all_lines3(oracle_lib, big, small, fen, leaf, depth, mode, pruned)


def test_sizes_and_header_fields():
    from fishnet_amd import gpu_nnue as G
    assert L3.LINE3_DTYPE.itemsize == G.LINE3_DTYPE.itemsize == 20 and L3.LINE3_DTYPE == G.LINE3_DTYPE
    assert [L3.LINE3_DTYPE.fields[n][1] for n in L3.LINE3_DTYPE.names] == [0, 4, 8, 10, 12, 14, 16, 18]
    assert G.PV_DTYPE.itemsize == 16 and G.MAX_QUIESCE_DEPTH3 == L3.MAX_DEPTH3 == 3 and 3 + G.MAX_QUIESCE_DEPTH3 == G.MAX_PV
    assert (G.LEAF_STATIC, G.LEAF_CHECKS, G.LEAF_QUIESCE) == (0, 1, 2) and G.STAT_RANK3_NS == 130
    hdr = open(os.path.join(ROOT, "include", "gpu_nnue.h")).read()
    body = re.search(r"typedef struct gn_line3 \{(.*?)\} gn_line3;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(d.split()[0], d.split()[1]) for d in body.split(";") if d.strip()]
    assert [f for _, f in fields] == list(L3.LINE3_DTYPE.names)
    assert [t for t, _ in fields] == ["int32_t", "int32_t"] + ["uint16_t"] * 6
    for name, value in (("GN_LEAF_STATIC", "0"), ("GN_LEAF_CHECKS", "1"), ("GN_LEAF_QUIESCE", "2"),
                        ("GN_STAT_RANK3_NS", "130"), ("GN_MAX_QUIESCE_DEPTH3", "(GN_MAX_PV - 3)")):
        assert re.search(r"#define %s\s+%s\s" % (name, re.escape(value)), hdr), name
    assert re.search(r"#define GN_ABI_VERSION 4\b", hdr)
    for sym in ("gn_evaluate_lines3", "gn_evaluate_games_lines3", "gn_rank_lines3_device"):
        assert sym in G.EXPORTS


def test_mate_in_two_and_its_tie(rule):
    ls = rule(L3.MATE_IN_2)
    assert len(ls) == 33
    (a, pa), (b, pb) = ls[0], ls[1]
    assert a == (31997, 2, mv("b5b7"), mv("e8d8"), mv("a6a8"), R.FLAG_MATE, 3, 0)
    assert b == (31997, 2, mv("a6a7"), mv("e8d8"), mv("b5b8"), R.FLAG_MATE, 3, 0)
    assert a[2] < b[2] and pa == list(a[2:5]) and pb == list(b[2:5])
    assert ls[2][0][0] < R.VALUE_MATE_IN_MAX_PLY


def test_best_move_changes_with_the_third_ply(rule, oracle_lib, oracle_nets):
    big, small = oracle_nets
    two = R2.all_lines2(oracle_lib, big, small, L3.MATE_IN_2, 0)
    assert two[0][2] == mv("a6a7") and two[0][0] == -892  # (the synthetic nets' static value)
    assert rule(L3.MATE_IN_2)[0][0][2] == mv("b5b7")


def test_mated_by_the_reply(rule):
    ls = rule(L3.MATED_IN_2)
    assert [l for l, _ in ls] == [
        (-31998, -1, mv("e8d8"), mv("a6a8"), 0, R.FLAG_MATE | R.FLAG_NO_MOVES, 2, 0),
        (-31998, -1, mv("e8f8"), mv("a6a8"), 0, R.FLAG_MATE | R.FLAG_NO_MOVES, 2, 0)]
    assert [pv for _, pv in ls] == [[mv("e8d8"), mv("a6a8")], [mv("e8f8"), mv("a6a8")]]


def test_moves_that_end_the_game_at_ply_one(rule):
    assert L3.PLY1_ENDS in L3.static_fens()
    ls = rule(L3.PLY1_ENDS)
    assert ls[0][0] == (31999, 1, mv("h2h8"), 0, 0, R.FLAG_MATE | R.FLAG_IN_CHECK | R.FLAG_NO_MOVES, 1, 0) and ls[0][1] == [mv("h2h8")]
    stale = [l for l, _ in ls if l[6] == 1 and l[0] == 0]
    assert len(stale) == 6 and all(l[5] == R.FLAG_NO_MOVES and l[3] == l[4] == 0 and l[1] == 0 for l in stale)
    assert all(l[6] in (1, 3) for l, _ in ls)


def test_defenders_side_of_a_mate_in_two(rule):
    """`mate -2` at plies == 3: only a leaf rule that searches sees the mating promotion."""
    fen = L3.quiesce_fens(1)[0]
    (l, pv), = rule(fen, L3.LEAF_QUIESCE, 1)
    assert l == (-31996, -2, mv("h8g8"), mv("a6a7"), mv("g8h8"), R.FLAG_MATE | L3.FLAG_SEARCHED, 3, 0)
    assert len(pv) == 4 and pv[:3] == list(l[2:5]) and pv[3] & 0xFFF == mv("a7a8") and pv[3] >> 12 == 7  # a7a8q
    (s, spv), = rule(fen)
    assert abs(s[0]) < R.VALUE_MATE_IN_MAX_PLY and not s[5] & L3.FLAG_SEARCHED and len(spv) == 3


def test_empty_positions(rule, oracle_lib, oracle_nets):
    big, small = oracle_nets
    for fen in (L3.BAD_FEN, L3.MATED, "k7/8/8/8/8/8/5q2/7K w - - 0 1"):
        assert rule(fen) == []
    lines, pvs = L3.lines3(oracle_lib, big, small, [L3.BAD_FEN, L3.MATED_IN_2], 0, 0, 0, 3)
    assert [tuple(x) for x in lines[0].tolist()] == [L3.EMPTY3] * 3 and tuple(lines[1, 2].tolist()) == L3.EMPTY3
    assert not pvs[0].view(np.uint16).any() and pvs[1]["len"].tolist() == [2, 2, 0]


LEAVES = ((L3.LEAF_STATIC, 0, False, "static"), (L3.LEAF_CHECKS, 0, False, "static"), (L3.LEAF_QUIESCE, 1, False, "quiesce1"),
          (L3.LEAF_QUIESCE, 2, False, "quiesce2"), (L3.LEAF_QUIESCE, 1, True, "quiesce2"))


def _set(name):
    return L3.static_fens() if name == "static" else L3.quiesce_fens(1 if name == "quiesce1" else 2)


@pytest.mark.parametrize("leaf,depth,pruned,name", LEAVES)
def test_consequences_on_the_rule(rule, oracle_lib, oracle_nets, leaf, depth, pruned, name):
    """Played out from p with child_fen alone, every PV's moves are legal where they are played and it
    ends in the position whose own value -- mate, stalemate or the static final_v -- carried back by
    negate_ply once per move is the line's value; the order is value descending, then the move; and
    the flags and plies agree with the PV."""
    big, small = oracle_nets
    O = oracle_lib
    for fen in _set(name):
        ls = rule(fen, leaf, depth, 0, pruned)
        assert [(-l[0], l[2]) for l, _ in ls] == sorted((-l[0], l[2]) for l, _ in ls)
        for l, pv in ls:
            assert pv[:l[6]] == [l[2], l[3], l[4]][:l[6]] and [l[2], l[3], l[4]][l[6]:] == [0] * (3 - l[6])
            assert len(pv) <= L3.PV.MAX_PV and (len(pv) == l[6] or (leaf == L3.LEAF_QUIESCE and l[6] == 3 and l[5] & L3.FLAG_SEARCHED))
            assert bool(l[5] & R.FLAG_NO_MOVES) == (l[6] < 3) and not l[5] & (R.FLAG_NO_SCORE | 512)
            f = fen
            for m in pv:
                assert m in O.legal_moves(f)
                f = O.child_fen(f, m)
            if leaf == L3.LEAF_CHECKS and l[5] & L3.FLAG_SEARCHED:
                continue  # (the check extension's replies are not reported: the PV stops above them)
            if O.legal_moves(f):
                v = int(O.eval_fens(big, small, [f], 0)["final_v"][0])
            else:
                v = -R.VALUE_MATE if int(O.eval_fens(big, small, [f], 0)["flags"][0]) & R.FLAG_IN_CHECK else 0
            for _ in pv:
                v = R.negate_ply(v)
            assert v == l[0], (fen, l, pv)


@pytest.mark.parametrize("leaf,depth,pruned,name", LEAVES)
def test_root_step_restatement_equals_the_rule(oracle_lib, oracle_nets, leaf, depth, pruned, name):
    """root_step over arrays made from the rule's own two-ply lines gives the rule's three-ply lines."""
    from contextlib import nullcontext
    big, small = oracle_nets
    O = oracle_lib
    fens = _set(name)
    offsets, moves, flags, clines, cpvs, materials = [0], [], [], [], [], []
    P = O.eval_params()
    for fen in fens:
        try:
            _, ms, kids = O.expand_eval(big, small, fen, 0)
        except ValueError:
            ms, kids = [], []
        materials.append(R.wdl_material(fen, P) if ms else 0)
        for m, k in zip(ms, kids):
            c = O.child_fen(fen, m)
            with (L3.S.pruned() if pruned else nullcontext()):
                l2 = L3.all_lines2(O, big, small, c, leaf, depth, 0)
                pv = L3.line2_pv(O, big, small, c, l2[0], leaf, depth, 0) if l2 else []
            moves.append(m), flags.append(int(k["flags"]))
            clines.append(l2[0] if l2 else R2.EMPTY2), cpvs.append(L3._pv(pv))
        offsets.append(len(moves))
    clines = np.array(clines, dtype=R2.LINE2_DTYPE)
    cpvs = np.array(cpvs, dtype=L3.PV_DTYPE)
    for K in (1, 3, 8):
        lines, pvs = L3.root_step(P, materials, offsets, moves, flags, clines, cpvs, K)
        want, wpvs = L3.lines3(O, big, small, fens, leaf, depth, 0, K, pruned)
        assert lines.tobytes() == want.tobytes() and pvs.tobytes() == wpvs.tobytes()
    # every range is clamped to total: the children at and beyond it do not exist
    total = offsets[2] - 1
    lines, _ = L3.root_step(P, materials, offsets, moves, flags, clines, None, 8, total=total)
    assert (lines[2:]["flags"] == R.FLAG_NO_SCORE).all() and (lines[1]["plies"] > 0).sum() == min(8, offsets[2] - offsets[1] - 1)


# ---- the conditions on the GPU tests' inputs ------------------------------------------------------

def test_static_set_covers_every_segment_shape(rule, oracle_lib, oracle_nets):
    big, small = oracle_nets
    fens = L3.static_fens()
    assert 12 <= len(fens) <= 20 and L3.MOVES_218 in fens and L3.BAD_FEN in fens and L3.MATED in fens
    counts = [len(rule(f)) for f in fens]
    assert max(counts) == 218 > 64 and any(33 <= c <= 64 for c in counts) and any(0 < c < 8 for c in counts)
    assert counts.count(0) >= 3 and any(0 < c < 3 for c in counts)
    changed = [f for f in fens if rule(f) and rule(f)[0][0][2] != R2.all_lines2(oracle_lib, big, small, f, 0)[0][2]]
    assert L3.MATE_IN_2 in changed and len(changed) >= 2
    plies = {l[6] for f in fens for l, _ in rule(f)}
    assert plies == {1, 2, 3}
    ends = {l[0] for f in fens for l, _ in rule(f) if l[6] == 1}
    assert ends == {31999, 0}  # a move that mates and a move that stalemates, each at plies 1
    # the check-extended rule differs from the static one somewhere, and carries its flag
    ext = [l for f in fens for l, _ in rule(f, L3.LEAF_CHECKS)]
    assert any(l[5] & L3.FLAG_SEARCHED for l in ext) and ext != [l for f in fens for l, _ in rule(f)]


@pytest.mark.parametrize("depth", (1, 2))
def test_quiescent_sets_have_searched_lines_with_and_without_tails(rule, depth):
    fens = L3.quiesce_fens(depth)
    assert len(fens) <= 8
    ls = [x for f in fens for x in rule(f, L3.LEAF_QUIESCE, depth)]
    assert any(l[5] & L3.FLAG_SEARCHED and len(pv) > 3 for l, pv in ls)
    assert any(not l[5] & L3.FLAG_SEARCHED for l, _ in ls)
    assert any(l[5] & L3.FLAG_SEARCHED and len(pv) == 3 for l, pv in ls)  # searched, the leaf stands pat
    assert max(len(pv) for _, pv in ls) <= 3 + depth
    if depth == 2:
        assert max(len(pv) for _, pv in ls) == 5


def test_pruned_set_changes_a_value(rule):
    fens = L3.quiesce_fens(2)
    plain = [l[0] for f in fens for l, _ in sorted(rule(f, L3.LEAF_QUIESCE, 1), key=lambda x: x[0][2])]
    pruned = [l[0] for f in fens for l, _ in sorted(rule(f, L3.LEAF_QUIESCE, 1, 0, True), key=lambda x: x[0][2])]
    assert len(plain) == len(pruned) and sum(a != b for a, b in zip(plain, pruned)) >= 3
