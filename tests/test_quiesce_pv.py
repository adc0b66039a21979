"""The quiescence's own variation (include/gpu_nnue.h at gn_pv) without a GPU: the rule's restatement
(tests/quiesce_pv_rule.py) on the inputs tests/test_gpu_quiesce_pv.py uses -- the replay identity, the
rule's consequences, the conditions on the inputs (PV lengths and both kinds of ties occur, counted as
quiesce_pv_rule states) -- and the binding."""
import collections
import os

import pytest

import lines_param_sets as LP
import lines_rule as R
import quiesce_pv_rule as PV
import quiesce_rule as Q
from test_quiesce import inputs, inputs3


@pytest.fixture(scope="module")
def nets(oracle_lib, oracle_nets):
    return (oracle_lib,) + tuple(oracle_nets)


def _searched(O, big, small, fens, mode):
    for fen in fens:
        for m, c, check, live, static, srch in Q.leaves(O, big, small, fen, mode) or []:
            if srch:
                yield fen, m, c, check, static


def _measure(O, big, small, fens, depth, mode):
    """(PV lengths among the searched leaves, the tie counts), the replay identity and the rule's
    consequences asserted on every searched leaf."""
    lengths, counts = collections.Counter(), PV.Counts()
    for fen, m, c, check, static in _searched(O, big, small, fens, mode):
        pv = PV.pvq(O, big, small, c, depth, mode, check, static)
        assert len(pv) <= depth
        # (replayed asserts that every move is legal where it is played, and noisy unless in check)
        assert PV.replayed(O, big, small, c, pv, mode, check, static) == Q.Q(O, big, small, c, depth, mode, check, static)[0], \
            (fen, m, depth, mode, pv)
        if check:
            assert len(pv) >= 1  # no stand pat in check
        lengths[len(pv)] += 1
        PV.count_ties(O, big, small, c, depth, mode, check, static, counts)
    return lengths, counts


@pytest.mark.parametrize("mode", (0, 1))
def test_replay_identity_and_lengths(nets, mode):
    O, big, small = nets
    for depth, fens in ((1, inputs()), (2, inputs()), (3, inputs3())):
        lengths, counts = _measure(O, big, small, fens, depth, mode)
        n = sum(lengths.values())
        print(f"mode {mode} depth {depth}: {n} searched leaves, PV lengths {dict(sorted(lengths.items()))}, "
              f"{counts.move_ties} move ties, {counts.stand_pat_ties} stand-pat ties on {counts.nodes} visited nodes")
        assert n == (516 if depth == 3 else 2027)
        if depth == 2 and mode == 0:
            assert lengths[2] >= 500 and lengths[1] >= 100 and lengths[0] >= 500
            assert counts.move_ties >= 5 and counts.stand_pat_ties >= 1
        if depth == 3:
            assert lengths[3] >= 100


@pytest.mark.parametrize("name", ("clamp0", "rule50/clamp"))
def test_both_tie_rules_decide_under_the_tie_forcing_sets(nets, name):
    O, big, small = nets
    with LP.under(O, name):
        lengths, counts = _measure(O, big, small, inputs3(), 2, 0)
    print(f"{name}: PV lengths {dict(sorted(lengths.items()))}, {counts.move_ties} move ties, "
          f"{counts.stand_pat_ties} stand-pat ties on {counts.nodes} visited nodes")
    assert counts.stand_pat_ties >= 1000 and counts.move_ties >= 50


def test_tie_rules_at_depth_1_under_clamp0(nets):
    """Under clamp0 every ordinary value is 0: a leaf not in check whose moves reach nothing better
    stands pat (the shorter PV), and a leaf in check plays the smallest of its best moves."""
    O, big, small = nets
    with LP.under(O, "clamp0"):
        seen_check = seen_quiet = 0
        for fen, m, c, check, static in _searched(O, big, small, inputs3(), 0):
            pv = PV.pvq(O, big, small, c, 1, 0, check, static)
            vals = [(R.negate_ply(Q.Q(O, big, small, k[1], 0, 0, k[2], k[3])[0]), k[0])
                    for k in Q.searched_moves(O, big, small, c, 0, check)]
            top = max(v for v, _ in vals)
            if check:
                assert pv == (min(mv for v, mv in vals if v == top),)
                seen_check += 1
            elif top <= static:
                assert pv == ()
                seen_quiet += 1
        assert seen_check >= 5 and seen_quiet >= 100


def test_pv_of_a_line(nets):
    """gn_pv of the rule's lines: [move] + the tail exactly on searched lines, empty lines empty, and a
    drawn line (the history forms) without a tail although its leaf would be searched."""
    import history_rule as H
    O, big, small = nets
    fens = Q.fixture_fens()
    lines = Q.lines(O, big, small, fens, 2, 0, 8)
    pvs = PV.line_pvs(O, big, small, fens, lines, 2, 0)
    empty = (lines["flags"] & R.FLAG_NO_SCORE) != 0
    srch = (lines["flags"] & Q.FLAG_SEARCHED) != 0
    assert (pvs["len"][empty] == 0).all() and (pvs["len"][~empty & ~srch] == 1).all()
    assert (pvs["moves"][:, :, 0] == lines["move"]).all() and (pvs["len"][srch] >= 1).all() and (pvs["len"][srch] > 1).any()
    assert (pvs["len"] <= 1 + 2).all() and not pvs["reserved"].any()
    heads = PV.line_pvs(O, big, small, fens, lines, 2, 0, with_tails=False)
    assert (heads["len"] == (~empty).astype(int)).all()
    fen = fens[-1]
    drawn = H.drawn_moves(O, [fen], 0)
    rows = Q._table([Q.all_lines(O, big, small, fen, 2, 0, drawn)[:8]], 8, R.LINE_DTYPE, R.EMPTY)
    dpv = PV.line_pvs(O, big, small, [fen], rows, 2, 0)
    assert (dpv["len"][0, :3] == 1).all() and (dpv["len"][0, 3:] == 0).all()
    two = Q.lines2(O, big, small, fens, 1, 0, 8)
    pv2 = PV.line2_pvs(O, big, small, fens, two, 1, 0)
    live = (two["flags"] & R.FLAG_NO_SCORE) == 0
    s2 = live & ((two["flags"] & Q.FLAG_SEARCHED) != 0)
    assert (pv2["len"][live & ~s2] == two["plies"][live & ~s2]).all() and (two["plies"][s2] == 2).all()
    assert (pv2["len"][s2] >= 2).all() and (pv2["len"][s2] == 3).any() and (pv2["len"] <= 3).all()


def test_binding_has_the_pv_calls():
    """The six exports, the struct, the statistic and the library's symbols (absent before this feature)."""
    from fishnet_amd import build, gpu_nnue as G
    names = ("gn_quiesce_pv_device", "gn_line_pvs_device", "gn_line2_pvs_device", "gn_evaluate_lines2_quiescent_pv",
             "gn_evaluate_games_lines2_quiescent_pv", "gn_evaluate_games_lines_quiescent_pv")
    assert all(n in G.EXPORTS for n in names)
    assert G.STAT_PV_NS == 129 and G.MAX_PV == PV.MAX_PV == 6 and G.PV_DTYPE == PV.PV_DTYPE and G.PV_DTYPE.itemsize == 16
    build.build()
    L = G.lib()
    assert all(hasattr(L, n) for n in names)
    hdr = open(os.path.join(os.path.dirname(R.HERE), "include", "gpu_nnue.h")).read()
    assert "#define GN_STAT_PV_NS 129" in hdr and "#define GN_ABI_VERSION 4" in hdr
    assert "#define GN_MAX_PV (2 + GN_MAX_QUIESCE_DEPTH)" in hdr
