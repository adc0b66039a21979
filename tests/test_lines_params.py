"""What the parameter sets of tests/lines_param_sets.py do to the ranked lines, measured on the CPU
with the restated rules alone: how many ties among ordinary values each set forces at depth 1, among
a child's best replies at depth 2, and between lines drawn by rule and undrawn ones.  These are the
coverage conditions of tests/test_gpu_lines_params.py: they keep its comparisons biting on the sort
keys' lower fields (move, reply, draw bit) when a net, a seed or a fixture changes.  Every threshold
sits well below the figure measured today, which the assertion message prints."""
import itertools

import numpy as np
import pytest

import history_rule as H
import lines2_rule as R2
import lines_param_sets as LP
import lines_rule as R

FX = R.fixture_fens()


def _ordinary(flags):
    return not flags & (R.FLAG_NO_MOVES | R.FLAG_MATE)


def _ordinary_tie(ls):
    """Two of the ranked depth-1 lines ls tie at a value that is neither a mate nor a game's end."""
    for _, grp in itertools.groupby(ls, key=lambda l: l[0]):
        if sum(1 for l in grp if _ordinary(l[3])) >= 2:
            return True
    return False


def depth1_ties(O, big, small, fens, mode):
    """(positions, with an ordinary tie among the top 8, with more than 8 lines, with an ordinary tie
    across lines 8 and 9)."""
    top8 = more8 = across = 0
    for f in fens:
        ls = R.all_lines(O, big, small, f, mode)
        top8 += _ordinary_tie(ls[:8])
        if len(ls) > 8:
            more8 += 1
            across += ls[7][0] == ls[8][0] and _ordinary(ls[7][3]) and _ordinary(ls[8][3])
    return len(fens), top8, more8, across


def depth2_ties(O, big, small, fens, mode):
    """(children that have replies, those whose best replies tie, those with two ordinary best replies)."""
    n = tie = ordinary = 0
    for f in fens:
        for _, _, replies in R2.child_replies(O, big, small, f, mode) or ():
            if not replies:
                continue
            n += 1
            best = [l for l in replies if l[0] == replies[0][0]]
            tie += len(best) >= 2
            ordinary += sum(1 for l in best if _ordinary(l[3])) >= 2
    return n, tie, ordinary


def history_ties(O, big, small, games, mode):
    """(positions, those with a drawn line and an undrawn static one of equal value adjacent within
    the first 9 lines, children with replies, those whose best replies tie between a drawn and an undrawn
    grandchild, of those: the drawn reply wins, the undrawn one wins)."""
    positions = adjacent = children = tied = drawn_wins = undrawn_wins = 0
    for root, moves, skip in games:
        fens = O.replay_game(root, moves)[0]
        for k in range(len(fens)):
            if k in skip:
                continue
            positions += 1
            ls = H.all_lines(O, big, small, fens, k, mode)[:9]
            adjacent += any(a[0] == b[0] and (a[3] ^ b[3]) & H.FLAG_DRAW and not (a[3] | b[3]) & R.FLAG_NO_MOVES
                            for a, b in zip(ls, ls[1:]))
            drawn = H.drawn_moves(O, fens, k)
            for m, c, alive in H._children(O, fens[k]):
                if not alive or m in drawn:
                    continue
                children += 1
                rl = H.all_lines(O, big, small, list(fens[:k + 1]) + [c], k + 1, mode)
                best = [l[3] & H.FLAG_DRAW for l in rl if l[0] == rl[0][0]]
                if any(best) and not all(best):
                    tied += 1
                    drawn_wins += bool(best[0])
                    undrawn_wins += not best[0]
    return positions, adjacent, children, tied, drawn_wins, undrawn_wins


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_depth1_clamp0_ties_everywhere(oracle_lib, oracle_nets, mode):
    fens = LP.depth1_fens()
    with LP.under(oracle_lib, "clamp0"):
        n, top8, more8, across = depth1_ties(oracle_lib, *oracle_nets, fens, mode)
    msg = f"mode {mode}: {top8} of {n} positions tie among the top 8, {across} of {more8} across lines 8 and 9"
    assert n == len(FX) + LP.N_RANDOM1 and top8 >= 0.8 * n and more8 >= 0.8 * n and across >= 0.8 * more8, msg


def test_depth2_best_replies_tie_under_the_clamp_only(oracle_lib, oracle_nets):
    fens = LP.depth2_fens()
    msgs = []
    with LP.under(oracle_lib, "rule50/clamp"):
        for mode in (0, 1):
            n, tie, ordinary = depth2_ties(oracle_lib, *oracle_nets, fens, mode)
            msgs.append(f"rule50/clamp mode {mode}: {ordinary} of {n} children have two ordinary best replies ({tie} tie)")
            assert n >= 500 and ordinary >= 0.5 * n, msgs
    n, tie, ordinary = depth2_ties(oracle_lib, *oracle_nets, fens, 0)
    msgs.append(f"defaults mode 0: {tie} of {n} children's best replies tie ({ordinary} at an ordinary value)")
    assert n >= 500 and tie < 0.05 * n, msgs  # the gap the sets close


def test_history_draws_tie_with_undrawn_lines_under_clamp0_only(oracle_lib, oracle_nets):
    games = LP.history_games()
    with LP.under(oracle_lib, "clamp0"):
        got = history_ties(oracle_lib, *oracle_nets, games, 1)
    positions, adjacent, children, tied, drawn_wins, undrawn_wins = got
    msg = (f"clamp0 mode 1: {adjacent} of {positions} positions with a drawn line next to an undrawn one of equal value; "
           f"{tied} of {children} children's best replies tie drawn with undrawn: the drawn reply wins {drawn_wins} "
           f"times, the undrawn one {undrawn_wins} times")
    assert len(games) == 15 and adjacent >= 50 and tied >= 100 and drawn_wins >= 20 and undrawn_wins >= 20, msg
    d = history_ties(oracle_lib, *oracle_nets, games, 1)
    assert d[0] == positions and d[2] == children and d[1] == 0 and d[3] == 0, f"defaults mode 1: {d}"


def test_poly_keeps_the_order_and_material_changes_it(oracle_lib, oracle_nets):
    """Depth 1, mode FULL, the 8 lines the GPU test compares."""
    fens = LP.depth1_fens()
    base = R.lines(oracle_lib, *oracle_nets, fens, 0, 8)
    has_line = (base[:, 0]["flags"] & R.FLAG_NO_SCORE) == 0
    figures = {}
    for name in ("ties-poly", "material"):
        with LP.under(oracle_lib, name):
            ls = R.lines(oracle_lib, *oracle_nets, fens, 0, 8)
        assert np.array_equal((ls[:, 0]["flags"] & R.FLAG_NO_SCORE) == 0, has_line)
        figures[name] = (int((ls != base).any(axis=1).sum()), int((ls["move"] != base["move"]).any(axis=1).sum()))
    msg = f"of {int(has_line.sum())} positions with a line, (some line differs, the move order differs): {figures}"
    for name in figures:
        assert figures[name][0] >= 0.9 * has_line.sum(), msg
    assert figures["ties-poly"][1] == 0 and figures["material"][1] >= 10, msg


def test_restated_to_cp_follows_every_set(oracle_lib, synth_small_path):
    """lines_rule.to_cp with the set's win-rate parameters == the oracle's own final_cp (the positions
    of tests/test_lines.py::test_helper_score_arithmetic)."""
    O = oracle_lib
    small = O.Net(synth_small_path)
    seen = set()
    for name in LP.LINE_SETS:
        with LP.under(O, name) as P:
            assert bytes(O.eval_params()) == bytes(P)
            for fen in (R.START, FX[8], FX[9]):
                parent = O.expand_eval(None, small, fen, 2)[0]
                assert R.to_cp(parent[2], R.wdl_material(fen, P), P) == parent[3], (name, fen, parent)
                seen.add((name, parent[3]))
        assert bytes(O.eval_params()) != bytes(P)  # the defaults are back
    assert len({cp for name, cp in seen if name == "ties-poly"}) >= 2  # (not all zero)
