"""Check-extended ranked lines (include/gpu_nnue.h at gn_line, "check-extended") without a GPU: the
rule's Python restatement (tests/lines_extended_rule.py) on the fixed positions of
tests/golden/lines_extended_fens.txt, its invariant against the oracle's own score rule, the
binding, and the conditions on the inputs the GPU tests (tests/test_gpu_lines_extended.py) rank."""
import os

import pytest

import history_rule as H
import lines2_rule as R2
import lines_extended_rule as X
import lines_rule as R

FX = X.fixture_fens()
mv = R2.uci_move
MODE = 0  # FULL: both nets


@pytest.fixture(scope="module")
def nets(oracle_lib, oracle_nets):
    return (oracle_lib,) + tuple(oracle_nets)


def one_ply_inputs():
    from fishnet_amd import gpu_nnue as G
    return FX + R.fixture_fens() + G.boards_to_fens(G.random_positions(X.SEED1, 0, X.N_RANDOM1, 160))


def two_ply_inputs():
    from fishnet_amd import gpu_nnue as G
    return FX + R2.fixture_fens() + G.boards_to_fens(G.random_positions(X.SEED2, 0, X.N_RANDOM2, 160))


def test_fixture_file():
    assert FX == [X.MATING_REPLY, X.MATE_IN_2, X.TWO_PLY_A, X.TWO_PLY_B, X.TWO_PLY_MATE, X.FIFTY]


def test_a_check_that_allows_a_mating_reply(nets):
    """The mate values are forced through every reply: they do not depend on the net."""
    O, big, small = nets
    for mode in (0, 1, 2):
        ls = {l[2]: l for l in X.all_lines(O, big, small, X.MATING_REPLY, mode)}
        assert ls[mv("e4e7")] == (-31998, -1, mv("e4e7"), R.FLAG_MATE | R.FLAG_IN_CHECK | X.FLAG_SEARCHED)
        plain = {l[2]: l for l in R.all_lines(O, big, small, X.MATING_REPLY, mode)}
        assert not plain[mv("e4e7")][3] & (R.FLAG_MATE | X.FLAG_SEARCHED)  # today: a static number


def test_mate_in_two_through_a_check(nets):
    O, big, small = nets
    for mode in (0, 1, 2):
        ls = X.all_lines(O, big, small, X.MATE_IN_2, mode)
        by = {l[2]: l for l in ls}
        for m in (mv("e7f7"), mv("e7f8")):
            assert by[m] == (31997, 2, m, R.FLAG_MATE | R.FLAG_IN_CHECK | X.FLAG_SEARCHED)
        tied = [l[2] for l in ls if l[0] == 31997]  # ties to the smaller move
        assert tied == sorted(tied) and tied.index(mv("e7f7")) + 1 == tied.index(mv("e7f8"))


def test_two_plies_chosen_reply_extended(nets):
    O, big, small = nets
    for fen in (X.TWO_PLY_A, X.TWO_PLY_B, X.TWO_PLY_MATE):
        ext = X.all_lines2(O, big, small, fen, MODE)
        assert sum(1 for l in ext[:8] if l[4] & X.FLAG_SEARCHED) >= 1, fen
        assert all(l[5] == 2 and l[3] for l in ext if l[4] & X.FLAG_SEARCHED)  # plies stays 2: a reply is shown
        assert ext != R2.all_lines2(O, big, small, fen, MODE)
    for mode in (0, 1, 2):
        by = {l[2]: l for l in X.all_lines2(O, big, small, X.TWO_PLY_MATE, mode)}
        assert by[mv("d7b5")] == (-31996, -2, mv("d7b5"), mv("b2c2"), R.FLAG_MATE | X.FLAG_SEARCHED, 2)


def test_the_draw_comes_before_the_extension(nets):
    O, big, small = nets
    m = mv("a1a8")
    child = O.child_fen(X.FIFTY, m)
    assert int(child.split()[4]) == 100 and O.legal_moves(child)
    drawn = H.drawn_moves(O, [X.FIFTY], 0)
    assert drawn[m] == "fifty"
    hist = {l[2]: l for l in X.all_lines(O, big, small, X.FIFTY, MODE, drawn)}
    assert hist[m] == (0, 0, m, X.FLAG_DRAW | R.FLAG_IN_CHECK)
    plain = {l[2]: l for l in X.all_lines(O, big, small, X.FIFTY, MODE)}
    assert plain[m][3] == R.FLAG_IN_CHECK | X.FLAG_SEARCHED and plain[m][0] != 0
    # the games forms: a game of one position
    assert X.game_lines(O, big, small, [X.FIFTY], (), MODE, 8, True)[0].tolist() == [
        l for l in X.all_lines(O, big, small, X.FIFTY, MODE, drawn)[:8]]
    assert X.game_lines(O, big, small, [X.FIFTY], (), MODE, 8, False)[0].tolist() == [
        l for l in X.all_lines(O, big, small, X.FIFTY, MODE)[:8]]


def test_extended_value_is_the_oracles_score_rule(nets):
    """The invariant the feature rests on: for every extended leaf x, rule_score(value(x, 2)), the
    mate flag and the best reply are what the oracle's own evaluation of x reports."""
    O, big, small = nets
    P = O.eval_params()
    checked = mates = 0
    for fen in one_ply_inputs():
        for m, c, check, alive, _ in X.leaves(O, big, small, fen, MODE) or []:
            if not (check and alive):
                continue
            v, best = X.value(O, big, small, c, 2, MODE)
            score, mate = R.rule_score(v, R.wdl_material(c, P), P)
            e = O.eval_fen(big, small, c, MODE)
            assert (score, mate, best) == (e[4], e[5] & R.FLAG_MATE, e[6]) and e[5] & X.FLAG_SEARCHED, (fen, m)
            checked += 1
            mates += bool(mate)
    assert checked >= 100 and mates >= 1


def test_equal_to_the_plain_rule_where_nothing_is_extended(nets):
    O, big, small = nets
    same = differ = 0
    for fen in one_ply_inputs():
        ext = X.all_lines(O, big, small, fen, MODE)
        if any(l[3] & X.FLAG_SEARCHED for l in ext):
            differ += 1
        else:
            assert ext == R.all_lines(O, big, small, fen, MODE), fen
            same += 1
    assert same >= 20 and differ >= 20
    for fen in two_ply_inputs()[:24]:
        ext = X.all_lines2(O, big, small, fen, MODE)
        kids = X.leaves(O, big, small, fen, MODE) or []
        if not any(e != X.NOT_EXTENDED for _, c, _, alive, _ in kids if alive
                   for e in X.extensions(O, big, small, c, MODE)):
            assert ext == R2.all_lines2(O, big, small, fen, MODE), fen


def test_conditions_on_the_gpu_inputs(nets):
    """What tests/test_gpu_lines_extended.py asserts of its inputs, met by the reference alone: these
    make the GPU tests fail on code that does not extend."""
    O, big, small = nets
    for mode in (0, 1):
        extended = differ = mate_lines = 0
        lens = set()
        for fen in one_ply_inputs():
            ext, plain = X.all_lines(O, big, small, fen, mode), R.all_lines(O, big, small, fen, mode)
            lens.add(len(ext))
            extended += sum(1 for e in X.extensions(O, big, small, fen, mode) if e != X.NOT_EXTENDED)
            differ += [l[:3] for l in ext[:8]] != [l[:3] for l in plain[:8]]
            mate_lines += sum(1 for l in ext[:8] if l[3] & X.FLAG_SEARCHED and l[3] & R.FLAG_MATE)
        assert extended >= 100 and differ >= 20 and mate_lines >= 1
        assert any(0 < n < 8 for n in lens) and any(n > 32 for n in lens)
        searched = mates = 0
        for fen in two_ply_inputs():
            top = X.all_lines2(O, big, small, fen, mode)[:8]
            searched += sum(1 for l in top if l[4] & X.FLAG_SEARCHED)
            mates += sum(1 for l in top if l[4] & X.FLAG_SEARCHED and l[4] & R.FLAG_MATE)
        assert searched >= 4 and mates >= 1


def test_binding_has_the_extended_calls():
    """The six exports, NOT_EXTENDED, the two statistics and the library's symbols (absent before
    this feature)."""
    from fishnet_amd import build, gpu_nnue as G
    names = ("gn_extend_checks_device", "gn_rank_children_extended_device", "gn_rank_lines2_extended_device",
             "gn_evaluate_lines2_extended", "gn_evaluate_games_lines2_extended", "gn_evaluate_games_lines_extended")
    assert all(n in G.EXPORTS for n in names)
    assert G.NOT_EXTENDED == X.NOT_EXTENDED == -2 ** 31 and (G.STAT_EXTEND_NS, G.STAT_EXTENDED_LEAVES) == (124, 125)
    build.build()
    L = G.lib()
    assert all(hasattr(L, n) for n in G.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(R.HERE), "include", "gpu_nnue.h")).read()
    assert "#define GN_NOT_EXTENDED INT32_MIN" in hdr and "#define GN_ABI_VERSION 4" in hdr
    assert "#define GN_STAT_EXTEND_NS 124" in hdr and "#define GN_STAT_EXTENDED_LEAVES 125" in hdr
