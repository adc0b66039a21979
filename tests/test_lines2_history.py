"""CPU-only checks of the two-ply ranked lines with game-history draws (include/gpu_nnue.h at
gn_line2): the C-ABI surface, and the properties of the fixtures tests/golden/history_games.txt
and tests/golden/lines2_history_games.txt under the rule restated from the CPU oracle alone
(tests/lines2_history_rule.py), mode FULL, top 8."""
import numpy as np
import pytest

import history_rule as H
import lines2_history_rule as H2
import lines2_rule as R2
import lines_rule as R


@pytest.fixture(scope="module")
def G():
    from fishnet_amd import build, gpu_nnue
    build.build()
    return gpu_nnue


@pytest.fixture(scope="module")
def replayed(oracle_lib):
    """[(fens of positions 0..=moves, skip)] of both fixtures' games."""
    return [(oracle_lib.replay_game(root, moves)[0], skip) for root, moves, skip in H2.both_fixtures()]


@pytest.fixture(scope="module")
def lines(oracle_lib, oracle_nets, replayed):
    """Per game, lines[positions, 8] by the restated rule, mode FULL."""
    big, small = oracle_nets
    return [H2.game_lines2(oracle_lib, big, small, fens, skip, 0, 8) for fens, skip in replayed]


def test_exports_and_constants(G):
    lib = G.lib()
    for s in ("gn_rank_lines2_history_device", "gn_evaluate_games_lines2", "gn_evaluate_games_lines2_history"):
        assert s in G.EXPORTS and hasattr(lib, s), s
    for m in ("evaluate_games_lines2", "evaluate_games_lines2_history", "rank_lines2_history_device"):
        assert callable(getattr(G.GpuNnue, m)), m
    assert G.FLAG_DRAW == H2.FLAG_DRAW == 512 and G.LINE2_DTYPE == H2.LINE2_DTYPE and G.LINE2_DTYPE.itemsize == 16
    assert G.STAT_RANK2_NS == 122 and G.STAT_KEYS_NS == 123
    assert lib.gn_abi_version() == 4


def test_fixture_size_and_forced_replies(oracle_lib, replayed):
    new = H2.fixture_games()
    assert 3 <= len(new) <= 16 and sum(len(f) for f, _ in replayed[-len(new):]) <= 400
    roots = [root for root, _, _ in new]
    assert roots[:3] == ["7k/5Q2/5K2/6P1/8/8/8/8 w - - 0 1", "k7/2Q5/2K5/1P6/8/8/8/8 w - - 0 1",
                         "8/8/8/8/6p1/5k2/5q2/7K b - - 0 1"]
    assert [m.split()[:4] for _, m, _ in new[:3]] == ["f7f8 h8h7 f8f7 h7h8".split(), "c7c8 a8a7 c8c7 a7a8".split(),
                                                      "f2f1 h1h2 f1f2 h2h1".split()]
    for (_, moves, skip), (fens, _) in zip(new[:3], replayed[-len(new):]):
        assert moves.split() == moves.split()[:4] * 3 and not skip and len(fens) == 13
        assert all(len(oracle_lib.legal_moves(fens[k])) == 1 for k in range(1, 13, 2))


def test_perpetual_check_position_6(oracle_lib, oracle_nets, replayed, lines):
    """Position 6 of each perpetual: the depth-1 rule draws nothing, the top 8 hold a drawn line of
    two plies, and its reply is the single forced one, into a third occurrence."""
    O = oracle_lib
    big, small = oracle_nets
    found = 0
    for (fens, _), ls in list(zip(replayed, lines))[-len(H2.fixture_games()):][:3]:
        assert not H.drawn_moves(O, fens, 6)
        drawn = ls[6][(ls[6]["flags"] & H2.FLAG_DRAW) != 0]
        assert len(drawn) >= 1 and (drawn["plies"] == 2).all()
        forced = 0
        for l in drawn:
            c = O.child_fen(fens[6], int(l["move"]))
            if O.legal_moves(c) == [int(l["reply"])]:
                g = H.identity(O.child_fen(c, int(l["reply"])))
                assert [H.identity(f) for f in fens[:7]].count(g) == 2
                forced += 1
        assert forced >= 1
        # neither existing rule gives these lines
        assert ls[6].tolist() != R2.lines2(O, big, small, [fens[6]], 0, 8)[0].tolist()
        found += 1
    assert found == 3


def test_fixture_properties(oracle_lib, oracle_nets, replayed, lines):
    O = oracle_lib
    big, small = oracle_nets
    deep_without_child_draw = fifty2 = plies1 = same = differ = 0
    for (fens, skip), ls in zip(replayed, lines):
        plain = R2.lines2(O, big, small, fens, 0, 8)
        for k in range(len(fens)):
            if k in skip:
                assert ls[k].tolist() == [H2.EMPTY2] * 8
                continue
            draw = (ls[k]["flags"] & H2.FLAG_DRAW) != 0
            deep = draw & (ls[k]["plies"] == 2)
            if deep.any() and not H.drawn_moves(O, fens, k):
                deep_without_child_draw += 1
            for l in ls[k][deep]:
                g = O.child_fen(O.child_fen(fens[k], int(l["move"])), int(l["reply"]))
                fifty2 += int(g.split()[4]) >= 100
            plies1 += int((draw & (ls[k]["plies"] == 1)).sum())
            if ls[k].tolist() == plain[k].tolist():
                same += 1
            else:
                differ += 1
    assert deep_without_child_draw >= 3 and fifty2 >= 6 and plies1 >= 100
    assert same >= 30 and differ >= 30
    every = np.concatenate(lines).reshape(-1)
    drawn = every[(every["flags"] & H2.FLAG_DRAW) != 0]
    assert (drawn["value"] == 0).all() and (drawn["score"] == 0).all()
    assert not (drawn["flags"] & (R.FLAG_NO_MOVES | R.FLAG_MATE | R.FLAG_NO_SCORE)).any()
    full = every[(every["flags"] & R.FLAG_NO_SCORE) == 0]
    assert ((full["plies"] == 1) == (full["reply"] == 0)).all() and np.isin(full["plies"], (1, 2)).all()


def test_draws_nothing_is_the_plain_rule(oracle_lib, oracle_nets, replayed, lines):
    """Where no child and no grandchild is drawn the lines are lines2_rule's; both cases occur."""
    O = oracle_lib
    big, small = oracle_nets
    quiet = loud = 0
    for (fens, skip), ls in zip(replayed, lines):
        for k in range(len(fens)):
            if k in skip:
                continue
            if H2.draws_nothing(O, big, small, fens, k, 0):
                assert ls[k].tolist() == R2.lines2(O, big, small, [fens[k]], 0, 8)[0].tolist(), fens[k]
                quiet += 1
            else:
                loud += 1
    assert quiet >= 10 and loud >= 30
