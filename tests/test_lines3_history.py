"""CPU-only checks of the three-ply ranked lines with game-history draws (include/gpu_nnue.h at
gn_line3, "game history"): the C-ABI surface, and the shapes that tests/golden/lines3_history_games.txt
must hold at the positions tests/test_gpu_lines3_history.py uses (tests/lines3_history_rule.py CHOSEN),
under the rule restated from the CPU oracle alone, mode FULL, top 8."""
import numpy as np
import pytest

import history_rule as H
import lines2_rule as R2
import lines3_history_rule as H3
import lines_rule as R

DRAW = H3.FLAG_DRAW


@pytest.fixture(scope="module")
def G():
    from fishnet_amd import build, gpu_nnue
    build.build()
    return gpu_nnue


@pytest.fixture(scope="module")
def games():
    return H3.fixture_games()


@pytest.fixture(scope="module")
def replayed(oracle_lib, games):
    return [oracle_lib.replay_game(root, moves)[0] for root, moves, _ in games]


@pytest.fixture(scope="module")
def lines(oracle_lib, oracle_nets, replayed):
    """{(game, position): (history lines, plain lines)} at the chosen positions, every line, ranked."""
    big, small = oracle_nets
    return {(g, k): ([l[0] for l in H3.all_lines3(oracle_lib, big, small, replayed[g], k, 0)],
                     [l[0] for l in H3.plain_lines3(oracle_lib, big, small, replayed[g], k, 0)])
            for g, ks in H3.CHOSEN.items() for k in ks}


def _top_draw_plies(ls):
    return {l[6] for l in ls[:8] if l[5] & DRAW}


def test_exports_and_constants(G):
    lib = G.lib()
    for s in ("gn_evaluate_games_lines3_history", "gn_rank_lines3_history_device", "gn_rank_lines2_ahead_device"):
        assert s in G.EXPORTS and hasattr(lib, s), s
    for m in ("evaluate_games_lines3_history", "rank_lines3_history_device", "rank_lines2_ahead_device"):
        assert callable(getattr(G.GpuNnue, m)), m
    assert G.FLAG_DRAW == DRAW == 512 and G.LINE3_DTYPE == H3.LINE3_DTYPE
    assert G.STAT_RANK3_NS == 130 and G.STAT_KEYS_NS == 123
    assert lib.gn_abi_version() == 4


def test_fixture_is_small_and_chosen_positions_exist(games, replayed):
    assert 5 <= len(games) <= 12 and sum(len(f) for f in replayed) <= 60
    assert set(H3.CHOSEN) == set(range(len(games)))
    assert all(root != R.START for root, _, _ in games)  # no root is the start position
    for g, ks in H3.CHOSEN.items():
        assert all(0 <= k < len(replayed[g]) for k in ks)
    # the rule stays cheap: sparse positions
    assert all(len(f.split()[0].replace("/", "").translate({ord(c): None for c in "12345678"})) <= 6
               for fens in replayed for f in fens)


def test_shuffle_third_occurrence_at_each_level(oracle_lib, replayed, lines):
    """Game 0 (and the perpetual, game 7): positions 0 and 4 are equal, position 0 is the window's first,
    and the third occurrence lies at distance 4 from position 4 at the child of 7, a grandchild of 6 and
    a great-grandchild of 5."""
    for g in (0, 7):
        fens = replayed[g]
        ids = [H.identity(f) for f in fens]
        assert ids[0] == ids[4] and ids.count(ids[0]) == 2 and len(fens) == 8
        assert H3.draw_depths(oracle_lib, fens, 7).get(1) == {"threefold"}
        assert "threefold" in H3.draw_depths(oracle_lib, fens, 6).get(2, ())
        assert "threefold" in H3.draw_depths(oracle_lib, fens, 5).get(3, ())
        assert 1 not in H3.draw_depths(oracle_lib, fens, 6) and 1 not in H3.draw_depths(oracle_lib, fens, 5)
        # position 4: every candidate is a second occurrence at most: nothing is drawn, the lines are the plain ones
        assert H3.draw_depths(oracle_lib, fens, 4) == {}
        occ = H.occurrences(oracle_lib, fens, 4)
        assert max(occ.values()) == 1
        assert lines[(g, 4)][0] == lines[(g, 4)][1] and not any(l[5] & DRAW for l in lines[(g, 4)][0])
    # the drawn lines the top 8 show: the child (plies 1), the reply (2) and the answer (3)
    assert 1 in _top_draw_plies(lines[(0, 7)][0]) and 2 in {l[6] for l in lines[(0, 6)][0] if l[5] & DRAW}
    assert 2 in _top_draw_plies(lines[(3, 6)][0]) and 1 in {l[6] for l in lines[(3, 7)][0] if l[5] & DRAW}
    assert _top_draw_plies(lines[(7, 7)][0]) == {1} and _top_draw_plies(lines[(7, 5)][0]) == {3}
    for key in ((0, 7), (3, 6), (7, 5), (7, 6), (7, 7)):
        assert lines[key][0][:8] != lines[key][1][:8], key  # the no-history rule gives other lines
    # the perpetual's positions 5 and 7 have one legal move, and line 1 of each is the drawn one
    assert len(lines[(7, 5)][0]) == 1 and len(lines[(7, 7)][0]) == 1
    assert lines[(7, 5)][0][0][:2] == (0, 0) and lines[(7, 5)][0][0][6] == 3
    assert lines[(7, 7)][0][0][3:5] == (0, 0) and lines[(7, 7)][0][0][6] == 1


def test_draw_changes_line_1s_move(lines):
    h, p = lines[(7, 6)]
    assert h[0][2] != p[0][2]


def test_fifty_move_part_alone(oracle_lib, games, replayed, lines):
    """Games 4, 5, 6: rule50 97, 98, 99 at the root and no history: the fifty-move part reaches the
    great-grandchild, the grandchild and the child."""
    for g, (r50, ply) in zip((4, 5, 6), ((97, 3), (98, 2), (99, 1))):
        assert games[g][1] == "" and int(replayed[g][0].split()[4]) == r50 and len(replayed[g]) == 1
        assert H3.draw_depths(oracle_lib, replayed[g], 0) == {ply: {"fifty"}}
        h, p = lines[(g, 0)]
        assert ply in _top_draw_plies(h) and h[:8] != p[:8] and not any(l[5] & DRAW for l in p)
        quiet = [l for l in h if l[6] == ply and l[5] & DRAW]
        assert quiet and all(l[0] == 0 and l[1] == 0 for l in quiet)


def test_mate_beats_the_draw_and_a_drawn_child_gives_check(oracle_lib, replayed, lines):
    fen = replayed[6][0]
    h, _ = lines[(6, 0)]
    by_move = {l[2]: l for l in h}
    mate = by_move[R2.uci_move("h2h8")]
    child = oracle_lib.child_fen(fen, R2.uci_move("h2h8"))
    assert int(child.split()[4]) == 100 and not oracle_lib.legal_moves(child)
    assert mate[0] == R.VALUE_MATE - 1 and mate[5] & R.FLAG_NO_MOVES and mate[5] & R.FLAG_IN_CHECK and not mate[5] & DRAW
    assert mate[6] == 1 and h[0] == mate
    check = by_move[R2.uci_move("h2a2")]
    assert check[5] == DRAW | R.FLAG_IN_CHECK and check[:2] == (0, 0) and check[3:5] == (0, 0) and check[6] == 1
    assert sum(1 for l in h if l[5] & DRAW) == len(h) - 1


def test_the_same_game_twice(oracle_lib, games, replayed, lines):
    """Games 1 and 2 are one game: an even number of positions, so that the copies' equal positions lie
    at even distances in one key array; within a copy the child of position 3 is a second occurrence
    and nothing is drawn, counted across the copies it would be drawn."""
    assert games[1] == games[2] and len(replayed[1]) % 2 == 0
    fens = replayed[1]
    assert H3.draw_depths(oracle_lib, fens, 3) == {}
    assert lines[(1, 3)][0] == lines[(1, 3)][1] == lines[(2, 3)][0]
    across = list(fens) + list(fens)
    assert H3.draw_depths(oracle_lib, across, len(fens) + 3).get(1) == {"threefold"}
    assert int(fens[4].split()[4]) >= len(fens) + 4  # the clock would let a walk reach the other copy


def test_skipped_positions_are_history(oracle_lib, games, replayed):
    root, moves, skip = games[3]
    assert skip == (1, 4) and root.split()[1] == "b"
    fens = replayed[3]
    assert H3.draw_depths(oracle_lib, fens, 7).get(1) == {"threefold"}
    assert 3 in H3.draw_depths(oracle_lib, fens, 5)
    big = small = None
    lines, pvs = H3.game_lines3(oracle_lib, big, small, fens, skip, 0, 3, only=(4,))
    assert all(tuple(x) == H3.EMPTY3 for x in lines[4].tolist()) and not pvs["len"].any()
    # without the skipped positions in the history, position 7's child would be a second occurrence
    assert H.drawn_moves(oracle_lib, [f for k, f in enumerate(fens) if k not in skip], 5) == {}


def test_game_lines3_table(oracle_lib, oracle_nets, replayed):
    big, small = oracle_nets
    lines, pvs = H3.game_lines3(oracle_lib, big, small, replayed[7], (), 0, 3, only=(5, 7))
    assert lines.shape == (8, 3) and lines.dtype == H3.LINE3_DTYPE
    assert not lines[4].view(np.uint16).any() and not lines[6].view(np.uint16).any()
    assert lines[5][0]["plies"] == 3 and pvs[5][0]["len"] == 3 and lines[5][1].tolist() == H3.EMPTY3
    assert lines[7][0]["plies"] == 1 and pvs[7][0]["len"] == 1
    assert pvs[5][0]["moves"][:3].tolist() == [int(lines[5][0][f]) for f in ("move", "reply", "reply2")]
