"""Ranked lines per position (MultiPV; include/gpu_nnue.h at gn_line) without a GPU: the rule's
Python restatement (tests/lines_rule.py) on the fixed positions of tests/golden/lines_fens.txt,
the binding, and the coverage of the positions the GPU tests (tests/test_gpu_lines.py) rank."""
import os

import numpy as np
import pytest

import lines_rule as R

FX = R.fixture_fens()
BIG218, KQ, ROOKS, ONE_REPLY, SIX_REPLIES, STALEMATED, MATED = FX[:7]


@pytest.fixture(scope="module")
def small_only(oracle_lib, synth_small_path):
    """(oracle, big, small, mode): the seeded small net in mode SMALL."""
    return oracle_lib, None, oracle_lib.Net(synth_small_path), 2


def test_fixture_file():
    assert len(FX) == 10 and R.START in FX


def test_helper_218_moves(small_only):
    O, big, small, mode = small_only
    ls = R.all_lines(O, big, small, BIG218, mode)
    assert len(ls) == 218
    top = R.lines(O, big, small, [BIG218], mode, 8)[0]
    assert top[:7]["value"].tolist() == [31999] * 7 and top[:7]["score"].tolist() == [1] * 7
    assert all(f & R.FLAG_MATE and f & R.FLAG_NO_MOVES and f & R.FLAG_IN_CHECK for f in top[:7]["flags"])
    assert top[:7]["move"].tolist() == sorted(top[:7]["move"].tolist())
    assert sum(1 for l in ls if l[0] == 31999) == 7
    stalemating = sorted(l[2] for l in ls if l[3] & R.FLAG_NO_MOVES and not l[3] & R.FLAG_IN_CHECK)
    assert len(stalemating) == 175
    # The 175 stalemating moves tie at 0 and rank among themselves by ascending move, the first of
    # them the smallest-encoded one.  (They do not start at line 8 with this net: the other 36
    # moves leave black to move far behind, a static value the rule negates to white's side, so
    # those that come out positive rank between the mates and the draws.)
    zero = [l for l in ls if l[0] == 0]
    assert [l[2] for l in zero if l[3] & R.FLAG_NO_MOVES] == stalemating
    assert all(l[1] == 0 and l[3] == R.FLAG_NO_MOVES for l in zero if l[3] & R.FLAG_NO_MOVES)
    first0 = next(i for i, l in enumerate(ls) if l[0] == 0)
    assert ls[first0][2] == min(l[2] for l in zero)
    assert first0 == 7 + sum(1 for l in ls if 0 < l[0] < 31999)
    assert top[7]["value"] == max(l[0] for l in ls if l[0] < 31999) and not top[7]["flags"] & R.FLAG_NO_MOVES


def test_helper_mates_first(small_only):
    O, big, small, mode = small_only
    for fen, n in ((KQ, 27), (ROOKS, 23)):
        ls = R.all_lines(O, big, small, fen, mode)
        assert len(ls) == n
        assert ls[0][0] == 31999 and ls[0][1] == 1 and ls[0][3] & R.FLAG_MATE and ls[1][0] < 31999
    ls = R.all_lines(O, big, small, KQ, mode)
    assert sum(1 for l in ls if l[3] & R.FLAG_NO_MOVES and not l[3] & R.FLAG_IN_CHECK) == 6
    assert sum(1 for l in ls if l[3] & R.FLAG_IN_CHECK and not l[3] & R.FLAG_NO_MOVES) == 4


def test_helper_empty_lines(small_only):
    O, big, small, mode = small_only
    got = R.lines(O, big, small, [ONE_REPLY, SIX_REPLIES, STALEMATED, MATED, "garbage"], mode, 8)
    empty = np.array([R.EMPTY], dtype=R.LINE_DTYPE)[0]
    assert got[0, 0]["flags"] & R.FLAG_NO_SCORE == 0 and (got[0, 1:] == empty).all()
    assert (got[1, :6]["flags"] & R.FLAG_NO_SCORE == 0).all() and (got[1, 6:] == empty).all()
    assert (got[2:] == empty).all()
    # values descending, ties by ascending move
    six = got[1, :6]
    assert all((a["value"], -int(a["move"])) > (b["value"], -int(b["move"])) for a, b in zip(six, six[1:]))


def test_helper_score_arithmetic(oracle_lib):
    """to_cp restated == the oracle's own final_cp wherever a record's final_v is the value."""
    O = oracle_lib
    from fishnet_amd import synthnet
    small = O.Net(synthnet.cached_synth_net(128, 2))
    P = O.eval_params()
    for fen in (R.START, FX[8], FX[9]):
        parent, _, kids = O.expand_eval(None, small, fen, 2)
        assert R.to_cp(parent[2], R.wdl_material(fen, P), P) == parent[3]
    assert R.rule_score(31999, 0, P) == (1, R.FLAG_MATE) and R.rule_score(-31998, 0, P) == (-1, R.FLAG_MATE)
    assert R.rule_score(31997, 0, P) == (2, R.FLAG_MATE) and R.rule_score(-32000, 0, P) == (0, R.FLAG_MATE)
    assert [R.round_half_away(x) for x in (0.5, -0.5, 1.4999, -2.5, 2.0)] == [1, -1, 1, -3, 2]
    assert R.negate_ply(-32000) == 31999 and R.negate_ply(31999) == -31998 and R.negate_ply(100) == -100


def test_binding_has_lines():
    """LINE_DTYPE, the two exports and the library's symbols (absent before this feature)."""
    from fishnet_amd import build, gpu_nnue as G
    assert G.LINE_DTYPE.itemsize == 12 and G.LINE_DTYPE == R.LINE_DTYPE
    assert "gn_rank_children_device" in G.EXPORTS and "gn_evaluate_games_lines" in G.EXPORTS
    build.build()
    L = G.lib()
    assert all(hasattr(L, name) for name in G.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(R.HERE), "include", "gpu_nnue.h")).read()
    assert "#define GN_MAX_LINES 8" in hdr and G.MAX_LINES == 8 and "#define GN_ABI_VERSION 4" in hdr


def test_coverage_of_the_gpu_positions(small_only):
    """What tests/test_gpu_lines.py ranks (the fixture + the seeded random set) holds every case
    the kernel treats differently: segments of 0, 1, fewer than K = 8, more than 64 and more than
    128 children (one, two and more passes of a wave or half wave), ties among the top 8, a
    stalemating and a mating child."""
    O, big, small, mode = small_only
    from fishnet_amd import gpu_nnue as G
    fens = FX + G.boards_to_fens(G.random_positions(R.SEED, 0, R.N_RANDOM, 160))
    assert len(fens) == 10 + R.N_RANDOM
    all_ls = [R.all_lines(O, big, small, f, mode) for f in fens]
    lens = {len(l) for l in all_ls}
    assert 0 in lens and 1 in lens and any(1 < n < 8 for n in lens)
    assert any(32 < n <= 64 for n in lens) and any(n > 64 for n in lens) and any(n > 128 for n in lens)
    assert any(len({l[0] for l in ls[:8]}) < len(ls[:8]) for ls in all_ls)
    flags = [l[3] for ls in all_ls for l in ls]
    assert any(f & R.FLAG_NO_MOVES and not f & R.FLAG_IN_CHECK for f in flags)
    assert any(f & R.FLAG_NO_MOVES and f & R.FLAG_IN_CHECK for f in flags)
    # more than the fixture's own: the random set has mates and in-check parents too
    rnd = all_ls[10:]
    assert any(l[3] & R.FLAG_MATE for ls in rnd for l in ls)
