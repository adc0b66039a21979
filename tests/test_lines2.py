"""Two-ply ranked lines (include/gpu_nnue.h at gn_line2) without a GPU: the rule's Python
restatement (tests/lines2_rule.py) on the fixed positions of tests/golden/lines2_fens.txt, the
binding, and the coverage of the positions the GPU tests (tests/test_gpu_lines2.py) rank."""
import os

import numpy as np
import pytest

import lines2_rule as R2
import lines_rule as R

FX = R2.fixture_fens()


@pytest.fixture(scope="module")
def small_only(oracle_lib, synth_small_path):
    """(oracle, big, small, mode): the seeded small net in mode SMALL."""
    return oracle_lib, None, oracle_lib.Net(synth_small_path), 2


@pytest.fixture(scope="module")
def fixture_lines(small_only):
    """Per fixture position: (its children's depth-1 lines, its two-ply lines)."""
    O, big, small, mode = small_only
    return [(R2.child_replies(O, big, small, f, mode), R2.all_lines2(O, big, small, f, mode)) for f in FX]


def test_fixture_file():
    assert FX[:10] == R.fixture_fens() and R2.MATE_IN_ONE in FX and R2.TWO_MATES in FX and len(FX) == 12


def test_a_move_that_allows_mate_in_one(small_only):
    O, big, small, mode = small_only
    ls = {l[2]: l for l in R2.all_lines2(O, big, small, R2.MATE_IN_ONE, mode)}
    assert len(ls) == 19
    l = ls[R2.uci_move("g2g4")]
    assert l == (-31998, -1, R2.uci_move("g2g4"), R2.uci_move("d8h4"), R.FLAG_MATE, 2)
    # it is the only such move, and it ranks last
    assert [m for m, x in ls.items() if x[4] & R.FLAG_MATE] == [l[2]]
    assert R2.all_lines2(O, big, small, R2.MATE_IN_ONE, mode)[-1] == l
    # depth 1 values the same move by the child's static evaluation: no mate in sight
    d1 = {x[2]: x for x in R.all_lines(O, big, small, R2.MATE_IN_ONE, mode)}
    assert not d1[l[2]][3] & R.FLAG_MATE


def test_tied_mating_replies_go_to_the_smaller_encoding(small_only):
    O, big, small, mode = small_only
    ls = {l[2]: l for l in R2.all_lines2(O, big, small, R2.TWO_MATES, mode)}
    assert len(ls) == 6
    a1, b1 = R2.uci_move("a8a1"), R2.uci_move("b8b1")
    assert (a1, b1) == (3584, 3649)
    replies = R.all_lines(O, big, small, O.child_fen(R2.TWO_MATES, R2.uci_move("c5c6")), mode)
    assert [(x[0], x[2]) for x in replies[:3]][:2] == [(31999, a1), (31999, b1)] and replies[2][0] < 31999
    assert ls[R2.uci_move("c5c6")] == (-31998, -1, R2.uci_move("c5c6"), a1, R.FLAG_MATE, 2)
    assert sum(1 for l in ls.values() if l[4] & R.FLAG_MATE) == 1


def test_lines_that_end_the_game_and_empty_lines(small_only):
    O, big, small, mode = small_only
    BIG218, KQ, _, ONE_REPLY, SIX_REPLIES, STALEMATED, MATED = FX[:7]
    top = R2.lines2(O, big, small, [BIG218], mode, 8)[0]
    # the 7 mating moves: value 31999, mate 1, no reply, one ply, ascending moves
    assert top[:7]["value"].tolist() == [31999] * 7 and top[:7]["score"].tolist() == [1] * 7
    assert top[:7]["reply"].tolist() == [0] * 7 and top[:7]["plies"].tolist() == [1] * 7
    assert all(f == R.FLAG_MATE | R.FLAG_NO_MOVES | R.FLAG_IN_CHECK for f in top[:7]["flags"])
    assert top[:7]["move"].tolist() == sorted(top[:7]["move"].tolist())
    assert top[7]["value"] < 31999 and not top[7]["flags"] & R.FLAG_MATE
    stale = [l for l in R2.all_lines2(O, big, small, KQ, mode) if l[4] & R.FLAG_NO_MOVES and not l[4] & R.FLAG_IN_CHECK]
    assert len(stale) == 6 and all(l[:2] == (0, 0) and l[3:] == (0, R.FLAG_NO_MOVES, 1) for l in stale)
    got = R2.lines2(O, big, small, [ONE_REPLY, SIX_REPLIES, STALEMATED, MATED, "garbage"], mode, 8)
    empty = np.array([R2.EMPTY2], dtype=R2.LINE2_DTYPE)[0]
    assert got[0, 0]["plies"] == 2 and (got[0, 1:] == empty).all()
    assert (got[1, :6]["flags"] & R.FLAG_NO_SCORE == 0).all() and (got[1, 6:] == empty).all()
    assert (got[2:] == empty).all()
    six = got[1, :6]
    assert all((a["value"], -int(a["move"])) > (b["value"], -int(b["move"])) for a, b in zip(six, six[1:]))


def test_coverage_of_the_fixed_positions(small_only, fixture_lines):
    """The fixed positions alone (the GPU tests add seeded random ones) hold every case
    rank_lines2_kernel treats differently."""
    O, big, small, mode = small_only
    kids = [(check, replies) for ks, _ in fixture_lines for _, check, replies in (ks or [])]
    # a child with more than 32 replies: a second pass of the group's lanes
    assert any(len(r) > 32 for _, r in kids) and any(0 < len(r) <= 32 for _, r in kids)
    # children without a reply: mated, stalemated
    assert any(not r and check for check, r in kids) and any(not r and not check for check, r in kids)
    # a child in check with replies: its static value is not used
    assert any(r and check for check, r in kids)
    # parents with fewer moves than groups, more than 64, and none
    n_moves = [len(l2) for _, l2 in fixture_lines]
    assert any(0 < n < 8 for n in n_moves) and any(n > 64 for n in n_moves) and 0 in n_moves
    assert all(ks is not None for ks, _ in fixture_lines)  # every fixed position parses
    # a two-way tie for a child's best reply
    assert any(len(r) > 1 and r[0][0] == r[1][0] for _, r in kids)
    # ties among a parent's top 8
    assert any(len({l[0] for l in l2[:8]}) < len(l2[:8]) for _, l2 in fixture_lines)
    # what the feature exists for: a first line whose move is not depth 1's first move
    differs = [f for f, (_, l2) in zip(FX, fixture_lines)
               if l2 and l2[0][2] != R.all_lines(O, big, small, f, mode)[0][2]]
    assert differs


def test_binding_has_lines2():
    """LINE2_DTYPE, the two exports and the library's symbols (absent before this feature)."""
    from fishnet_amd import build, gpu_nnue as G
    assert G.LINE2_DTYPE.itemsize == 16 and G.LINE2_DTYPE == R2.LINE2_DTYPE
    assert "gn_rank_lines2_device" in G.EXPORTS and "gn_evaluate_lines2" in G.EXPORTS
    assert G.STAT_RANK2_NS == 122
    build.build()
    L = G.lib()
    assert all(hasattr(L, name) for name in G.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(R.HERE), "include", "gpu_nnue.h")).read()
    assert "#define GN_STAT_RANK2_NS 122" in hdr and "#define GN_ABI_VERSION 4" in hdr
    assert "} gn_line2;" in hdr and G.ABI_VERSION == 4
