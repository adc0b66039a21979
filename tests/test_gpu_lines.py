"""Ranked lines per position (MultiPV; include/gpu_nnue.h at gn_line) on the GPU against the rule
restated from the CPU oracle (tests/lines_rule.py): gn_expand_device + gn_rank_children_device,
and gn_evaluate_games_lines."""
import json
import os

import numpy as np
import pytest

import lines_rule as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KS = (1, 3, 8)
MODES = (0, 1)  # FULL, BIG


def _expand_and_rank(ctx, boards, mode, ks):
    """gn_expand_device, then gn_rank_children_device for every K of ks on its device-resident
    outputs: (parent records, {K: lines[n, K]})."""
    from fishnet_amd import gpu_nnue as G
    n = len(boards)
    cap = 256 * n
    b = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                       ("mv", cap * 2), ("co", cap * G.EVAL_SIZE), ("ln", n * 8 * 12))}
    b["b"].upload(boards)
    ctx.expand_device(b["b"], n, mode, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
    out = {}
    for K in ks:
        ctx.rank_children_device(b["b"], n, b["off"], b["mv"], b["co"], K, b["ln"])
        ctx.synchronize()
        out[K] = b["ln"].download(G.LINE_DTYPE, n * K).reshape(n, K)
    parents = b["po"].download(G.EVAL_DTYPE, n)
    for x in b.values():
        x.free()
    return parents, out


@pytest.fixture(scope="module")
def positions():
    from fishnet_amd import gpu_nnue as G
    fens = R.fixture_fens() + G.boards_to_fens(G.random_positions(R.SEED, 0, R.N_RANDOM, 160))
    return fens, G.pack_fens(fens)[0]


@pytest.fixture(scope="module")
def expected(positions, oracle_nets, oracle_lib):
    """The helper's 8 lines of every position, per mode (computed once; K < 8 is its prefix)."""
    big, small = oracle_nets
    return {mode: R.lines(oracle_lib, big, small, positions[0], mode, 8) for mode in MODES}


@pytest.fixture(scope="module")
def ranked(gpu_ctx, positions):
    return {mode: _expand_and_rank(gpu_ctx, positions[1], mode, KS) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
def test_rank_children_device_vs_rule(ranked, expected, positions, mode, K):
    got, exp = ranked[mode][1][K], expected[mode][:, :K]
    assert got.shape == exp.shape
    for i in np.flatnonzero((got != exp).any(axis=1))[:5]:
        assert got[i].tolist() == exp[i].tolist(), (positions[0][i], mode, K)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("mode", MODES)
def test_prefix_property(ranked, mode):
    lines = ranked[mode][1]
    assert np.array_equal(lines[8][:, :3], lines[3]) and np.array_equal(lines[8][:, :1], lines[1])


def test_line_one_agrees_with_the_score_rule(gpu_ctx, oracle_nets, oracle_lib):
    """In-check parents none of whose replies is in check with a legal move: line 1 is the
    position's score / best_move (the score rule does not go deeper there)."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    g = json.load(open(os.path.join(HERE, "golden", "score_fens.json")))
    fens = sorted({r[0] for r in g["results"]["full"] if r[6] & G.FLAG_SEARCHED} | set(R.fixture_fens()))
    rec = oracle_lib.eval_fens(big, small, fens, 0)
    sel = [f for f, r in zip(fens, rec) if r["flags"] & G.FLAG_SEARCHED
           and not R.reply_in_check_with_move(oracle_lib, big, small, f, 0)]
    assert len(sel) >= 2 and R.fixture_fens()[3] in sel
    parents, lines = _expand_and_rank(gpu_ctx, G.pack_fens(sel)[0], 0, (1,))
    exp = oracle_lib.eval_fens(big, small, sel, 0)
    assert np.array_equal(parents, exp)
    for f, p, l in zip(sel, parents, lines[1][:, 0]):
        assert p["flags"] & G.FLAG_SEARCHED, f
        assert l["move"] == p["best_move"] and l["score"] == p["score"], f
        assert (l["flags"] & G.FLAG_MATE) == (p["flags"] & G.FLAG_MATE), f


# ---- gn_evaluate_games_lines ------------------------------------------------------------------
K_GAMES = 3


@pytest.fixture(scope="module")
def games():
    from fishnet_amd import gpu_nnue as G
    ucis = G.random_games_uci(0x5EED11E6, 0, 64, 80)
    out = [(R.START, u, (2, 40) if g % 5 == 0 else ()) for g, u in enumerate(ucis)]
    out[7] = (R.START, "e2e4 e7e5 e1e3 g8f6", ())  # an illegal move
    out[11] = ("not a fen", "e2e4", ())             # a bad root
    out[13] = (R.fixture_fens()[0], "", (0,))       # its only position skipped
    return out


@pytest.fixture(scope="module")
def games_lines(gpu_ctx, games):
    return gpu_ctx.evaluate_games_lines(games, K_GAMES, 0)


def test_games_lines_positions_equal_evaluate_games(gpu_ctx, games, games_lines):
    from fishnet_amd import gpu_nnue as G
    offs, status, pos, lines = games_lines
    arr, _keep = G._games_array(games)
    for children in (False, True):
        ref = gpu_ctx.evaluate_games_arrays(arr, len(games), 0, children=children)
        assert offs.tobytes() == ref[0].tobytes() and status.tobytes() == ref[1].tobytes()
        assert pos.tobytes() == ref[2].tobytes()
    assert status[7] == G.E_ILLEGAL_MOVE and status[11] == G.E_INVALID and offs[8] == offs[7] and offs[12] == offs[11]
    assert lines.shape == (len(pos), K_GAMES) and len(pos) > 4000


def test_games_lines_vs_rule(games, games_lines, oracle_nets, oracle_lib):
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    offs, status, pos, lines = games_lines
    # every 23rd position, every skipped one, and the positions around the failed games
    sample, fens = [], {}
    for g, (root, uci, skip) in enumerate(games):
        if status[g]:
            continue
        fs = G.boards_to_fens(G.replay_game(root, uci)[0])
        assert len(fs) == offs[g + 1] - offs[g]
        for p, f in enumerate(fs):
            at = int(offs[g]) + p
            if at % 23 == 0 or p in skip or g in (6, 8, 10, 12, 13):
                sample.append(at), fens.setdefault(at, (f, p in skip))
    assert len(sample) >= 200
    empty = np.array([R.EMPTY] * K_GAMES, dtype=R.LINE_DTYPE)
    live = [at for at in sample if not fens[at][1]]
    exp = R.lines(oracle_lib, big, small, [fens[at][0] for at in live], 0, K_GAMES)
    for at, e in zip(live, exp):
        assert lines[at].tolist() == e.tolist(), fens[at][0]
    skipped = [at for at in sample if fens[at][1]]
    assert len(skipped) >= 20
    for at in skipped:
        assert pos[at]["flags"] & G.FLAG_SKIPPED and np.array_equal(lines[at], empty)


def test_games_lines_chunked_and_two_slots(gpu_ctx, games, games_lines, synth_big_path, synth_small_path):
    """The same bytes from >= 3 chunks (GN_OPT_CHUNK_PARENTS 1,000 of ~5,000 evaluated positions)
    and from a context over two device slots."""
    from fishnet_amd import gpu_nnue as G
    assert len(games_lines[2]) >= 3 * 1000 + 200
    try:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 1000)
        chunked = gpu_ctx.evaluate_games_lines(games, K_GAMES, 0)
    finally:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        sharded = two.evaluate_games_lines(games, K_GAMES, 0)
    finally:
        two.close()
    for other in (chunked, sharded):
        for a, b in zip(games_lines, other):
            assert a.tobytes() == b.tobytes()
    assert gpu_ctx.get_option(G.STAT_RANK_NS) > 0
    # games without a skipped position (the path that ranks straight into the caller's array)
    offs, _, pos, lines = games_lines
    o2, s2, p2, l2 = gpu_ctx.evaluate_games_lines(games[21:25], K_GAMES, 0)
    a, b = int(offs[21]), int(offs[25])
    assert not s2.any() and p2.tobytes() == pos[a:b].tobytes() and l2.tobytes() == lines[a:b].tobytes()


def test_lines_argument_checks(gpu_ctx, games, games_lines):
    from fishnet_amd import gpu_nnue as G
    for k in (0, 9):
        with pytest.raises(G.GnError) as e:
            gpu_ctx.evaluate_games_lines(games[:2], k, 0)
        assert e.value.code == G.E_INVALID
        d = gpu_ctx.alloc(4096)
        with pytest.raises(G.GnError) as e:
            gpu_ctx.rank_children_device(d, 1, d, d, d, k, d)
        assert e.value.code == G.E_INVALID
        d.free()
    # a too-small position capacity: GN_E_CAPACITY with the offsets filled
    arr, _keep = G._games_array(games)
    ng = len(games)
    offs, status = np.zeros(ng + 1, dtype=np.uint32), np.zeros(ng, dtype=np.int32)
    pos, lines = np.zeros(16, dtype=G.EVAL_DTYPE), np.zeros((16, K_GAMES), dtype=G.LINE_DTYPE)
    rc = G.lib().gn_evaluate_games_lines(gpu_ctx.h, arr, ng, 0, K_GAMES, offs.ctypes.data, status.ctypes.data,
                                         pos.ctypes.data, 16, lines.ctypes.data)
    assert rc == G.E_CAPACITY and offs.tobytes() == games_lines[0].tobytes()
    again = gpu_ctx.evaluate_games_lines(games, K_GAMES, 0)
    for a, b in zip(games_lines, again):
        assert a.tobytes() == b.tobytes()
