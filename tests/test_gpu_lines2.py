"""Two-ply ranked lines (include/gpu_nnue.h at gn_line2) on the GPU: gn_expand2_device +
gn_rank_lines2_device against the rule restated from the CPU oracle (tests/lines2_rule.py) and,
on a wide seeded set, against gn_rank_children_device over the children as parents;
gn_evaluate_lines2 against the device path."""
import numpy as np
import pytest

import lines2_rule as R2
import lines_rule as R

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
MODES = (0, 1)  # FULL, BIG


def _free(bufs):
    for v in bufs.values():
        if hasattr(v, "free"):
            v.free()


def _expand2_and_rank(ctx, boards, mode, ks):
    """gn_expand2_device, then gn_rank_lines2_device for every K of ks on its device-resident
    outputs: (parent records, {K: lines[n, K]})."""
    from fishnet_amd import gpu_nnue as G
    from test_gpu_parity import _expand2
    n = len(boards)
    d_b, d_ln = ctx.alloc(n * 32), ctx.alloc(n * 8 * 16)
    d_b.upload(boards)
    _, _, out = _expand2(ctx, d_b, n, mode)
    lines = {}
    for K in ks:
        ctx.rank_lines2_device(d_b, n, out, K, d_ln)
        ctx.synchronize()
        lines[K] = d_ln.download(G.LINE2_DTYPE, n * K).reshape(n, K)
    parents = out["po"].download(G.EVAL_DTYPE, n)
    _free(out), d_b.free(), d_ln.free()
    return parents, lines


@pytest.fixture(scope="module")
def positions():
    from fishnet_amd import gpu_nnue as G
    fens = R2.fixture_fens() + G.boards_to_fens(G.random_positions(R2.SEED, 0, R2.N_RANDOM, 160))
    return fens, G.pack_fens(fens)[0]


@pytest.fixture(scope="module")
def expected(positions, oracle_nets, oracle_lib):
    """The helper's 8 lines of every position, per mode (computed once; K < 8 is its prefix)."""
    big, small = oracle_nets
    return {mode: R2.lines2(oracle_lib, big, small, positions[0], mode, 8) for mode in MODES}


@pytest.fixture(scope="module")
def ranked(gpu_ctx, positions):
    return {mode: _expand2_and_rank(gpu_ctx, positions[1], mode, KS) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
def test_rank_lines2_device_vs_rule(ranked, expected, positions, mode, K):
    got, exp = ranked[mode][1][K], expected[mode][:, :K]
    assert got.shape == exp.shape and got.dtype == exp.dtype
    for i in np.flatnonzero((got != exp).any(axis=1))[:5]:
        assert got[i].tolist() == exp[i].tolist(), (positions[0][i], mode, K)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("mode", MODES)
def test_prefix_property(ranked, mode):
    lines = ranked[mode][1]
    assert np.array_equal(lines[8][:, :3], lines[3]) and np.array_equal(lines[8][:, :1], lines[1])


def test_wide_vs_rank_children_over_the_children(gpu_ctx, oracle_lib):
    """512 seeded positions (~15 k children, ~0.5 M grandchildren): gn_rank_children_device over the
    children as parents, K = 1, gives every child's (R(c), reply) (the header's relation to
    gn_line); negate_ply, the order and rule_score restated here give every parent's 8 lines."""
    from fishnet_amd import gpu_nnue as G
    from test_gpu_parity import _expand2
    ctx, K = gpu_ctx, 8
    boards = G.random_positions(R2.SEED + 1, 0, R2.N_WIDE, 160)
    fens = G.boards_to_fens(boards)
    n = len(boards)
    d_b, d_ln = ctx.alloc(n * 32), ctx.alloc(n * K * 16)
    d_b.upload(boards)
    t, g, out = _expand2(ctx, d_b, n, 0)
    assert t > 10 * n and g > 10 * t
    ctx.rank_lines2_device(d_b, n, out, K, d_ln)
    d_l1 = ctx.alloc(t * 12)
    ctx.rank_children_device(out["ch"], t, out["goff"], out["gmv"], out["gco"], 1, d_l1)
    ctx.synchronize()
    got = d_ln.download(G.LINE2_DTYPE, n * K).reshape(n, K)
    l1 = d_l1.download(G.LINE_DTYPE, t)
    off, mv = out["off"].download(np.uint32, n + 1), out["mv"].download(np.uint16, t)
    co, goff = out["co"].download(G.EVAL_DTYPE, t), out["goff"].download(np.uint32, t + 1)
    _free(out), d_b.free(), d_ln.free(), d_l1.free()
    # the segment lengths the lane and group loops ran over
    glen, clen = np.diff(goff.astype(np.int64)), np.diff(off.astype(np.int64))
    assert (glen > 32).any() and (glen == 0).any() and (clen > 40).any() and (clen < 8).any()
    none = (l1["flags"] & G.FLAG_NO_SCORE) != 0
    assert np.array_equal(none, glen == 0)
    check = (co["flags"] & G.FLAG_IN_CHECK) != 0
    P = oracle_lib.eval_params()
    exp = np.zeros((n, K), dtype=G.LINE2_DTYPE)
    exp[:] = np.array([R2.EMPTY2], dtype=G.LINE2_DTYPE)[0]
    for i in range(n):
        material = R.wdl_material(fens[i], P)
        ls = []
        for c in range(int(off[i]), int(off[i + 1])):
            r_c = (-R.VALUE_MATE if check[c] else 0) if none[c] else int(l1[c]["value"])
            v = R.negate_ply(r_c)
            score, mate = R.rule_score(v, material, P)
            fl = mate | (G.FLAG_IN_CHECK if check[c] else 0) | (G.FLAG_NO_MOVES if none[c] else 0)
            ls.append((v, score, int(mv[c]), 0 if none[c] else int(l1[c]["move"]), fl, 1 if none[c] else 2))
        ls.sort(key=lambda l: (-l[0], l[2]))
        for k, l in enumerate(ls[:K]):
            exp[i, k] = l
    for i in np.flatnonzero((got != exp).any(axis=1))[:5]:
        assert got[i].tolist() == exp[i].tolist(), fens[i]
    assert np.array_equal(got, exp)


MATED, STALEMATED = R2.fixture_fens()[6], R2.fixture_fens()[5]


def test_evaluate_lines2_vs_device_path(gpu_ctx, ranked, positions, synth_big_path, synth_small_path):
    from fishnet_amd import gpu_nnue as G
    fens = positions[0]
    for mode, K in ((0, 8), (1, 3)):
        out, lines = gpu_ctx.evaluate_lines2(fens, K, mode)
        assert gpu_ctx.get_option(G.STAT_RANK2_NS) > 0  # (any other host-buffer call resets it)
        assert lines.dtype == G.LINE2_DTYPE and lines.shape == (len(fens), K)
        assert lines.tobytes() == ranked[mode][1][K].tobytes()
        assert out.tobytes() == ranked[mode][0].tobytes()
        assert out.tobytes() == gpu_ctx.expand_and_evaluate(fens, mode)[0].tobytes()
        assert gpu_ctx.get_option(G.STAT_RANK2_NS) == 0 and gpu_ctx.get_option(G.STAT_RANK_NS) == 0
    out, lines = gpu_ctx.evaluate_lines2(fens, 3, 0)
    # several chunks (the last one short), and two device slots
    try:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 7)
        chunked = gpu_ctx.evaluate_lines2(fens, 3, 0)
    finally:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        sharded = two.evaluate_lines2(fens, 3, 0)
    finally:
        two.close()
    for other in (chunked, sharded):
        assert other[0].tobytes() == out.tobytes() and other[1].tobytes() == lines.tobytes()
    assert lines.tobytes() == ranked[0][1][3].tobytes()


def test_evaluate_lines2_bad_and_finished_positions(gpu_ctx):
    from fishnet_amd import gpu_nnue as G
    K = 3
    empty = np.array([R2.EMPTY2] * K, dtype=G.LINE2_DTYPE)
    out, lines = gpu_ctx.evaluate_lines2(["not a fen", MATED, R.START, STALEMATED], K, 0)
    assert out[0].tolist() == (0, 0, 0, 0, 0, G.FLAG_BAD_FEN | G.FLAG_NO_SCORE, 0)
    assert out[1]["flags"] & G.FLAG_NO_MOVES and out[1]["flags"] & G.FLAG_MATE and out[1]["flags"] & G.FLAG_IN_CHECK
    assert out[3]["flags"] & G.FLAG_NO_MOVES and not out[3]["flags"] & G.FLAG_IN_CHECK
    for i in (0, 1, 3):
        assert np.array_equal(lines[i], empty)
    assert (lines[2]["plies"] == 2).all() and (lines[2]["flags"] & G.FLAG_NO_SCORE == 0).all()
    assert gpu_ctx.get_option(G.STAT_RANK2_NS) > 0
    # only positions without a line: the child and grandchild buffers are never read
    out, lines = gpu_ctx.evaluate_lines2(["not a fen", MATED], K, 0)
    assert np.array_equal(lines[0], empty) and np.array_equal(lines[1], empty)
    out, lines = gpu_ctx.evaluate_lines2([], K, 0)
    assert len(out) == 0 and lines.shape == (0, K)
    assert G.lib().gn_evaluate_lines2(gpu_ctx.h, None, 0, 0, K, None, None) == 0


def test_lines2_argument_checks(gpu_ctx, ranked, positions):
    from fishnet_amd import gpu_nnue as G
    d = gpu_ctx.alloc(4096)
    bufs = {k: d for k in ("off", "ch", "co", "mv", "goff", "gmv", "gco")}
    for k in (0, 9):
        with pytest.raises(G.GnError) as e:
            gpu_ctx.evaluate_lines2(positions[0][:2], k, 0)
        assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.rank_lines2_device(d, 1, bufs, k, d)
        assert e.value.code == G.E_INVALID
    d.free()
    out, lines = gpu_ctx.evaluate_lines2(positions[0], 3, 0)
    assert lines.tobytes() == ranked[0][1][3].tobytes() and out.tobytes() == ranked[0][0].tobytes()
    again = _expand2_and_rank(gpu_ctx, positions[1], 0, (3,))
    assert again[1][3].tobytes() == ranked[0][1][3].tobytes() and again[0].tobytes() == ranked[0][0].tobytes()
