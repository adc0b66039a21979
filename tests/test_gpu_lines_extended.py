"""Check-extended ranked lines (include/gpu_nnue.h at gn_line, "check-extended") on the GPU against
the rule restated from the CPU oracle (tests/lines_extended_rule.py): gn_extend_checks_device with
gn_rank_children_extended_device and gn_rank_lines2_extended_device over an expansion's outputs, and
the host-buffer calls gn_evaluate_lines2_extended, gn_evaluate_games_lines_extended and
gn_evaluate_games_lines2_extended."""
import ctypes as C

import numpy as np
import pytest

import guarded_buffers as GB
import lines2_history_rule as H2
import lines2_rule as R2
import lines_extended_rule as X
import lines_param_sets as LP
import lines_rule as R

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
MODES = (0, 1)  # FULL, BIG
K_GAMES = 8
GUARD = 64      # int32 entries on either side of d_ext inside its allocation
SENTINEL = 0x5A5A5A5A


class _At:
    """A device pointer `nbytes` into a DeviceBuffer."""

    def __init__(self, buf, nbytes):
        self.ptr = C.c_void_p(buf.addr + nbytes)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _extend(ctx, d_parents, n, d_off, d_mv, d_rec, total, mode):
    """gn_extend_checks_device into exactly `total` entries inside a larger allocation: (the buffer,
    d_ext as a pointer into it, the count).  The surrounding entries must come back unchanged."""
    buf = ctx.alloc((total + 2 * GUARD) * 4)
    buf.upload(np.full(total + 2 * GUARD, SENTINEL, dtype=np.int32))
    d_ext = _At(buf, GUARD * 4)
    ne = ctx.extend_checks_device(d_parents, n, d_off, d_mv, d_rec, total, mode, d_ext)
    return buf, d_ext, ne


def _ext_of(buf, total):
    """d_ext downloaded, after checking that nothing was written around it."""
    all_ = buf.download(np.int32, total + 2 * GUARD)
    assert (all_[:GUARD] == SENTINEL).all() and (all_[GUARD + total:] == SENTINEL).all()
    return all_[GUARD:GUARD + total]


# ---- inputs -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def inputs1():
    """The fixtures, tests/golden/lines_fens.txt and 128 seeded positions: ~4 k children."""
    from fishnet_amd import gpu_nnue as G
    fens = X.fixture_fens() + R.fixture_fens() + G.boards_to_fens(G.random_positions(X.SEED1, 0, X.N_RANDOM1, 160))
    return fens, G.pack_fens(fens)[0]


@pytest.fixture(scope="module")
def inputs2():
    """The fixtures, tests/golden/lines2_fens.txt and 48 seeded positions: ~45 k grandchildren."""
    from fishnet_amd import gpu_nnue as G
    fens = X.fixture_fens() + R2.fixture_fens() + G.boards_to_fens(G.random_positions(X.SEED2, 0, X.N_RANDOM2, 160))
    return fens, G.pack_fens(fens)[0]


# ---- 1: one ply, the device path ----------------------------------------------------------------

def _level1(ctx, boards, mode, ks=KS):
    """gn_expand_device -> gn_extend_checks_device -> the extended ranking for every K of ks, and the
    plain ranking (K = 8) of the same expansion."""
    from fishnet_amd import gpu_nnue as G
    n = len(boards)
    cap = 256 * n
    b = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                       ("mv", cap * 2), ("co", cap * G.EVAL_SIZE), ("ln", n * 8 * 12))}
    b["b"].upload(boards)
    total = ctx.expand_device(b["b"], n, mode, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
    r = {"total": total, "off": b["off"].download(np.uint32, n + 1), "mv": b["mv"].download(np.uint16, total),
         "co": b["co"].download(G.EVAL_DTYPE, total), "ch": b["ch"].download(G.BOARD_DTYPE, total)}
    b["ext"], d_ext, r["extended"] = _extend(ctx, b["b"], n, b["off"], b["mv"], b["co"], total, mode)
    r["ext"] = _ext_of(b["ext"], total)
    r["co_after"] = b["co"].download(G.EVAL_DTYPE, total)
    r["lines"] = {}
    for K in ks:
        ctx.rank_children_extended_device(b["b"], n, b["off"], b["mv"], b["co"], d_ext, K, b["ln"])
        ctx.synchronize()
        r["lines"][K] = b["ln"].download(G.LINE_DTYPE, n * K).reshape(n, K)
    ctx.rank_children_device(b["b"], n, b["off"], b["mv"], b["co"], 8, b["ln"])
    ctx.synchronize()
    r["plain"] = b["ln"].download(G.LINE_DTYPE, n * 8).reshape(n, 8)
    ctx.rank_children_extended_device(b["b"], n, b["off"], b["mv"], b["co"], None, 8, b["ln"])
    ctx.synchronize()
    r["no_ext"] = b["ln"].download(G.LINE_DTYPE, n * 8).reshape(n, 8)
    for x in b.values():
        x.free()
    return r


@pytest.fixture(scope="module")
def level1(gpu_ctx, inputs1):
    return {mode: _level1(gpu_ctx, inputs1[1], mode) for mode in MODES}


@pytest.fixture(scope="module")
def expected1(oracle_lib, oracle_nets, inputs1):
    big, small = oracle_nets
    return {mode: X.lines(oracle_lib, big, small, inputs1[0], mode, 8) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_extension_entries_vs_rule(level1, inputs1, oracle_lib, oracle_nets, mode):
    """d_ext entry by entry, the count, the untouched child records and the untouched surroundings."""
    big, small = oracle_nets
    r = level1[mode]
    assert 3500 <= r["total"] <= 6000
    assert r["co"].tobytes() == r["co_after"].tobytes()  # the extension only reads the caller's records
    want_count = 0
    for i, fen in enumerate(inputs1[0]):
        a, b = int(r["off"][i]), int(r["off"][i + 1])
        kids = X.leaves(oracle_lib, big, small, fen, mode) or []
        want = dict(zip((k[0] for k in kids), X.extensions(oracle_lib, big, small, fen, mode)))
        assert len(kids) == b - a
        got = dict(zip((int(m) for m in r["mv"][a:b]), (int(e) for e in r["ext"][a:b])))
        assert got == want, fen
        want_count += sum(1 for e in want.values() if e != X.NOT_EXTENDED)
    assert r["extended"] == want_count == int((r["ext"] != X.NOT_EXTENDED).sum())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
def test_rank_children_extended_vs_rule(level1, expected1, inputs1, mode, K):
    lines, exp = level1[mode]["lines"][K], expected1[mode][:, :K]
    for i in np.flatnonzero((lines != exp).any(axis=1))[:5]:
        assert lines[i].tolist() == exp[i].tolist(), (inputs1[0][i], mode, K)
    assert np.array_equal(lines, exp)


@pytest.mark.parametrize("mode", MODES)
def test_conditions_on_the_one_ply_inputs(level1, mode):
    """The inputs exercise the feature (met by the reference alone, tests/test_lines_extended.py), so
    that this file fails on code that does not extend."""
    from fishnet_amd import gpu_nnue as G
    r = level1[mode]
    ext, plain = r["lines"][8], r["plain"]
    assert r["extended"] >= 100
    assert sum(1 for a, b in zip(ext, plain) if a[["value", "score", "move"]].tobytes() !=
               b[["value", "score", "move"]].tobytes()) >= 20
    both = G.FLAG_SEARCHED | G.FLAG_MATE
    assert ((ext["flags"] & both) == both).any() and not (plain["flags"] & G.FLAG_SEARCHED).any()
    counts = np.diff(r["off"])
    assert ((counts > 0) & (counts < 8)).any() and (counts > 32).any()
    assert r["no_ext"].tobytes() == plain.tobytes()  # d_ext NULL, d_hist NULL: the plain ranking


def test_extended_leaves_score_as_positions(gpu_ctx, level1, oracle_lib):
    """The invariant on the device: an extended leaf's value is what gn_evaluate_batch_mode scores
    for that position."""
    from fishnet_amd import gpu_nnue as G
    P = oracle_lib.eval_params()
    for mode in MODES:
        r = level1[mode]
        at = np.flatnonzero(r["ext"] != X.NOT_EXTENDED)
        fens = G.boards_to_fens(r["ch"][at])
        ev = gpu_ctx.evaluate_batch(fens, mode)
        for j, fen, e in zip(at, fens, ev):
            score, mate = R.rule_score(int(r["ext"][j]), R.wdl_material(fen, P), P)
            assert (int(e["score"]), int(e["flags"]) & G.FLAG_MATE) == (score, mate) and e["flags"] & G.FLAG_SEARCHED, fen
            assert int(e["best_move"]) != 0


def test_one_tie_forcing_parameter_set(gpu_ctx, oracle_lib, oracle_nets, inputs1):
    """value_clamp = 0: every ordinary value is 0, extended or static, and the move encoding decides."""
    big, small = oracle_nets
    fens, boards = inputs1[0][:48], inputs1[1][:48]
    with LP.under(oracle_lib, "clamp0", gpu_ctx):
        r = _level1(gpu_ctx, boards, 0, ks=(8,))
        exp = X.lines(oracle_lib, big, small, fens, 0, 8)
    assert np.array_equal(r["lines"][8], exp)
    zero = (exp["value"] == 0) & ((exp["flags"] & R.FLAG_NO_SCORE) == 0)
    assert (zero & ((exp["flags"] & X.FLAG_SEARCHED) != 0)).any() and (zero & ((exp["flags"] & X.FLAG_SEARCHED) == 0)).any()


# ---- 2: two plies, the device path --------------------------------------------------------------

def _level2(ctx, boards, mode, ks):
    from fishnet_amd import gpu_nnue as G
    from test_gpu_parity import _expand2
    n = len(boards)
    d_b, d_ln = ctx.alloc(n * 32), ctx.alloc(n * 8 * 16)
    d_b.upload(boards)
    t, g, out = _expand2(ctx, d_b, n, mode)
    r = {"t": t, "g": g, "ch": out["ch"].download(G.BOARD_DTYPE, t), "gco": out["gco"].download(G.EVAL_DTYPE, g)}
    buf, d_gext, r["extended"] = _extend(ctx, out["ch"], t, out["goff"], out["gmv"], out["gco"], g, mode)
    r["gext"] = _ext_of(buf, g)
    assert r["gco"].tobytes() == out["gco"].download(G.EVAL_DTYPE, g).tobytes()
    r["lines"] = {}
    for K in ks:
        ctx.rank_lines2_extended_device(d_b, n, out, d_gext, K, d_ln)
        ctx.synchronize()
        r["lines"][K] = d_ln.download(G.LINE2_DTYPE, n * K).reshape(n, K)
    # the relation to gn_line: the extended one-ply ranking over the children as parents, K = 1
    d_l1 = ctx.alloc(max(t, 1) * 12)
    ctx.rank_children_extended_device(out["ch"], t, out["goff"], out["gmv"], out["gco"], d_gext, 1, d_l1)
    ctx.synchronize()
    r["child_line1"] = d_l1.download(G.LINE_DTYPE, t)
    r["off"], r["mv"] = out["off"].download(np.uint32, n + 1), out["mv"].download(np.uint16, t)
    for x in list(out.values()) + [d_b, d_ln, d_l1, buf]:
        if hasattr(x, "free"):
            x.free()
    return r


@pytest.fixture(scope="module")
def level2(gpu_ctx, inputs2):
    return {0: _level2(gpu_ctx, inputs2[1], 0, KS), 1: _level2(gpu_ctx, inputs2[1], 1, (8,))}


@pytest.fixture(scope="module")
def expected2(oracle_lib, oracle_nets, inputs2):
    big, small = oracle_nets
    return {mode: X.lines2(oracle_lib, big, small, inputs2[0], mode, 8) for mode in MODES}


@pytest.mark.parametrize("mode,K", [(0, 1), (0, 3), (0, 8), (1, 8)])
def test_rank_lines2_extended_vs_rule(level2, expected2, inputs2, mode, K):
    from fishnet_amd import gpu_nnue as G
    lines, exp = level2[mode]["lines"][K], expected2[mode][:, :K]
    for i in np.flatnonzero((lines != exp).any(axis=1))[:5]:
        assert lines[i].tolist() == exp[i].tolist(), (inputs2[0][i], mode, K)
    assert np.array_equal(lines, exp)
    if K == 8:
        assert 30000 <= level2[mode]["g"] <= 70000
        searched = (lines["flags"] & G.FLAG_SEARCHED) != 0
        assert searched.sum() >= 4 and (searched & ((lines["flags"] & G.FLAG_MATE) != 0)).any()
        assert (lines["plies"][searched] == 2).all()


def test_relation_to_the_one_ply_lines(level2, inputs2, oracle_lib, oracle_nets):
    """For a child with a reply, (R(c), reply) is line 1 of the extended one-ply ranking over the
    children as parents: against the rule for every child, and inside the two-ply lines."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    r = level2[0]
    fens = G.boards_to_fens(r["ch"])
    want = X.lines(oracle_lib, big, small, fens, 0, 1)[:, 0]
    assert np.array_equal(r["child_line1"], want)
    seen = 0
    for i in range(len(inputs2[0])):
        a, b = int(r["off"][i]), int(r["off"][i + 1])
        by_move = {int(m): r["child_line1"][a + j] for j, m in enumerate(r["mv"][a:b])}
        for l in r["lines"][8][i]:
            if l["plies"] == 2:
                c = by_move[int(l["move"])]
                assert (R.negate_ply(int(c["value"])), int(c["move"])) == (int(l["value"]), int(l["reply"]))
                assert bool(c["flags"] & G.FLAG_SEARCHED) == bool(l["flags"] & G.FLAG_SEARCHED)
                seen += 1
    assert seen >= 300


# ---- 3: the host calls --------------------------------------------------------------------------

def test_evaluate_lines2_extended(gpu_ctx, level2, inputs2, synth_big_path, synth_small_path):
    from fishnet_amd import gpu_nnue as G
    fens = inputs2[0]
    out, lines = gpu_ctx.evaluate_lines2_extended(fens, 8, 0)
    assert gpu_ctx.get_option(G.STAT_EXTEND_NS) > 0
    assert gpu_ctx.get_option(G.STAT_EXTENDED_LEAVES) == level2[0]["extended"] > 0
    assert lines.tobytes() == level2[0]["lines"][8].tobytes()
    pout, plines = gpu_ctx.evaluate_lines2(fens, 8, 0)
    assert gpu_ctx.get_option(G.STAT_EXTEND_NS) == 0 and gpu_ctx.get_option(G.STAT_EXTENDED_LEAVES) == 0
    assert out.tobytes() == pout.tobytes() and lines.tobytes() != plines.tobytes()
    try:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 7)
        chunked = gpu_ctx.evaluate_lines2_extended(fens, 8, 0)
        assert gpu_ctx.get_option(G.STAT_EXTENDED_LEAVES) == level2[0]["extended"]
    finally:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        sharded = two.evaluate_lines2_extended(fens, 8, 0)
        assert two.get_option(G.STAT_EXTENDED_LEAVES) == level2[0]["extended"]
    finally:
        two.close()
    assert _same((out, lines), chunked) and _same((out, lines), sharded)


def test_equal_to_the_plain_call_where_nothing_is_extended(gpu_ctx, inputs2, oracle_lib, oracle_nets):
    """The positions none of whose grandchildren is in check with a legal move (by the rule):
    GN_STAT_EXTENDED_LEAVES is 0 and the lines are the plain call's bytes."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    quiet = []
    for f in inputs2[0]:
        kids = X.leaves(oracle_lib, big, small, f, 0)
        if kids and not any(e != X.NOT_EXTENDED for _, c, _, alive, _ in kids if alive
                            for e in X.extensions(oracle_lib, big, small, c, 0)):
            quiet.append(f)
    assert 8 <= len(quiet) < len(inputs2[0])
    out, lines = gpu_ctx.evaluate_lines2_extended(quiet, 8, 0)
    assert gpu_ctx.get_option(G.STAT_EXTENDED_LEAVES) == 0
    pout, plines = gpu_ctx.evaluate_lines2(quiet, 8, 0)
    assert out.tobytes() == pout.tobytes() and lines.tobytes() == plines.tobytes()
    assert not (lines["flags"] & G.FLAG_SEARCHED).any()


# ---- 4: the games calls -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def games():
    """Both history fixtures' games, then each extended fixture position as a game without moves."""
    return H2.both_fixtures() + [(f, "", ()) for f in X.fixture_fens()]


@pytest.fixture(scope="module")
def replayed(oracle_lib, games):
    return [oracle_lib.replay_game(root, moves)[0] for root, moves, _ in games]


@pytest.fixture(scope="module")
def games_got(gpu_ctx, games):
    """{(plies, history): (offsets, status, records, lines, extend ns, extended leaves)}"""
    from fishnet_amd import gpu_nnue as G
    out = {}
    for plies, call in ((1, gpu_ctx.evaluate_games_lines_extended), (2, gpu_ctx.evaluate_games_lines2_extended)):
        for history in (False, True):
            res = call(games, K_GAMES, 0, history=history)
            out[(plies, history)] = res + (gpu_ctx.get_option(G.STAT_EXTEND_NS), gpu_ctx.get_option(G.STAT_EXTENDED_LEAVES))
    return out


@pytest.mark.parametrize("history", (False, True))
@pytest.mark.parametrize("plies", (1, 2))
def test_games_calls_vs_rule(gpu_ctx, games_got, games, replayed, oracle_lib, oracle_nets, plies, history):
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    offs, status, pos, lines, ns, leaves = games_got[(plies, history)]
    rule = X.game_lines if plies == 1 else X.game_lines2
    exp = np.concatenate([rule(oracle_lib, big, small, fens, skip, 0, K_GAMES, history)
                          for fens, (_, _, skip) in zip(replayed, games)])
    assert not status.any() and lines.shape == exp.shape and lines.dtype == exp.dtype
    for i in np.flatnonzero((lines != exp).any(axis=1))[:5]:
        g = int(np.searchsorted(offs, i, side="right")) - 1
        assert lines[i].tolist() == exp[i].tolist(), (g, i - int(offs[g]), replayed[g][i - int(offs[g])], plies, history)
    assert np.array_equal(lines, exp)
    assert ns > 0 and leaves > 0 and (lines["flags"] & G.FLAG_SEARCHED).any()
    assert bool((lines["flags"] & G.FLAG_DRAW).any()) == history
    # offsets, status and records are the plain calls' bytes; a plain call resets the statistics
    if plies == 1:
        plain = gpu_ctx.evaluate_games_lines(games, K_GAMES, 0, history=history)
    else:
        plain = gpu_ctx.evaluate_games_lines2(games, K_GAMES, 0, history=history)
    assert gpu_ctx.get_option(G.STAT_EXTEND_NS) == 0 and gpu_ctx.get_option(G.STAT_EXTENDED_LEAVES) == 0
    assert _same((offs, status, pos), plain[:3]) and not (plain[3]["flags"] & G.FLAG_SEARCHED).any()
    # skipped positions have only empty lines
    empty = np.array([R.EMPTY if plies == 1 else R2.EMPTY2], dtype=lines.dtype)[0]
    skipped = np.flatnonzero(pos["flags"] & G.FLAG_SKIPPED)
    assert len(skipped) >= 1 and all((lines[i] == empty).all() for i in skipped)


@pytest.mark.parametrize("plies", (1, 2))
def test_games_calls_same_bytes_from_every_path(gpu_ctx, games_got, games, plies, synth_big_path, synth_small_path):
    from fishnet_amd import gpu_nnue as G
    base = games_got[(plies, True)]
    name = "evaluate_games_lines_extended" if plies == 1 else "evaluate_games_lines2_extended"
    others = []
    try:
        for pipeline, chunk in ((0, 0), (2, 5), (0, 5)):
            gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, pipeline)
            gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, chunk)
            others.append(getattr(gpu_ctx, name)(games, K_GAMES, 0, history=True))
            assert gpu_ctx.get_option(G.STAT_EXTENDED_LEAVES) == base[5]
    finally:
        gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, 2)
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        others.append(getattr(two, name)(games, K_GAMES, 0, history=True))
        assert two.get_option(G.STAT_EXTENDED_LEAVES) == base[5]
    finally:
        two.close()
    assert len(base[2]) >= 10 * 5
    for o in others:
        assert _same(base[:4], o)


# ---- 5: arguments and buffer sizes --------------------------------------------------------------

def test_argument_checks(gpu_ctx, games):
    from fishnet_amd import gpu_nnue as G
    d = gpu_ctx.alloc(4096)
    bufs = {k: d for k in ("off", "ch", "co", "mv", "goff", "gmv", "gco")}
    for k in (0, 9):
        for call in (gpu_ctx.evaluate_games_lines_extended, gpu_ctx.evaluate_games_lines2_extended):
            with pytest.raises(G.GnError) as e:
                call(games[:2], k, 0, history=True)
            assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.evaluate_lines2_extended([R.START], k, 0)
        assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.rank_children_extended_device(d, 1, d, d, d, d, k, d)
        assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.rank_lines2_extended_device(d, 1, bufs, d, k, d)
        assert e.value.code == G.E_INVALID
    # total == 0 with NULL buffers: GN_OK, nothing extended; a NULL buffer with leaves: GN_E_INVALID
    assert gpu_ctx.extend_checks_device(None, 0, None, None, None, 0, 0, None) == 0
    assert gpu_ctx.extend_checks_device(d, 1, d, None, None, 0, 0, None) == 0
    with pytest.raises(G.GnError) as e:
        gpu_ctx.extend_checks_device(d, 1, d, d, d, 1, 0, None)
    assert e.value.code == G.E_INVALID
    with pytest.raises(G.GnError) as e:
        gpu_ctx.extend_checks_device(d, 1, d, d, d, 1, 7, d)
    assert e.value.code == G.E_INVALID
    d.free()
    # empty input
    out, lines = gpu_ctx.evaluate_lines2_extended([], 3, 0)
    assert len(out) == 0 and lines.shape == (0, 3)
    for call in (gpu_ctx.evaluate_games_lines_extended, gpu_ctx.evaluate_games_lines2_extended):
        offs, status, pos, lines = call([], 3, 0)
        assert list(offs) == [0] and len(pos) == 0
    # a failed game has no positions; the others are still evaluated
    some = [games[0], (R.START, "e2e4 e7e5 e1e3", ()), ("not a fen", "e2e4", ()), (X.FIFTY, "", ())]
    for call, plain in ((gpu_ctx.evaluate_games_lines_extended, gpu_ctx.evaluate_games_lines),
                        (gpu_ctx.evaluate_games_lines2_extended, gpu_ctx.evaluate_games_lines2)):
        offs, status, pos, lines = call(some, 3, 0, history=True)
        assert list(status[1:3]) == [G.E_ILLEGAL_MOVE, G.E_INVALID] and offs[2] == offs[1] == offs[3]
        assert int(offs[4] - offs[3]) == 1
        assert _same((offs, status, pos), plain(some, 3, 0, history=True)[:3])
        last = lines[int(offs[3])]
        draw = last[(last["flags"] & G.FLAG_DRAW) != 0]
        assert len(draw) >= 1 and not (draw["flags"] & G.FLAG_SEARCHED).any()  # the draw comes first
        assert (call(some, 3, 0, history=False)[3][int(offs[3])]["flags"] & G.FLAG_DRAW).sum() == 0


def test_no_net_for_the_mode(synth_big_path):
    from fishnet_amd import gpu_nnue as G
    big_only = G.GpuNnue(synth_big_path, None)
    try:
        d = big_only.alloc(4096)
        with pytest.raises(G.GnError) as e:
            big_only.extend_checks_device(d, 1, d, d, d, 1, 0, d)
        assert e.value.code == G.E_NONET
        d.free()
    finally:
        big_only.close()


def test_exact_size_host_outputs(gpu_ctx, games, games_got, inputs2, level2):
    """The host-buffer calls with outputs of exactly the sizes they are told: nothing is written
    outside them, and what is written is what the bindings' calls returned."""
    from fishnet_amd import gpu_nnue as G
    L = G.lib()
    fens = inputs2[0][:20]
    arr, _keep = G._fen_array(fens)
    s = GB.GuardedSet()
    rc = L.gn_evaluate_lines2_extended(gpu_ctx.h, arr, len(fens), 0, 8, s.add("out", len(fens), G.EVAL_DTYPE),
                                       s.add("lines", len(fens) * 8, G.LINE2_DTYPE))
    assert rc == 0
    s.check()
    assert s["lines"].bytes() == level2[0]["lines"][8][:20].tobytes()
    garr, _keep2 = G._games_array(games)
    ng = len(games)
    for plies, name, dtype in ((1, "gn_evaluate_games_lines_extended", G.LINE_DTYPE),
                               (2, "gn_evaluate_games_lines2_extended", G.LINE2_DTYPE)):
        offs, status, pos, lines = games_got[(plies, True)][:4]
        p = len(pos)
        s = GB.GuardedSet()
        rc = getattr(L, name)(gpu_ctx.h, garr, ng, 0, K_GAMES, 1, s.add("offs", ng + 1, np.uint32),
                              s.add("status", ng, np.int32), s.add("pos", p, G.EVAL_DTYPE), p,
                              s.add("lines", p * K_GAMES, dtype))
        assert rc == 0
        s.check()
        assert (s["offs"].bytes(), s["pos"].bytes(), s["lines"].bytes()) == (offs.tobytes(), pos.tobytes(), lines.tobytes())
        # one position too few: GN_E_CAPACITY, the offsets filled, no record or line written
        s = GB.GuardedSet()
        rc = getattr(L, name)(gpu_ctx.h, garr, ng, 0, K_GAMES, 1, s.add("offs", ng + 1, np.uint32),
                              s.add("status", ng, np.int32), s.add("pos", p - 1, G.EVAL_DTYPE), p - 1,
                              s.add("lines", (p - 1) * K_GAMES, dtype))
        assert rc == G.E_CAPACITY
        s.check()
        assert s["offs"].bytes() == offs.tobytes() and s["pos"].untouched() and s["lines"].untouched()
