"""Quiescent ranked lines (include/gpu_nnue.h at gn_line, "quiescent") on the GPU against the rule
restated from the CPU oracle (tests/quiesce_rule.py): gn_quiesce_device entry by entry, its d_ext
through gn_rank_children_extended_device and gn_rank_lines2_extended_device, and the host-buffer calls
gn_evaluate_lines2_quiescent, gn_evaluate_games_lines_quiescent and gn_evaluate_games_lines2_quiescent.

Sizes (the rule's own counts; tests/test_quiesce.py checks the bounds on the CPU, every test here
asserts them again): the one-ply set is the 12 fixtures, tests/golden/lines_fens.txt and 64 seeded
positions, 2,458 leaves of which 2,027 are searched, with 8.6 k nodes below them at depth 1 and 48 k at
depth 2; depth 3 runs the fixtures and 16 seeded positions, 615 leaves, 516 searched, 57 k nodes.  The
two-ply set is the fixtures and 3 seeded positions: 3,619 grandchildren, 2,878 searched, 84 k
nodes at depth 2.  The games are 45 positions."""
import ctypes as C

import numpy as np
import pytest

import history_rule as H
import lines2_rule as R2
import lines_rule as R
import quiesce_rule as Q

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


def _quiesce(ctx, d_parents, n, d_off, d_mv, d_rec, total, mode, depth):
    """gn_quiesce_device into exactly `total` entries inside a larger allocation: (the buffer, d_ext as
    a pointer into it, searched, nodes).  The surrounding entries must come back unchanged."""
    buf = ctx.alloc((total + 2 * GUARD) * 4)
    buf.upload(np.full(total + 2 * GUARD, SENTINEL, dtype=np.int32))
    d_ext = _At(buf, GUARD * 4)
    ns, nn = ctx.quiesce_device(d_parents, n, d_off, d_mv, d_rec, total, mode, depth, d_ext)
    return buf, d_ext, ns, nn


def _ext_of(buf, total):
    """d_ext downloaded, after checking that nothing was written around it."""
    all_ = buf.download(np.int32, total + 2 * GUARD)
    assert (all_[:GUARD] == SENTINEL).all() and (all_[GUARD + total:] == SENTINEL).all()
    return all_[GUARD:GUARD + total]


# ---- inputs -------------------------------------------------------------------------------------

def _packed(fens):
    from fishnet_amd import gpu_nnue as G
    return fens, G.pack_fens(fens)[0]


@pytest.fixture(scope="module")
def inputs1():
    """The fixtures, tests/golden/lines_fens.txt and 64 seeded positions (depth 1 and 2)."""
    from fishnet_amd import gpu_nnue as G
    return _packed(Q.fixture_fens() + R.fixture_fens() + G.boards_to_fens(G.random_positions(Q.SEED, 0, Q.N_RANDOM, 160)))


@pytest.fixture(scope="module")
def inputs3():
    """The fixtures and 16 seeded positions (depth 3)."""
    from fishnet_amd import gpu_nnue as G
    return _packed(Q.fixture_fens() + G.boards_to_fens(G.random_positions(Q.SEED, 0, Q.N_RANDOM3, 160)))


@pytest.fixture(scope="module")
def inputs2():
    """The fixtures and a handful of seeded positions (two plies)."""
    from fishnet_amd import gpu_nnue as G
    return _packed(Q.fixture_fens() + G.boards_to_fens(G.random_positions(Q.SEED2, 0, Q.N_RANDOM2, 160)))


# ---- 1, 2: one ply, the device path -------------------------------------------------------------

def _level1(ctx, boards, mode, depths, ks=KS):
    """gn_expand_device, then per depth gn_quiesce_device and the extended ranking for every K of ks;
    and the plain ranking (K = 8) of the same expansion."""
    from fishnet_amd import gpu_nnue as G
    n = len(boards)
    cap = 256 * n
    b = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                       ("mv", cap * 2), ("co", cap * G.EVAL_SIZE), ("ln", n * 8 * 12))}
    b["b"].upload(boards)
    total = ctx.expand_device(b["b"], n, mode, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
    r = {"total": total, "off": b["off"].download(np.uint32, n + 1), "mv": b["mv"].download(np.uint16, total),
         "co": b["co"].download(G.EVAL_DTYPE, total), "depth": {}}
    for depth in depths:
        buf, d_ext, ns, nn = _quiesce(ctx, b["b"], n, b["off"], b["mv"], b["co"], total, mode, depth)
        x = r["depth"][depth] = {"searched": ns, "nodes": nn, "ext": _ext_of(buf, total), "lines": {}}
        x["co_after"] = b["co"].download(G.EVAL_DTYPE, total)
        for K in ks:
            ctx.rank_children_extended_device(b["b"], n, b["off"], b["mv"], b["co"], d_ext, K, b["ln"])
            ctx.synchronize()
            x["lines"][K] = b["ln"].download(G.LINE_DTYPE, n * K).reshape(n, K)
        buf.free()
    ctx.rank_children_device(b["b"], n, b["off"], b["mv"], b["co"], 8, b["ln"])
    ctx.synchronize()
    r["plain"] = b["ln"].download(G.LINE_DTYPE, n * 8).reshape(n, 8)
    for x in b.values():
        x.free()
    return r


@pytest.fixture(scope="module")
def level1(gpu_ctx, inputs1, inputs3):
    return {mode: {"a": _level1(gpu_ctx, inputs1[1], mode, (1, 2)), "b": _level1(gpu_ctx, inputs3[1], mode, (3,), ks=(8,))}
            for mode in MODES}


def _set_of(depth, inputs1, inputs3):
    return ("b", inputs3[0]) if depth == 3 else ("a", inputs1[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", (1, 2, 3))
def test_quiesce_entries_vs_rule(level1, inputs1, inputs3, oracle_lib, oracle_nets, mode, depth):
    """d_ext entry by entry, searched and nodes against the rule's counts, the untouched child records
    and the untouched surroundings; at least 100 searched and 20 unsearched leaves."""
    big, small = oracle_nets
    which, fens = _set_of(depth, inputs1, inputs3)
    r = level1[mode][which]
    x = r["depth"][depth]
    assert r["co"].tobytes() == x["co_after"].tobytes()  # the quiescence only reads the caller's records
    ws = wn = 0
    for i, fen in enumerate(fens):
        a, b = int(r["off"][i]), int(r["off"][i + 1])
        kids = Q.leaves(oracle_lib, big, small, fen, mode) or []
        ext, ns, nn = Q.extensions(oracle_lib, big, small, fen, depth, mode)
        assert len(kids) == b - a
        want = dict(zip((k[0] for k in kids), ext))
        got = dict(zip((int(m) for m in r["mv"][a:b]), (int(e) for e in x["ext"][a:b])))
        assert got == want, (fen, depth)
        ws, wn = ws + ns, wn + nn
    print(f"depth {depth} mode {mode}: {r['total']} leaves, {ws} searched, {wn} nodes")
    assert x["searched"] == ws == int((x["ext"] != Q.NOT_EXTENDED).sum()) and x["nodes"] == wn
    assert ws >= 100 and r["total"] - ws >= 20 and wn <= 150000


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth,K", [(1, 1), (1, 3), (1, 8), (2, 1), (2, 3), (2, 8), (3, 8)])
def test_rank_children_with_quiescent_ext_vs_rule(level1, inputs1, inputs3, oracle_lib, oracle_nets, mode, depth, K):
    """The extended ranking fed the quiescence's d_ext against the rule's lines."""
    big, small = oracle_nets
    which, fens = _set_of(depth, inputs1, inputs3)
    lines = level1[mode][which]["depth"][depth]["lines"][K]
    exp = Q.lines(oracle_lib, big, small, fens, depth, mode, K)
    for i in np.flatnonzero((lines != exp).any(axis=1))[:5]:
        assert lines[i].tolist() == exp[i].tolist(), (fens[i], mode, depth, K)
    assert np.array_equal(lines, exp)


@pytest.mark.parametrize("mode", MODES)
def test_conditions_on_the_one_ply_inputs(level1, mode):
    """The inputs exercise the feature: a top-8 that differs from the plain ranking, a mate score
    through a capture, searched lines where the plain ranking has none, and a value that depth 2 changes."""
    from fishnet_amd import gpu_nnue as G
    r = level1[mode]["a"]
    q1, q2, plain = r["depth"][1]["lines"][8], r["depth"][2]["lines"][8], r["plain"]
    cols = ["value", "score", "move"]
    assert sum(1 for a, b in zip(q2, plain) if a[cols].tobytes() != b[cols].tobytes()) >= 1
    both = G.FLAG_SEARCHED | G.FLAG_MATE
    assert ((q2["flags"] & both) == both).any() and not (plain["flags"] & G.FLAG_SEARCHED).any()
    assert (r["depth"][1]["ext"] != r["depth"][2]["ext"]).any() and q1.tobytes() != q2.tobytes()


def test_entries_no_parent_covers_are_not_extended(gpu_ctx, inputs3):
    """d_ext holds GN_NOT_EXTENDED everywhere else, also where the offsets given cover fewer than
    `total` leaves: the call without its last parents writes the same head and an unextended tail."""
    from fishnet_amd import gpu_nnue as G
    boards = inputs3[1][:12]
    n, cap = len(boards), 256 * len(boards)
    b = {k: gpu_ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                           ("mv", cap * 2), ("co", cap * G.EVAL_SIZE))}
    b["b"].upload(boards)
    total = gpu_ctx.expand_device(b["b"], n, 0, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
    off = b["off"].download(np.uint32, n + 1)
    buf, _, ns, nn = _quiesce(gpu_ctx, b["b"], n, b["off"], b["mv"], b["co"], total, 0, 2)
    full = _ext_of(buf, total)
    buf.free()
    m = n - 3
    head = int(off[m])
    assert 0 < head < total
    buf, _, ns2, _ = _quiesce(gpu_ctx, b["b"], m, b["off"], b["mv"], b["co"], total, 0, 2)
    part = _ext_of(buf, total)
    buf.free()
    assert np.array_equal(part[:head], full[:head]) and (part[head:] == Q.NOT_EXTENDED).all()
    assert ns2 == int((full[:head] != Q.NOT_EXTENDED).sum()) and (full[head:] != Q.NOT_EXTENDED).any()
    for x in b.values():
        x.free()


# ---- 3: two plies, the device path --------------------------------------------------------------

def _level2(ctx, boards, mode, depths, K=8):
    from fishnet_amd import gpu_nnue as G
    from test_gpu_parity import _expand2
    n = len(boards)
    d_b, d_ln = ctx.alloc(n * 32), ctx.alloc(n * 8 * 16)
    d_b.upload(boards)
    t, g, out = _expand2(ctx, d_b, n, mode)
    r = {"t": t, "g": g, "gco": out["gco"].download(G.EVAL_DTYPE, g), "depth": {}}
    for depth in depths:
        buf, d_gext, ns, nn = _quiesce(ctx, out["ch"], t, out["goff"], out["gmv"], out["gco"], g, mode, depth)
        x = r["depth"][depth] = {"searched": ns, "nodes": nn, "gext": _ext_of(buf, g)}
        assert r["gco"].tobytes() == out["gco"].download(G.EVAL_DTYPE, g).tobytes()
        ctx.rank_lines2_extended_device(d_b, n, out, d_gext, K, d_ln)
        ctx.synchronize()
        x["lines"] = d_ln.download(G.LINE2_DTYPE, n * K).reshape(n, K)
        buf.free()
    for x in list(out.values()) + [d_b, d_ln]:
        if hasattr(x, "free"):
            x.free()
    return r


@pytest.fixture(scope="module")
def level2(gpu_ctx, inputs2):
    return {mode: _level2(gpu_ctx, inputs2[1], mode, (1, 2)) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", (1, 2))
def test_rank_lines2_with_quiescent_ext_vs_rule(level2, inputs2, oracle_lib, oracle_nets, mode, depth):
    """gn_expand2_device, gn_quiesce_device over the grandchildren (the children as parents), then
    gn_rank_lines2_extended_device: the lines and the counts against the rule."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    x = level2[mode]["depth"][depth]
    exp = Q.lines2(oracle_lib, big, small, inputs2[0], depth, mode, 8)
    for i in np.flatnonzero((x["lines"] != exp).any(axis=1))[:5]:
        assert x["lines"][i].tolist() == exp[i].tolist(), (inputs2[0][i], mode, depth)
    assert np.array_equal(x["lines"], exp)
    ws = wn = 0
    for fen in inputs2[0]:
        for _, c, _, live, _, _ in Q.leaves(oracle_lib, big, small, fen, mode):
            if live:
                _, ns, nn = Q.extensions(oracle_lib, big, small, c, depth, mode)
                ws, wn = ws + ns, wn + nn
    print(f"two plies, depth {depth} mode {mode}: {level2[mode]['g']} grandchildren, {ws} searched, {wn} nodes")
    assert (x["searched"], x["nodes"]) == (ws, wn) and ws >= 100 and wn <= 150000
    searched = (x["lines"]["flags"] & G.FLAG_SEARCHED) != 0
    assert searched.sum() >= 4 and (x["lines"]["plies"][searched] == 2).all()


# ---- 4: the host-buffer calls -------------------------------------------------------------------

def test_evaluate_lines2_quiescent(gpu_ctx, level2, inputs2, synth_big_path, synth_small_path):
    from fishnet_amd import gpu_nnue as G
    fens = inputs2[0]
    want = level2[0]["depth"][2]
    out, lines = gpu_ctx.evaluate_lines2_quiescent(fens, 8, 2, 0)
    assert gpu_ctx.get_option(G.STAT_QUIESCE_NS) > 0
    assert gpu_ctx.get_option(G.STAT_QUIESCE_LEAVES) == want["searched"] > 0
    assert gpu_ctx.get_option(G.STAT_QUIESCE_NODES) == want["nodes"] > 0
    assert gpu_ctx.get_option(G.STAT_EXTEND_NS) == 0 and gpu_ctx.get_option(G.STAT_EXTENDED_LEAVES) == 0
    assert lines.tobytes() == want["lines"].tobytes()
    pout, plines = gpu_ctx.evaluate_lines2(fens, 8, 0)
    assert [gpu_ctx.get_option(s) for s in (G.STAT_QUIESCE_NS, G.STAT_QUIESCE_LEAVES, G.STAT_QUIESCE_NODES)] == [0, 0, 0]
    assert out.tobytes() == pout.tobytes() and lines.tobytes() != plines.tobytes()
    chunked = []
    try:
        for chunk in (1, 7):
            gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, chunk)
            chunked.append(gpu_ctx.evaluate_lines2_quiescent(fens, 8, 2, 0))
            assert gpu_ctx.get_option(G.STAT_QUIESCE_NODES) == want["nodes"]
    finally:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        sharded = two.evaluate_lines2_quiescent(fens, 8, 2, 0)
        assert two.get_option(G.STAT_QUIESCE_LEAVES) == want["searched"]
    finally:
        two.close()
    assert all(_same((out, lines), c) for c in chunked) and _same((out, lines), sharded)
    d1 = gpu_ctx.evaluate_lines2_quiescent(fens, 8, 1, 0)[1]
    assert d1.tobytes() == level2[0]["depth"][1]["lines"].tobytes()


def test_equal_to_the_plain_calls_where_nothing_is_searched(gpu_ctx, oracle_lib):
    """Positions without a searched leaf at either level: the statistics are 0 and the lines are the
    plain calls' bytes."""
    from fishnet_amd import gpu_nnue as G
    quiet = ["4k3/8/8/8/8/8/8/4K3 w - - 0 1", "4k3/p7/8/8/8/8/P7/4K3 w - - 0 1", "7k/8/8/8/8/8/8/K6N w - - 0 1"]
    for f in quiet:  # no capture, check, en passant or promotion within two plies
        for m in oracle_lib.legal_moves(f):
            c = oracle_lib.child_fen(f, m)
            for f2 in (c, *(oracle_lib.child_fen(c, m2) for m2 in oracle_lib.legal_moves(c))):
                assert oracle_lib.legal_moves(f2) and not any(Q.noisy(oracle_lib, f2, x) for x in oracle_lib.legal_moves(f2))
    out, lines = gpu_ctx.evaluate_lines2_quiescent(quiet, 8, 2, 0)
    assert gpu_ctx.get_option(G.STAT_QUIESCE_LEAVES) == 0 and gpu_ctx.get_option(G.STAT_QUIESCE_NODES) == 0
    pout, plines = gpu_ctx.evaluate_lines2(quiet, 8, 0)
    assert out.tobytes() == pout.tobytes() and lines.tobytes() == plines.tobytes()
    assert not (lines["flags"] & G.FLAG_SEARCHED).any()
    games = [(f, "", ()) for f in quiet]
    got = gpu_ctx.evaluate_games_lines_quiescent(games, 8, 2, 0, history=True)
    assert gpu_ctx.get_option(G.STAT_QUIESCE_LEAVES) == 0
    assert _same(got, gpu_ctx.evaluate_games_lines(games, 8, 0, history=True))


@pytest.fixture(scope="module")
def games():
    """Four games of tests/golden/history_games.txt (the opening, a repetition, a fifty-move root whose
    quiet moves are drawn while its captures are searched, one with skipped positions), then each
    fixture position as a game without moves."""
    g = H.fixture_games()
    assert g[4][0].split()[4] == "99"
    return [g[0], g[1], g[4], g[10]] + [(f, "", ()) for f in Q.fixture_fens()]


@pytest.fixture(scope="module")
def replayed(oracle_lib, games):
    return [oracle_lib.replay_game(root, moves)[0] for root, moves, _ in games]


DEPTH_GAMES = {1: 2, 2: 1}  # the games calls' depth: one-ply lines at depth 2, two-ply lines at depth 1


@pytest.fixture(scope="module")
def games_got(gpu_ctx, games):
    """{(plies, history): (offsets, status, records, lines, ns, searched leaves, nodes)}"""
    from fishnet_amd import gpu_nnue as G
    out = {}
    for plies, call in ((1, gpu_ctx.evaluate_games_lines_quiescent), (2, gpu_ctx.evaluate_games_lines2_quiescent)):
        for history in (False, True):
            res = call(games, K_GAMES, DEPTH_GAMES[plies], 0, history=history)
            out[(plies, history)] = res + tuple(gpu_ctx.get_option(s) for s in (G.STAT_QUIESCE_NS, G.STAT_QUIESCE_LEAVES,
                                                                               G.STAT_QUIESCE_NODES))
    return out


@pytest.mark.parametrize("history", (False, True))
@pytest.mark.parametrize("plies", (1, 2))
def test_games_calls_vs_rule(gpu_ctx, games_got, games, replayed, oracle_lib, oracle_nets, plies, history):
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    offs, status, pos, lines, ns, leaves, nodes = games_got[(plies, history)]
    rule = Q.game_lines if plies == 1 else Q.game_lines2
    exp = np.concatenate([rule(oracle_lib, big, small, fens, skip, DEPTH_GAMES[plies], 0, K_GAMES, history)
                          for fens, (_, _, skip) in zip(replayed, games)])
    assert not status.any() and lines.shape == exp.shape and lines.dtype == exp.dtype
    for i in np.flatnonzero((lines != exp).any(axis=1))[:5]:
        g = int(np.searchsorted(offs, i, side="right")) - 1
        assert lines[i].tolist() == exp[i].tolist(), (g, i - int(offs[g]), replayed[g][i - int(offs[g])], plies, history)
    assert np.array_equal(lines, exp)
    assert ns > 0 and leaves > 0 and nodes > 0 and (lines["flags"] & G.FLAG_SEARCHED).any()
    assert bool((lines["flags"] & G.FLAG_DRAW).any()) == history
    # a draw takes precedence over a searched leaf: the last fixture's three moves all reach rule50 = 100
    # and a leaf with a capture
    assert games[-1][0] == Q.FIXTURES[-1][1] and Q.FIXTURES[-1][0] == "fifty_before_searched"
    assert not (((lines["flags"] & G.FLAG_DRAW) != 0) & ((lines["flags"] & G.FLAG_SEARCHED) != 0)).any()
    if plies == 1:
        assert all(l[5] for l in Q.leaves(oracle_lib, big, small, games[-1][0], 0))  # every leaf would be searched
        row = lines[int(offs[len(games) - 1])][:3]
        want = (G.FLAG_DRAW, 0) if history else (0, G.FLAG_SEARCHED)
        assert [(int(f) & G.FLAG_DRAW, int(f) & G.FLAG_SEARCHED) for f in row["flags"]] == [want] * 3
    # offsets, status and records are the plain calls' bytes; a plain call resets the statistics
    if plies == 1:
        plain = gpu_ctx.evaluate_games_lines(games, K_GAMES, 0, history=history)
    else:
        plain = gpu_ctx.evaluate_games_lines2(games, K_GAMES, 0, history=history)
    assert [gpu_ctx.get_option(s) for s in (G.STAT_QUIESCE_NS, G.STAT_QUIESCE_LEAVES, G.STAT_QUIESCE_NODES)] == [0, 0, 0]
    assert _same((offs, status, pos), plain[:3]) and not (plain[3]["flags"] & G.FLAG_SEARCHED).any()
    skipped = np.flatnonzero(pos["flags"] & G.FLAG_SKIPPED)
    empty = np.array([R.EMPTY if plies == 1 else R2.EMPTY2], dtype=lines.dtype)[0]
    assert len(skipped) >= 1 and all((lines[i] == empty).all() for i in skipped)


@pytest.mark.parametrize("plies", (1, 2))
def test_games_calls_same_bytes_from_every_path(gpu_ctx, games_got, games, plies, synth_big_path, synth_small_path):
    from fishnet_amd import gpu_nnue as G
    base = games_got[(plies, True)]
    name = "evaluate_games_lines_quiescent" if plies == 1 else "evaluate_games_lines2_quiescent"
    others = []
    try:
        for pipeline, chunk in ((0, 0), (2, 1), (2, 7), (0, 7)):
            gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, pipeline)
            gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, chunk)
            others.append(getattr(gpu_ctx, name)(games, K_GAMES, DEPTH_GAMES[plies], 0, history=True))
            assert (gpu_ctx.get_option(G.STAT_QUIESCE_LEAVES), gpu_ctx.get_option(G.STAT_QUIESCE_NODES)) == base[5:7]
    finally:
        gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, 2)
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        others.append(getattr(two, name)(games, K_GAMES, DEPTH_GAMES[plies], 0, history=True))
        assert (two.get_option(G.STAT_QUIESCE_LEAVES), two.get_option(G.STAT_QUIESCE_NODES)) == base[5:7]
    finally:
        two.close()
    for o in others:
        assert _same(base[:4], o)


# ---- 5: errors and statistics -------------------------------------------------------------------

def test_argument_checks(gpu_ctx, games):
    from fishnet_amd import gpu_nnue as G
    d = gpu_ctx.alloc(4096)
    for depth in (0, 5):
        for call in (gpu_ctx.evaluate_games_lines_quiescent, gpu_ctx.evaluate_games_lines2_quiescent):
            with pytest.raises(G.GnError) as e:
                call(games[:2], 3, depth, 0, history=True)
            assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.evaluate_lines2_quiescent([R.START], 3, depth, 0)
        assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.quiesce_device(d, 1, d, d, d, 1, 0, depth, d)
        assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:  # ... with nothing to do as well
            gpu_ctx.quiesce_device(None, 0, None, None, None, 0, 0, depth, None)
        assert e.value.code == G.E_INVALID
    for k in (0, 9):
        with pytest.raises(G.GnError) as e:
            gpu_ctx.evaluate_lines2_quiescent([R.START], k, 2, 0)
        assert e.value.code == G.E_INVALID
    # total == 0 with NULL buffers: GN_OK, nothing searched; a NULL buffer with leaves, a bad mode: GN_E_INVALID
    assert gpu_ctx.quiesce_device(None, 0, None, None, None, 0, 0, 2, None) == (0, 0)
    assert gpu_ctx.quiesce_device(d, 1, d, None, None, 0, 0, 2, None) == (0, 0)
    with pytest.raises(G.GnError) as e:
        gpu_ctx.quiesce_device(d, 1, d, d, d, 1, 0, 2, None)
    assert e.value.code == G.E_INVALID
    with pytest.raises(G.GnError) as e:
        gpu_ctx.quiesce_device(d, 1, d, d, d, 1, 7, 2, d)
    assert e.value.code == G.E_INVALID
    d.free()
    out, lines = gpu_ctx.evaluate_lines2_quiescent([], 3, 2, 0)
    assert len(out) == 0 and lines.shape == (0, 3)
    for call in (gpu_ctx.evaluate_games_lines_quiescent, gpu_ctx.evaluate_games_lines2_quiescent):
        offs, status, pos, lines = call([], 3, 2, 0)
        assert list(offs) == [0] and len(pos) == 0


def test_no_net_for_the_mode(synth_big_path):
    from fishnet_amd import gpu_nnue as G
    big_only = G.GpuNnue(synth_big_path, None)
    try:
        d = big_only.alloc(4096)
        with pytest.raises(G.GnError) as e:
            big_only.quiesce_device(d, 1, d, d, d, 1, 0, 2, d)
        assert e.value.code == G.E_NONET
        d.free()
    finally:
        big_only.close()


def test_exact_size_host_outputs_and_capacity(gpu_ctx, games, games_got):
    """position_out and the offsets with outputs of exactly the sizes told, and one position too few:
    GN_E_CAPACITY with the offsets filled and nothing else written, as the plain calls."""
    import guarded_buffers as GB
    from fishnet_amd import gpu_nnue as G
    L = G.lib()
    garr, _keep = G._games_array(games)
    ng = len(games)
    for plies, name, dtype in ((1, "gn_evaluate_games_lines_quiescent", G.LINE_DTYPE),
                               (2, "gn_evaluate_games_lines2_quiescent", G.LINE2_DTYPE)):
        offs, status, pos, lines = games_got[(plies, True)][:4]
        p = len(pos)
        s = GB.GuardedSet()
        rc = getattr(L, name)(gpu_ctx.h, garr, ng, 0, K_GAMES, 1, DEPTH_GAMES[plies], s.add("offs", ng + 1, np.uint32),
                              s.add("status", ng, np.int32), s.add("pos", p, G.EVAL_DTYPE), p,
                              s.add("lines", p * K_GAMES, dtype))
        assert rc == 0
        s.check()
        assert (s["offs"].bytes(), s["pos"].bytes(), s["lines"].bytes()) == (offs.tobytes(), pos.tobytes(), lines.tobytes())
        s = GB.GuardedSet()
        rc = getattr(L, name)(gpu_ctx.h, garr, ng, 0, K_GAMES, 1, DEPTH_GAMES[plies], s.add("offs", ng + 1, np.uint32),
                              s.add("status", ng, np.int32), s.add("pos", p - 1, G.EVAL_DTYPE), p - 1,
                              s.add("lines", (p - 1) * K_GAMES, dtype))
        assert rc == G.E_CAPACITY
        s.check()
        assert s["offs"].bytes() == offs.tobytes() and s["pos"].untouched() and s["lines"].untouched()
