"""The quiescence's own variation (include/gpu_nnue.h at gn_pv) on the GPU against the rule restated
from the CPU oracle (tests/quiesce_pv_rule.py): gn_quiesce_pv_device entry by entry, also under the
tie-forcing parameter sets; gn_line_pvs_device / gn_line2_pvs_device after the extended rankings; the
three host-buffer calls gn_evaluate_lines2_quiescent_pv, gn_evaluate_games_lines_quiescent_pv and
gn_evaluate_games_lines2_quiescent_pv; and every PV of the host calls replayed without the rule.

The inputs are tests/test_gpu_quiesce.py's, by its seeds and counts (tests/test_quiesce_pv.py checks
on the CPU that they exercise both tie rules and every PV length)."""
import ctypes as C

import numpy as np
import pytest

import history_rule as H
import lines_param_sets as LP
import lines_rule as R
import quiesce_pv_rule as PV
import quiesce_rule as Q

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
MODES = (0, 1)  # FULL, BIG
K_GAMES = 8
D = Q.MAX_DEPTH
GUARD = 64      # entries on either side of d_ext / d_tail inside their allocations
SENTINEL = 0x5A5A5A5A
SENTINEL16 = 0x5A5A
DEPTH_GAMES = {1: 2, 2: 1}  # the games calls' depth, as tests/test_gpu_quiesce.py's


class _At:
    """A device pointer `nbytes` into a DeviceBuffer."""

    def __init__(self, buf, nbytes):
        self.ptr = C.c_void_p(buf.addr + nbytes)


def _same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _packed(fens):
    from fishnet_amd import gpu_nnue as G
    return fens, G.pack_fens(fens)[0]


@pytest.fixture(scope="module")
def inputs1():
    from fishnet_amd import gpu_nnue as G
    return _packed(Q.fixture_fens() + R.fixture_fens() + G.boards_to_fens(G.random_positions(Q.SEED, 0, Q.N_RANDOM, 160)))


@pytest.fixture(scope="module")
def inputs3():
    from fishnet_amd import gpu_nnue as G
    return _packed(Q.fixture_fens() + G.boards_to_fens(G.random_positions(Q.SEED, 0, Q.N_RANDOM3, 160)))


@pytest.fixture(scope="module")
def inputs2():
    from fishnet_amd import gpu_nnue as G
    return _packed(Q.fixture_fens() + G.boards_to_fens(G.random_positions(Q.SEED2, 0, Q.N_RANDOM2, 160)))


def _quiesce_both(ctx, d_parents, n, d_off, d_mv, d_rec, total, mode, depth):
    """gn_quiesce_device, then gn_quiesce_pv_device with d_ext and d_tail each inside a larger
    allocation of sentinels: (the tail buffer, d_tail, the tails[total, D]).  d_ext, searched and nodes
    must be the first call's, and nothing around either output may change."""
    ext = ctx.alloc((total + 2 * GUARD) * 4)
    ext.upload(np.full(total + 2 * GUARD, SENTINEL, dtype=np.int32))
    ns, nn = ctx.quiesce_device(d_parents, n, d_off, d_mv, d_rec, total, mode, depth, _At(ext, GUARD * 4))
    want = ext.download(np.int32, total + 2 * GUARD)
    ext.upload(np.full(total + 2 * GUARD, SENTINEL, dtype=np.int32))
    tail = ctx.alloc((total * D + 2 * GUARD) * 2)
    tail.upload(np.full(total * D + 2 * GUARD, SENTINEL16, dtype=np.uint16))
    d_tail = _At(tail, GUARD * 2)
    got = ctx.quiesce_pv_device(d_parents, n, d_off, d_mv, d_rec, total, mode, depth, _At(ext, GUARD * 4), d_tail)
    assert got == (ns, nn)
    assert ext.download(np.int32, total + 2 * GUARD).tobytes() == want.tobytes()
    all_ = tail.download(np.uint16, total * D + 2 * GUARD)
    assert (all_[:GUARD] == SENTINEL16).all() and (all_[GUARD + total * D:] == SENTINEL16).all()
    return ext, _At(ext, GUARD * 4), tail, d_tail, all_[GUARD:GUARD + total * D].reshape(total, D), want[GUARD:GUARD + total]


def _level1(ctx, boards, mode, depths, ks=KS):
    """gn_expand_device, then per depth both quiescence calls, the extended ranking and
    gn_line_pvs_device for every K of ks (with the tails and without), and the plain ranking's PVs."""
    from fishnet_amd import gpu_nnue as G
    n = len(boards)
    cap = 256 * n
    b = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                       ("mv", cap * 2), ("co", cap * G.EVAL_SIZE), ("ln", n * 8 * 12),
                                       ("pv", (n * 8 + 2) * 16))}
    b["b"].upload(boards)
    total = ctx.expand_device(b["b"], n, mode, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
    r = {"total": total, "off": b["off"].download(np.uint32, n + 1), "mv": b["mv"].download(np.uint16, total), "depth": {}}

    def pvs(K, d_tail):
        b["pv"].upload(np.full((n * 8 + 2) * 8, SENTINEL16, dtype=np.uint16))
        ctx.line_pvs_device(n, b["off"], b["mv"], d_tail, b["ln"], K, _At(b["pv"], 16))
        ctx.synchronize()
        raw = b["pv"].download(np.uint16, (n * 8 + 2) * 8)
        assert (raw[:8] == SENTINEL16).all() and (raw[8 + n * K * 8:] == SENTINEL16).all()
        return raw[8:8 + n * K * 8].view(G.PV_DTYPE).reshape(n, K)

    for depth in depths:
        ext, d_ext, tail, d_tail, tails, ev = _quiesce_both(ctx, b["b"], n, b["off"], b["mv"], b["co"], total, mode, depth)
        x = r["depth"][depth] = {"tails": tails, "ext": ev, "lines": {}, "pvs": {}, "heads": {}}
        for K in ks:
            ctx.rank_children_extended_device(b["b"], n, b["off"], b["mv"], b["co"], d_ext, K, b["ln"])
            ctx.synchronize()
            x["lines"][K] = b["ln"].download(G.LINE_DTYPE, n * K).reshape(n, K)
            x["pvs"][K] = pvs(K, d_tail)
            x["heads"][K] = pvs(K, None)
        last_tail = (tail, d_tail)
        ext.free()
        if depth != depths[-1]:
            tail.free()
    ctx.rank_children_device(b["b"], n, b["off"], b["mv"], b["co"], 8, b["ln"])
    ctx.synchronize()
    r["plain"] = b["ln"].download(G.LINE_DTYPE, n * 8).reshape(n, 8)
    r["plain_pvs"] = pvs(8, last_tail[1])  # no line is searched: the tails given are not used
    last_tail[0].free()
    for x in b.values():
        x.free()
    return r


@pytest.fixture(scope="module")
def level1(gpu_ctx, inputs1, inputs3):
    return {mode: {"a": _level1(gpu_ctx, inputs1[1], mode, (1, 2)), "b": _level1(gpu_ctx, inputs3[1], mode, (3,), ks=(8,))}
            for mode in MODES}


def _check_tails(O, big, small, fens, r, tails, ext, depth, mode):
    """Every leaf's d_tail row against the rule's; returns the PV lengths among the searched leaves."""
    lengths = {}
    for i, fen in enumerate(fens):
        a, b = int(r["off"][i]), int(r["off"][i + 1])
        want = PV.tails(O, big, small, fen, depth, mode)
        assert len(want) == b - a
        for j in range(a, b):
            m = int(r["mv"][j])
            assert tails[j].tolist() == PV.tail_row(want[m]), (fen, m, depth, mode)
            if ext[j] != Q.NOT_EXTENDED:
                lengths[len(want[m])] = lengths.get(len(want[m]), 0) + 1
            else:
                assert not tails[j].any()
    return lengths


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", (1, 2, 3))
def test_quiesce_pv_entries_vs_rule(level1, inputs1, inputs3, oracle_lib, oracle_nets, mode, depth):
    """d_tail entry by entry; d_ext, searched and nodes are gn_quiesce_device's bytes and the
    surroundings untouched (_quiesce_both); unsearched leaves have all-zero tails."""
    big, small = oracle_nets
    which, fens = ("b", inputs3[0]) if depth == 3 else ("a", inputs1[0])
    r = level1[mode][which]
    x = r["depth"][depth]
    lengths = _check_tails(oracle_lib, big, small, fens, r, x["tails"], x["ext"], depth, mode)
    print(f"depth {depth} mode {mode}: PV lengths among the searched leaves {dict(sorted(lengths.items()))}")
    assert sum(lengths.values()) == int((x["ext"] != Q.NOT_EXTENDED).sum()) == (516 if depth == 3 else 2027)
    assert lengths.get(depth, 0) >= 100


@pytest.mark.parametrize("name", ("clamp0", "rule50/clamp"))
def test_quiesce_pv_entries_under_tie_forcing_sets(gpu_ctx, inputs3, oracle_lib, oracle_nets, name):
    """Depth 2 on the depth-3 set under the sets that make both tie rules decide."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    fens, boards = inputs3
    n, cap = len(boards), 256 * len(boards)
    with LP.under(oracle_lib, name, gpu_ctx):
        b = {k: gpu_ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4),
                                               ("ch", cap * 32), ("mv", cap * 2), ("co", cap * G.EVAL_SIZE))}
        try:
            b["b"].upload(boards)
            total = gpu_ctx.expand_device(b["b"], n, 0, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
            r = {"off": b["off"].download(np.uint32, n + 1), "mv": b["mv"].download(np.uint16, total)}
            ext, _, tail, _, tails, ev = _quiesce_both(gpu_ctx, b["b"], n, b["off"], b["mv"], b["co"], total, 0, 2)
            ext.free(), tail.free()
        finally:
            for x in b.values():
                x.free()
        lengths = _check_tails(oracle_lib, big, small, fens, r, tails, ev, 2, 0)
        counts = PV.Counts()
        for fen in fens:
            for m, c, check, live, static, srch in Q.leaves(oracle_lib, big, small, fen, 0) or []:
                if srch:
                    PV.count_ties(oracle_lib, big, small, c, 2, 0, check, static, counts)
    print(f"{name}: PV lengths {dict(sorted(lengths.items()))}, {counts.move_ties} move ties, "
          f"{counts.stand_pat_ties} stand-pat ties")
    assert sum(lengths.values()) == 516 and counts.stand_pat_ties >= 1000 and counts.move_ties >= 50


def test_tails_no_parent_covers_are_zero(gpu_ctx, inputs3):
    """With fewer parents than `total` covers, the covered tails are the full call's and the rest 0."""
    from fishnet_amd import gpu_nnue as G
    boards = inputs3[1][:12]
    n, cap = len(boards), 256 * len(boards)
    b = {k: gpu_ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                           ("mv", cap * 2), ("co", cap * G.EVAL_SIZE))}
    b["b"].upload(boards)
    total = gpu_ctx.expand_device(b["b"], n, 0, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
    off = b["off"].download(np.uint32, n + 1)
    ext, _, tail, _, full, _ = _quiesce_both(gpu_ctx, b["b"], n, b["off"], b["mv"], b["co"], total, 0, 2)
    ext.free(), tail.free()
    m = n - 3
    head = int(off[m])
    assert 0 < head < total
    ext, _, tail, _, part, _ = _quiesce_both(gpu_ctx, b["b"], m, b["off"], b["mv"], b["co"], total, 0, 2)
    ext.free(), tail.free()
    assert np.array_equal(part[:head], full[:head]) and not part[head:].any() and full[head:].any()
    for x in b.values():
        x.free()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth,K", [(1, 1), (1, 3), (1, 8), (2, 1), (2, 3), (2, 8), (3, 8)])
def test_line_pvs_device_vs_rule(level1, inputs1, inputs3, oracle_lib, oracle_nets, mode, depth, K):
    """gn_line_pvs_device after the extended ranking: with the tails, with d_tail NULL (heads only), and
    on the plain ranking's lines (nothing searched: no tails)."""
    big, small = oracle_nets
    which, fens = ("b", inputs3[0]) if depth == 3 else ("a", inputs1[0])
    r = level1[mode][which]
    x = r["depth"][depth]
    lines = Q.lines(oracle_lib, big, small, fens, depth, mode, K)
    assert np.array_equal(x["lines"][K], lines)
    exp = PV.line_pvs(oracle_lib, big, small, fens, lines, depth, mode)
    for i in np.flatnonzero((x["pvs"][K] != exp).any(axis=1))[:5]:
        assert x["pvs"][K][i].tolist() == exp[i].tolist(), (fens[i], mode, depth, K)
    assert x["pvs"][K].tobytes() == exp.tobytes()
    if K == 8:
        assert (exp["len"] > 1).sum() >= 4 and int(exp["len"].max()) == 1 + depth
    assert x["heads"][K].tobytes() == PV.line_pvs(oracle_lib, big, small, fens, lines, depth, mode, with_tails=False).tobytes()
    if K == 8:
        assert not (r["plain"]["flags"] & Q.FLAG_SEARCHED).any()
        assert r["plain_pvs"].tobytes() == PV.line_pvs(oracle_lib, big, small, fens, r["plain"], depth, mode).tobytes()
        assert int(r["plain_pvs"]["len"].max()) == 1


# ---- two plies, the device path -----------------------------------------------------------------

def _level2(ctx, boards, mode, depths):
    from fishnet_amd import gpu_nnue as G
    from test_gpu_parity import _expand2
    n = len(boards)
    d_b, d_ln, d_pv = ctx.alloc(n * 32), ctx.alloc(n * 8 * 16), ctx.alloc((n * 8 + 2) * 16)
    d_b.upload(boards)
    t, g, out = _expand2(ctx, d_b, n, mode)
    r = {"depth": {}}

    def pvs(K, d_gtail):
        d_pv.upload(np.full((n * 8 + 2) * 8, SENTINEL16, dtype=np.uint16))
        ctx.line2_pvs_device(n, out, d_gtail, d_ln, K, _At(d_pv, 16))
        ctx.synchronize()
        raw = d_pv.download(np.uint16, (n * 8 + 2) * 8)
        assert (raw[:8] == SENTINEL16).all() and (raw[8 + n * K * 8:] == SENTINEL16).all()
        return raw[8:8 + n * K * 8].view(G.PV_DTYPE).reshape(n, K)

    for depth in depths:
        ext, d_gext, tail, d_gtail, tails, ev = _quiesce_both(ctx, out["ch"], t, out["goff"], out["gmv"], out["gco"], g, mode, depth)
        x = r["depth"][depth] = {"lines": {}, "pvs": {}, "heads": {}}
        for K in KS:
            ctx.rank_lines2_extended_device(d_b, n, out, d_gext, K, d_ln)
            ctx.synchronize()
            x["lines"][K] = d_ln.download(G.LINE2_DTYPE, n * K).reshape(n, K)
            x["pvs"][K] = pvs(K, d_gtail)
            x["heads"][K] = pvs(K, None)
        if depth == depths[-1]:
            ctx.rank_lines2_device(d_b, n, out, 8, d_ln)
            ctx.synchronize()
            r["plain"] = d_ln.download(G.LINE2_DTYPE, n * 8).reshape(n, 8)
            r["plain_pvs"] = pvs(8, d_gtail)
        ext.free(), tail.free()
    for x in list(out.values()) + [d_b, d_ln, d_pv]:
        if hasattr(x, "free"):
            x.free()
    return r


@pytest.fixture(scope="module")
def level2(gpu_ctx, inputs2):
    return {mode: _level2(gpu_ctx, inputs2[1], mode, (1, 2)) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", (1, 2))
def test_line2_pvs_device_vs_rule(level2, inputs2, oracle_lib, oracle_nets, mode, depth):
    big, small = oracle_nets
    fens = inputs2[0]
    x = level2[mode]["depth"][depth]
    for K in KS:
        lines = Q.lines2(oracle_lib, big, small, fens, depth, mode, K)
        assert np.array_equal(x["lines"][K], lines)
        exp = PV.line2_pvs(oracle_lib, big, small, fens, lines, depth, mode)
        for i in np.flatnonzero((x["pvs"][K] != exp).any(axis=1))[:5]:
            assert x["pvs"][K][i].tolist() == exp[i].tolist(), (fens[i], mode, depth, K)
        assert x["pvs"][K].tobytes() == exp.tobytes()
        heads = PV.line2_pvs(oracle_lib, big, small, fens, lines, depth, mode, with_tails=False)
        assert x["heads"][K].tobytes() == heads.tobytes()
    assert int(exp["len"].max()) == 2 + depth and (exp["len"] > 2).sum() >= 4
    if depth == 2:
        plain = level2[mode]["plain"]
        assert not (plain["flags"] & Q.FLAG_SEARCHED).any()
        assert level2[mode]["plain_pvs"].tobytes() == PV.line2_pvs(oracle_lib, big, small, fens, plain, 2, mode).tobytes()


# ---- the host-buffer calls ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def games():
    g = H.fixture_games()
    assert g[4][0].split()[4] == "99"
    return [g[0], g[1], g[4], g[10]] + [(f, "", ()) for f in Q.fixture_fens()]


@pytest.fixture(scope="module")
def replayed(oracle_lib, games):
    return [oracle_lib.replay_game(root, moves)[0] for root, moves, _ in games]


QSTATS = ("STAT_QUIESCE_LEAVES", "STAT_QUIESCE_NODES")


def _qstats(ctx):
    from fishnet_amd import gpu_nnue as G
    return [ctx.get_option(getattr(G, s)) for s in QSTATS]


@pytest.fixture(scope="module")
def games_got(gpu_ctx, games):
    """{(plies, history): (offsets, status, records, lines, pvs)}, each checked against the quiescent
    call's bytes and statistics."""
    from fishnet_amd import gpu_nnue as G
    out = {}
    for plies, name in ((1, "evaluate_games_lines_quiescent"), (2, "evaluate_games_lines2_quiescent")):
        for history in (False, True):
            res = getattr(gpu_ctx, name + "_pv")(games, K_GAMES, DEPTH_GAMES[plies], 0, history=history)
            stats, pv_ns = _qstats(gpu_ctx), gpu_ctx.get_option(G.STAT_PV_NS)
            assert pv_ns > 0 and gpu_ctx.get_option(G.STAT_QUIESCE_NS) > 0
            plain = getattr(gpu_ctx, name)(games, K_GAMES, DEPTH_GAMES[plies], 0, history=history)
            assert gpu_ctx.get_option(G.STAT_PV_NS) == 0 and _qstats(gpu_ctx) == stats and stats[0] > 0
            assert _same(res[:4], plain)
            out[(plies, history)] = res
    return out


@pytest.mark.parametrize("history", (False, True))
@pytest.mark.parametrize("plies", (1, 2))
def test_games_calls_vs_rule(games_got, games, replayed, oracle_lib, oracle_nets, plies, history):
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    offs, status, pos, lines, pvs = games_got[(plies, history)]
    depth = DEPTH_GAMES[plies]
    fens = [f for fs in replayed for f in fs]
    assert len(fens) == len(lines) == len(pvs) and pvs.dtype == G.PV_DTYPE and pvs.shape == lines.shape
    rule = PV.line_pvs if plies == 1 else PV.line2_pvs
    exp = rule(oracle_lib, big, small, fens, lines, depth, 0)
    for i in np.flatnonzero((pvs != exp).any(axis=1))[:5]:
        assert pvs[i].tolist() == exp[i].tolist(), (fens[i], plies, history)
    assert pvs.tobytes() == exp.tobytes()
    assert int(pvs["len"].max()) == plies + depth
    skipped = np.flatnonzero(pos["flags"] & G.FLAG_SKIPPED)
    assert len(skipped) >= 1 and not pvs[skipped].view(np.uint16).any()
    if plies == 1:  # the last fixture's moves all reach rule50 = 100 and a leaf with a capture
        assert games[-1][0] == Q.FIXTURES[-1][1] and Q.FIXTURES[-1][0] == "fifty_before_searched"
        row, prow = lines[int(offs[len(games) - 1])][:3], pvs[int(offs[len(games) - 1])][:3]
        if history:
            assert all(int(f) & G.FLAG_DRAW for f in row["flags"]) and prow["len"].tolist() == [1, 1, 1]
        else:
            assert all(int(f) & G.FLAG_SEARCHED for f in row["flags"]) and (prow["len"] >= 1).all()


@pytest.mark.parametrize("plies", (1, 2))
def test_games_calls_same_bytes_from_every_path(gpu_ctx, games_got, games, plies, synth_big_path, synth_small_path):
    from fishnet_amd import gpu_nnue as G
    base = games_got[(plies, True)]
    name = "evaluate_games_lines_quiescent_pv" if plies == 1 else "evaluate_games_lines2_quiescent_pv"
    others = []
    try:
        for pipeline, chunk in ((0, 0), (2, 1), (2, 7), (0, 7)):
            gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, pipeline)
            gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, chunk)
            others.append(getattr(gpu_ctx, name)(games, K_GAMES, DEPTH_GAMES[plies], 0, history=True))
            assert gpu_ctx.get_option(G.STAT_PV_NS) > 0
    finally:
        gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, 2)
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        others.append(getattr(two, name)(games, K_GAMES, DEPTH_GAMES[plies], 0, history=True))
        assert two.get_option(G.STAT_PV_NS) > 0
    finally:
        two.close()
    for o in others:
        assert _same(base, o)


def test_evaluate_lines2_quiescent_pv(gpu_ctx, level2, inputs2, synth_big_path, synth_small_path):
    """The FEN call: the quiescent call's bytes, the device path's PVs, every chunk size and two shards."""
    from fishnet_amd import gpu_nnue as G
    fens = inputs2[0]
    out, lines, pvs = gpu_ctx.evaluate_lines2_quiescent_pv(fens, 8, 2, 0)
    stats = _qstats(gpu_ctx)
    assert gpu_ctx.get_option(G.STAT_PV_NS) > 0 and stats[0] > 0
    assert pvs.tobytes() == level2[0]["depth"][2]["pvs"][8].tobytes()
    q = gpu_ctx.evaluate_lines2_quiescent(fens, 8, 2, 0)
    assert gpu_ctx.get_option(G.STAT_PV_NS) == 0 and _qstats(gpu_ctx) == stats
    assert _same((out, lines), q)
    others = []
    try:
        for chunk in (1, 7):
            gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, chunk)
            others.append(gpu_ctx.evaluate_lines2_quiescent_pv(fens, 8, 2, 0))
            assert _qstats(gpu_ctx) == stats
    finally:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        others.append(two.evaluate_lines2_quiescent_pv(fens, 8, 2, 0))
    finally:
        two.close()
    assert all(_same((out, lines, pvs), o) for o in others)
    for K in (1, 3):
        assert gpu_ctx.evaluate_lines2_quiescent_pv(fens, K, 2, 0)[2].tobytes() == level2[0]["depth"][2]["pvs"][K].tobytes()
    bad = gpu_ctx.evaluate_lines2_quiescent_pv(["not a fen", R.START], 3, 2, 0)
    assert int(bad[0]["flags"][0]) & G.FLAG_BAD_FEN and not bad[2][0].view(np.uint16).any() and bad[2]["len"][1].all()


# ---- oracle-free: every PV replayed -------------------------------------------------------------

def _replay_check(ctx, O, fens, lines, pvs, plies, mode):
    """Every non-empty PV played out with the oracle's child_fen alone: each move legal where it is
    played, and negate_ply applied len times to the end's own value -- mate / stalemate / a draw by the
    line's flags, else the static final_v of gn_evaluate_batch_mode for the end FEN -- is line.value."""
    from fishnet_amd import gpu_nnue as G
    ends, items = [], []
    for i, fen in enumerate(fens):
        for ln, pv in zip(lines[i], pvs[i]):
            n = int(pv["len"])
            if not n:
                assert int(ln["flags"]) & G.FLAG_NO_SCORE
                continue
            f = fen
            for m in pv["moves"][:n].tolist():
                assert m in O.legal_moves(f), (fen, pv)
                f = O.child_fen(f, m)
            assert not pv["moves"][n:].any() and not pv["reserved"]
            items.append((fen, ln, n, len(ends)))
            ends.append(f)
    rec = ctx.evaluate_batch(ends, mode)
    tails = 0
    for fen, ln, n, e in items:
        fl = int(ln["flags"])
        if fl & G.FLAG_DRAW:
            v = 0
            assert n == (1 if plies == 1 else int(ln["plies"]))
        elif int(rec["flags"][e]) & G.FLAG_NO_MOVES:
            v = -R.VALUE_MATE if int(rec["flags"][e]) & G.FLAG_IN_CHECK else 0
        else:
            v = int(rec["final_v"][e])
        for _ in range(n):
            v = R.negate_ply(v)
        assert v == int(ln["value"]), (fen, ln, n, ends[e])
        tails += n > plies
    return tails


@pytest.mark.parametrize("history", (False, True))
@pytest.mark.parametrize("plies", (1, 2))
def test_host_pvs_replayed_without_the_rule(gpu_ctx, games_got, replayed, oracle_lib, plies, history):
    offs, status, pos, lines, pvs = games_got[(plies, history)]
    fens = [f for fs in replayed for f in fs]
    assert _replay_check(gpu_ctx, oracle_lib, fens, lines, pvs, plies, 0) >= 20


@pytest.mark.parametrize("mode", MODES)
def test_lines2_pvs_replayed_without_the_rule(gpu_ctx, inputs2, oracle_lib, mode):
    out, lines, pvs = gpu_ctx.evaluate_lines2_quiescent_pv(inputs2[0], 8, 2, mode)
    assert _replay_check(gpu_ctx, oracle_lib, inputs2[0], lines, pvs, 2, mode) >= 20


# ---- errors and exact-size outputs --------------------------------------------------------------

def test_argument_checks(gpu_ctx, games):
    from fishnet_amd import gpu_nnue as G
    L = G.lib()
    d = gpu_ctx.alloc(4096)
    for depth in (0, 5):
        for call in (gpu_ctx.evaluate_games_lines_quiescent_pv, gpu_ctx.evaluate_games_lines2_quiescent_pv):
            with pytest.raises(G.GnError) as e:
                call(games[:2], 3, depth, 0, history=True)
            assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.evaluate_lines2_quiescent_pv([R.START], 3, depth, 0)
        assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.quiesce_pv_device(d, 1, d, d, d, 1, 0, depth, d, d)
        assert e.value.code == G.E_INVALID
    for k in (0, 9):
        with pytest.raises(G.GnError) as e:
            gpu_ctx.evaluate_lines2_quiescent_pv([R.START], k, 2, 0)
        assert e.value.code == G.E_INVALID
        for call in (gpu_ctx.evaluate_games_lines_quiescent_pv, gpu_ctx.evaluate_games_lines2_quiescent_pv):
            with pytest.raises(G.GnError) as e:
                call(games[:2], k, 2, 0)
            assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.line_pvs_device(1, d, d, None, d, k, d)
        assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.line2_pvs_device(1, {"off": d, "mv": d, "goff": d, "gmv": d}, None, d, k, d)
        assert e.value.code == G.E_INVALID
    # a NULL d_tail with leaves, a NULL d_pvs / d_lines with positions: GN_E_INVALID; nothing to do: GN_OK
    with pytest.raises(G.GnError) as e:
        gpu_ctx.quiesce_pv_device(d, 1, d, d, d, 1, 0, 2, d, None)
    assert e.value.code == G.E_INVALID
    assert gpu_ctx.quiesce_pv_device(None, 0, None, None, None, 0, 0, 2, None, None) == (0, 0)
    for args in ((1, d, d, None, None, 3, d), (1, d, d, None, d, 3, None), (1, None, d, None, d, 3, d)):
        with pytest.raises(G.GnError) as e:
            gpu_ctx.line_pvs_device(*args)
        assert e.value.code == G.E_INVALID
    gpu_ctx.line_pvs_device(0, None, None, None, None, 3, None)
    d.free()
    # NULL pvs
    garr, _keep = G._games_array(games[:2])
    offs, status = np.zeros(3, dtype=np.uint32), np.zeros(2, dtype=np.int32)
    pos = np.zeros(64, dtype=G.EVAL_DTYPE)
    for name, dtype in (("gn_evaluate_games_lines_quiescent_pv", G.LINE_DTYPE),
                        ("gn_evaluate_games_lines2_quiescent_pv", G.LINE2_DTYPE)):
        lines = np.zeros(64 * 3, dtype=dtype)
        rc = getattr(L, name)(gpu_ctx.h, garr, 2, 0, 3, 1, 2, offs.ctypes.data, status.ctypes.data, pos.ctypes.data, 64,
                              lines.ctypes.data, None)
        assert rc == G.E_INVALID
    farr, _keep2 = G._fen_array([R.START])
    out, lines = np.zeros(1, dtype=G.EVAL_DTYPE), np.zeros(3, dtype=G.LINE2_DTYPE)
    assert L.gn_evaluate_lines2_quiescent_pv(gpu_ctx.h, farr, 1, 0, 3, 2, out.ctypes.data, lines.ctypes.data, None) == G.E_INVALID
    out, lines, pvs = gpu_ctx.evaluate_lines2_quiescent_pv([], 3, 2, 0)
    assert len(out) == 0 and lines.shape == pvs.shape == (0, 3)
    for call in (gpu_ctx.evaluate_games_lines_quiescent_pv, gpu_ctx.evaluate_games_lines2_quiescent_pv):
        offs, status, pos, lines, pvs = call([], 3, 2, 0)
        assert list(offs) == [0] and len(pos) == 0 and len(pvs) == 0


def test_exact_size_host_outputs_and_capacity(gpu_ctx, games, games_got, inputs2):
    """Outputs of exactly the sizes told between guards, and one position too few: GN_E_CAPACITY with the
    offsets filled and nothing else written, the PVs included."""
    import guarded_buffers as GB
    from fishnet_amd import gpu_nnue as G
    L = G.lib()
    garr, _keep = G._games_array(games)
    ng = len(games)
    for plies, name, dtype in ((1, "gn_evaluate_games_lines_quiescent_pv", G.LINE_DTYPE),
                               (2, "gn_evaluate_games_lines2_quiescent_pv", G.LINE2_DTYPE)):
        offs, status, pos, lines, pvs = games_got[(plies, True)]
        p = len(pos)
        s = GB.GuardedSet()
        rc = getattr(L, name)(gpu_ctx.h, garr, ng, 0, K_GAMES, 1, DEPTH_GAMES[plies], s.add("offs", ng + 1, np.uint32),
                              s.add("status", ng, np.int32), s.add("pos", p, G.EVAL_DTYPE), p,
                              s.add("lines", p * K_GAMES, dtype), s.add("pvs", p * K_GAMES, G.PV_DTYPE))
        assert rc == 0
        s.check()
        assert (s["offs"].bytes(), s["pos"].bytes(), s["lines"].bytes(), s["pvs"].bytes()) == \
            (offs.tobytes(), pos.tobytes(), lines.tobytes(), pvs.tobytes())
        s = GB.GuardedSet()
        rc = getattr(L, name)(gpu_ctx.h, garr, ng, 0, K_GAMES, 1, DEPTH_GAMES[plies], s.add("offs", ng + 1, np.uint32),
                              s.add("status", ng, np.int32), s.add("pos", p - 1, G.EVAL_DTYPE), p - 1,
                              s.add("lines", (p - 1) * K_GAMES, dtype), s.add("pvs", (p - 1) * K_GAMES, G.PV_DTYPE))
        assert rc == G.E_CAPACITY
        s.check()
        assert s["offs"].bytes() == offs.tobytes() and s["pos"].untouched() and s["lines"].untouched() and s["pvs"].untouched()
    fens = inputs2[0]
    farr, _keep2 = G._fen_array(fens)
    want = gpu_ctx.evaluate_lines2_quiescent_pv(fens, 3, 2, 0)
    s = GB.GuardedSet()
    rc = L.gn_evaluate_lines2_quiescent_pv(gpu_ctx.h, farr, len(fens), 0, 3, 2, s.add("out", len(fens), G.EVAL_DTYPE),
                                           s.add("lines", len(fens) * 3, G.LINE2_DTYPE), s.add("pvs", len(fens) * 3, G.PV_DTYPE))
    assert rc == 0
    s.check()
    assert (s["out"].bytes(), s["lines"].bytes(), s["pvs"].bytes()) == tuple(x.tobytes() for x in want)
