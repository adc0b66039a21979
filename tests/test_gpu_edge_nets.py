"""GPU parity on the edge nets (tests/edge_nets.py) and the row-cover positions
(tests/golden/row_cover_fens.txt): the nets and positions that tests/test_edge_coverage.py shows
to reach every feature-transformer row, both sides of fc_0's and fc_1's clips and the int8
extremes of every weight matrix.  Everything is compared integer for integer with the oracle.
"""
import numpy as np
import pytest

import edge_nets
from test_gpu_parity import _cmp, _expand2, special_fens

pytestmark = pytest.mark.gpu

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
N_BATCH = 32773
PREFIXES = (700, 4099, 8195, 16387, 32773)  # 1, 2, 4, 8, 16 positions per big-net workgroup
THREADS = 16


def _ctx(big, small):
    from fishnet_amd import build, gpu_nnue as G
    build.build()
    return G.GpuNnue(edge_nets.edge_net(*big) if big else None, edge_nets.edge_net(*small) if small else None)


def _nets(oracle_lib, big, small):
    return (oracle_lib.Net(edge_nets.edge_net(*big)) if big else None,
            oracle_lib.Net(edge_nets.edge_net(*small)) if small else None)


@pytest.fixture(scope="module")
def edge_ctx():
    ctx = _ctx((3072, 1), (128, 2))
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def edge_oracle(oracle_lib):
    return _nets(oracle_lib, (3072, 1), (128, 2))


@pytest.fixture(scope="module")
def F():
    return edge_nets.fixture_fens()


@pytest.fixture(scope="module")
def batch(edge_ctx, F):
    """32,773 boards: whole device random games, then F, then runs of one repeated position (40
    and 17); boards 32 and 100 zeroed.  -> (boards, valid mask, FENs of the valid boards)."""
    from fishnet_amd import gpu_nnue as G
    plies = 80
    n_game = N_BATCH - len(F) - 57
    games = -(-n_game // (plies + 1))
    d = edge_ctx.alloc(games * (plies + 1) * 32)
    edge_ctx.random_games_device(0x5EED0E00, 0, games, plies, d)
    edge_ctx.synchronize()
    g = d.download(G.BOARD_DTYPE, games * (plies + 1))[:n_game]
    d.free()
    fb, ok = G.pack_fens(F)
    assert ok.all()
    boards = np.concatenate([g, fb, np.repeat(g[5:6], 40), np.repeat(g[70:71], 17)])
    boards[32] = np.zeros(1, dtype=G.BOARD_DTYPE)
    boards[100] = np.zeros(1, dtype=G.BOARD_DTYPE)
    assert len(boards) == N_BATCH
    valid = boards["occ"] != 0
    return boards, valid, G.boards_to_fens(boards[valid])


def _eval_prefixes(ctx, batch, oracle_lib, nets, mode, prefixes, options=((1, None),)):
    """evaluate_device on prefixes of the batch under (OPT_KING_SORT, OPT_XCD_SWIZZLE mask) settings
    (None: the default mask), against one oracle pass over the whole batch."""
    from fishnet_amd import gpu_nnue as G
    boards, valid, fens = batch
    exp = oracle_lib.eval_fens(nets[0], nets[1], fens, mode, threads=THREADS)
    pos = np.cumsum(valid) - 1  # index of a valid board among the valid ones
    d_b, d_o = ctx.alloc(boards.nbytes), ctx.alloc(len(boards) * G.EVAL_SIZE)
    d_b.upload(boards)
    swz0 = ctx.get_option(G.OPT_XCD_SWIZZLE)
    try:
        for ksort, swz in options:
            ctx.set_option(G.OPT_KING_SORT, ksort)
            ctx.set_option(G.OPT_XCD_SWIZZLE, swz0 if swz is None else swz)
            for n in prefixes:
                ctx.evaluate_device(d_b, n, mode, d_o)
                got = d_o.download(G.EVAL_DTYPE, n)
                v = valid[:n]
                nv = int(v.sum())
                assert pos[n - 1] == nv - 1
                try:
                    _cmp(got[v], exp[:nv], fens[:nv])
                except AssertionError as e:
                    raise AssertionError(f"mode {mode} n {n} king_sort {ksort} swizzle {swz}: {e}") from None
                assert (got[~v]["flags"] & G.FLAG_BAD_FEN).all() and (~v).sum() == 2
    finally:
        ctx.set_option(G.OPT_KING_SORT, 1)
        ctx.set_option(G.OPT_XCD_SWIZZLE, swz0)
        d_b.free()
        d_o.free()


# (OPT_KING_SORT, OPT_XCD_SWIZZLE): sorted at any size / input order, crossed with the swizzle mask
# 0, the default (9: bit 1, the batch-evaluation bit, is clear, so eval_net launches as with 0) and
# 7 (bit 1 set: launch_eval_net's grid rounded up to 8 and each XCD's contiguous range of tiles)
LOCALITY = ((2, 0), (2, None), (2, 7), (0, 0), (0, None), (0, 7))


def test_eval_net_3072_every_tile_size(edge_ctx, edge_oracle, oracle_lib, batch):
    """eval_net_kernel<3072> at 1, 2, 4, 8 and 16 positions per workgroup (batches of 700, 4,099,
    8,195, 16,387 and 32,773), king-sorted and in input order, with GN_OPT_XCD_SWIZZLE 0, its
    default 9 (tiles in dispatch order, as with 0) and 7 (the XCD tile order of batch evaluation)."""
    _eval_prefixes(edge_ctx, batch, oracle_lib, (edge_oracle[0], None), 1, PREFIXES, LOCALITY)


def test_eval_net_3072_stress_every_tile_size(oracle_lib, batch):
    """The same under constant int16 wrapping of the accumulators (stress edge net)."""
    ctx = _ctx((3072, 11, True), None)
    try:
        _eval_prefixes(ctx, batch, oracle_lib, _nets(oracle_lib, (3072, 11, True), None), 1, PREFIXES, LOCALITY)
    finally:
        ctx.close()


def test_eval_net_1024_tile_sizes(oracle_lib, batch):
    """eval_net_kernel<1024> (a 1024-wide net as the big net) at 1, 2 and 16 positions per workgroup."""
    ctx = _ctx((1024, 5), None)
    try:
        _eval_prefixes(ctx, batch, oracle_lib, _nets(oracle_lib, (1024, 5), None), 1, (700, 4099, 32773))
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [0, 2])
def test_eval_full_and_small_modes(edge_ctx, edge_oracle, oracle_lib, batch, mode):
    """Edge big + edge small net in modes FULL (selection, re-evaluation marks) and SMALL."""
    _eval_prefixes(edge_ctx, batch, oracle_lib, edge_oracle, mode, (4099, 32773))
    if mode == 0:
        e = oracle_lib.eval_fens(edge_oracle[0], edge_oracle[1], batch[2][-2000:], 0, threads=THREADS)
        assert (e["flags"] & 2).any() and (e["flags"] & 8).any() and ((e["flags"] & 10) == 0).any()


# ---- expansion -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def parents(edge_ctx, F):
    """6 device games x 81 positions, 200 of the row-cover positions, the special positions."""
    from fishnet_amd import gpu_nnue as G
    d = edge_ctx.alloc(6 * 81 * 32)
    edge_ctx.random_games_device(0x5EED0E01, 0, 6, 80, d)
    edge_ctx.synchronize()
    g = d.download(G.BOARD_DTYPE, 6 * 81)
    d.free()
    fens = G.boards_to_fens(g) + edge_nets.row_cover_fens()[::7][:200] + special_fens()
    boards, ok = G.pack_fens(fens)
    assert ok.all()
    return boards, fens


def _oracle_expansion(oracle_lib, nets, fens, mode):
    """(parents, offsets, children sorted by move within each parent, sorted moves)."""
    par, cnt, kids = oracle_lib.expand_eval_batch(nets[0], nets[1], fens, mode, True, threads=THREADS,
                                                  keep_children=True)
    assert (cnt >= 0).all()
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    mv = np.zeros(off[-1], dtype=np.uint16)
    ch = np.zeros(off[-1], dtype=kids.dtype)
    for i, f in enumerate(fens):
        m = np.array(oracle_lib.legal_moves(f), dtype=np.uint16)
        assert len(m) == cnt[i]
        o = np.argsort(m, kind="stable")
        mv[off[i]:off[i + 1]] = m[o]
        ch[off[i]:off[i + 1]] = kids[i, :cnt[i]][o]
    return par, off, ch, mv


def _cmp_expansion(got, exp, fens, what):
    """Every parent and every child (children matched by move) against the oracle's."""
    po, off, mv, co = got
    par, eoff, ech, emv = exp
    try:
        _cmp(po, par, fens)
    except AssertionError as e:
        raise AssertionError(f"{what}: parents: {e}") from None
    assert np.array_equal(off.astype(np.int64), eoff), what
    mv, co = mv.copy(), co.copy()
    for i in range(len(fens)):
        lo, hi = int(eoff[i]), int(eoff[i + 1])
        o = np.argsort(mv[lo:hi], kind="stable")
        mv[lo:hi], co[lo:hi] = mv[lo:hi][o], co[lo:hi][o]
    assert np.array_equal(mv, emv), what
    bad = np.nonzero(co != ech)[0]
    if len(bad):
        j = int(bad[0])
        i = int(np.searchsorted(eoff, j, side="right") - 1)
        raise AssertionError(f"{what}: {len(bad)} of {len(co)} children differ; first: parent {fens[i]!r} move "
                             f"{int(mv[j])}: gpu={co[j]} oracle={ech[j]}")


def _expander(ctx, boards, cap):
    from fishnet_amd import gpu_nnue as G
    n = len(boards)
    bufs = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4),
                                              ("ch", cap * 32), ("mv", cap * 2), ("co", cap * G.EVAL_SIZE))}
    bufs["b"].upload(boards)

    def run(mode, slices=3, chain=81, kc=1, inc=1):
        ctx.set_option(G.OPT_STREAM_SLICES, slices)
        ctx.set_option(G.OPT_CHAIN, chain)
        ctx.set_option(G.OPT_KING_CACHE, kc)
        ctx.set_option(G.OPT_INCREMENTAL_CHILDREN, inc)
        try:
            t = ctx.expand_device(bufs["b"], n, mode, bufs["po"], bufs["off"], bufs["ch"], bufs["mv"], bufs["co"], cap)
        finally:
            ctx.set_option(G.OPT_STREAM_SLICES, 3)
            ctx.set_option(G.OPT_CHAIN, 81)
            ctx.set_option(G.OPT_KING_CACHE, 1)
            ctx.set_option(G.OPT_INCREMENTAL_CHILDREN, 1)
        assert t == cap
        return (bufs["po"].download(G.EVAL_DTYPE, n), bufs["off"].download(np.uint32, n + 1),
                bufs["mv"].download(np.uint16, t), bufs["co"].download(G.EVAL_DTYPE, t))

    def free():
        for b in bufs.values():
            b.free()
    return run, free


@pytest.mark.parametrize("mode", [1, 0])
def test_expansion_3072_every_path(edge_ctx, edge_oracle, oracle_lib, parents, mode):
    """The planned stream in three column slices and whole rows, chained walk + king cache on,
    off and with 5-parent blocks, incremental children and full refreshes: every parent and
    every child equal to the oracle's."""
    boards, fens = parents
    exp = _oracle_expansion(oracle_lib, edge_oracle, fens, mode)
    run, free = _expander(edge_ctx, boards, int(exp[1][-1]))
    try:
        for slices in (3, 1):
            for chain, kc in ((81, 1), (1, 0), (-5, 1)):
                for inc in (1, 0):
                    _cmp_expansion(run(mode, slices, chain, kc, inc), exp, fens,
                                   f"mode {mode} slices {slices} chain {chain} king cache {kc} incremental {inc}")
    finally:
        free()


def test_expansion_3072_stress(oracle_lib, parents):
    boards, fens = parents
    ctx = _ctx((3072, 11, True), None)
    try:
        exp = _oracle_expansion(oracle_lib, _nets(oracle_lib, (3072, 11, True), None), fens, 1)
        run, free = _expander(ctx, boards, int(exp[1][-1]))
        try:
            for slices in (3, 1):
                _cmp_expansion(run(1, slices), exp, fens, f"stress slices {slices}")
        finally:
            free()
    finally:
        ctx.close()


def test_expansion_1024(oracle_lib, parents):
    boards, fens = parents
    ctx = _ctx((1024, 5), None)
    try:
        exp = _oracle_expansion(oracle_lib, _nets(oracle_lib, (1024, 5), None), fens, 1)
        run, free = _expander(ctx, boards, int(exp[1][-1]))
        try:
            for chain, kc in ((81, 1), (1, 0)):
                _cmp_expansion(run(1, 3, chain, kc), exp, fens, f"L1 1024 chain {chain} king cache {kc}")
        finally:
            free()
    finally:
        ctx.close()


def test_expansion_128_small_mode(edge_ctx, edge_oracle, oracle_lib, parents):
    boards, fens = parents
    exp = _oracle_expansion(oracle_lib, edge_oracle, fens, 2)
    run, free = _expander(edge_ctx, boards, int(exp[1][-1]))
    try:
        _cmp_expansion(run(2), exp, fens, "mode SMALL")
    finally:
        free()


def test_expand2_on_edge_net(edge_ctx, edge_oracle, oracle_lib):
    """gn_expand2_device, 3072 edge net, mode BIG, one 40-ply game: level 1 equals
    gn_expand_device; the grandchildren of 60 seeded children equal the oracle's."""
    from fishnet_amd import gpu_nnue as G
    n = 41
    d_b = edge_ctx.alloc(n * 32)
    out, b1 = {}, {}
    try:
        edge_ctx.random_games_device(0x5EED0E02, 0, 1, 40, d_b)
        edge_ctx.synchronize()
        t, g, out = _expand2(edge_ctx, d_b, n, 1)
        assert t > 0 and g > 10 * t
        po, co = out["po"].download(G.EVAL_DTYPE, n), out["co"].download(G.EVAL_DTYPE, t)
        b1 = {k: edge_ctx.alloc(sz) for k, sz in (("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", t * 32),
                                                    ("mv", t * 2), ("co", t * G.EVAL_SIZE))}
        assert edge_ctx.expand_device(d_b, n, 1, b1["po"], b1["off"], b1["ch"], b1["mv"], b1["co"], t) == t
        assert np.array_equal(b1["po"].download(G.EVAL_DTYPE, n), po)
        assert np.array_equal(b1["off"].download(np.uint32, n + 1), out["off"].download(np.uint32, n + 1))
        assert np.array_equal(b1["mv"].download(np.uint16, t), out["mv"].download(np.uint16, t))
        assert np.array_equal(b1["co"].download(G.EVAL_DTYPE, t), co)
        goff = out["goff"].download(np.uint32, t + 1)
        gmv, gco = out["gmv"].download(np.uint16, g), out["gco"].download(G.EVAL_DTYPE, g)
        children = out["ch"].download(G.BOARD_DTYPE, t)
        pick = np.sort(np.random.default_rng(11).choice(t, size=60, replace=False))
        fens = G.boards_to_fens(children[pick])
        exp = _oracle_expansion(oracle_lib, (edge_oracle[0], None), fens, 1)
        for k, j in enumerate(pick):
            lo, hi = int(goff[j]), int(goff[j + 1])
            o = np.argsort(gmv[lo:hi], kind="stable")
            elo, ehi = int(exp[1][k]), int(exp[1][k + 1])
            assert np.array_equal(gmv[lo:hi][o], exp[3][elo:ehi]), fens[k]
            assert np.array_equal(gco[lo:hi][o], exp[2][elo:ehi]), fens[k]
    finally:
        for b in list(b1.values()) + [v for v in out.values() if hasattr(v, "free")] + [d_b]:
            b.free()


# ---- host-facing paths -----------------------------------------------------------------------

def _game_fens(seed, games, plies):
    from fishnet_amd import gpu_nnue as G
    return [G.boards_to_fens(G.replay_game(START, u)[0]) for u in G.random_games_uci(seed, 0, games, plies)]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fast_batch_graphs_on_edge_nets(edge_ctx, edge_oracle, oracle_lib, F, mode):
    """The small-batch graphs (GN_OPT_FAST_BATCH) at their size-class edges, on positions of F and
    of games: equal to the oracle and to the general path."""
    from fishnet_amd import gpu_nnue as G
    pool = F[::3] + [f for g in _game_fens(0x5EED0E03, 48, 80) for f in g]
    pool = pool[:4096]
    assert len(pool) == 4096
    exp = oracle_lib.eval_fens(edge_oracle[0], edge_oracle[1], pool, mode, threads=THREADS)
    try:
        for n in (1, 127, 128, 129, 1000, 4096):
            edge_ctx.set_option(G.OPT_FAST_BATCH, 1)
            fast = edge_ctx.evaluate_batch(pool[:n], mode)
            edge_ctx.set_option(G.OPT_FAST_BATCH, 0)
            slow = edge_ctx.evaluate_batch(pool[:n], mode)
            _cmp(fast, exp[:n], pool[:n])
            _cmp(slow, exp[:n], pool[:n])
    finally:
        edge_ctx.set_option(G.OPT_FAST_BATCH, 1)


@pytest.mark.parametrize("mode", [1, 2])
def test_child_records_with_loud_nets(oracle_lib, mode):
    """Evaluations far from zero (PSQT x 48: |final_cp| in the thousands) through the 12-byte
    gn_child records of gn_evaluate_games and gn_expand_and_evaluate: every decoded child equals
    children_from_evals of the oracle's record."""
    from fishnet_amd import gpu_nnue as G
    loud = ((3072, 1, False, edge_nets.LOUD), (128, 2, False, edge_nets.LOUD))
    ctx = _ctx(*loud)
    try:
        nets = _nets(oracle_lib, *loud)
        ucis = G.random_games_uci(0x5EED0E04, 0, 8, 40)
        res = ctx.evaluate_games([(START, u, ()) for u in ucis], mode, children=True)
        fens = [f for u in ucis for f in G.boards_to_fens(G.replay_game(START, u)[0])]
        par, eoff, ech, emv = _oracle_expansion(oracle_lib, nets, fens, mode)
        ech = G.children_from_evals(ech)
        assert np.abs(par["final_cp"]).max() >= 1000
        i = 0
        for r in res:
            assert r["status"] == 0
            for e, (mv, kids) in zip(r["evals"], r["children"]):
                assert tuple(e) == tuple(par[i]), fens[i]
                o = np.argsort(mv, kind="stable")
                lo, hi = int(eoff[i]), int(eoff[i + 1])
                assert np.array_equal(mv[o], emv[lo:hi]) and np.array_equal(kids[o], ech[lo:hi]), fens[i]
                i += 1
        assert i == len(fens)
        p2, off2, mv2, kids2 = ctx.expand_and_evaluate(fens, mode)
        _cmp(p2, par, fens)
        assert np.array_equal(off2.astype(np.int64), eoff)
        for i in range(len(fens)):
            lo, hi = int(eoff[i]), int(eoff[i + 1])
            o = np.argsort(mv2[lo:hi], kind="stable")
            assert np.array_equal(mv2[lo:hi][o], emv[lo:hi]) and np.array_equal(kids2[lo:hi][o], ech[lo:hi]), fens[i]
    finally:
        ctx.close()


def test_1024_wide_net_in_the_small_slot(oracle_lib, F):
    """A 1024-wide net loaded as the small net: mode FULL selects, evaluates and marks the
    re-evaluations in launches of their own (only the 128-wide kernel does it in one), and the
    small-batch graphs are skipped.  Modes FULL, BIG and SMALL, fast batch on and off."""
    from fishnet_amd import gpu_nnue as G
    ctx = _ctx((3072, 1), (1024, 5))
    try:
        nets = _nets(oracle_lib, (3072, 1), (1024, 5))
        fens = F[::4][:300]
        assert len(fens) == 300
        for mode in (0, 1, 2):
            exp = oracle_lib.eval_fens(nets[0], nets[1], fens, mode, threads=THREADS)
            if mode == 0:
                assert (exp["flags"] & 2).any() and (exp["flags"] & 8).any() and ((exp["flags"] & 10) == 0).any()
            for fast in (1, 0):
                ctx.set_option(G.OPT_FAST_BATCH, fast)
                _cmp(ctx.evaluate_batch(fens, mode), exp, fens)
    finally:
        ctx.close()
