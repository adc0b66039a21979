"""The column slices' packed partial sums and the plan's own pinfo markers on the GPU.

The big net is tests/part_pack_nets.py's range net: fc_0 rows of all -128 (buckets 0, 7) and all +127
(buckets 1, 6), and a feature transformer that puts a slice's 1,024 activations at 126 (the
transform's maximum) or at 0 by position, so that single slices store values at both ends of the
24-bit range (tests/test_part_pack.py::test_range_net_drives_single_slices_to_both_ends shows that on
the oracle).  Parents: one whole 81-ply device game (chained parents, PINFO_ALIAS; king-move
children; tiles of two buckets as captures come) and the hand-picked positions whose children cross
a layer-stack bucket.  Every record is compared with the oracle and between the paths.
"""
import numpy as np
import pytest

import part_pack_nets as N
import plan_snapshot
from plan_replay import PINFO_ALIAS
from test_gpu_edge_nets import _cmp_expansion, _expander, _oracle_expansion

pytestmark = pytest.mark.gpu

MODE_FULL, MODE_BIG = 0, 1
# (GN_OPT_STREAM_SLICES, GN_OPT_CHAIN, GN_OPT_KING_CACHE): sliced and whole-row, chain and king cache
# on and the plain path
PATHS = ((3, 81, 1), (1, 81, 1), (3, 1, 0), (1, 1, 0))
BAD = 40  # the parent the fill test zeroes (inside the game: the chain breaks there)


@pytest.fixture(scope="module")
def world(oracle_lib, synth_small_path):
    from fishnet_amd import build, gpu_nnue as G
    build.build()
    path = N.range_net()
    ctx = G.GpuNnue(path, synth_small_path)
    d = ctx.alloc(81 * 32)
    ctx.random_games_device(0x5EED0E24, 0, 1, 80, d)
    ctx.synchronize()
    game = d.download(G.BOARD_DTYPE, 81)
    d.free()
    fens = G.boards_to_fens(game) + [oracle_lib.normalize_fen(f) for f in N.PICKED]
    boards, ok = G.pack_fens(fens)
    assert ok.all()
    nets = (oracle_lib.Net(path), oracle_lib.Net(synth_small_path))
    exp = {}

    def oracle(mode):
        if mode not in exp:
            exp[mode] = _oracle_expansion(oracle_lib, nets, fens, mode)
        return exp[mode]
    yield ctx, boards, fens, oracle
    ctx.close()


@pytest.mark.parametrize("mode", [MODE_BIG, MODE_FULL])
def test_packed_sums_equal_whole_rows_plain_path_and_oracle(world, mode):
    ctx, boards, fens, oracle = world
    exp = oracle(mode)
    run, free = _expander(ctx, boards, int(exp[1][-1]))
    try:
        got = {}
        for slices, chain, kc in PATHS:
            got[(slices, chain, kc)] = g = run(mode, slices, chain, kc)
            _cmp_expansion(g, exp, fens, f"mode {mode} slices {slices} chain {chain} king cache {kc}")
        first = got[PATHS[0]]
        for p in PATHS[1:]:
            for name, a, b in zip(("parents", "offsets", "moves", "children"), first, got[p]):
                assert a.tobytes() == b.tobytes(), (mode, p, name)
    finally:
        free()
    if mode == MODE_FULL:  # both nets were taken: the masks leave slots unevaluated
        small = (exp[2]["flags"] & 2) != 0
        assert small.any() and not small.all()


def _check_pinfo(G, ctx, run, oracle, perm):
    """One FULL expansion of the parents base[perm] with parent BAD zeroed: the records equal the
    oracle's, and pinfo.y >= 0 exactly at the positions the big net evaluates."""
    par, eoff, ech, emv = oracle(MODE_FULL)
    po, off, mv, co = run(MODE_FULL)
    snap = plan_snapshot.take(G, ctx)
    n, t = len(perm), len(co)
    assert snap.hdr["slices"] == 3 and snap.hdr["np"] == n and snap.hdr["npos"] == n + t == len(snap.pinfo)
    ev = np.zeros(n + t, bool)
    aliased = 0
    for i, src in enumerate(perm):
        lo, hi = int(off[i]), int(off[i + 1])
        if i == BAD:
            assert lo == hi and po[i]["flags"] & G.FLAG_BAD_FEN
            continue
        elo, ehi = int(eoff[src]), int(eoff[src + 1])
        o = np.argsort(mv[lo:hi], kind="stable")
        assert tuple(po[i]) == tuple(par[src]), i
        assert np.array_equal(mv[lo:hi][o], emv[elo:ehi]) and np.array_equal(co[lo:hi][o], ech[elo:ehi]), i
        ev[i] = (par[src]["flags"] & 2) == 0
        ev[n + lo + o] = (ech[elo:ehi]["flags"] & 2) == 0
        aliased += bool(snap.pinfo[i, 1] >= 0 and snap.pinfo[i, 1] & PINFO_ALIAS)
    y = snap.pinfo[:, 1]
    wrong = np.flatnonzero((y >= 0) != ev)
    assert len(wrong) == 0, (len(wrong), int(wrong[0]), int(y[wrong[0]]), bool(ev[wrong[0]]))
    assert ev.any() and not ev[:n].all() and not ev[n:].all()
    return ev, aliased


def test_plan_marks_unevaluated_slots_without_a_fill(world):
    """pinfo is not filled before the plan: plan_kernel writes (0, -1) for every slot it does not
    evaluate.  Mode BIG first (every pinfo.y >= 0 but the invalid parent's), then mode FULL twice in
    the same buffers with different masks (the parents rotated by 29): after each run pinfo.y < 0
    exactly at the positions the small net alone evaluates and at the invalid parent -- nothing of
    the run before shows through."""
    from fishnet_amd import gpu_nnue as G
    ctx, boards, fens, oracle = world
    n = len(boards)
    par, eoff, _, _ = oracle(MODE_FULL)
    cnt = np.diff(eoff)
    ctx.set_option(G.OPT_EXPAND_PIPELINE, 0)
    try:
        evs = []
        for k, shift in enumerate((0, 0, 29)):
            perm = np.roll(np.arange(n), shift)
            b = boards[perm].copy()
            b[BAD] = np.zeros(1, dtype=G.BOARD_DTYPE)
            run, free = _expander(ctx, b, int(cnt.sum() - cnt[perm[BAD]]))
            try:
                if k == 0:
                    run(MODE_BIG)
                    y = plan_snapshot.take(G, ctx).pinfo[:, 1]
                    assert np.flatnonzero(y < 0).tolist() == [BAD]
                    continue
                ev, aliased = _check_pinfo(G, ctx, run, oracle, perm)
                assert aliased > 0  # chained parents of the game
                evs.append(ev)
            finally:
                free()
        assert len(evs[0]) != len(evs[1]) or (evs[0] != evs[1]).any()  # the masks differed
    finally:
        ctx.set_option(G.OPT_EXPAND_PIPELINE, 2)
