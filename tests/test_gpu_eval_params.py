"""Every gn_eval_params field on the GPU against the parameterised oracle (tests/eval_param_sets.py:
the sets, the input list; tests/test_eval_params.py pins that oracle on the CPU).  Every device
path that reads the parameters runs under non-default values: the fused 128-wide selection,
classify / reeval as launches of their own, finalize (with the sliced stream's branch), the score
rule's to_cp, the captured small-batch graphs.  Everything is compared integer for integer; each
test restores the defaults on both sides and ends with a default run against the default oracle.
"""
import contextlib

import numpy as np
import pytest

import edge_nets
import eval_param_sets as S
from test_gpu_edge_nets import _cmp_expansion, _expander, _oracle_expansion
from test_gpu_parity import _cmp, special_fens

pytestmark = pytest.mark.gpu

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
NAMED = list(S.NAMED)
EXPANSION_SETS = ("weights", "small-vs-big", "material", "rule50/clamp") + S.EXTREMES


@pytest.fixture(scope="module")
def fens():
    return S.input_fens()


@pytest.fixture(scope="module")
def sets(oracle_lib):
    return dict(S.all_sets(oracle_lib))


@contextlib.contextmanager
def _params(ctx, oracle_lib, p):
    """Both sides under p; both back at their defaults afterwards."""
    from fishnet_amd import gpu_nnue as G
    try:
        ctx.set_eval_params(S.as_gpu(p))
        oracle_lib.set_eval_params(p)
        yield
    finally:
        oracle_lib.set_eval_params(None)
        ctx.set_eval_params(G.default_eval_params())


def _defaults_again(ctx, oracle_lib, nets, fens, mode=0):
    from fishnet_amd import gpu_nnue as G
    assert bytes(ctx.eval_params()) == bytes(G.default_eval_params()) == bytes(oracle_lib.eval_params())
    _cmp(ctx.evaluate_batch(fens, mode), S.oracle_records(oracle_lib, nets, fens, None, mode), fens)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_batch_every_set(gpu_ctx, oracle_nets, oracle_lib, fens, sets, mode):
    """gn_evaluate_batch over the input list under every named set and every single-field set, as a
    captured graph and on the general path.  The single-field runs alternate with default runs, so
    a graph that survived gn_set_eval_params in either direction would show."""
    from fishnet_amd import gpu_nnue as G
    default = G.default_eval_params()
    order = [(n, sets[n]) for n in NAMED]
    for k in S.SINGLE:
        order += [(S.single_name(k), sets[S.single_name(k)]), ("defaults", None)]
    try:
        for fast in (1, 0):
            gpu_ctx.set_option(G.OPT_FAST_BATCH, fast)
            for name, p in order:
                gpu_ctx.set_eval_params(default if p is None else S.as_gpu(p))
                f0 = gpu_ctx.get_option(G.STAT_FAST_BATCHES)
                got = gpu_ctx.evaluate_batch(fens, mode)
                assert gpu_ctx.get_option(G.STAT_FAST_BATCHES) - f0 == fast, (name, fast)
                try:
                    _cmp(got, S.oracle_records(oracle_lib, oracle_nets, fens, p, mode), fens)
                except AssertionError as e:
                    raise AssertionError(f"set {name!r} mode {mode} fast batch {fast}: {e}") from None
    finally:
        gpu_ctx.set_option(G.OPT_FAST_BATCH, 1)
        gpu_ctx.set_eval_params(default)
        oracle_lib.set_eval_params(None)
    _defaults_again(gpu_ctx, oracle_lib, oracle_nets, fens, mode)


def test_evaluate_device_4099(gpu_ctx, oracle_nets, oracle_lib, fens, sets):
    """gn_evaluate_device at 4,099 boards (the king sort, eval_net_kernel<128>'s multi-position tiles
    with the fused selection), mode FULL, the named sets: the input list padded with device games."""
    from fishnet_amd import gpu_nnue as G
    n, plies = 4099, 80
    games = -(-(n - len(fens)) // (plies + 1))
    d = gpu_ctx.alloc(games * (plies + 1) * 32)
    gpu_ctx.random_games_device(0x5EED0E51, 0, games, plies, d)
    gpu_ctx.synchronize()
    g = d.download(G.BOARD_DTYPE, games * (plies + 1))[:n - len(fens)]
    d.free()
    fb, ok = G.pack_fens(fens)
    assert ok.all()
    boards = np.concatenate([fb, g])
    all_fens = fens + G.boards_to_fens(g)
    assert len(boards) == n == len(all_fens)
    d_b, d_o = gpu_ctx.alloc(n * 32), gpu_ctx.alloc(n * G.EVAL_SIZE)
    d_b.upload(boards)
    try:
        for name in NAMED:
            with _params(gpu_ctx, oracle_lib, sets[name]):
                exp = oracle_lib.eval_fens(*oracle_nets, all_fens, 0, threads=S.THREADS)
                gpu_ctx.evaluate_device(d_b, n, 0, d_o)
                try:
                    _cmp(d_o.download(G.EVAL_DTYPE, n), exp, all_fens)
                except AssertionError as e:
                    raise AssertionError(f"set {name!r}: {e}") from None
        gpu_ctx.evaluate_device(d_b, n, 0, d_o)
        _cmp(d_o.download(G.EVAL_DTYPE, n), oracle_lib.eval_fens(*oracle_nets, all_fens, 0, threads=S.THREADS), all_fens)
    finally:
        d_b.free()
        d_o.free()
    _defaults_again(gpu_ctx, oracle_lib, oracle_nets, fens)


def test_1024_wide_small_slot(oracle_lib, fens, sets):
    """A 1024-wide net in the small slot: mode FULL's selection and re-evaluation marks run as
    classify_kernel and reeval_kernel launches of their own.  300 positions; weights, small-vs-big
    and the extremes."""
    from fishnet_amd import build, gpu_nnue as G
    build.build()
    big_p, small_p = edge_nets.edge_net(3072, 1), edge_nets.edge_net(1024, 5)
    ctx = G.GpuNnue(big_p, small_p)
    try:
        nets = (oracle_lib.Net(big_p), oracle_lib.Net(small_p))
        sub = (fens[::2] + fens[1::2])[:300]
        assert len(sub) == 300
        d0 = oracle_lib.eval_fens(*nets, sub, 0, threads=S.THREADS)
        assert (d0["flags"] & 2).any() and (d0["flags"] & 8).any() and ((d0["flags"] & 10) == 0).any()
        for name in ("weights", "small-vs-big") + S.EXTREMES:
            with _params(ctx, oracle_lib, sets[name]):
                exp = {m: oracle_lib.eval_fens(*nets, sub, m, threads=S.THREADS) for m in (0, 1, 2)}
                if name == "small-vs-big":
                    assert ((exp[0]["flags"] & 8) != 0).sum() >= 10
                for fast in (1, 0):
                    ctx.set_option(G.OPT_FAST_BATCH, fast)
                    for m in (0, 1, 2):
                        try:
                            _cmp(ctx.evaluate_batch(sub, m), exp[m], sub)
                        except AssertionError as e:
                            raise AssertionError(f"set {name!r} mode {m} fast batch {fast}: {e}") from None
        ctx.set_option(G.OPT_FAST_BATCH, 1)
        assert bytes(ctx.eval_params()) == bytes(G.default_eval_params()) == bytes(oracle_lib.eval_params())
        _cmp(ctx.evaluate_batch(sub, 0), d0, sub)
    finally:
        oracle_lib.set_eval_params(None)
        ctx.close()


@pytest.fixture(scope="module")
def parents(gpu_ctx):
    """147 parents: two device games of 40 plies, the special positions, 30 score-fixture positions."""
    from fishnet_amd import gpu_nnue as G
    d = gpu_ctx.alloc(2 * 41 * 32)
    gpu_ctx.random_games_device(0x5EED0E52, 0, 2, 40, d)
    gpu_ctx.synchronize()
    g = d.download(G.BOARD_DTYPE, 2 * 41)
    d.free()
    pf = G.boards_to_fens(g) + special_fens() + S.score_fixture_fens()[::2][:30]
    boards, ok = G.pack_fens(pf)
    assert ok.all() and len(pf) <= 150
    return boards, pf


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_expand_device(gpu_ctx, oracle_nets, oracle_lib, parents, sets, mode):
    """gn_expand_device (classify / reeval launches, the planned big net, finalize and, in mode
    BIG with three stream slices, its branch that rebuilds the outputs from the slices' partial sums),
    incremental children and full refreshes.  Under the extremes the big net's stream evaluates no
    slot (all small) or every slot of mode FULL."""
    boards, pf = parents
    exp0 = _oracle_expansion(oracle_lib, oracle_nets, pf, mode)
    run, free = _expander(gpu_ctx, boards, int(exp0[1][-1]))
    settings = [(3, 1), (3, 0)] + ([(1, 1), (1, 0)] if mode == 1 else [])
    try:
        for name in EXPANSION_SETS:
            with _params(gpu_ctx, oracle_lib, sets[name]):
                exp = _oracle_expansion(oracle_lib, oracle_nets, pf, mode)
                if name == "all small" and mode == 0:
                    assert (exp[0]["flags"] & 2).all() and (exp[2]["flags"] & 2).all()
                if name in ("never small", "always re-evaluated") and mode == 0:
                    assert not (exp[0]["flags"] & 2).any() and not (exp[2]["flags"] & 2).any()
                for slices, inc in settings:
                    _cmp_expansion(run(mode, slices=slices, inc=inc), exp, pf,
                                   f"set {name!r} mode {mode} slices {slices} incremental {inc}")
        _cmp_expansion(run(mode), exp0, pf, f"defaults again, mode {mode}")
    finally:
        free()
    _defaults_again(gpu_ctx, oracle_lib, oracle_nets, pf, mode)


def test_games_and_child_records(gpu_ctx, oracle_nets, oracle_lib, sets):
    """gn_evaluate_games with children and gn_expand_and_evaluate under the ties sets and
    rule50/clamp, 4 games of 40 plies: the decoded 12-byte gn_child records equal children_from_evals
    of the oracle's, the scored parents equal the oracle's."""
    from fishnet_amd import gpu_nnue as G
    ucis = G.random_games_uci(0x5EED0E53, 0, 4, 40)
    gf = [f for u in ucis for f in G.boards_to_fens(G.replay_game(START, u)[0])]

    def check(mode, what):
        par, eoff, ech, emv = _oracle_expansion(oracle_lib, oracle_nets, gf, mode)
        ech = G.children_from_evals(ech)
        res = gpu_ctx.evaluate_games([(START, u, ()) for u in ucis], mode, children=True)
        i = 0
        for r in res:
            assert r["status"] == 0
            for e, (mv, kids) in zip(r["evals"], r["children"]):
                assert tuple(e) == tuple(par[i]), (what, gf[i])
                o = np.argsort(mv, kind="stable")
                lo, hi = int(eoff[i]), int(eoff[i + 1])
                assert np.array_equal(mv[o], emv[lo:hi]) and np.array_equal(kids[o], ech[lo:hi]), (what, gf[i])
                i += 1
        assert i == len(gf)
        p2, off2, mv2, kids2 = gpu_ctx.expand_and_evaluate(gf, mode)
        _cmp(p2, par, gf)
        assert np.array_equal(off2.astype(np.int64), eoff), what
        for i in range(len(gf)):
            lo, hi = int(eoff[i]), int(eoff[i + 1])
            o = np.argsort(mv2[lo:hi], kind="stable")
            assert np.array_equal(mv2[lo:hi][o], emv[lo:hi]) and np.array_equal(kids2[lo:hi][o], ech[lo:hi]), (what, gf[i])

    for name in S.TIES + ("rule50/clamp",):
        with _params(gpu_ctx, oracle_lib, sets[name]):
            for mode in (0, 1):
                check(mode, f"set {name!r} mode {mode}")
    check(0, "defaults again")
    _defaults_again(gpu_ctx, oracle_lib, oracle_nets, gf)


def test_score_fixture_as_positions(gpu_ctx, oracle_nets, oracle_lib, sets):
    """The score fixture under the ties sets and material: score, GN_FLAG_MATE, GN_FLAG_SEARCHED and
    best_move (rule_score's to_cp with the searched position's material) equal the parameterised
    oracle's, and the mate distances are those of the defaults."""
    from fishnet_amd import gpu_nnue as G
    sf = S.score_fixture_fens()
    for mode in (0, 1, 2):
        d = S.oracle_records(oracle_lib, oracle_nets, sf, None, mode)
        mate = (d["flags"] & G.FLAG_MATE) != 0
        searched = (d["flags"] & G.FLAG_SEARCHED) != 0
        assert mate.sum() >= 20 and (searched & ~mate).sum() >= 20
        for name in S.TIES + ("material",):
            exp = S.oracle_records(oracle_lib, oracle_nets, sf, sets[name], mode)
            with _params(gpu_ctx, oracle_lib, sets[name]):
                got = gpu_ctx.evaluate_batch(sf, mode)
                par = gpu_ctx.expand_and_evaluate(sf, mode)[0]
            for rec in (got, par):
                try:
                    _cmp(rec, exp, sf)
                except AssertionError as e:
                    raise AssertionError(f"set {name!r} mode {mode}: {e}") from None
                assert np.array_equal((rec["flags"] & G.FLAG_MATE) != 0, mate)
                assert np.array_equal(rec["score"][mate], d["score"][mate])
                assert np.array_equal(rec["flags"] & (G.FLAG_SEARCHED | G.FLAG_NO_MOVES | G.FLAG_IN_CHECK),
                                      d["flags"] & (G.FLAG_SEARCHED | G.FLAG_NO_MOVES | G.FLAG_IN_CHECK))
            assert (got["score"][searched & ~mate] != d["score"][searched & ~mate]).any(), name  # (the set bites)
    _defaults_again(gpu_ctx, oracle_lib, oracle_nets, sf)
