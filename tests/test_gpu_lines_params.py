"""The ranked-lines family on the GPU under non-default gn_eval_params, in every mode and at every
K: rank_children_kernel and rank_lines2_kernel with their history variants, through the four device
calls and the five host calls, against the restated rules (tests/lines_rule.py, lines2_rule.py,
history_rule.py, lines2_history_rule.py), which read the oracle's current parameters.

The sets (tests/lines_param_sets.py) force what the default parameters almost never produce: equal
ordinary values, so that the order rests on the sort keys' lower fields -- the move, the reply and,
in the history variants, the draw bit below them -- and scores that differ from the defaults'
wherever a launch site passed stale or default parameters to rule_score.  tests/test_lines_params.py
measures on the CPU that the sets do so on these inputs.  Everything is compared byte for byte;
whatever runs under a set is computed and compared inside one `with`, and every test ends with a
default run against the default rule.
"""
import numpy as np
import pytest

import history_rule as H
import lines2_history_rule as H2
import lines2_rule as R2
import lines_param_sets as LP
import lines_rule as R

pytestmark = pytest.mark.gpu
KS = tuple(range(1, 9))
MODES = (0, 1, 2)  # FULL, BIG, SMALL
N_HISTORY = len(H.fixture_games())
# results later tests compare with; a test that finds its entry missing (run alone) computes it
_DEVICE2 = {}  # (set, mode) -> (parent records, {K: lines}): gn_expand2_device + gn_rank_lines2_device
_EXPECTED2 = {}  # (set, mode) -> lines2_rule.lines2(..., 8)
_GAMES_HISTORY = {}  # (set, mode) -> (gn_evaluate_games_lines_history's result, ..._lines2_history's), K = 8


def _cmp(got, exp, names, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, what
    for i in np.flatnonzero((got != exp).any(axis=1))[:3]:
        assert got[i].tolist() == exp[i].tolist(), (what, names[i])
    assert np.array_equal(got, exp) and got.tobytes() == exp.tobytes(), what


@pytest.fixture(scope="module")
def depth1():
    from fishnet_amd import gpu_nnue as G
    fens = LP.depth1_fens()
    return fens, G.pack_fens(fens)[0]


@pytest.fixture(scope="module")
def depth2():
    from fishnet_amd import gpu_nnue as G
    fens = LP.depth2_fens()
    return fens, G.pack_fens(fens)[0]


@pytest.fixture(scope="module")
def history(oracle_lib):
    """(games, each game's FENs, every position's label, the skipped positions' flat indices)."""
    games = LP.history_games()
    replayed = [oracle_lib.replay_game(root, moves)[0] for root, moves, _ in games]
    names = [(g, k, f) for g, fens in enumerate(replayed) for k, f in enumerate(fens)]
    skipped = [i for i, (g, k, _) in enumerate(names) if k in games[g][2]]
    return games, replayed, names, skipped


# ---- 1: depth 1, the device call ----------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_rank_children_device_every_set_every_k(gpu_ctx, oracle_lib, oracle_nets, depth1, mode):
    """One gn_expand_device per set, then gn_rank_children_device for K = 1..8 on its resident
    outputs, against the first K of the rule's 8 lines."""
    from test_gpu_history import _Expansion
    fens, boards = depth1
    top = {}
    for name in tuple(LP.LINE_SETS) + ((LP.ALL_SMALL,) if mode == 0 else ()) + (None,):
        with LP.under(oracle_lib, name, gpu_ctx):
            e = _Expansion(gpu_ctx, boards, mode)
            try:
                got = {K: e.rank(K) for K in KS}
            finally:
                e.free()
            exp = R.lines(oracle_lib, *oracle_nets, fens, mode, 8)
            for K in KS:
                _cmp(got[K], exp[:, :K], fens, f"set {name!r} mode {mode} K {K}")
                assert np.array_equal(got[K], got[8][:, :K]), (name, mode, K)  # the exact prefix
        top[name] = got[8]
    c0 = top["clamp0"]  # eight lines of value 0: the move order alone (129 of the 138 positions by the rule)
    assert ((c0["value"][:, 0] == 0) & (c0["value"][:, 7] == 0) & ((c0[:, 7]["flags"] & R.FLAG_NO_SCORE) == 0)).sum() >= 50
    assert (top[None]["value"][:, 0] != 0).sum() >= 100  # the last run was a default one (136 by the rule)


# ---- 2: depth 2, the device call ----------------------------------------------------------------

def _device2(ctx, oracle_lib, oracle_nets, depth2, name, mode):
    """Under the set already: the device path's (parents, {K: lines}) and the rule's 8 lines."""
    from test_gpu_lines2 import _expand2_and_rank
    key = (name, mode)
    if key not in _DEVICE2:
        _DEVICE2[key] = _expand2_and_rank(ctx, depth2[1], mode, KS)
        _EXPECTED2[key] = R2.lines2(oracle_lib, *oracle_nets, depth2[0], mode, 8)
    return _DEVICE2[key], _EXPECTED2[key]


@pytest.mark.parametrize("mode", MODES)
def test_rank_lines2_device_every_set_every_k(gpu_ctx, oracle_lib, oracle_nets, depth2, mode):
    """gn_expand2_device + gn_rank_lines2_device for K = 1..8 against lines2_rule.lines2."""
    fens = depth2[0]
    for name in ("clamp0", "rule50/clamp", "ties-poly", None):
        with LP.under(oracle_lib, name, gpu_ctx):
            (_, got), exp = _device2(gpu_ctx, oracle_lib, oracle_nets, depth2, name, mode)
            for K in KS:
                _cmp(got[K], exp[:, :K], fens, f"set {name!r} mode {mode} K {K}")
    poly, default = _DEVICE2[("ties-poly", mode)][1][8], _DEVICE2[(None, mode)][1][8]
    live = (default["flags"] & (R.FLAG_NO_SCORE | R.FLAG_MATE)) == 0
    assert live.sum() >= 200 and (poly["score"][live] != default["score"][live]).mean() >= 0.9  # the set bites
    assert np.array_equal(poly["move"], default["move"]) and np.array_equal(poly["value"], default["value"])


# ---- 3: the host calls read the current parameters ----------------------------------------------

def test_evaluate_lines2_under_a_set(gpu_ctx, oracle_lib, oracle_nets, depth2):
    """gn_evaluate_lines2 in three chunks (the last one short): the device path's bytes."""
    from fishnet_amd import gpu_nnue as G
    fens = depth2[0]
    assert 2 * 16 < len(fens) < 3 * 16
    try:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 16)
        for name, mode in (("rule50/clamp", 2), ("ties-poly", 0), (None, 2)):
            with LP.under(oracle_lib, name, gpu_ctx):
                (parents, dev), exp = _device2(gpu_ctx, oracle_lib, oracle_nets, depth2, name, mode)
                out, lines = gpu_ctx.evaluate_lines2(fens, 8, mode)
                _cmp(lines, exp, fens, f"set {name!r} mode {mode}: gn_evaluate_lines2 against the rule")
                assert lines.tobytes() == dev[8].tobytes() and out.tobytes() == parents.tobytes(), (name, mode)
    finally:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)


def test_evaluate_games_lines_under_a_set(gpu_ctx, oracle_lib, oracle_nets):
    """gn_evaluate_games_lines over 8 games of 40 plies, K = 8, every position against the rule."""
    from fishnet_amd import gpu_nnue as G
    games = LP.random_games()
    fens = [f for root, uci, _ in games for f in G.boards_to_fens(G.replay_game(root, uci)[0])]
    assert len(fens) == LP.N_GAMES * (LP.GAME_PLIES + 1)
    scores = {}
    for name, mode in (("rule50/clamp", 2), ("ties-poly", 0), (None, 0)):
        with LP.under(oracle_lib, name, gpu_ctx):
            offs, status, pos, lines = gpu_ctx.evaluate_games_lines(games, 8, mode)
            assert not status.any() and int(offs[-1]) == len(fens)
            _cmp(lines, R.lines(oracle_lib, *oracle_nets, fens, mode, 8), fens, f"set {name!r} mode {mode}")
        scores[name] = lines["score"]
    assert (scores["ties-poly"] != scores[None]).mean() >= 0.9  # (both in mode FULL)


# ---- 4: history, the games calls ----------------------------------------------------------------

def _games_history(ctx, games, name, mode):
    """Under the set already: both history games calls at K = 8."""
    key = (name, mode)
    if key not in _GAMES_HISTORY:
        _GAMES_HISTORY[key] = (ctx.evaluate_games_lines_history(games, 8, mode),
                               ctx.evaluate_games_lines2_history(games, 8, mode))
    return _GAMES_HISTORY[key]


@pytest.mark.parametrize("mode", (1, 2))
def test_games_history_calls_under_clamp0(gpu_ctx, oracle_lib, oracle_nets, history, mode):
    """gn_evaluate_games_lines_history and gn_evaluate_games_lines2_history over both fixtures: under
    clamp0 a line drawn by rule ties with every static line, at the child and at the reply."""
    from fishnet_amd import gpu_nnue as G
    games, replayed, names, skipped = history
    big, small = oracle_nets
    assert len(games) == 15 and len(skipped) >= 2
    for name in ("clamp0", None):
        with LP.under(oracle_lib, name, gpu_ctx):
            one, two = _games_history(gpu_ctx, games, name, mode)
            exp1 = np.concatenate([H.game_lines(oracle_lib, big, small, fens, skip, mode, 8)
                                   for fens, (_, _, skip) in zip(replayed, games)])
            exp2 = np.concatenate([H2.game_lines2(oracle_lib, big, small, fens, skip, mode, 8)
                                   for fens, (_, _, skip) in zip(replayed, games)])
            for got, exp, call in ((one, exp1, "gn_evaluate_games_lines_history"),
                                   (two, exp2, "gn_evaluate_games_lines2_history")):
                offs, status, pos, lines = got
                assert not status.any() and [int(o) for o in offs] == [0] + list(np.cumsum([len(f) for f in replayed]))
                _cmp(lines, exp, names, f"set {name!r} mode {mode}: {call}")
                assert (pos[skipped]["flags"] & G.FLAG_SKIPPED).all()
                assert (lines[skipped]["flags"] == G.FLAG_NO_SCORE).all() and not lines[skipped]["move"].any()
            draw = (two[3]["flags"] & G.FLAG_DRAW) != 0
            assert (draw & (two[3]["plies"] == 2)).any() and (draw & (two[3]["plies"] == 1)).any(), (name, mode)
            assert (one[3]["flags"] & G.FLAG_DRAW).any(), (name, mode)
        if name == "clamp0":  # drawn lines next to undrawn static ones of the same value, in either order
            l = one[3]
            pair = (l[:, :-1]["value"] == l[:, 1:]["value"]) & (((l[:, :-1]["flags"] | l[:, 1:]["flags"])
                                                                 & (G.FLAG_NO_MOVES | G.FLAG_NO_SCORE)) == 0)
            first, second = (l[:, :-1]["flags"] & G.FLAG_DRAW) != 0, (l[:, 1:]["flags"] & G.FLAG_DRAW) != 0
            assert (pair & first & ~second).any(axis=1).sum() >= 20 and (pair & ~first & second).any(axis=1).sum() >= 20


# ---- 5: history, the device calls ---------------------------------------------------------------

def test_history_device_calls_under_clamp0(gpu_ctx, oracle_lib, oracle_nets, history):
    """gn_rank_children_history_device and gn_rank_lines2_history_device (the gn_board / uint32_t
    instantiations) on the 144-ply game and on a perpetual check, keys from gn_position_keys_device:
    the games calls' bytes and the rule's, under clamp0, ties-poly and the defaults."""
    from fishnet_amd import gpu_nnue as G
    from test_gpu_history import _Expansion, _device_keys
    from test_gpu_lines2_history import _Expansion2
    games, replayed, names, _ = history
    big, small = oracle_nets
    mode = 1

    def device_lines(game):
        root, moves, skip = games[game]
        assert not skip
        boards = G.replay_game(root, moves)[0]
        n = len(boards)
        entries = [(0, i) for i in range(n)]
        e = _Expansion(gpu_ctx, boards, mode)
        d_k = _device_keys(gpu_ctx, e)
        try:
            one = e.rank(8, d_k, n, entries)
        finally:
            e.free(), d_k.free()
        e2 = _Expansion2(gpu_ctx, boards, mode)
        try:
            two = e2.rank(8, n, entries)
        finally:
            e2.free()
        return one, two

    assert len(replayed[11]) == 145
    scores = {}
    # (ties-poly: these two launch sites' parameters show in the scores, which clamp0 makes all 0)
    for name in ("clamp0", "ties-poly", None):
        with LP.under(oracle_lib, name, gpu_ctx):
            base = _games_history(gpu_ctx, games, name, mode)
            for game in (11, N_HISTORY):
                one, two = device_lines(game)
                a, b = (int(x) for x in base[0][0][game:game + 2])
                label = names[a:b]
                _cmp(one, base[0][3][a:b], label, f"set {name!r}: gn_rank_children_history_device, game {game}")
                _cmp(two, base[1][3][a:b], label, f"set {name!r}: gn_rank_lines2_history_device, game {game}")
                assert (one["flags"] & G.FLAG_DRAW).any() and (two["flags"] & G.FLAG_DRAW).any()
                fens = replayed[game]
                _cmp(one, H.game_lines(oracle_lib, big, small, fens, (), mode, 8), label, f"set {name!r}, game {game}: the rule")
                _cmp(two, H2.game_lines2(oracle_lib, big, small, fens, (), mode, 8), label, f"set {name!r}, game {game}: the rule")
                scores[(name, game)] = (one["score"], two["score"])
    for k in (0, 1):
        poly, default = scores[("ties-poly", 11)][k], scores[(None, 11)][k]
        assert (default != 0).sum() >= 100 and (poly[default != 0] != default[default != 0]).mean() >= 0.9


# ---- 6: restoration -----------------------------------------------------------------------------

def test_defaults_are_back(gpu_ctx, oracle_lib):
    from fishnet_amd import gpu_nnue as G
    assert bytes(gpu_ctx.eval_params()) == bytes(G.default_eval_params()) == bytes(oracle_lib.eval_params())
