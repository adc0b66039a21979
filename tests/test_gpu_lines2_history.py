"""Two-ply ranked lines from games, with game-history draws (include/gpu_nnue.h at gn_line2), on the
GPU against the rule restated from the CPU oracle (tests/lines2_history_rule.py):
gn_evaluate_games_lines2, gn_evaluate_games_lines2_history and gn_rank_lines2_history_device over
the fixtures tests/golden/history_games.txt and tests/golden/lines2_history_games.txt and 16 random
40-ply games."""
import numpy as np
import pytest

import history_rule as H
import lines2_history_rule as H2
import lines2_rule as R2
import lines_rule as R

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
MODES = (0, 1)  # FULL, BIG
K_GAMES = 3
N_HISTORY = len(H.fixture_games())  # the perpetual checks follow history_games.txt's games


@pytest.fixture(scope="module")
def fixture_games():
    return H2.both_fixtures()


@pytest.fixture(scope="module")
def replayed(oracle_lib, fixture_games):
    return [oracle_lib.replay_game(root, moves)[0] for root, moves, _ in fixture_games]


@pytest.fixture(scope="module")
def expected(oracle_lib, oracle_nets, fixture_games, replayed):
    """{mode: lines[positions, 8]} of the fixtures by the restated rule (K < 8 is its prefix)."""
    big, small = oracle_nets
    return {mode: np.concatenate([H2.game_lines2(oracle_lib, big, small, fens, skip, mode, 8)
                                  for fens, (_, _, skip) in zip(replayed, fixture_games)]) for mode in MODES}


@pytest.fixture(scope="module")
def got(gpu_ctx, fixture_games):
    return {(mode, K): gpu_ctx.evaluate_games_lines2_history(fixture_games, K, mode) for mode in MODES for K in KS}


@pytest.fixture(scope="module")
def random_games():
    from fishnet_amd import gpu_nnue as G
    ucis = G.random_games_uci(0x5EED11E6, 0, 16, 40)
    out = [(R.START, u, (2, 30) if g % 5 == 0 else ()) for g, u in enumerate(ucis)]
    out[7] = (R.START, "e2e4 e7e5 e1e3 g8f6", ())  # an illegal move
    out[11] = ("not a fen", "e2e4", ())             # a bad root
    out[13] = (R.fixture_fens()[0], "", (0,))       # its only position skipped
    return out


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1: the rule --------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
def test_games_lines2_history_vs_rule(got, expected, replayed, mode, K):
    offs, status, pos, lines = got[(mode, K)]
    exp = expected[mode][:, :K]
    assert not status.any() and lines.shape == exp.shape and lines.dtype == exp.dtype
    assert [int(o) for o in offs] == [0] + list(np.cumsum([len(f) for f in replayed]))
    for i in np.flatnonzero((lines != exp).any(axis=1))[:5]:
        g = int(np.searchsorted(offs, i, side="right")) - 1
        assert lines[i].tolist() == exp[i].tolist(), (g, i - int(offs[g]), replayed[g][i - int(offs[g])], mode, K)
    assert np.array_equal(lines, exp)


def test_perpetual_check_position_6(oracle_lib, got, replayed):
    """What separates this rule from both existing ones, as the GPU returns it."""
    from fishnet_amd import gpu_nnue as G
    offs, _, _, lines = got[(0, 8)]
    for g in range(N_HISTORY, N_HISTORY + 3):
        assert not H.drawn_moves(oracle_lib, replayed[g], 6)
        ls = lines[int(offs[g]) + 6]
        deep = ls[((ls["flags"] & G.FLAG_DRAW) != 0) & (ls["plies"] == 2)]
        assert len(deep) >= 1 and (deep["value"] == 0).all() and (deep["reply"] != 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_prefix_property(got, mode):
    assert np.array_equal(got[(mode, 8)][3][:, :3], got[(mode, 3)][3])
    assert np.array_equal(got[(mode, 8)][3][:, :1], got[(mode, 1)][3])


# ---- 2: the plain games form --------------------------------------------------------------------

@pytest.fixture(scope="module")
def plain_random(gpu_ctx, random_games):
    return gpu_ctx.evaluate_games_lines2(random_games, K_GAMES, 0)


def test_plain_games_form(gpu_ctx, random_games, plain_random):
    from fishnet_amd import gpu_nnue as G
    offs, status, pos, lines = plain_random
    arr, _keep = G._games_array(random_games)
    ref = gpu_ctx.evaluate_games_arrays(arr, len(random_games), 0, children=False)
    assert _same((offs, status, pos), ref[:3])
    assert status[7] == G.E_ILLEGAL_MOVE and status[11] == G.E_INVALID and offs[8] == offs[7] and offs[12] == offs[11]
    assert int(offs[14] - offs[13]) == 1 and pos[int(offs[13])]["flags"] & G.FLAG_SKIPPED
    fens, skipped = [], []
    for g, (root, uci, skip) in enumerate(random_games):
        if status[g]:
            continue
        boards = G.replay_game(root, uci)[0]
        assert len(boards) == int(offs[g + 1] - offs[g])
        fens += G.boards_to_fens(boards)
        skipped += [p in skip for p in range(len(boards))]
    skipped = np.array(skipped)
    assert len(fens) == len(pos) and 500 <= len(fens) <= 700 and 5 <= skipped.sum() <= 16
    _, want = gpu_ctx.evaluate_lines2(fens, K_GAMES, 0)
    want[skipped] = np.array([R2.EMPTY2], dtype=G.LINE2_DTYPE)[0]
    for i in np.flatnonzero((lines != want).any(axis=1))[:5]:
        assert lines[i].tolist() == want[i].tolist(), fens[i]
    assert lines.tobytes() == want.tobytes()
    assert not (lines["flags"] & G.FLAG_DRAW).any()


# ---- 3: neutrality ------------------------------------------------------------------------------

def test_neutral_where_nothing_is_drawn(gpu_ctx, oracle_lib, oracle_nets, fixture_games, replayed, random_games,
                                        plain_random, got):
    from fishnet_amd import gpu_nnue as G
    O = oracle_lib
    big, small = oracle_nets
    before = plain_random
    hist = gpu_ctx.evaluate_games_lines2_history(random_games, K_GAMES, 0)
    after = gpu_ctx.evaluate_games_lines2(random_games, K_GAMES, 0)
    assert _same(before, after)  # the plain call: the same bytes before and after a history call
    assert _same(before[:3], hist[:3])  # offsets, status, records
    offs, status, _, plain = before
    checked = differ = 0
    for g, (root, uci, skip) in enumerate(random_games):
        if status[g]:
            continue
        fens = None
        for p in range(int(offs[g + 1] - offs[g])):
            at = int(offs[g]) + p
            if at % 5:
                continue
            fens = fens or O.replay_game(root, uci)[0]
            if p in skip or H2.draws_nothing(O, big, small, fens, p, 0):
                assert hist[3][at].tobytes() == plain[at].tobytes(), (g, p, fens[p])
                checked += 1
            else:
                differ += 1
    assert checked >= 100 and differ <= checked // 10
    # the fixtures: records and offsets equal, and the lines wherever the rule draws nothing
    fplain = gpu_ctx.evaluate_games_lines2(fixture_games, 8, 0)
    fhist = got[(0, 8)]
    assert _same(fplain[:3], fhist[:3])
    quiet = drawn = 0
    for g, (fens, (_, _, skip)) in enumerate(zip(replayed, fixture_games)):
        for p in range(len(fens)):
            at = int(fplain[0][g]) + p
            if p in skip or H2.draws_nothing(O, big, small, fens, p, 0):
                assert fhist[3][at].tobytes() == fplain[3][at].tobytes(), (g, p)
                quiet += 1
            else:
                drawn += 1
    assert quiet >= 10 and drawn >= 30
    assert not (fplain[3]["flags"] & G.FLAG_DRAW).any() and not (plain["flags"] & G.FLAG_DRAW).any()


# ---- 4: the same bytes from every path ----------------------------------------------------------

def test_same_bytes_chunked_two_slots_in_place_and_gathered(gpu_ctx, got, fixture_games, synth_big_path,
                                                            synth_small_path):
    from fishnet_amd import gpu_nnue as G
    base = got[(0, K_GAMES)]
    plain = gpu_ctx.evaluate_games_lines2(fixture_games, K_GAMES, 0)
    assert gpu_ctx.get_option(G.STAT_RANK2_NS) > 0 and gpu_ctx.get_option(G.STAT_KEYS_NS) == 0
    assert gpu_ctx.get_option(G.STAT_RANK_NS) == 0
    again = gpu_ctx.evaluate_games_lines2_history(fixture_games, K_GAMES, 0)
    assert _same(base, again)
    assert gpu_ctx.get_option(G.STAT_RANK2_NS) > 0 and gpu_ctx.get_option(G.STAT_KEYS_NS) > 0
    try:  # chunks of exactly 16 parents: they cut inside games (the longest has 129 positions)
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 16)
        chunked = gpu_ctx.evaluate_games_lines2_history(fixture_games, K_GAMES, 0)
        pchunked = gpu_ctx.evaluate_games_lines2(fixture_games, K_GAMES, 0)
    finally:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    assert len(base[2]) >= 10 * 16 and _same(base, chunked) and _same(plain, pchunked)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        sharded = two.evaluate_games_lines2_history(fixture_games, K_GAMES, 0)
        assert two.get_option(G.STAT_KEYS_NS) > 0
        psharded = two.evaluate_games_lines2(fixture_games, K_GAMES, 0)
    finally:
        two.close()
    assert _same(base, sharded) and _same(plain, psharded)
    # without the skip game every shard runs in place; with it the shard is gathered
    skip_games = [g for g, (_, _, skip) in enumerate(fixture_games) if skip]
    assert len(skip_games) == 1
    s = skip_games[0]
    rest = fixture_games[:s] + fixture_games[s + 1:]
    for call, (offs, _, pos, lines) in ((gpu_ctx.evaluate_games_lines2_history, base),
                                        (gpu_ctx.evaluate_games_lines2, plain)):
        o2, s2, p2, l2 = call(rest, K_GAMES, 0)
        a, b = int(offs[s]), int(offs[s + 1])
        assert not s2.any()
        assert p2.tobytes() == np.concatenate([pos[:a], pos[b:]]).tobytes()
        assert l2.tobytes() == np.concatenate([lines[:a], lines[b:]]).tobytes()


# ---- 5: the device call -------------------------------------------------------------------------

class _Expansion2:
    """gn_expand2_device of boards and their keys, kept on the device for the ranking calls."""

    def __init__(self, ctx, boards, mode):
        from test_gpu_parity import _expand2
        self.ctx, self.n = ctx, len(boards)
        n = self.n
        self.d_b, self.d_ln, self.d_hist, self.d_k = ctx.alloc(n * 32), ctx.alloc(n * 8 * 16), ctx.alloc(n * 8), ctx.alloc(n * 8)
        self.d_b.upload(boards)
        _, _, self.out = _expand2(ctx, self.d_b, n, mode)
        ctx.position_keys_device(self.d_b, n, self.d_k)

    def rank(self, K, n_keys=0, hist=None):
        from fishnet_amd import gpu_nnue as G
        if hist is None:
            self.ctx.rank_lines2_device(self.d_b, self.n, self.out, K, self.d_ln)
        else:
            self.d_hist.upload(np.asarray(hist, dtype=G.HISTORY_DTYPE))
            self.ctx.rank_lines2_history_device(self.d_b, self.n, self.out, self.d_k, n_keys, self.d_hist, K, self.d_ln)
        self.ctx.synchronize()
        return self.d_ln.download(G.LINE2_DTYPE, self.n * K).reshape(self.n, K)

    def free(self):
        for x in list(self.out.values()) + [self.d_b, self.d_ln, self.d_hist, self.d_k]:
            if hasattr(x, "free"):
                x.free()


@pytest.mark.parametrize("game", (N_HISTORY, 11))
def test_device_call_equals_the_games_call(gpu_ctx, got, fixture_games, game):
    from fishnet_amd import gpu_nnue as G
    root, moves, skip = fixture_games[game]
    assert not skip
    boards = G.replay_game(root, moves)[0]
    n = len(boards)
    exp = _Expansion2(gpu_ctx, boards, 0)
    lines = exp.rank(8, n, [(0, i) for i in range(n)])
    exp.free()
    offs, _, _, want = got[(0, 8)]
    want = want[int(offs[game]):int(offs[game + 1])]
    draw = (want["flags"] & G.FLAG_DRAW) != 0
    assert (draw & (want["plies"] == 1)).any() and (draw & (want["plies"] == 2)).any()
    assert lines.tobytes() == want.tobytes()


def test_no_history_and_the_bound(gpu_ctx, oracle_lib, oracle_nets, fixture_games, replayed):
    """Every entry first > self: the plain ranking wherever the parent's rule50 < 98, the fifty-move
    rule at both levels elsewhere.  An entry with self >= n_keys is no history either, although the
    keys that would make a draw lie in the allocation beyond n_keys."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    boards = np.concatenate([G.replay_game(root, moves)[0] for root, moves, _ in fixture_games])
    fens = [f for game in replayed for f in game]
    n = len(boards)
    exp = _Expansion2(gpu_ctx, boards, 0)
    plain = exp.rank(8)
    none = exp.rank(8, n, [(1, 0)] * n)
    r50 = boards["rule50"]
    assert (r50 < 98).sum() >= 100 and (r50 >= 98).sum() >= 30
    assert none[r50 < 98].tobytes() == plain[r50 < 98].tobytes()
    for i in np.flatnonzero(r50 >= 98):
        want = H2.game_lines2(oracle_lib, big, small, [fens[i]], (), 0, 8)[0]  # a game of one position: no history
        assert none[i].tolist() == want.tolist(), fens[i]
    draw = (none["flags"] & G.FLAG_DRAW) != 0
    assert (draw & (none["plies"] == 1)).any() and (draw & (none["plies"] == 2)).any()
    # the bound: the first perpetual's parents with their true entries (first, self), but only its
    # first 4 keys declared: parents 0..3 have their history, parents 4.. (self >= n_keys) none
    a = sum(len(f) for f in replayed[:N_HISTORY])
    m = len(replayed[N_HISTORY])
    entries = [(a, i) if a <= i < a + m else (1, 0) for i in range(n)]
    full = exp.rank(8, n, entries)
    fdraw = (full[a:a + m]["flags"] & G.FLAG_DRAW) != 0  # (with every key declared: threefolds at both levels)
    assert (fdraw & (full[a:a + m]["plies"] == 1)).any() and (fdraw & (full[a:a + m]["plies"] == 2)).any()
    clamp = exp.rank(8, a + 4, entries)
    assert clamp[a + 4:a + m].tobytes() == none[a + 4:a + m].tobytes()
    assert clamp[a:a + 4].tobytes() == full[a:a + 4].tobytes()
    assert not (clamp[a:a + m]["flags"] & G.FLAG_DRAW).any()
    exp.free()


# ---- 6: arguments -------------------------------------------------------------------------------

def test_argument_checks(gpu_ctx, got, fixture_games):
    from fishnet_amd import gpu_nnue as G
    d = gpu_ctx.alloc(4096)
    bufs = {k: d for k in ("off", "ch", "co", "mv", "goff", "gmv", "gco")}
    for k in (0, 9):
        for call in (gpu_ctx.evaluate_games_lines2, gpu_ctx.evaluate_games_lines2_history):
            with pytest.raises(G.GnError) as e:
                call(fixture_games[:2], k, 0)
            assert e.value.code == G.E_INVALID
        with pytest.raises(G.GnError) as e:
            gpu_ctx.rank_lines2_history_device(d, 1, bufs, d, 1, d, k, d)
        assert e.value.code == G.E_INVALID
    d.free()
    # a too-small position capacity: GN_E_CAPACITY with the offsets filled; a following call is correct
    arr, _keep = G._games_array(fixture_games)
    ng = len(fixture_games)
    for name in ("gn_evaluate_games_lines2_history", "gn_evaluate_games_lines2"):
        offs, status = np.zeros(ng + 1, dtype=np.uint32), np.zeros(ng, dtype=np.int32)
        pos, lines = np.zeros(16, dtype=G.EVAL_DTYPE), np.zeros((16, K_GAMES), dtype=G.LINE2_DTYPE)
        rc = getattr(G.lib(), name)(gpu_ctx.h, arr, ng, 0, K_GAMES, offs.ctypes.data, status.ctypes.data,
                                    pos.ctypes.data, 16, lines.ctypes.data)
        assert rc == G.E_CAPACITY and offs.tobytes() == got[(0, K_GAMES)][0].tobytes()
        assert not lines["plies"].any()  # nothing was written
    assert _same(got[(0, K_GAMES)], gpu_ctx.evaluate_games_lines2_history(fixture_games, K_GAMES, 0))
