"""Game-history draws in ranked lines (include/gpu_nnue.h at gn_history) on the GPU against the
rule restated from the CPU oracle (tests/history_rule.py): gn_position_keys_device,
gn_rank_children_history_device and gn_evaluate_games_lines_history, over the fixture
tests/golden/history_games.txt and the 64 random games of tests/test_gpu_lines.py."""
import numpy as np
import pytest

import history_rule as H
import lines_rule as R

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
MODES = (0, 1)  # FULL, BIG
K_GAMES = 3


@pytest.fixture(scope="module")
def fixture_games():
    return H.fixture_games()


@pytest.fixture(scope="module")
def replayed(oracle_lib, fixture_games):
    return [oracle_lib.replay_game(root, moves)[0] for root, moves, _ in fixture_games]


@pytest.fixture(scope="module")
def expected(oracle_lib, oracle_nets, fixture_games, replayed):
    """{mode: lines[positions, 8]} of the fixture by the restated rule (K < 8 is its prefix)."""
    big, small = oracle_nets
    return {mode: np.concatenate([H.game_lines(oracle_lib, big, small, fens, skip, mode, 8)
                                  for fens, (_, _, skip) in zip(replayed, fixture_games)]) for mode in MODES}


@pytest.fixture(scope="module")
def got(gpu_ctx, fixture_games):
    return {(mode, K): gpu_ctx.evaluate_games_lines_history(fixture_games, K, mode) for mode in MODES for K in KS}


@pytest.fixture(scope="module")
def random_games():
    from fishnet_amd import gpu_nnue as G
    ucis = G.random_games_uci(0x5EED11E6, 0, 64, 80)
    out = [(R.START, u, (2, 40) if g % 5 == 0 else ()) for g, u in enumerate(ucis)]
    out[7] = (R.START, "e2e4 e7e5 e1e3 g8f6", ())  # an illegal move
    out[11] = ("not a fen", "e2e4", ())             # a bad root
    out[13] = (R.fixture_fens()[0], "", (0,))       # its only position skipped
    return out


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- keys ---------------------------------------------------------------------------------------

def test_device_keys_equal_host_keys(gpu_ctx, fixture_games):
    from fishnet_amd import gpu_nnue as G
    boards = np.concatenate([G.random_positions(0x5EED4158, 0, 4096, 160)] +
                            [G.replay_game(root, moves)[0] for root, moves, _ in fixture_games])
    bad = boards[:3].copy()
    bad["occ"] = 0  # rejected boards: key 0
    boards = np.concatenate([boards, bad])
    n = len(boards)
    d_b, d_k = gpu_ctx.alloc(n * 32), gpu_ctx.alloc(n * 8)
    d_b.upload(boards)
    gpu_ctx.position_keys_device(d_b, n, d_k)
    gpu_ctx.synchronize()
    keys = d_k.download(np.uint64, n)
    d_b.free(), d_k.free()
    host = G.position_keys(boards)
    assert np.array_equal(keys, host) and (host[-3:] == 0).all() and (host[:-3] != 0).all()


# ---- the rule -----------------------------------------------------------------------------------

def test_expected_shows_draws(expected):
    """The fixture's expected output, computed on the CPU, carries draws within the top 8."""
    for mode in MODES:
        assert int((expected[mode]["flags"] & H.FLAG_DRAW != 0).sum()) >= 10
        drawn = expected[mode][expected[mode]["flags"] & H.FLAG_DRAW != 0]
        assert (drawn["value"] == 0).all() and (drawn["score"] == 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
def test_games_lines_history_vs_rule(got, expected, fixture_games, replayed, mode, K):
    offs, status, pos, lines = got[(mode, K)]
    exp = expected[mode][:, :K]
    assert not status.any() and lines.shape == exp.shape
    assert [int(o) for o in offs] == [0] + list(np.cumsum([len(f) for f in replayed]))
    for i in np.flatnonzero((lines != exp).any(axis=1))[:5]:
        g = int(np.searchsorted(offs, i, side="right")) - 1
        assert lines[i].tolist() == exp[i].tolist(), (g, replayed[g][i - int(offs[g])], mode, K)
    assert np.array_equal(lines, exp)


@pytest.mark.parametrize("mode", MODES)
def test_prefix_property(got, mode):
    assert np.array_equal(got[(mode, 8)][3][:, :3], got[(mode, 3)][3])
    assert np.array_equal(got[(mode, 8)][3][:, :1], got[(mode, 1)][3])


# ---- neutrality ---------------------------------------------------------------------------------

def test_neutral_where_nothing_is_drawn(gpu_ctx, oracle_lib, fixture_games, replayed, random_games):
    from fishnet_amd import gpu_nnue as G
    O = oracle_lib
    before = gpu_ctx.evaluate_games_lines(random_games, K_GAMES, 0)
    hist = gpu_ctx.evaluate_games_lines_history(random_games, K_GAMES, 0)
    after = gpu_ctx.evaluate_games_lines(random_games, K_GAMES, 0)
    assert _same(before, after)  # the plain call: the same bytes before and after a history call
    assert _same(before[:3], hist[:3])  # offsets, status, records
    offs, status, _, plain = before
    # every 23rd position and the positions around the failed games (as test_games_lines_vs_rule samples)
    checked = differ = 0
    for g, (root, uci, skip) in enumerate(random_games):
        if status[g]:
            continue
        fens = None
        for p in range(int(offs[g + 1] - offs[g])):
            at = int(offs[g]) + p
            if not (at % 23 == 0 or p in skip or g in (6, 8, 10, 12, 13)):
                continue
            fens = fens or O.replay_game(root, uci)[0]
            if p in skip or not H.drawn_moves(O, fens, p):
                assert hist[3][at].tobytes() == plain[at].tobytes(), (g, p, fens[p])
                checked += 1
            else:
                differ += 1
    assert checked >= 200 and differ <= checked // 10
    # the fixture: records and offsets equal, and the lines wherever the rule draws nothing
    fplain = gpu_ctx.evaluate_games_lines(fixture_games, 8, 0)
    fhist = gpu_ctx.evaluate_games_lines_history(fixture_games, 8, 0)
    assert _same(fplain[:3], fhist[:3])
    quiet = drawn = 0
    for g, (fens, (_, _, skip)) in enumerate(zip(replayed, fixture_games)):
        for p in range(len(fens)):
            at = int(fplain[0][g]) + p
            if p in skip or not H.drawn_moves(O, fens, p):
                assert fhist[3][at].tobytes() == fplain[3][at].tobytes(), (g, p)
                quiet += 1
            else:
                drawn += 1
    assert quiet >= 30 and drawn >= 30
    assert not (fplain[3]["flags"] & G.FLAG_DRAW).any()


# ---- the same bytes from every path ------------------------------------------------------------

def test_same_bytes_chunked_two_slots_in_place_and_gathered(gpu_ctx, got, fixture_games, synth_big_path,
                                                            synth_small_path):
    from fishnet_amd import gpu_nnue as G
    base = got[(0, K_GAMES)]
    again = gpu_ctx.evaluate_games_lines_history(fixture_games, K_GAMES, 0)
    assert _same(base, again)
    assert gpu_ctx.get_option(G.STAT_RANK_NS) > 0 and gpu_ctx.get_option(G.STAT_KEYS_NS) > 0
    try:  # 12 games of at most 129 positions, chunks cut at game starts: at least 3 chunks
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 20)
        chunked = gpu_ctx.evaluate_games_lines_history(fixture_games, K_GAMES, 0)
    finally:
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    assert len(base[2]) >= 3 * 20 + 100 and _same(base, chunked)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        sharded = two.evaluate_games_lines_history(fixture_games, K_GAMES, 0)
        assert two.get_option(G.STAT_KEYS_NS) > 0
    finally:
        two.close()
    assert _same(base, sharded)
    # without the skip game every shard runs in place; with it the shard is gathered
    skip_games = [g for g, (_, _, skip) in enumerate(fixture_games) if skip]
    assert len(skip_games) == 1
    s = skip_games[0]
    rest = fixture_games[:s] + fixture_games[s + 1:]
    offs, _, pos, lines = base
    o2, s2, p2, l2 = gpu_ctx.evaluate_games_lines_history(rest, K_GAMES, 0)
    a, b = int(offs[s]), int(offs[s + 1])
    assert not s2.any()
    assert p2.tobytes() == np.concatenate([pos[:a], pos[b:]]).tobytes()
    assert l2.tobytes() == np.concatenate([lines[:a], lines[b:]]).tobytes()
    # a plain lines call reports no key time
    gpu_ctx.evaluate_games_lines(rest[:2], K_GAMES, 0)
    assert gpu_ctx.get_option(G.STAT_KEYS_NS) == 0 and gpu_ctx.get_option(G.STAT_RANK_NS) > 0


# ---- the device calls ---------------------------------------------------------------------------

class _Expansion:
    """gn_expand_device of boards, its outputs kept on the device for the ranking calls."""

    def __init__(self, ctx, boards, mode):
        from fishnet_amd import gpu_nnue as G
        self.ctx, self.n = ctx, len(boards)
        n, cap = self.n, 256 * len(boards)
        self.b = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4),
                                                ("ch", cap * 32), ("mv", cap * 2), ("co", cap * G.EVAL_SIZE),
                                                ("ln", n * 8 * 12), ("hist", n * 8))}
        self.b["b"].upload(boards)
        ctx.expand_device(self.b["b"], n, mode, self.b["po"], self.b["off"], self.b["ch"], self.b["mv"], self.b["co"], cap)

    def rank(self, K, keys=None, n_keys=0, hist=None):
        from fishnet_amd import gpu_nnue as G
        b = self.b
        if hist is None:
            self.ctx.rank_children_device(b["b"], self.n, b["off"], b["mv"], b["co"], K, b["ln"])
        else:
            b["hist"].upload(np.asarray(hist, dtype=G.HISTORY_DTYPE))
            self.ctx.rank_children_history_device(b["b"], self.n, b["off"], b["mv"], b["co"], keys, n_keys, b["hist"], K,
                                                  b["ln"])
        self.ctx.synchronize()
        return b["ln"].download(G.LINE_DTYPE, self.n * K).reshape(self.n, K)

    def free(self):
        for x in self.b.values():
            x.free()


def _device_keys(ctx, exp):
    d_k = ctx.alloc(exp.n * 8)
    ctx.position_keys_device(exp.b["b"], exp.n, d_k)
    return d_k


@pytest.mark.parametrize("game", (1, 11))
def test_device_call_equals_the_games_call(gpu_ctx, got, fixture_games, game):
    from fishnet_amd import gpu_nnue as G
    root, moves, skip = fixture_games[game]
    assert not skip
    boards = G.replay_game(root, moves)[0]
    n = len(boards)
    exp = _Expansion(gpu_ctx, boards, 0)
    d_k = _device_keys(gpu_ctx, exp)
    lines = exp.rank(8, d_k, n, [(0, i) for i in range(n)])
    exp.free(), d_k.free()
    offs, _, _, want = got[(0, 8)]
    want = want[int(offs[game]):int(offs[game + 1])]
    assert (want["flags"] & G.FLAG_DRAW).any() and lines.tobytes() == want.tobytes()


def test_no_history_and_the_bound(gpu_ctx, oracle_lib, oracle_nets, fixture_games, replayed):
    """Every entry first > self: the plain ranking wherever the parent's rule50 < 99, the fifty-move
    rule elsewhere.  An entry with self >= n_keys is no history either, although the keys that
    would make a draw lie in the allocation beyond n_keys (an unclamped read stays inside it)."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    boards = np.concatenate([G.replay_game(root, moves)[0] for root, moves, _ in fixture_games])
    fens = [f for game in replayed for f in game]
    n = len(boards)
    exp = _Expansion(gpu_ctx, boards, 0)
    d_k = _device_keys(gpu_ctx, exp)
    plain = exp.rank(8)
    none = exp.rank(8, d_k, n, [(1, 0)] * n)
    r50 = boards["rule50"]
    assert (r50 < 99).sum() >= 100 and (r50 >= 99).sum() >= 30
    assert none[r50 < 99].tobytes() == plain[r50 < 99].tobytes()
    for i in np.flatnonzero(r50 >= 99):
        want = H.game_lines(oracle_lib, big, small, [fens[i]], (), 0, 8)[0]  # a game of one position: no history
        assert none[i].tolist() == want.tolist(), fens[i]
    assert (none["flags"] & G.FLAG_DRAW).any()
    # the bound: game 1's parents with their true entries (first, self), but only the first 4 keys
    # declared: parents 0..3 have their history, parents 4.. (self >= n_keys) none
    a = sum(len(f) for f in replayed[:1])
    m = len(replayed[1])
    full = exp.rank(8, d_k, n, [(a, i) if a <= i < a + m else (1, 0) for i in range(n)])
    assert (full[a:a + m]["flags"] & G.FLAG_DRAW).sum() >= 6  # (with every key declared: threefolds)
    clamp = exp.rank(8, d_k, a + 4, [(a, i) if a <= i < a + m else (1, 0) for i in range(n)])
    assert clamp[a:a + m].tobytes() == none[a:a + m].tobytes()
    assert not (clamp[a:a + m]["flags"] & G.FLAG_DRAW).any()
    exp.free(), d_k.free()


def test_argument_checks(gpu_ctx, got, fixture_games):
    from fishnet_amd import gpu_nnue as G
    for k in (0, 9):
        with pytest.raises(G.GnError) as e:
            gpu_ctx.evaluate_games_lines_history(fixture_games[:2], k, 0)
        assert e.value.code == G.E_INVALID
        d = gpu_ctx.alloc(4096)
        with pytest.raises(G.GnError) as e:
            gpu_ctx.rank_children_history_device(d, 1, d, d, d, d, 1, d, k, d)
        assert e.value.code == G.E_INVALID
        d.free()
    # a too-small position capacity: GN_E_CAPACITY with the offsets filled; a following call is correct
    arr, _keep = G._games_array(fixture_games)
    ng = len(fixture_games)
    offs, status = np.zeros(ng + 1, dtype=np.uint32), np.zeros(ng, dtype=np.int32)
    pos, lines = np.zeros(16, dtype=G.EVAL_DTYPE), np.zeros((16, K_GAMES), dtype=G.LINE_DTYPE)
    rc = G.lib().gn_evaluate_games_lines_history(gpu_ctx.h, arr, ng, 0, K_GAMES, offs.ctypes.data, status.ctypes.data,
                                                 pos.ctypes.data, 16, lines.ctypes.data)
    assert rc == G.E_CAPACITY and offs.tobytes() == got[(0, K_GAMES)][0].tobytes()
    assert _same(got[(0, K_GAMES)], gpu_ctx.evaluate_games_lines_history(fixture_games, K_GAMES, 0))
