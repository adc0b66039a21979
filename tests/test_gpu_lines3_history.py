"""Three-ply ranked lines from games with game-history draws (include/gpu_nnue.h at gn_line3, "game
history") on the GPU: gn_evaluate_games_lines3_history against the rule restated from the CPU oracle
(tests/lines3_history_rule.py) at the chosen positions of tests/golden/lines3_history_games.txt
(tests/test_lines3_history.py checks on the CPU that they hold every shape); the library against its own
two-ply history calls under the check-extended and the quiescent leaf rule; neutrality where nothing
can be drawn; the same bytes from every chunk size, pipeline setting and shard count; the device calls
gn_rank_lines2_ahead_device and gn_rank_lines3_history_device on the chain gn_expand_device ->
gn_expand2_device over the children; the argument checks, and the existing calls' bytes around a
history three-ply call."""
import numpy as np
import pytest

import history_rule as H
import lines2_rule as R2
import lines3_history_rule as H3
import lines3_rule as L3
import lines_rule as R
from test_gpu_lines3 import SENTINEL16, _At, _expand

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
MODES = (0, 1)  # FULL, BIG
DRAW = H3.FLAG_DRAW
NO_HISTORY = (1, 0)  # a gn_history entry with first > self


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def games():
    return H3.fixture_games()


@pytest.fixture(scope="module")
def replayed(oracle_lib, games):
    return [oracle_lib.replay_game(root, moves)[0] for root, moves, _ in games]


@pytest.fixture(scope="module")
def chosen(replayed):
    """The rows of the call's outputs that the rule is computed for: [(row, game, position)]."""
    starts = np.cumsum([0] + [len(f) for f in replayed])
    return [(int(starts[g]) + k, g, k) for g, ks in sorted(H3.CHOSEN.items()) for k in ks]


@pytest.fixture(scope="module")
def expected(oracle_lib, oracle_nets, games, replayed):
    """{mode: (lines[positions, 8], pvs[positions, 8])} by the restated rule, at the chosen positions."""
    big, small = oracle_nets
    out = {}
    for mode in MODES:
        parts = [H3.game_lines3(oracle_lib, big, small, fens, skip, mode, 8, only=H3.CHOSEN[g])
                 for g, (fens, (_, _, skip)) in enumerate(zip(replayed, games))]
        out[mode] = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return out


@pytest.fixture(scope="module")
def got(gpu_ctx, games):
    """(mode, K) -> (offsets, status, positions, lines, pvs) of the history call, static leaves."""
    memo = {}

    def call(mode, K):
        if (mode, K) not in memo:
            memo[(mode, K)] = gpu_ctx.evaluate_games_lines3_history(games, K, L3.LEAF_STATIC, 0, mode)
        return memo[(mode, K)]
    return call


@pytest.fixture(scope="module")
def plain(gpu_ctx, games):
    return gpu_ctx.evaluate_games_lines3(games, 8, L3.LEAF_STATIC, 0, 0)


# ---- 1: the rule --------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
def test_games_lines3_history_vs_rule(got, expected, replayed, chosen, mode, K):
    offs, status, pos, lines, pvs = got(mode, K)
    exp, epv = expected[mode]
    assert not status.any() and lines.shape == (len(exp), K) and pvs.shape == lines.shape
    assert [int(o) for o in offs] == [0] + list(np.cumsum([len(f) for f in replayed]))
    for row, g, k in chosen:
        assert lines[row].tolist() == exp[row, :K].tolist(), (g, k, replayed[g][k], mode, K)
        assert pvs[row].tobytes() == epv[row, :K].tobytes(), (g, k, replayed[g][k], mode, K, pvs[row], epv[row, :K])
    rows = [r for r, _, _ in chosen]
    assert lines[rows].tobytes() == exp[rows, :K].tobytes() and pvs[rows].tobytes() == epv[rows, :K].tobytes()


def test_shapes_as_the_gpu_returns_them(got, plain, games, chosen):
    """The three kinds of drawn line by plies, the skipped positions' empty lines, the mate that beats the
    draw, the checking drawn child, and a line 1 whose move the draw changes."""
    from fishnet_amd import gpu_nnue as G
    offs, _, pos, lines, pvs = got(0, 8)
    row = {(g, k): r for r, g, k in chosen}
    drawn = lambda key, plies: ((lines[row[key]]["flags"] & DRAW) != 0) & (lines[row[key]]["plies"] == plies)
    assert drawn((0, 7), 1).any() and drawn((3, 6), 2).any() and drawn((7, 5), 3)[0] and drawn((7, 7), 1)[0]
    assert drawn((4, 0), 3).any() and drawn((5, 0), 2).any() and drawn((6, 0), 1).sum() == 7
    for key in ((0, 4), (7, 4), (1, 3), (2, 3)):  # second occurrences only; one game listed twice
        assert not (lines[row[key]]["flags"] & DRAW).any()
        assert lines[row[key]].tobytes() == plain[3][row[key]].tobytes()
    assert lines[row[(1, 3)]].tobytes() == lines[row[(2, 3)]].tobytes()
    for k in games[3][2]:  # skipped: history for the others, empty themselves
        r = int(offs[3]) + k
        assert int(pos["flags"][r]) & G.FLAG_SKIPPED and all(x == L3.EMPTY3 for x in lines[r].tolist())
        assert not pvs[r].view(np.uint16).any()
    mate = lines[row[(6, 0)]][0]
    assert int(mate["move"]) == R2.uci_move("h2h8") and int(mate["flags"]) == G.FLAG_MATE | G.FLAG_NO_MOVES | G.FLAG_IN_CHECK
    checks = lines[row[(6, 0)]][1:]
    assert (checks["flags"] == (DRAW | G.FLAG_IN_CHECK)).any() and (checks["value"] == 0).all()
    assert lines[row[(7, 6)]][0]["move"] != plain[3][row[(7, 6)]][0]["move"]
    assert not (plain[3]["flags"] & DRAW).any()
    # every PV is the line's own moves: a drawn leaf is never searched
    for r in range(len(lines)):
        for ln, pv in zip(lines[r], pvs[r]):
            assert int(pv["len"]) == int(ln["plies"])
            assert pv["moves"][:3].tolist() == [int(ln["move"]), int(ln["reply"]), int(ln["reply2"])]


@pytest.mark.parametrize("mode", MODES)
def test_prefix_property(got, mode):
    assert np.array_equal(got(mode, 8)[3][:, :3], got(mode, 3)[3]) and np.array_equal(got(mode, 8)[4][:, :3], got(mode, 3)[4])
    assert np.array_equal(got(mode, 8)[3][:, :1], got(mode, 1)[3]) and np.array_equal(got(mode, 8)[4][:, :1], got(mode, 1)[4])


# ---- 2: consequence (a), the library against its own two-ply history calls ----------------------

@pytest.mark.parametrize("leaf", (L3.LEAF_CHECKS, L3.LEAF_QUIESCE))
def test_lines_equal_the_two_ply_history_calls_on_the_extended_games(gpu_ctx, oracle_lib, games, replayed, chosen, leaf):
    """For every line of the chosen positions whose child has a legal move and is not drawn: the game
    cut at position k with the line's move appended, every position but k + 1 skipped, through
    gn_evaluate_games_lines2_extended / _quiescent_pv with history = 1 at n_lines = 1."""
    from fishnet_amd import gpu_nnue as G
    depth = 1 if leaf == L3.LEAF_QUIESCE else 0
    offs, status, pos, lines, pvs = gpu_ctx.evaluate_games_lines3_history(games, 8, leaf, depth, 0)
    assert not status.any()
    items, ext = [], []
    for row, g, k in chosen:
        root, moves, skip = games[g]
        if k in skip:
            continue
        drawn = H.drawn_moves(oracle_lib, replayed[g], k)
        for j, ln in enumerate(lines[row]):
            fl, m = int(ln["flags"]), int(ln["move"])
            if fl & G.FLAG_NO_SCORE:
                continue
            if m in drawn:
                assert fl & DRAW and int(ln["plies"]) == 1 and not fl & (G.FLAG_SEARCHED | G.FLAG_NO_MOVES)
                assert (int(ln["value"]), int(ln["reply"]), int(ln["reply2"])) == (0, 0, 0) and int(pvs[row, j]["len"]) == 1
                continue
            if int(ln["plies"]) == 1:  # the child has no legal move
                assert fl & G.FLAG_NO_MOVES and not fl & DRAW
                continue
            items.append((row, j, g, k))
            ext.append((root, " ".join(moves.split()[:k] + [G.move_to_uci(m)]), tuple(range(k + 1))))
    assert len(items) >= 60
    if leaf == L3.LEAF_QUIESCE:
        o2, s2, _, l2, p2 = gpu_ctx.evaluate_games_lines2_quiescent_pv(ext, 1, depth, 0, history=True)
    else:
        o2, s2, _, l2 = gpu_ctx.evaluate_games_lines2_extended(ext, 1, 0, history=True)
        p2 = None
    assert not s2.any()
    keep = G.FLAG_NO_MOVES | G.FLAG_SEARCHED | DRAW
    deep = 0
    for e, (row, j, g, k) in enumerate(items):
        ln, L = lines[row, j], l2[int(o2[e + 1]) - 1, 0]
        what = (g, k, G.move_to_uci(int(ln["move"])), leaf)
        assert int(o2[e + 1] - o2[e]) == k + 2 and not int(L["flags"]) & G.FLAG_NO_SCORE, what
        assert int(ln["value"]) == R.negate_ply(int(L["value"])), what
        assert (int(ln["reply"]), int(ln["reply2"]), int(ln["plies"])) == (int(L["move"]), int(L["reply"]), 1 + int(L["plies"])), what
        assert int(ln["flags"]) & keep == int(L["flags"]) & keep, what
        pv = pvs[row, j]
        if p2 is not None:
            q = p2[int(o2[e + 1]) - 1, 0]
            assert pv["moves"][:int(pv["len"])].tolist() == [int(ln["move"])] + q["moves"][:int(q["len"])].tolist(), what
        else:
            assert pv["moves"][:int(pv["len"])].tolist() == [int(ln["move"]), int(ln["reply"]), int(ln["reply2"])][:int(ln["plies"])], what
        deep += bool(int(ln["flags"]) & DRAW)
    assert deep >= 10  # draws that L carries: at the reply and at the answer


# ---- 3: consequences (b) and (c) ----------------------------------------------------------------

@pytest.fixture(scope="module")
def random_games():
    from fishnet_amd import gpu_nnue as G
    ucis = G.random_games_uci(0x5EED33E7, 0, 8, 12)
    out = [(R.START, u, (2, 9) if g % 3 == 0 else ()) for g, u in enumerate(ucis)]
    out[5] = (R.START, "e2e4 e7e5 e1e3 g8f6", ())  # an illegal move
    return out


@pytest.mark.parametrize("leaf", (L3.LEAF_STATIC, L3.LEAF_CHECKS))
def test_neutral_where_nothing_can_be_drawn(gpu_ctx, random_games, leaf):
    """Seeded random games of 12 plies: a position whose clock is below 97 and whose game so far holds no
    identity twice has nothing drawn at any of the three levels; its lines and PVs are gn_evaluate_games_lines3's
    byte for byte, and the front (offsets, status, records) is, always."""
    from fishnet_amd import gpu_nnue as G
    before = gpu_ctx.evaluate_games_lines3(random_games, 3, leaf, 0, 0)
    hist = gpu_ctx.evaluate_games_lines3_history(random_games, 3, leaf, 0, 0)
    assert _same(before[:3], hist[:3])
    offs, status = before[0], before[1]
    assert status[5] == G.E_ILLEGAL_MOVE and not np.delete(status, 5).any()
    quiet = 0
    for g, (root, uci, skip) in enumerate(random_games):
        if status[g]:
            continue
        fens = G.boards_to_fens(G.replay_game(root, uci)[0])
        ids = [H.identity(f) for f in fens]
        for k in range(len(fens)):
            at = int(offs[g]) + k
            if int(fens[k].split()[4]) < 97 and max(ids[:k + 1].count(i) for i in ids[:k + 1]) < 2:
                assert hist[3][at].tobytes() == before[3][at].tobytes(), (g, k, fens[k])
                assert hist[4][at].tobytes() == before[4][at].tobytes(), (g, k, fens[k])
                quiet += 1
    assert quiet >= 80 and not (hist[3]["flags"] & DRAW).any()


def test_front_is_the_plain_calls(got, plain):
    assert _same(got(0, 8)[:3], plain[:3])


# ---- 4: the same bytes from every path ----------------------------------------------------------

def test_same_bytes_from_every_path(gpu_ctx, got, games, synth_big_path, synth_small_path):
    """GN_OPT_CHUNK_PARENTS 1, 3 (cuts inside one root's children and across games) and the default,
    GN_OPT_EXPAND_PIPELINE 0 and 2, and a two-shard context; the statistics of the history call."""
    from fishnet_amd import gpu_nnue as G
    base = got(0, 3)
    q = gpu_ctx.evaluate_games_lines3_history(games, 3, L3.LEAF_QUIESCE, 1, 0)
    gpu_ctx.evaluate_games_lines3(games, 3, L3.LEAF_STATIC, 0, 0)
    assert gpu_ctx.get_option(G.STAT_RANK3_NS) > 0 and gpu_ctx.get_option(G.STAT_KEYS_NS) == 0
    others, qothers = [], []
    try:
        for pipeline, chunk in ((2, 1), (2, 3), (0, 3), (0, 0)):
            gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, pipeline)
            gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, chunk)
            others.append(gpu_ctx.evaluate_games_lines3_history(games, 3, L3.LEAF_STATIC, 0, 0))
            assert gpu_ctx.get_option(G.STAT_RANK3_NS) > 0 and gpu_ctx.get_option(G.STAT_KEYS_NS) >= 0
            assert gpu_ctx.get_option(G.STAT_RANK2_NS) > 0 and gpu_ctx.host_stages()["total"] > 0
            if chunk == 3:
                qothers.append(gpu_ctx.evaluate_games_lines3_history(games, 3, L3.LEAF_QUIESCE, 1, 0))
    finally:
        gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, 2)
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        others.append(two.evaluate_games_lines3_history(games, 3, L3.LEAF_STATIC, 0, 0))
        assert two.get_option(G.STAT_RANK3_NS) > 0
        two.set_option(G.OPT_CHUNK_PARENTS, 3)
        others.append(two.evaluate_games_lines3_history(games, 3, L3.LEAF_STATIC, 0, 0))
        qothers.append(two.evaluate_games_lines3_history(games, 3, L3.LEAF_QUIESCE, 1, 0))
    finally:
        two.close()
    for o in others:
        assert _same(base, o)
    for o in qothers:
        assert _same(q, o)
    # without PVs; and without the game that skips positions (every shard in place, nothing gathered)
    o2 = gpu_ctx.evaluate_games_lines3_history(games, 3, L3.LEAF_STATIC, 0, 0, pvs=False)
    assert o2[4] is None and _same(o2[:4], base[:4])
    o3 = gpu_ctx.evaluate_games_lines3_history(games[:3] + games[4:], 3, L3.LEAF_STATIC, 0, 0)
    offs = base[0]
    rows = list(range(int(offs[3]))) + list(range(int(offs[4]), int(offs[-1])))
    assert o3[3].tobytes() == base[3][rows].tobytes() and o3[4].tobytes() == base[4][rows].tobytes()


# ---- 5: the device calls ------------------------------------------------------------------------

class _Chain:
    """gn_expand_device of every fixture position, gn_expand2_device over the children, and the positions'
    keys in an allocation of exactly n_keys entries; the second and later games have first > 0."""

    def __init__(self, ctx, games, mode=0):
        from fishnet_amd import gpu_nnue as G
        from test_gpu_parity import _expand2
        self.ctx = ctx
        per = [G.replay_game(root, moves)[0] for root, moves, _ in games]
        boards = np.concatenate(per)
        self.n = n = len(boards)
        starts = np.cumsum([0] + [len(p) for p in per])
        self.game_of = np.repeat(np.arange(len(per)), [len(p) for p in per])
        self.first = starts[self.game_of]
        self.b, self.total, self.off, self.mv, self.flags = _expand(ctx, boards, mode)
        self.t2, self.g2, self.out = _expand2(ctx, self.b["ch"], self.total, mode)
        self.d_k = ctx.alloc(n * 8)
        ctx.position_keys_device(self.b["b"], n, self.d_k)
        # the roots' entries: their true (first, self), but no history for game 4's single position
        self.hist = np.array([NO_HISTORY if self.game_of[i] == 4 else (int(self.first[i]), i) for i in range(n)],
                             dtype=G.HISTORY_DTYPE)
        self.chist = np.repeat(self.hist, np.diff(self.off.astype(np.int64)))
        self.d_hist, self.d_chist = ctx.alloc(n * 8), ctx.alloc(max(self.total, 1) * 8)
        self.d_hist.upload(self.hist), self.d_chist.upload(self.chist)
        self.d_cl, self.d_cp = ctx.alloc(self.total * 16), ctx.alloc(self.total * 16)

    def rank2(self, ahead=None, hist=True):
        """The children's line 1: gn_rank_lines2_extended_device (ahead None) or gn_rank_lines2_ahead_device."""
        from fishnet_amd import gpu_nnue as G
        kw = dict(d_keys=self.d_k, n_keys=self.n, d_hist=self.d_chist) if hist else {}
        if ahead is None:
            self.ctx.rank_lines2_extended_device(self.b["ch"], self.total, self.out, None, 1, self.d_cl, **kw)
        else:
            self.ctx.rank_lines2_ahead_device(self.b["ch"], self.total, self.out, None, ahead, 1, self.d_cl, **kw)
        self.ctx.line2_pvs_device(self.total, self.out, None, self.d_cl, 1, self.d_cp)
        self.ctx.synchronize()
        return self.d_cl.download(G.LINE2_DTYPE, self.total)

    def rank3(self, K, hist, with_pvs=True, total=None):
        """gn_rank_lines3_history_device (hist "null": d_hist NULL; None: gn_rank_lines3_device) with its
        outputs inside allocations of sentinels, one entry on either side."""
        from fishnet_amd import gpu_nnue as G
        ctx, n, b = self.ctx, self.n, self.b
        total = self.total if total is None else total
        d_ln, d_pv = ctx.alloc((n * K + 2) * 20), ctx.alloc((n * K + 2) * 16)
        d_ln.upload(np.full((n * K + 2) * 10, SENTINEL16, dtype=np.uint16))
        d_pv.upload(np.full((n * K + 2) * 8, SENTINEL16, dtype=np.uint16))
        o_ln, o_pv = _At(d_ln, 20), (_At(d_pv, 16) if with_pvs else None)
        cp = self.d_cp if with_pvs else None
        if hist is None:
            ctx.rank_lines3_device(b["b"], n, b["off"], b["mv"], b["co"], total, self.d_cl, cp, K, o_ln, o_pv)
        else:
            ctx.rank_lines3_history_device(b["b"], n, b["off"], b["mv"], b["co"], total, self.d_cl, cp, b["ch"], self.d_k,
                                           n, None if hist == "null" else self.d_hist, K, o_ln, o_pv)
        ctx.synchronize()
        raw, praw = d_ln.download(np.uint16, (n * K + 2) * 10), d_pv.download(np.uint16, (n * K + 2) * 8)
        d_ln.free(), d_pv.free()
        assert (raw[:10] == SENTINEL16).all() and (raw[10 + n * K * 10:] == SENTINEL16).all()
        assert (praw[:8] == SENTINEL16).all() and (praw[8 + n * K * 8:] == SENTINEL16).all()
        if not with_pvs:
            assert (praw == SENTINEL16).all()
        return raw[10:10 + n * K * 10].view(G.LINE3_DTYPE).reshape(n, K), \
            (praw[8:8 + n * K * 8].view(G.PV_DTYPE).reshape(n, K) if with_pvs else None)

    def free(self):
        for x in list(self.b.values()) + list(self.out.values()) + [self.d_k, self.d_hist, self.d_chist, self.d_cl, self.d_cp]:
            if hasattr(x, "free"):
                x.free()


@pytest.fixture(scope="module")
def chain(gpu_ctx, games):
    c = _Chain(gpu_ctx, games)
    yield c
    c.free()


def test_rank_lines2_ahead_device(chain, oracle_lib, oracle_nets, replayed, chosen):
    """ahead = 0 is gn_rank_lines2_extended_device byte for byte, with and without history; ahead = 1 gives
    the rule's L for every child of the chosen positions (an empty line where the child has no move)."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    assert chain.total > 300 and (chain.first[chain.game_of >= 1] > 0).all()
    for hist in (True, False):
        assert chain.rank2(0, hist).tobytes() == chain.rank2(None, hist).tobytes()
    assert chain.rank2(1, False).tobytes() == chain.rank2(None, False).tobytes()  # d_hist NULL: no history at all
    zero, one = chain.rank2(0), chain.rank2(1)
    assert zero.tobytes() != one.tobytes()
    checked = drawn = 0
    for row, g, k in chosen:
        fens = replayed[g]
        kids = {m: (c, alive) for m, c, alive in H._children(oracle_lib, fens[k])}
        assert sorted(kids) == sorted(chain.mv[int(chain.off[row]):int(chain.off[row + 1])].tolist())
        for j in range(int(chain.off[row]), int(chain.off[row + 1])):
            m = int(chain.mv[j])
            c, alive = kids[m]
            L = H3.child_line(oracle_lib, big, small, fens, k, c, 0) if alive else None
            assert one[j].tolist() == (R2.EMPTY2 if L is None else L), (g, k, G.move_to_uci(m))
            checked += 1
            drawn += bool(L and L[4] & DRAW)
    assert checked >= 200 and drawn >= 40


@pytest.mark.parametrize("K", KS)
def test_rank_lines3_history_device(chain, got, plain, games, expected, chosen, K):
    """The whole chain equals the games call (and so the rule) at every position that is not skipped;
    d_hist NULL is gn_rank_lines3_device byte for byte; outputs inside sentinels."""
    offs, _, _, want, wpv = got(0, K)
    skipped = [int(offs[g]) + k for g, (_, _, skip) in enumerate(games) for k in skip]
    keep = [i for i in range(chain.n) if i not in skipped]
    chain.rank2(1)
    lines, pvs = chain.rank3(K, True)
    assert lines[keep].tobytes() == want[keep].tobytes() and pvs[keep].tobytes() == wpv[keep].tobytes()
    rows = [r for r, g, k in chosen if r not in skipped]
    assert lines[rows].tobytes() == expected[0][0][rows, :K].tobytes()
    nopv, none = chain.rank3(K, True, with_pvs=False)
    assert none is None and nopv.tobytes() == lines.tobytes()
    # no history at all: the plain kernel's bytes, from the plain child lines
    chain.rank2(None, False)
    a, apv = chain.rank3(K, "null")
    b, bpv = chain.rank3(K, None)
    assert a.tobytes() == b.tobytes() and apv.tobytes() == bpv.tobytes()
    assert a[keep].tobytes() == plain[3][keep, :K].tobytes() and not (a["flags"] & DRAW).any()
    # "no history" entries for every root, over the history child lines: only the fifty-move part at the child
    if K == 8:
        from fishnet_amd import gpu_nnue as G
        chain.rank2(1)
        chain.d_hist.upload(np.array([NO_HISTORY] * chain.n, dtype=G.HISTORY_DTYPE))
        try:
            c, _ = chain.rank3(K, True)
        finally:
            chain.d_hist.upload(chain.hist)
        row = {(g, k): r for r, g, k in chosen}
        assert c[row[(6, 0)]].tobytes() == want[row[(6, 0)]].tobytes()  # rule50 99: every quiet child is drawn
        # the perpetual's position 7: its only child is a third occurrence, which no history cannot see
        assert int(want[row[(7, 7)]][0]["plies"]) == 1 and int(c[row[(7, 7)]][0]["plies"]) > 1


def test_rank_lines3_history_device_total_0_and_cut(chain):
    """total == 0: every line is empty and no input buffer is read (they may be NULL); a total that cuts
    inside a root's children clamps every range, as gn_rank_lines3_device does."""
    from fishnet_amd import gpu_nnue as G
    ctx = chain.ctx
    d_ln = ctx.alloc(9 * 3 * 20)
    d_ln.upload(np.full(9 * 3 * 10, SENTINEL16, dtype=np.uint16))
    ctx.rank_lines3_history_device(None, 9, None, None, None, 0, None, None, None, None, 0, chain.d_hist, 3, d_ln)
    ctx.synchronize()
    empty = d_ln.download(G.LINE3_DTYPE, 27)
    d_ln.free()
    assert all(tuple(x) == L3.EMPTY3 for x in empty.tolist())
    ctx.rank_lines3_history_device(None, 0, None, None, None, 0, None, None, None, None, 0, None, 3, None)
    chain.rank2(1)
    full, _ = chain.rank3(3, True)
    cut = int(chain.off[chain.n - 2]) + 2  # inside the last but one root's children
    part, _ = chain.rank3(3, True, total=cut)
    assert part[:chain.n - 2].tobytes() == full[:chain.n - 2].tobytes()
    assert all(tuple(x) == L3.EMPTY3 for x in part[chain.n - 1].tolist())
    assert (part[chain.n - 2]["flags"] & G.FLAG_NO_SCORE).sum() >= 1 and part[chain.n - 2][0]["plies"] > 0


# ---- 6: arguments, and the existing calls -------------------------------------------------------

def test_argument_checks(gpu_ctx, games):
    from fishnet_amd import gpu_nnue as G
    ctx = gpu_ctx
    want = ctx.evaluate_games_lines3_history(games[:2], 3)

    def invalid(f):
        with pytest.raises(G.GnError) as e:
            f()
        assert e.value.code == G.E_INVALID
        assert _same(ctx.evaluate_games_lines3_history(games[:2], 3), want)

    d = ctx.alloc(4096)
    bufs = {k: d for k in ("off", "ch", "co", "mv", "goff", "gmv", "gco")}
    for k in (0, 9):
        invalid(lambda: ctx.evaluate_games_lines3_history(games[:2], k))
        invalid(lambda: ctx.rank_lines3_history_device(d, 1, d, d, d, 1, d, d, d, d, 1, d, k, d, d))
        invalid(lambda: ctx.rank_lines2_ahead_device(d, 1, bufs, None, 1, k, d, d, 1, d))
    for leaf, depth in ((-1, 0), (3, 0), (L3.LEAF_QUIESCE, 0), (L3.LEAF_QUIESCE, 4), (L3.LEAF_STATIC, 1), (L3.LEAF_CHECKS, 2)):
        invalid(lambda: ctx.evaluate_games_lines3_history(games[:2], 3, leaf, depth))
    for ahead in (-1, 2):
        invalid(lambda: ctx.rank_lines2_ahead_device(d, 1, bufs, None, ahead, 1, d, d, 1, d))
        invalid(lambda: ctx.rank_lines2_ahead_device(d, 1, bufs, None, ahead, 1, d))  # (also without a history)
    # the root step: d_pvs without d_child_pvs, NULL buffers that would be read, NULL keys with n_keys > 0
    invalid(lambda: ctx.rank_lines3_history_device(d, 1, d, d, d, 1, d, None, d, d, 1, d, 3, d, d))
    invalid(lambda: ctx.rank_lines3_history_device(d, 1, d, d, d, 1, d, None, None, d, 1, d, 3, d))
    invalid(lambda: ctx.rank_lines3_history_device(d, 1, d, d, d, 1, d, None, d, None, 1, d, 3, d))
    invalid(lambda: ctx.rank_lines3_history_device(d, 1, d, d, d, 1, None, None, d, d, 1, d, 3, d))
    invalid(lambda: ctx.rank_lines3_history_device(d, 1, d, d, d, 1, d, None, d, d, 1, d, 3, None))
    invalid(lambda: ctx.rank_lines2_ahead_device(d, 1, bufs, None, 1, 1, d, None, 1, d))
    d.free()
    # NULL lines with games; nothing to do
    garr, _keep = G._games_array(games[:2])
    offs, status, pos = np.zeros(3, dtype=np.uint32), np.zeros(2, dtype=np.int32), np.zeros(64, dtype=G.EVAL_DTYPE)
    assert G.lib().gn_evaluate_games_lines3_history(ctx.h, garr, 2, 0, 3, 0, 0, offs.ctypes.data, status.ctypes.data,
                                                    pos.ctypes.data, 64, None, None) == G.E_INVALID
    offs, status, pos, lines, pvs = ctx.evaluate_games_lines3_history([], 3)
    assert list(offs) == [0] and len(pos) == 0 and len(lines) == 0


def test_existing_calls_untouched(gpu_ctx, games):
    """gn_evaluate_games_lines3 and gn_evaluate_games_lines2_history give the same bytes before and after a
    history three-ply call on the same context."""
    before3 = gpu_ctx.evaluate_games_lines3(games, 8, L3.LEAF_QUIESCE, 1, 0)
    before2 = gpu_ctx.evaluate_games_lines2_history(games, 8, 0)
    gpu_ctx.evaluate_games_lines3_history(games, 8, L3.LEAF_QUIESCE, 1, 0)
    gpu_ctx.evaluate_games_lines3_history(games, 3, L3.LEAF_STATIC, 0, 1)
    assert _same(before3, gpu_ctx.evaluate_games_lines3(games, 8, L3.LEAF_QUIESCE, 1, 0))
    assert _same(before2, gpu_ctx.evaluate_games_lines2_history(games, 8, 0))
