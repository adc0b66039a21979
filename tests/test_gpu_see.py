"""Exchange evaluation and pruned quiescence (include/gpu_nnue.h at gn_line, "exchange evaluation") on
the GPU against the rule restated in Python (tests/see_rule.py): gn_see_device entry by entry, and with
GN_OPT_QUIESCE_SEE = 1 gn_quiesce_device / gn_quiesce_pv_device, both extended rankings, the host-buffer
calls and their _pv forms; then the option's hygiene and the rule's consequences.

The inputs are tests/test_gpu_quiesce.py's, by its seeds.  What the pruning does to them, by the rule
(tests/test_see.py asserts the conditions on the CPU; mode FULL, unpruned -> pruned):
  one-ply set, 2,458 leaves: 2,027 -> 1,936 searched (91 leaves have only losing noisy moves);
    depth 1: 8,582 -> 6,672 nodes, 301 searched leaves change their value, none upwards;
    depth 2: 47,888 -> 28,612 nodes, 538 values change, 444 of them upwards; 1,910 losing noisy moves
    at the leaves and 9,429 at the nodes the unpruned search visits below them;
  depth-3 set, 615 leaves: 516 -> 485 searched, 56,599 -> 23,983 nodes, 168 values change.
The device helpers are those of tests/test_gpu_quiesce.py and tests/test_gpu_quiesce_pv.py, run with the
option set."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import guarded_buffers as GB
import history_rule as H
import lines2_rule as R2
import lines_rule as R
import quiesce_rule as Q
import raw_boards as RB
import see_rule as S

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
MODES = (0, 1)  # FULL, BIG
K_GAMES = 8
DEPTH_GAMES = {1: 2, 2: 1}  # the games calls' depth, as tests/test_gpu_quiesce.py's
GUARD = GB.GUARD_BYTES // 4   # int32 entries on either side of d_see inside its allocation
SENTINEL = int(np.frombuffer(bytes([GB.GUARD_BYTE] * 4), dtype=np.int32)[0])


class _At:
    """A device pointer `nbytes` into a DeviceBuffer."""

    def __init__(self, buf, nbytes):
        self.ptr = C.c_void_p(buf.addr + nbytes)


def _same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@contextlib.contextmanager
def pruning(ctx, on=1):
    from fishnet_amd import gpu_nnue as G
    ctx.set_option(G.OPT_QUIESCE_SEE, on)
    try:
        yield ctx
    finally:
        ctx.set_option(G.OPT_QUIESCE_SEE, 0)


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


# ---- gn_see_device ------------------------------------------------------------------------------

class _Expanded:
    """gn_expand_device of `boards` (mode FULL), kept on the device: .b["b" | "off" | "mv" | ...]."""

    def __init__(self, ctx, boards):
        from fishnet_amd import gpu_nnue as G
        self.ctx, self.n = ctx, len(boards)
        n, cap = self.n, 256 * len(boards)
        self.b = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4),
                                                ("ch", cap * 32), ("mv", cap * 2), ("co", cap * G.EVAL_SIZE))}
        self.b["b"].upload(boards)
        self.total = ctx.expand_device(self.b["b"], n, 0, self.b["po"], self.b["off"], self.b["ch"], self.b["mv"],
                                       self.b["co"], cap)
        self.off = self.b["off"].download(np.uint32, n + 1)
        self.mv = self.b["mv"].download(np.uint16, self.total)

    def see(self, n=None, total=None):
        """gn_see_device into exactly `total` entries between guards; the guards must come back whole."""
        total = self.total if total is None else total
        buf = self.ctx.alloc((total + 2 * GUARD) * 4)
        buf.upload(np.full(total + 2 * GUARD, SENTINEL, dtype=np.int32))
        self.ctx.see_device(self.b["b"], self.n if n is None else n, self.b["off"], self.b["mv"], total, _At(buf, GUARD * 4))
        self.ctx.synchronize()
        all_ = buf.download(np.int32, total + 2 * GUARD)
        buf.free()
        assert (all_[:GUARD] == SENTINEL).all() and (all_[GUARD + total:] == SENTINEL).all()
        return all_[GUARD:GUARD + total]

    def free(self):
        for x in self.b.values():
            x.free()


@pytest.fixture(scope="module")
def see_set(inputs1):
    """The one-ply set and the positions of tests/golden/see_fens.txt (an en-passant capture, castling
    and promotions among their moves), as tests/test_see.py values them on the host."""
    return _packed(inputs1[0] + [r[1] for r in S.fixture_rows()])


@pytest.fixture(scope="module")
def expanded1(gpu_ctx, see_set):
    e = _Expanded(gpu_ctx, see_set[1])
    yield e
    e.free()


def _see_want(O, fens, e, values=S.DEFAULT_VALUES):
    want = np.full(e.total, Q.NOT_EXTENDED, dtype=np.int64)
    for i, fen in enumerate(fens):
        a, b = int(e.off[i]), int(e.off[i + 1])
        assert sorted(int(m) for m in e.mv[a:b]) == sorted(O.legal_moves(fen))
        for j in range(a, b):
            want[j] = S.see(O, fen, int(e.mv[j]), values)
    return want


def test_see_device_vs_rule(expanded1, see_set, oracle_lib):
    """Every entry after gn_expand_device of the set equals the rule; the guards are whole."""
    got, want = expanded1.see(), _see_want(oracle_lib, see_set[0], expanded1)
    bad = np.flatnonzero(got != want)
    assert not len(bad), [(int(j), int(got[j]), int(want[j])) for j in bad[:5]]
    assert expanded1.total >= 2458 and (want < 0).sum() >= 100 and (want > 0).sum() >= 100
    assert {int(m) >> 14 for m in expanded1.mv} == {0, 1, 2, 3}


def test_see_device_follows_the_eval_params(gpu_ctx, expanded1, see_set, oracle_lib):
    """The context's piece values: a set that reverses an order, then the defaults again."""
    before = expanded1.see()
    p = gpu_ctx.eval_params()
    saved = list(p.piece_value)
    assert tuple(saved) == S.DEFAULT_VALUES
    try:
        for i, v in enumerate(S.REVERSED_VALUES):
            p.piece_value[i] = v
        gpu_ctx.set_eval_params(p)
        got = expanded1.see()
    finally:
        for i, v in enumerate(saved):
            p.piece_value[i] = v
        gpu_ctx.set_eval_params(p)
    assert np.array_equal(got, _see_want(oracle_lib, see_set[0], expanded1, S.REVERSED_VALUES))
    assert not np.array_equal(got, before) and np.array_equal(expanded1.see(), before)


def test_see_device_rejected_parent_and_uncovered_entries(gpu_ctx, inputs3):
    """The moves of a parent the gate rejects, and the entries no offset covers, are GN_NOT_EXTENDED;
    every other entry is what the full call gives."""
    boards = inputs3[1][:12].copy()
    e = _Expanded(gpu_ctx, boards)
    try:
        full = e.see()
        assert (full != Q.NOT_EXTENDED).all()
        m = e.n - 3
        head = int(e.off[m])
        assert 0 < head < e.total
        part = e.see(n=m)
        assert np.array_equal(part[:head], full[:head]) and (part[head:] == Q.NOT_EXTENDED).all()
        short = e.see(total=head - 1)  # the offsets are clamped to total
        assert np.array_equal(short, full[:head - 1])
        bad = next(b for name, b, kind in RB.catalogue() if name == "R3/no-black-king")
        k = next(i for i in range(e.n) if e.off[i + 1] > e.off[i] and 0 < i < e.n - 1)
        boards[k] = bad
        e.b["b"].upload(boards)
        got = e.see()
        a, b = int(e.off[k]), int(e.off[k + 1])
        assert (got[a:b] == Q.NOT_EXTENDED).all()
        assert np.array_equal(got[:a], full[:a]) and np.array_equal(got[b:], full[b:])
    finally:
        e.free()


def test_see_device_argument_checks(gpu_ctx):
    from fishnet_amd import gpu_nnue as G
    d = gpu_ctx.alloc(4096)
    gpu_ctx.see_device(None, 0, None, None, 0, None)
    gpu_ctx.see_device(d, 1, d, None, 0, None)
    for args in ((None, 1, d, d, 1, d), (d, 1, None, d, 1, d), (d, 1, d, None, 1, d), (d, 1, d, d, 1, None)):
        with pytest.raises(G.GnError) as e:
            gpu_ctx.see_device(*args)
        assert e.value.code == G.E_INVALID
    with pytest.raises(G.GnError) as e:
        gpu_ctx.see_device(d, 1, d, d, 1, d, slot=7)
    assert e.value.code == G.E_INVALID
    gpu_ctx.synchronize()
    d.free()


# ---- pruned gn_quiesce_device and the one-ply ranking -------------------------------------------

@pytest.fixture(scope="module")
def level1(gpu_ctx, inputs1, inputs3):
    """tests/test_gpu_quiesce.py's device path with the option at 1, and the depth-1 run at 0."""
    import test_gpu_quiesce as TQ
    with pruning(gpu_ctx):
        out = {mode: {"a": TQ._level1(gpu_ctx, inputs1[1], mode, (1, 2)), "b": TQ._level1(gpu_ctx, inputs3[1], mode, (3,), ks=(8,))}
               for mode in MODES}
    out["unpruned"] = TQ._level1(gpu_ctx, inputs1[1], 0, (1, 2), ks=(8,))
    return out


def _set_of(depth, inputs1, inputs3):
    return ("b", inputs3[0]) if depth == 3 else ("a", inputs1[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", (1, 2, 3))
def test_pruned_quiesce_entries_vs_rule(level1, inputs1, inputs3, oracle_lib, oracle_nets, mode, depth):
    """d_ext entry by entry, *searched and *nodes against the rule's counts of the pruned tree."""
    big, small = oracle_nets
    which, fens = _set_of(depth, inputs1, inputs3)
    r = level1[mode][which]
    x = r["depth"][depth]
    ws = wn = un = 0
    for i, fen in enumerate(fens):
        a, b = int(r["off"][i]), int(r["off"][i + 1])
        kids = S.leaves(oracle_lib, big, small, fen, mode) or []
        ext, ns, nn = S.extensions(oracle_lib, big, small, fen, depth, mode)
        assert len(kids) == b - a
        want = dict(zip((k[0] for k in kids), ext))
        got = dict(zip((int(m) for m in r["mv"][a:b]), (int(e) for e in x["ext"][a:b])))
        assert got == want, (fen, depth)
        ws, wn = ws + ns, wn + nn
        un += Q.extensions(oracle_lib, big, small, fen, depth, mode)[2]
    print(f"depth {depth} mode {mode}: {r['total']} leaves, {ws} searched, {wn} nodes ({un} unpruned)")
    assert x["searched"] == ws == int((x["ext"] != Q.NOT_EXTENDED).sum()) and x["nodes"] == wn < un
    assert r["co"].tobytes() == x["co_after"].tobytes()
    if mode == 0:
        assert (ws, wn) == {1: (1936, 6672), 2: (1936, 28612), 3: (485, 23983)}[depth]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth,K", [(1, 1), (1, 3), (1, 8), (2, 1), (2, 3), (2, 8), (3, 8)])
def test_rank_children_with_pruned_ext_vs_rule(level1, inputs1, inputs3, oracle_lib, oracle_nets, mode, depth, K):
    big, small = oracle_nets
    which, fens = _set_of(depth, inputs1, inputs3)
    lines = level1[mode][which]["depth"][depth]["lines"][K]
    exp = S.lines(oracle_lib, big, small, fens, depth, mode, K)
    for i in np.flatnonzero((lines != exp).any(axis=1))[:5]:
        assert lines[i].tolist() == exp[i].tolist(), (fens[i], mode, depth, K)
    assert np.array_equal(lines, exp)
    if K == 8:
        assert not np.array_equal(lines, Q.lines(oracle_lib, big, small, fens, depth, mode, K))


def test_consequences_on_the_device(level1, inputs1, oracle_lib, oracle_nets):
    """Qs(x, 1) <= Q(x, 1) for a leaf not in check; the searched set under pruning is a subset; at depth 2
    a value rises; and the positions the rule says are unaffected have byte-equal lines."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    cut, full = level1[0]["a"], level1["unpruned"]
    check = (full["co"]["flags"] & G.FLAG_IN_CHECK) != 0
    for depth in (1, 2):
        a, b = full["depth"][depth]["ext"].astype(np.int64), cut["depth"][depth]["ext"].astype(np.int64)
        srch_a, srch_b = a != Q.NOT_EXTENDED, b != Q.NOT_EXTENDED
        assert not (srch_b & ~srch_a).any() and (srch_a & ~srch_b).sum() == 91
        both = srch_a & srch_b
        assert np.array_equal(a[both & check], b[both & check]) or depth == 2
        if depth == 1:
            assert (b[both & ~check] <= a[both & ~check]).all() and (b[both] < a[both]).any()
        else:
            assert (b[both] > a[both]).any()
        same = [i for i, fen in enumerate(inputs1[0]) if S.losing_below(oracle_lib, big, small, fen, depth, 0) == (0, 0)]
        assert len(same) >= 10
        la, lb = full["depth"][depth]["lines"][8], cut["depth"][depth]["lines"][8]
        assert la[same].tobytes() == lb[same].tobytes() and la.tobytes() != lb.tobytes()


# ---- the tails, and two plies -------------------------------------------------------------------

@pytest.fixture(scope="module")
def pv1(gpu_ctx, inputs1, inputs3):
    import test_gpu_quiesce_pv as TP
    with pruning(gpu_ctx):
        return {mode: {"a": TP._level1(gpu_ctx, inputs1[1], mode, (1, 2), ks=(8,)), "b": TP._level1(gpu_ctx, inputs3[1], mode, (3,), ks=(8,))}
                for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", (1, 2, 3))
def test_pruned_tails_vs_rule(pv1, level1, inputs1, inputs3, oracle_lib, oracle_nets, mode, depth):
    """d_tail = PVQs entry by entry (gn_quiesce_pv_device; its d_ext is gn_quiesce_device's), and the
    PVs of the ranked lines."""
    import quiesce_pv_rule as PV
    big, small = oracle_nets
    which, fens = _set_of(depth, inputs1, inputs3)
    r = pv1[mode][which]
    x = r["depth"][depth]
    assert np.array_equal(x["ext"], level1[mode][which]["depth"][depth]["ext"])
    longest = 0
    for i, fen in enumerate(fens):
        a, b = int(r["off"][i]), int(r["off"][i + 1])
        want = S.tails(oracle_lib, big, small, fen, depth, mode)
        for j in range(a, b):
            m = int(r["mv"][j])
            assert x["tails"][j].tolist() == PV.tail_row(want[m]), (fen, m, depth, mode)
            longest = max(longest, len(want[m]))
    assert longest == depth
    lines = S.lines(oracle_lib, big, small, fens, depth, mode, 8)
    assert x["pvs"][8].tobytes() == S.line_pvs(oracle_lib, big, small, fens, lines, depth, mode).tobytes()


@pytest.fixture(scope="module")
def level2(gpu_ctx, inputs2):
    import test_gpu_quiesce_pv as TP
    with pruning(gpu_ctx):
        return {mode: TP._level2(gpu_ctx, inputs2[1], mode, (2,)) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_rank_lines2_with_pruned_ext_vs_rule(level2, inputs2, oracle_lib, oracle_nets, mode):
    """gn_expand2_device, the pruned quiescence over the grandchildren, gn_rank_lines2_extended_device
    and gn_line2_pvs_device at depth 2 for every K."""
    big, small = oracle_nets
    fens = inputs2[0]
    x = level2[mode]["depth"][2]
    for K in KS:
        exp = S.lines2(oracle_lib, big, small, fens, 2, mode, K)
        for i in np.flatnonzero((x["lines"][K] != exp).any(axis=1))[:5]:
            assert x["lines"][K][i].tolist() == exp[i].tolist(), (fens[i], mode, K)
        assert np.array_equal(x["lines"][K], exp)
        assert x["pvs"][K].tobytes() == S.line2_pvs(oracle_lib, big, small, fens, exp, 2, mode).tobytes()
    assert not np.array_equal(exp, Q.lines2(oracle_lib, big, small, fens, 2, mode, 8))


# ---- the host-buffer calls ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def games():
    g = H.fixture_games()
    return [g[0], g[1], g[4], g[10]] + [(f, "", ()) for f in Q.fixture_fens()]


@pytest.fixture(scope="module")
def replayed(oracle_lib, games):
    return [oracle_lib.replay_game(root, moves)[0] for root, moves, _ in games]


def _host_calls(ctx, fens, games):
    """Every quiescent host-buffer call once, with PVs: {name: its outputs}."""
    out = {"lines2": ctx.evaluate_lines2_quiescent_pv(fens, 8, 2, 0)}
    for plies, name in ((1, "evaluate_games_lines_quiescent_pv"), (2, "evaluate_games_lines2_quiescent_pv")):
        for history in (False, True):
            out[(plies, history)] = getattr(ctx, name)(games, K_GAMES, DEPTH_GAMES[plies], 0, history=history)
    return out


@pytest.fixture(scope="module")
def host_got(gpu_ctx, inputs2, games):
    from fishnet_amd import gpu_nnue as G
    with pruning(gpu_ctx):
        out = _host_calls(gpu_ctx, inputs2[0], games)
        out["stats"] = [gpu_ctx.get_option(s) for s in (G.STAT_QUIESCE_LEAVES, G.STAT_QUIESCE_NODES)]
        plain = gpu_ctx.evaluate_lines2_quiescent(inputs2[0], 8, 2, 0)
        assert _same(out["lines2"][:2], plain)  # the forms without PVs give the same records and lines
        for plies, name in ((1, "evaluate_games_lines_quiescent"), (2, "evaluate_games_lines2_quiescent")):
            assert _same(out[(plies, True)][:4], getattr(gpu_ctx, name)(games, K_GAMES, DEPTH_GAMES[plies], 0, history=True))
    return out


def test_evaluate_lines2_quiescent_pruned_vs_rule(host_got, level2, inputs2, oracle_lib, oracle_nets):
    big, small = oracle_nets
    fens = inputs2[0]
    out, lines, pvs = host_got["lines2"]
    exp = S.lines2(oracle_lib, big, small, fens, 2, 0, 8)
    assert np.array_equal(lines, exp) and lines.tobytes() == level2[0]["depth"][2]["lines"][8].tobytes()
    assert pvs.tobytes() == S.line2_pvs(oracle_lib, big, small, fens, exp, 2, 0).tobytes()


@pytest.mark.parametrize("history", (False, True))
@pytest.mark.parametrize("plies", (1, 2))
def test_games_calls_pruned_vs_rule(host_got, games, replayed, oracle_lib, oracle_nets, plies, history):
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    offs, status, pos, lines, pvs = host_got[(plies, history)]
    rule = S.game_lines if plies == 1 else S.game_lines2
    exp = np.concatenate([rule(oracle_lib, big, small, fens, skip, DEPTH_GAMES[plies], 0, K_GAMES, history)
                          for fens, (_, _, skip) in zip(replayed, games)])
    assert not status.any() and lines.shape == exp.shape
    for i in np.flatnonzero((lines != exp).any(axis=1))[:5]:
        assert lines[i].tolist() == exp[i].tolist(), (i, plies, history)
    assert np.array_equal(lines, exp) and (lines["flags"] & G.FLAG_SEARCHED).any()
    assert bool((lines["flags"] & G.FLAG_DRAW).any()) == history
    fens = [f for fs in replayed for f in fs]
    prule = S.line_pvs if plies == 1 else S.line2_pvs
    assert pvs.tobytes() == prule(oracle_lib, big, small, fens, lines, DEPTH_GAMES[plies], 0).tobytes()
    unpruned = (Q.game_lines if plies == 1 else Q.game_lines2)
    assert not np.array_equal(exp, np.concatenate([unpruned(oracle_lib, big, small, f, skip, DEPTH_GAMES[plies], 0, K_GAMES, history)
                                                   for f, (_, _, skip) in zip(replayed, games)]))


def test_host_calls_same_bytes_from_every_path(gpu_ctx, host_got, inputs2, games, synth_big_path, synth_small_path):
    """GN_OPT_CHUNK_PARENTS 1 / 7 / default, GN_OPT_EXPAND_PIPELINE 0 / 2 and two shards of one device."""
    from fishnet_amd import gpu_nnue as G
    others = []
    try:
        with pruning(gpu_ctx):
            for pipeline, chunk in ((0, 0), (2, 1), (2, 7), (0, 7)):
                gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, pipeline)
                gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, chunk)
                others.append(_host_calls(gpu_ctx, inputs2[0], games))
                assert [gpu_ctx.get_option(s) for s in (G.STAT_QUIESCE_LEAVES, G.STAT_QUIESCE_NODES)] == host_got["stats"]
    finally:
        gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, 2)
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        with pruning(two):
            others.append(_host_calls(two, inputs2[0], games))
    finally:
        two.close()
    for o in others:
        for k, v in o.items():
            assert _same(host_got[k], v), k


def _is_noisy(O, fen, m):
    """Restated from the header, not taken from a rule module."""
    typ = m >> 14
    if typ == 3:
        return False
    return typ == 2 or (m & 63) in O._placement(fen) or (typ == 1 and (m >> 12) & 3 == 3)


def _replay(ctx, O, fens, lines, pvs, plies):
    """Every PV played out with the oracle's child_fen alone: each move legal where it is played; each
    move of the tail, unless its mover is in check, noisy with see >= 0 by gn_see_moves; and negate_ply
    applied len times to the end's own value is the line's value.  Returns the tail moves checked."""
    from fishnet_amd import gpu_nnue as G
    ends, items, steps = [], [], []
    for i, fen in enumerate(fens):
        for ln, pv in zip(lines[i], pvs[i]):
            n = int(pv["len"])
            if not n:
                assert int(ln["flags"]) & G.FLAG_NO_SCORE
                continue
            f = fen
            for k, m in enumerate(pv["moves"][:n].tolist()):
                assert m in O.legal_moves(f), (fen, pv)
                if k >= plies:
                    steps.append((f, m))
                f = O.child_fen(f, m)
            items.append((fen, ln, n, len(ends)))
            ends.append(f)
    rec = ctx.evaluate_batch(ends, 0)
    for fen, ln, n, e in items:
        fl = int(ln["flags"])
        if fl & G.FLAG_DRAW:
            v = 0
        elif int(rec["flags"][e]) & G.FLAG_NO_MOVES:
            v = -R.VALUE_MATE if int(rec["flags"][e]) & G.FLAG_IN_CHECK else 0
        else:
            v = int(rec["final_v"][e])
        for _ in range(n):
            v = R.negate_ply(v)
        assert v == int(ln["value"]), (fen, ln, n, ends[e])
    before = ctx.evaluate_batch([f for f, _ in steps], 0)
    sees = G.see_moves(G.pack_fens([f for f, _ in steps])[0], [m for _, m in steps])
    for (f, m), r, s in zip(steps, before, sees):
        if not int(r["flags"]) & G.FLAG_IN_CHECK:
            assert _is_noisy(O, f, m) and int(s) >= 0, (f, m, int(s))
    return len(steps)


def test_pruned_pvs_replayed_without_the_rule(gpu_ctx, host_got, inputs2, replayed, oracle_lib):
    out, lines, pvs = host_got["lines2"]
    tails = _replay(gpu_ctx, oracle_lib, inputs2[0], lines, pvs, 2)
    fens = [f for fs in replayed for f in fs]
    for plies in (1, 2):
        for history in (False, True):
            offs, status, pos, lines, pvs = host_got[(plies, history)]
            tails += _replay(gpu_ctx, oracle_lib, fens, lines, pvs, plies)
    assert tails >= 100


# ---- the option ---------------------------------------------------------------------------------

def test_option_hygiene(inputs2, games, synth_big_path, synth_small_path):
    """A context of its own: the outputs before the option was ever set, with it at 1, and at 0 again;
    the values it refuses; and the calls it must not change."""
    from fishnet_amd import gpu_nnue as G
    ctx = G.GpuNnue(synth_big_path, synth_small_path)
    try:
        fens = inputs2[0]
        assert ctx.get_option(G.OPT_QUIESCE_SEE) == 0
        before = _host_calls(ctx, fens, games)
        others = {"plain": ctx.evaluate_lines2(fens, 8, 0), "extended": ctx.evaluate_lines2_extended(fens, 8, 0),
                  "games": ctx.evaluate_games_lines(games, K_GAMES, 0, history=True),
                  "games_extended": ctx.evaluate_games_lines_extended(games, K_GAMES, 0, history=True),
                  "batch": (ctx.evaluate_batch(fens, 0),)}
        ctx.set_option(G.OPT_QUIESCE_SEE, 1)
        assert ctx.get_option(G.OPT_QUIESCE_SEE) == 1
        for bad in (2, -1):
            with pytest.raises(G.GnError) as e:
                ctx.set_option(G.OPT_QUIESCE_SEE, bad)
            assert e.value.code == G.E_INVALID and ctx.get_option(G.OPT_QUIESCE_SEE) == 1
        on = _host_calls(ctx, fens, games)
        assert all(not _same(before[k], on[k]) for k in before)
        assert _same(others["plain"], ctx.evaluate_lines2(fens, 8, 0))
        assert _same(others["extended"], ctx.evaluate_lines2_extended(fens, 8, 0))
        assert _same(others["games"], ctx.evaluate_games_lines(games, K_GAMES, 0, history=True))
        assert _same(others["games_extended"], ctx.evaluate_games_lines_extended(games, K_GAMES, 0, history=True))
        assert _same(others["batch"], (ctx.evaluate_batch(fens, 0),))
        ctx.set_option(G.OPT_QUIESCE_SEE, 0)
        assert ctx.get_option(G.OPT_QUIESCE_SEE) == 0
        for bad in (2, -1):
            with pytest.raises(G.GnError):
                ctx.set_option(G.OPT_QUIESCE_SEE, bad)
            assert ctx.get_option(G.OPT_QUIESCE_SEE) == 0
        after = _host_calls(ctx, fens, games)
        assert all(_same(before[k], after[k]) for k in before)
    finally:
        ctx.close()
