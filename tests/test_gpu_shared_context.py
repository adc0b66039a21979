"""What a C or Rust caller of the fishnet-facing calls depends on, beyond kernel parity:

1. one gn_ctx shared between threads (gpu_nnue.h: "calls on one context are serialised
   internally"): every evaluating call kind at once on one context gives each thread the bytes
   its call gives alone, and each thread its own gn_last_error;
2. caller-made output arrays: exactly the needed capacity works, one short fails with
   GN_E_CAPACITY and the offsets filled, and no byte outside the given capacity is written
   (guarded_buffers), with several chunks per device and a non-zero shard base;
3. the device replay (replay_games_kernel's resolve_uci) fails a game where the host replay
   (gn_replay_game) does, with the same status and message, for every kind of illegal move
   test_games.py knows.

Every comparison is exact equality of integers or bytes.  The module has its own contexts (it
changes GN_OPT_CHUNK_PARENTS and GN_OPT_COALESCE): one device slot, two slots on one device,
and two slots without a small net.
"""
import ctypes
import threading
import time
import traceback
from types import SimpleNamespace

import numpy as np
import pytest

import test_games as TG
from guarded_buffers import GUARD_BYTES, Guarded, GuardedSet

START = TG.START
CHUNK = 5     # GN_OPT_CHUNK_PARENTS: every game is a chunk of its own, a FEN list runs in blocks of 81
              # parents, gn_evaluate_lines2 in chunks of exactly 5
K_LINES = 3   # gn_evaluate_games_lines
K_LINES2 = 2  # gn_evaluate_lines2
ROUNDS = 6    # calls per thread in the concurrent test
FAILING = (START, "e2e4 e7e5 e1g1", ())
FAILING_ERROR = "move 3 (e1g1) is not legal"


def _illegal_games():
    """(root, moves) of test_games.py's nine illegal-move cases, then its long-token cases."""
    mark = [m for m in TG.test_illegal_moves_fail_the_game.pytestmark if m.name == "parametrize"][0]
    out = []
    for moves, _bad in mark.args[1]:
        out.append((TG.C960_CASTLE, moves[5:]) if moves.startswith("C960 ") else (START, moves))
    assert len(out) == 9
    return out, out + list(TG.LONG_TOKEN_GAMES)


NINE_ILLEGAL, ALL_ILLEGAL = _illegal_games()


# ---- the guard helper, on the CPU ----
def test_guard_helper_catches_writes_outside_the_array():
    g = Guarded(5, np.uint32, "probe")
    assert len(g.a) == 5 and g.untouched() and g.damaged() == []
    g.check()
    ctypes.memmove(g.ptr, b"\x01\x02\x03\x04", 4)  # .ptr is the array's first byte
    assert g.a[0] == 0x04030201 and not g.untouched()
    g.a[:] = 7  # every element written: the guards stay
    g.check()
    # one element past the end, from numpy, as a library with a wrong bound would write it
    np.ndarray(6, np.uint32, buffer=g.raw, offset=GUARD_BYTES)[5] = 7
    assert g.damaged() == [20, 21, 22, 23]
    with pytest.raises(AssertionError, match=r"probe\[5\].*\[20, 21, 22, 23\]"):
        g.check()
    h = Guarded(3, np.uint16, "before")
    ctypes.memset(h.ptr - 1, 0, 1)  # one byte before the start
    assert h.damaged() == [-1]
    with pytest.raises(AssertionError, match="before"):
        h.check()
    z = Guarded(0, np.int32, "empty")  # a zero-length array: the two guards meet
    assert len(z.a) == 0 and z.untouched()
    z.check()
    ctypes.memset(z.ptr, 0, 4)
    assert z.damaged() == [0, 1, 2, 3]
    s = GuardedSet()
    assert s.add("x", 2, np.int32) == s["x"].ptr
    s.check()
    s["x"].raw[-1] = 0
    with pytest.raises(AssertionError, match="x"):
        s.check()


# ---- inputs (host only) and contexts ----
@pytest.fixture(scope="module")
def G():
    from fishnet_amd import build, gpu_nnue
    build.build()
    return gpu_nnue


def _cycle(xs, n):
    return [xs[i % len(xs)] for i in range(n)]


@pytest.fixture(scope="module")
def data(G):
    ucis = G.random_games_uci(0x5EED5C7A, 0, 8, 40)
    good = [(START, u, ()) for u in ucis]
    npos = [len(u.split()) + 1 for u in ucis]
    fens = []  # the good games' positions, in order
    for u in ucis:
        fens += G.boards_to_fens(G.replay_game(START, u)[0])
    assert len(fens) == sum(npos) and sum(npos) >= 300
    d = SimpleNamespace(ucis=ucis, good=good, npos=npos, fens=fens)
    d.mix = good + [(START, ucis[0], (0, 7, npos[0] - 1, 1000)), FAILING]  # + skipped positions, + a failing game
    d.cap_games = [(r, u, (0, 7, npos[2] - 1) if i == 2 else ()) for i, (r, u, _) in enumerate(good)]
    d.b81 = fens[:40] + ["not a fen"] + fens[40:80]
    d.b100, d.b128 = fens[90:190], fens[150:278]  # the 81's size class (128 positions), other positions
    d.b1500, d.b4200 = _cycle(fens, 1500), _cycle(fens, 4200)
    d.expand = _cycle(fens, 165) + ["not a fen"] + _cycle(fens[7:], 164)  # 330: three blocks per shard of two
    d.lines2 = fens[3:15] + ["not a fen"] + fens[50:61]
    assert [len(x) for x in (d.b81, d.b100, d.b128, d.expand, d.lines2)] == [81, 100, 128, 330, 24]
    return d


_HUNG = []  # names of threads a concurrent test left running: nothing more may use the contexts


def _context(G, *args, **kw):
    ctx = G.GpuNnue(*args, **kw)
    ctx.set_option(G.OPT_CHUNK_PARENTS, CHUNK)
    yield ctx
    if _HUNG:
        ctx.h = ctypes.c_void_p()  # (a hung call still uses it: never freed)
    ctx.close()


@pytest.fixture(scope="module")
def one_slot(G, synth_big_path, synth_small_path):
    yield from _context(G, synth_big_path, synth_small_path)


@pytest.fixture(scope="module")
def two_slots(G, synth_big_path, synth_small_path):
    yield from _context(G, synth_big_path, synth_small_path, devices=[0, 0])


@pytest.fixture(scope="module")
def no_small_net(G, synth_big_path):
    yield from _context(G, synth_big_path, None, devices=[0, 0])


@pytest.fixture(params=["one_slot", "two_slots"])
def ctx(request, one_slot, two_slots):
    if _HUNG:
        pytest.fail(f"an earlier test left threads running in the library: {_HUNG}")
    return {"one_slot": one_slot, "two_slots": two_slots}[request.param]


# ---- raw calls with caller-made, guarded arrays ----
def _last_error(G):
    return (G.lib().gn_last_error() or b"").decode()


def _done(G, s, rc):
    s.rc, s.err = rc, _last_error(G)
    return s.check()


def raw_batch(G, ctx, fens, mode):
    s, n = GuardedSet(), len(fens)
    arr, _keep = G._fen_array(fens)
    return _done(G, s, G.lib().gn_evaluate_batch_mode(ctx.h, arr, n, mode, s.add("out", n, G.EVAL_DTYPE)))


def raw_expand(G, ctx, fens, mode, cap):
    s, n = GuardedSet(), len(fens)
    arr, _keep = G._fen_array(fens)
    return _done(G, s, G.lib().gn_expand_and_evaluate(
        ctx.h, arr, n, mode, s.add("parents", n, G.EVAL_DTYPE), s.add("coffs", n + 1, np.uint32),
        s.add("cmv", cap, np.uint16), s.add("cev", cap, G.CHILD_DTYPE), cap))


def raw_games(G, ctx, games, mode, children, pcap, ccap=0):
    s, ng = GuardedSet(), len(games)
    arr, _keep = G._games_array(games)
    offs, status = s.add("offs", ng + 1, np.uint32), s.add("status", ng, np.int32)
    pos = s.add("pos", pcap, G.EVAL_DTYPE)
    kid = (s.add("coffs", pcap + 1, np.uint32), s.add("cmv", ccap, np.uint16),
           s.add("cev", ccap, G.CHILD_DTYPE)) if children else (None, None, None)
    return _done(G, s, G.lib().gn_evaluate_games(ctx.h, arr, ng, mode, int(children), offs, status, pos, pcap,
                                                 kid[0], kid[1], kid[2], ccap))


def raw_games_lines(G, ctx, games, mode, n_lines, pcap):
    s, ng = GuardedSet(), len(games)
    arr, _keep = G._games_array(games)
    return _done(G, s, G.lib().gn_evaluate_games_lines(
        ctx.h, arr, ng, mode, n_lines, s.add("offs", ng + 1, np.uint32), s.add("status", ng, np.int32),
        s.add("pos", pcap, G.EVAL_DTYPE), pcap, s.add("lines", pcap * n_lines, G.LINE_DTYPE)))


def raw_lines2(G, ctx, fens, mode, n_lines):
    s, n = GuardedSet(), len(fens)
    arr, _keep = G._fen_array(fens)
    return _done(G, s, G.lib().gn_evaluate_lines2(ctx.h, arr, n, mode, n_lines, s.add("out", n, G.EVAL_DTYPE),
                                                  s.add("lines", n * n_lines, G.LINE2_DTYPE)))


def _generous_games(G, ctx, games, children, lines=0):
    """The first call of a caller that does not know the sizes: far more than needed.  -> (the call,
    positions needed, children needed)."""
    pcap = sum(len(m.split()) + 1 for _, m, _ in games) + 37
    gen = raw_games_lines(G, ctx, games, 0, lines, pcap) if lines else \
        raw_games(G, ctx, games, 0, children, pcap, 80 * pcap)
    assert gen.rc == 0, gen.err
    need_p = int(gen["offs"].a[-1])
    return gen, need_p, int(gen["coffs"].a[need_p]) if children and not lines else 0


def _same(got, ref, counts):
    """got's arrays are byte-equal to ref's over counts[name] elements (None: the whole of got's)."""
    assert set(counts) == set(got)
    for name, n in counts.items():
        n = len(got[name].a) if n is None else n
        assert got[name].bytes(n) == ref[name].bytes(n), name


def _per_game(s, n_lines=0):
    """Per game: its position records, its child offsets relative to its first child, its children's
    moves and records, its lines -- what may not depend on the other games of the call."""
    offs, out = s["offs"].a, []
    for g in range(len(offs) - 1):
        a, b = int(offs[g]), int(offs[g + 1])
        rec = [s["pos"].a[a:b].tobytes()]
        if "coffs" in s:
            co = s["coffs"].a
            c0, c1 = int(co[a]), int(co[b])
            rec += [(co[a:b + 1].astype(np.int64) - c0).tobytes(), s["cmv"].a[c0:c1].tobytes(),
                    s["cev"].a[c0:c1].tobytes()]
        if "lines" in s:
            rec.append(s["lines"].a[a * n_lines:b * n_lines].tobytes())
        out.append(rec)
    return out


# ---- 1. mixed concurrent calls on one context ----
@pytest.fixture(scope="module")
def anchor(G, one_slot, data, oracle_nets, oracle_lib):
    """The solo reference is the library's own serial result; here it is tied to the oracle once:
    every position record of the mixed games (eval_fens), and the first game's children
    (expand_eval).  -> the bytes of that call's arrays, which every configuration must reproduce."""
    big, small = oracle_nets
    arr, _keep = G._games_array(data.mix)
    offs, status, pos, coffs, cmv, cev, _ = one_slot.evaluate_games_arrays(arr, len(data.mix), 0, children=True)
    assert list(status) == [0] * 9 + [G.E_ILLEGAL_MOVE] and offs[9] == offs[10]
    kids = G.decode_children(cev)
    for g, (root, moves, skip) in enumerate(data.mix[:9]):
        fens, _ = oracle_lib.replay_game(root, moves)
        exp = oracle_lib.eval_fens(big, small, fens, 0)
        a = int(offs[g])
        assert int(offs[g + 1]) - a == len(fens)
        for i in range(len(fens)):
            if i in skip:
                assert tuple(pos[a + i]) == (0, 0, 0, 0, 0, G.FLAG_SKIPPED | G.FLAG_NO_SCORE, 0)
                assert coffs[a + i] == coffs[a + i + 1]
            else:
                assert tuple(pos[a + i]) == tuple(exp[i]), (g, i, fens[i])
        if g == 0:
            for i, fen in enumerate(fens):
                _p, m_exp, k_exp = oracle_lib.expand_eval(big, small, fen, 0)
                c0, c1 = int(coffs[a + i]), int(coffs[a + i + 1])
                assert dict(zip(cmv[c0:c1].tolist(), map(tuple, kids[c0:c1].tolist()))) == \
                    dict(zip(m_exp, map(tuple, G.children_from_evals(k_exp).tolist()))), fen
    return tuple(x.tobytes() for x in (offs, status, pos, coffs, cmv, cev))


def _call_kinds(G, ctx, nonet, data):
    """name -> a call on the shared context that returns its outputs as bytes."""
    def raw(arrays):
        return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)

    def games(children):
        arr, keep = G._games_array(data.mix)

        def call(_keep=keep):
            r = ctx.evaluate_games_arrays(arr, len(data.mix), 0, children=children)
            assert _last_error(G) == FAILING_ERROR  # this thread's failed game, after GN_OK
            return raw(r[:6] if children else r[:3])
        return call

    def expect_error(code, call):
        with pytest.raises(G.GnError) as e:
            call()
        msg = _last_error(G)  # this thread's own message, whatever the other threads fail with
        assert e.value.code == code and msg and str(e.value).endswith(msg), (code, msg, str(e.value))
        return code, msg

    def err_illegal():
        arr, _keep = G._games_array([data.good[1], (START, "e2e5", ()), data.good[2]])
        r = ctx.evaluate_games_arrays(arr, 3, 0, children=False)
        assert list(r[1]) == [0, G.E_ILLEGAL_MOVE, 0] and _last_error(G) == "move 1 (e2e5) is not legal"
        return raw(r[:3]) + expect_error(G.E_ILLEGAL_MOVE, lambda: G.replay_game(START, "e2e4 e7e5 g1f3 k9a1"))

    def err_invalid():
        return expect_error(G.E_INVALID, lambda: ctx.evaluate_lines2(data.lines2, 0)) + \
            expect_error(G.E_INVALID, lambda: ctx.evaluate_games_lines(data.mix, 9))

    def err_nonet():  # fails on both per-device worker threads of the two-slot context without a small net
        return expect_error(G.E_NONET, lambda: nonet.evaluate_batch(data.fens[:12], G.MODE_SMALL))

    return {
        "batch81_full": lambda: raw([ctx.evaluate_batch(data.b81, G.MODE_FULL)]),
        "batch81_big": lambda: raw([ctx.evaluate_batch(data.b81, G.MODE_BIG)]),
        # two more of batch81_full's class and mode: with GN_OPT_COALESCE 0 they share its two graph instances
        "batch100_full": lambda: raw([ctx.evaluate_batch(data.b100, G.MODE_FULL)]),
        "batch128_full": lambda: raw([ctx.evaluate_batch(data.b128, G.MODE_FULL)]),
        "batch1500": lambda: raw([ctx.evaluate_batch(data.b1500, G.MODE_FULL)]),
        "batch4200": lambda: raw([ctx.evaluate_batch(data.b4200, G.MODE_FULL)]),
        "games": games(False),
        "games_children": games(True),
        "games_lines": lambda: raw(ctx.evaluate_games_lines(data.mix, K_LINES, 0)),
        "lines2": lambda: raw(ctx.evaluate_lines2(data.lines2, K_LINES2, 0)),
        "expand": lambda: raw(ctx.expand_and_evaluate(data.expand, 0)),
        "err_illegal": err_illegal,
        "err_invalid": err_invalid,
        "err_nonet": err_nonet,
    }


def _shared_context_run(G, ctx, nonet, data, anchor, one_device):
    assert isinstance(G.lib(), ctypes.CDLL) and not isinstance(G.lib(), ctypes.PyDLL)  # calls release the GIL
    assert ctx.get_option(G.OPT_CHUNK_PARENTS) == CHUNK
    kinds = _call_kinds(G, ctx, nonet, data)
    # the reference: every call alone, before any thread starts
    solo, serial_s = {}, 0.0
    graphs = ctx.get_option(G.STAT_FAST_BATCHES)
    for name, call in kinds.items():
        t0 = time.perf_counter()
        solo[name] = call()
        serial_s += time.perf_counter() - t0
    # the five batches of <= 4,096 FENs ran as captured graphs on one slot; no batch does on two
    assert ctx.get_option(G.STAT_FAST_BATCHES) - graphs == (5 if one_device else 0)
    assert solo["games_children"] == anchor  # (the oracle's records and children)
    n = len(data.fens)  # the games' positions as a FEN batch: the same records
    assert solo["batch4200"][0][:n * G.EVAL_SIZE] == anchor[2][:n * G.EVAL_SIZE]
    assert len({solo[k][-1] for k in ("err_illegal", "err_invalid", "err_nonet")}) == 3  # three different messages

    limit_s = max(60.0, 50.0 * ROUNDS * serial_s)  # no performance number: only ends a hang
    barrier = threading.Barrier(len(kinds))
    got, spans, raised = {k: [] for k in kinds}, {k: [] for k in kinds}, {}

    def work(name, call):
        try:
            barrier.wait(timeout=limit_s)
            for _ in range(ROUNDS):
                t0 = time.perf_counter()
                out = call()
                spans[name].append((t0, time.perf_counter()))
                got[name].append(out)
        except BaseException:  # (pytest's own failures included)
            raised[name] = traceback.format_exc()

    threads = [threading.Thread(target=work, args=kv, name=kv[0], daemon=True) for kv in kinds.items()]
    deadline = time.perf_counter() + limit_s
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, deadline - time.perf_counter()))
    alive = [t.name for t in threads if t.is_alive()]
    if alive:
        _HUNG.extend(alive)
        pytest.fail(f"still running after {limit_s:.0f} s (the calls alone took {serial_s:.3f} s in all): {alive}")
    assert not raised, "\n".join(f"{k}:\n{v}" for k, v in raised.items())
    for name in kinds:
        assert len(got[name]) == ROUNDS
        for r, out in enumerate(got[name]):
            assert out == solo[name], f"{name}, round {r}: differs from the same call alone"
    merged = ctx.get_option(G.STAT_BATCH_CALLS) - ctx.get_option(G.STAT_BATCH_LAUNCHES)
    overlap = [(a, b) for a in kinds for b in kinds if a < b
               for (s0, e0) in spans[a] for (s1, e1) in spans[b] if s0 < e1 and s1 < e0]
    print(f"\nshared context: the {len(kinds)} calls alone {serial_s:.3f} s in all, join limit {limit_s:.0f} s, "
          f"{len(set(overlap))} pairs of call kinds overlapped, {merged} batch calls merged into another's launch")
    assert overlap, f"no two call kinds ran at the same time (serial sum {serial_s:.3f} s, limit {limit_s:.0f} s)"


@pytest.mark.gpu
def test_mixed_concurrent_calls_equal_solo_calls(G, ctx, one_slot, no_small_net, data, anchor):
    _shared_context_run(G, ctx, no_small_net, data, anchor, ctx is one_slot)


@pytest.mark.gpu
def test_mixed_concurrent_calls_without_coalescing(G, one_slot, no_small_net, data, anchor):
    if _HUNG:
        pytest.fail(f"an earlier test left threads running in the library: {_HUNG}")
    one_slot.set_option(G.OPT_COALESCE, 0)
    try:
        _shared_context_run(G, one_slot, no_small_net, data, anchor, True)
    finally:
        if not _HUNG:
            one_slot.set_option(G.OPT_COALESCE, 1)


# ---- 2. caller buffers: exact capacity, one short, nothing past the end ----
@pytest.mark.gpu
def test_batch_and_lines2_write_exactly_their_arrays(G, ctx, data):
    for mode in (G.MODE_FULL, G.MODE_BIG):
        for fens in (data.b81, data.b4200[:4100]):
            s = raw_batch(G, ctx, fens, mode)
            assert s.rc == 0, s.err
            assert s["out"].bytes() == ctx.evaluate_batch(fens, mode).tobytes()
    s = raw_lines2(G, ctx, data.lines2, 0, K_LINES2)  # 3 chunks per shard on two slots, 5 on one
    assert s.rc == 0, s.err
    out, lines = ctx.evaluate_lines2(data.lines2, K_LINES2, 0)
    assert s["out"].bytes() == out.tobytes() and s["lines"].bytes() == lines.tobytes()
    assert out[12]["flags"] == G.FLAG_BAD_FEN | G.FLAG_NO_SCORE


@pytest.mark.gpu
def test_expand_exact_capacity_and_one_short(G, ctx, data):
    n = len(data.expand)
    gen = raw_expand(G, ctx, data.expand, 0, 64 * n + 256)
    assert gen.rc == 0, gen.err
    need = int(gen["coffs"].a[n])
    assert need > 3 * 81 and gen["coffs"].a[165] == gen["coffs"].a[166]  # (the bad FEN has no children)
    full = {"parents": None, "coffs": None, "cmv": need, "cev": need}
    exact = raw_expand(G, ctx, data.expand, 0, need)
    assert exact.rc == 0, exact.err
    _same(exact, gen, full)
    short = raw_expand(G, ctx, data.expand, 0, need - 1)
    assert short.rc == G.E_CAPACITY and short.err == f"{need} children exceed capacity {need - 1}"
    assert short["coffs"].bytes() == gen["coffs"].bytes()
    again = raw_expand(G, ctx, data.expand, 0, need)
    assert again.rc == 0, again.err
    _same(again, gen, full)


@pytest.mark.gpu
@pytest.mark.parametrize("children", [False, True])
def test_games_exact_capacity_and_one_short(G, ctx, data, children):
    games = data.cap_games
    gen, need_p, need_c = _generous_games(G, ctx, games, children)
    assert need_p == sum(data.npos) and not gen["status"].a.any() and (need_c > 0) == children
    full = {"offs": None, "status": None, "pos": need_p}
    if children:
        full.update(coffs=need_p + 1, cmv=need_c, cev=need_c)
    exact = raw_games(G, ctx, games, 0, children, need_p, need_c)
    assert exact.rc == 0, exact.err
    _same(exact, gen, full)
    if children:
        short = raw_games(G, ctx, games, 0, True, need_p, need_c - 1)
        assert short.rc == G.E_CAPACITY and short.err == f"{need_c} children exceed capacity {need_c - 1}"
        for name in ("offs", "status", "coffs"):
            assert short[name].bytes() == gen[name].bytes(len(short[name].a)), name
    # one position short: the call ends before anything is evaluated or counted
    short = raw_games(G, ctx, games, 0, children, need_p - 1, need_c)
    assert short.rc == G.E_CAPACITY and short.err == f"{need_p} positions exceed capacity {need_p - 1}"
    for name in ("offs", "status"):
        assert short[name].bytes() == gen[name].bytes(), name
    if children:
        assert short["coffs"].untouched()  # (gpu_nnue.h: child_offsets is not written in this case)
    again = raw_games(G, ctx, games, 0, children, need_p, need_c)
    assert again.rc == 0, again.err
    _same(again, gen, full)


@pytest.mark.gpu
def test_games_lines_exact_capacity_and_one_short(G, ctx, data):
    games = data.cap_games
    gen, need_p, _ = _generous_games(G, ctx, games, True, lines=K_LINES)
    full = {"offs": None, "status": None, "pos": need_p, "lines": need_p * K_LINES}
    exact = raw_games_lines(G, ctx, games, 0, K_LINES, need_p)
    assert exact.rc == 0, exact.err
    _same(exact, gen, full)
    short = raw_games_lines(G, ctx, games, 0, K_LINES, need_p - 1)
    assert short.rc == G.E_CAPACITY and short.err == f"{need_p} positions exceed capacity {need_p - 1}"
    for name in ("offs", "status"):
        assert short[name].bytes() == gen[name].bytes(), name
    again = raw_games_lines(G, ctx, games, 0, K_LINES, need_p)
    assert again.rc == 0, again.err
    _same(again, gen, full)


@pytest.mark.gpu
def test_zero_length_calls(G, ctx):
    for mode in (G.MODE_FULL, G.MODE_BIG):
        assert raw_batch(G, ctx, [], mode).rc == 0
        s = raw_expand(G, ctx, [], mode, 0)
        assert s.rc == 0 and list(s["coffs"].a) == [0]
        for children in (False, True):
            s = raw_games(G, ctx, [], mode, children, 0, 0)
            assert s.rc == 0 and list(s["offs"].a) == [0]
            if children:
                assert list(s["coffs"].a) == [0]
        s = raw_games_lines(G, ctx, [], mode, K_LINES, 0)
        assert s.rc == 0 and list(s["offs"].a) == [0]
        assert raw_lines2(G, ctx, [], mode, K_LINES2).rc == 0


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["last_of_first_shard", "first_of_second_shard"])
def test_failing_game_in_the_middle(G, ctx, data, place):
    """A game that fails has no positions and changes nothing of the other games: their records,
    children and lines are those of the call without it, wherever the failing game lies in a
    device's share."""
    def with_failing(g):
        games = data.good[:g] + [FAILING] + data.good[g:]
        w = [len(m.split()) + 1 for _, m, _ in games]
        return games, G.partition(len(games), 2, w)

    want = {"last_of_first_shard": lambda g, b: b[1] - 1 == g, "first_of_second_shard": lambda g, b: b[1] == g}[place]
    at = [g for g in range(1, 8) if want(g, with_failing(g)[1])]
    assert at, "no place for the failing game gives this arrangement on two slots"
    g = at[0]
    games, bounds = with_failing(g)
    assert 0 < bounds[1] < len(games)
    for lines in (0, K_LINES):
        ref, _, _ = _generous_games(G, ctx, data.good, True, lines)
        got, _, _ = _generous_games(G, ctx, games, True, lines)
        assert list(got["status"].a) == [0] * g + [G.E_ILLEGAL_MOVE] + [0] * (8 - g) and got.err == FAILING_ERROR
        assert got["offs"].a[g] == got["offs"].a[g + 1] and got["offs"].a[-1] == ref["offs"].a[-1]
        per = _per_game(got, lines)
        assert per[:g] + per[g + 1:] == _per_game(ref, lines)


# ---- 3. the device replay against the host replay, for every kind of illegal move ----
@pytest.mark.gpu
def test_device_replay_fails_a_game_as_the_host_replay_does(G, ctx):
    for root, moves in ALL_ILLEGAL:
        code, msg = TG._replay_error(G, root, moves)
        assert code == G.E_ILLEGAL_MOVE
        s = raw_games(G, ctx, [(START, TG.OPERA, ()), (root, moves, ()), (START, "e2e4", ())], 0, False, 40)
        assert s.rc == 0 and list(s["status"].a) == [0, code, 0], (root, moves, s.err)
        assert s.err == msg, (root, moves)
        assert list(s["offs"].a) == [0, 34, 34, 36]


@pytest.mark.gpu
def test_nine_illegal_games_among_good_ones(G, ctx, data):
    games, bad = [], []
    for i, (root, moves) in enumerate(NINE_ILLEGAL):
        games += [data.good[i % 8], (root, moves, ())]
        bad.append(2 * i + 1)
    games.append(data.good[1])
    good = [g for i, g in enumerate(games) if i not in bad]
    ref, _, _ = _generous_games(G, ctx, good, True)
    got, _, _ = _generous_games(G, ctx, games, True)
    assert list(got["status"].a) == [G.E_ILLEGAL_MOVE if i in bad else 0 for i in range(len(games))]
    per = _per_game(got)
    assert all(per[i][0] == b"" for i in bad)
    assert [p for i, p in enumerate(per) if i not in bad] == _per_game(ref)
