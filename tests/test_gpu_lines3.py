"""Three-ply ranked lines (include/gpu_nnue.h at gn_line3) on the GPU: gn_rank_lines3_device on
made-up child lines against the numpy root step (tests/lines3_rule.py); the device chain
gn_expand_device -> gn_expand2_device + gn_rank_lines2_device over the children -> gn_rank_lines3_device,
gn_evaluate_lines3 and gn_evaluate_games_lines3 against the rule restated from the CPU oracle; every PV
replayed without the rule; the library against itself on a wider seeded set; the same bytes from every
chunk size, pipeline setting and shard count; the argument checks, the statistics, and the existing
calls' bytes around a three-ply call.

The inputs are tests/golden/lines3_fens.txt's sets (tests/test_lines3.py checks on the CPU that they
hold every segment shape, searched lines with and without tails, and values the pruning changes)."""
import ctypes as C

import numpy as np
import pytest

import lines2_rule as R2
import lines3_rule as L3
import lines_rule as R

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
MODES = (0, 1)  # FULL, BIG
SENTINEL16 = 0x5A5A
# (leaf, depth, GN_OPT_QUIESCE_SEE, the set's section)
CONFIGS = {"static": (L3.LEAF_STATIC, 0, False, "static"), "checks": (L3.LEAF_CHECKS, 0, False, "static"),
           "q1": (L3.LEAF_QUIESCE, 1, False, "quiesce1"), "q2": (L3.LEAF_QUIESCE, 2, False, "quiesce2"),
           "q1see": (L3.LEAF_QUIESCE, 1, True, "quiesce2")}
ROOTS9 = (L3.MOVES_218, L3.PLY1_ENDS, L3.MATE_IN_2, L3.MATED_IN_2, L3.BAD_FEN, L3.MATED,
          "rnbqkbnr/ppppp1pp/8/5p1Q/4P3/8/PPPP1PPP/RNB1KBNR b KQkq - 1 2",
          "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1", R.START)


class _At:
    """A device pointer `nbytes` into a DeviceBuffer."""

    def __init__(self, buf, nbytes):
        self.ptr = C.c_void_p(buf.addr + nbytes)


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _fens(section):
    return L3.static_fens() if section == "static" else L3.quiesce_fens(1 if section == "quiesce1" else 2)


def _diff(got, exp, fens, what):
    for i in np.flatnonzero((got != exp).any(axis=1))[:5]:
        assert got[i].tolist() == exp[i].tolist(), (fens[i], what)
    assert got.tobytes() == exp.tobytes()


@pytest.fixture(scope="module")
def expected(oracle_lib, oracle_nets):
    """rule(name, mode) -> (lines[n, 8], pvs[n, 8]) of the configuration's set, computed once each."""
    big, small = oracle_nets
    memo = {}

    def rule(name, mode=0):
        if (name, mode) not in memo:
            leaf, depth, pruned, section = CONFIGS[name]
            memo[(name, mode)] = L3.lines3(oracle_lib, big, small, _fens(section), leaf, depth, mode, 8, pruned)
        return memo[(name, mode)]
    return rule


@pytest.fixture(scope="module")
def see_ctx(synth_big_path, synth_small_path):
    from fishnet_amd import gpu_nnue as G
    ctx = G.GpuNnue(synth_big_path, synth_small_path)
    ctx.set_option(G.OPT_QUIESCE_SEE, 1)
    yield ctx
    ctx.close()


def _ctx_of(name, gpu_ctx, see_ctx):
    return see_ctx if CONFIGS[name][2] else gpu_ctx


# ---- the root step on made-up child lines -------------------------------------------------------

def _expand(ctx, boards, mode=0):
    """gn_expand_device of the boards: (buffers, total, offsets, moves, child flags)."""
    from fishnet_amd import gpu_nnue as G
    n, cap = len(boards), 256 * len(boards)
    b = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                       ("mv", cap * 2), ("co", cap * G.EVAL_SIZE))}
    b["b"].upload(boards)
    total = ctx.expand_device(b["b"], n, mode, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
    return b, total, b["off"].download(np.uint32, n + 1), b["mv"].download(np.uint16, total), \
        b["co"].download(G.EVAL_DTYPE, total)["flags"]


def _rank3(ctx, b, n, total, clines, cpvs, K, with_pvs, n_alloc=None):
    """gn_rank_lines3_device with its outputs inside allocations of sentinels, one entry on either
    side: (lines[n, K], pvs[n, K] or None); nothing around them may change."""
    from fishnet_amd import gpu_nnue as G
    n_alloc = len(clines) if n_alloc is None else n_alloc
    d_cl, d_cp = ctx.alloc(max(n_alloc, 1) * 16), ctx.alloc(max(n_alloc, 1) * 16)
    d_cl.upload(clines[:n_alloc]), d_cp.upload(cpvs[:n_alloc])
    d_ln, d_pv = ctx.alloc((n * K + 2) * 20), ctx.alloc((n * K + 2) * 16)
    d_ln.upload(np.full((n * K + 2) * 10, SENTINEL16, dtype=np.uint16))
    d_pv.upload(np.full((n * K + 2) * 8, SENTINEL16, dtype=np.uint16))
    ctx.rank_lines3_device(b["b"], n, b["off"], b["mv"], b["co"], total, d_cl, d_cp if with_pvs else None, K,
                           _At(d_ln, 20), _At(d_pv, 16) if with_pvs else None)
    ctx.synchronize()
    raw, praw = d_ln.download(np.uint16, (n * K + 2) * 10), d_pv.download(np.uint16, (n * K + 2) * 8)
    for x in (d_cl, d_cp, d_ln, d_pv):
        x.free()
    assert (raw[:10] == SENTINEL16).all() and (raw[10 + n * K * 10:] == SENTINEL16).all()
    assert (praw[:8] == SENTINEL16).all() and (praw[8 + n * K * 8:] == SENTINEL16).all()
    if not with_pvs:
        assert (praw == SENTINEL16).all()
    return raw[10:10 + n * K * 10].view(G.LINE3_DTYPE).reshape(n, K), \
        (praw[8:8 + n * K * 8].view(G.PV_DTYPE).reshape(n, K) if with_pvs else None)


def _made_up(kind, fens, off, mv, oracle_lib):
    """Hand-made child lines and PVs: an empty line exactly where the child has no legal move."""
    from fishnet_amd import gpu_nnue as G
    total = len(mv)
    rng = np.random.default_rng(0x5EED77E5)
    cl, cp = np.zeros(total, dtype=G.LINE2_DTYPE), np.zeros(total, dtype=G.PV_DTYPE)
    if kind == "equal":
        values = np.full(total, 77)
    elif kind == "mates":
        values = rng.choice([31999, 31997, 31995, -31998, -31996, 31753, -31753, 0, 250], total)
    else:
        values = rng.integers(-3000, 3000, total)
    for i, fen in enumerate(fens):
        for j in range(int(off[i]), int(off[i + 1])):
            if not oracle_lib.legal_moves(oracle_lib.child_fen(fen, int(mv[j]))):
                cl[j] = R2.EMPTY2
                continue
            plies = 1 if j % 5 == 0 else 2
            fl = (R.FLAG_NO_MOVES if plies == 1 else int(rng.choice([0, L3.FLAG_SEARCHED]))) | int(rng.choice([0, R.FLAG_IN_CHECK, R.FLAG_MATE]))
            reply, reply2 = 100 + j % 4000, (0 if plies == 1 else 200 + j % 3000)
            cl[j] = (int(values[j]), 0, reply, reply2, fl, plies)
            tail = [300 + j % 7 + k for k in range(int(rng.integers(0, 4)))] if fl & L3.FLAG_SEARCHED else []
            cp[j] = L3._pv([reply, reply2][:plies] + tail)
    return cl, cp


@pytest.fixture(scope="module")
def roots9(gpu_ctx):
    from fishnet_amd import gpu_nnue as G
    boards = G.pack_fens(list(ROOTS9))[0]
    b, total, off, mv, flags = _expand(gpu_ctx, boards)
    yield b, total, off, mv, flags
    for x in b.values():
        x.free()


@pytest.mark.parametrize("kind", ("equal", "mates", "random"))
@pytest.mark.parametrize("n", (1, 9))
def test_root_step_on_made_up_child_lines(gpu_ctx, roots9, oracle_lib, kind, n):
    """K = 1, 3, 8, with and without PVs, for one root (218 children: seven passes of its group) and for
    nine (a root count that does not fill a workgroup)."""
    b, total, off, mv, flags = roots9
    fens = list(ROOTS9)
    cl, cp = _made_up(kind, fens, off, mv, oracle_lib)
    assert int(off[1]) == 218 and ((cl["flags"][:218] & R.FLAG_NO_SCORE) != 0).sum() == 182
    P = oracle_lib.eval_params()
    materials = [R.wdl_material(f, P) if off[i + 1] > off[i] else 0 for i, f in enumerate(fens)]
    for K in KS:
        for with_pvs in (True, False):
            got, gpv = _rank3(gpu_ctx, b, n, total, cl, cp, K, with_pvs)
            exp, epv = L3.root_step(P, materials[:n], off[:n + 1], mv, flags, cl, cp if with_pvs else None, K)
            _diff(got, exp, fens, (kind, n, K))
            if with_pvs:
                _diff(gpv, epv, fens, (kind, n, K, "pvs"))
    if kind == "equal" and n == 9:  # the last root's children all have a move and tie: the order is the moves'
        got, _ = _rank3(gpu_ctx, b, n, total, cl, cp, 8, False)
        assert (got[-1]["value"] == -77).all() and (np.diff(got[-1]["move"].astype(int)) > 0).all()


def test_root_step_reads_nothing_beyond_total(gpu_ctx, roots9, oracle_lib):
    """total cuts inside the last root's children: the child arrays hold exactly `cut` entries, and the
    lines are those of offsets clamped to it; with total 0 every line is empty and no input is read."""
    from fishnet_amd import gpu_nnue as G
    b, total, off, mv, flags = roots9
    fens = list(ROOTS9)
    cl, cp = _made_up("random", fens, off, mv, oracle_lib)
    P = oracle_lib.eval_params()
    materials = [R.wdl_material(f, P) if off[i + 1] > off[i] else 0 for i, f in enumerate(fens)]
    for cut in (int(off[8]) + 3, int(off[7]) + 1, 100):
        got, gpv = _rank3(gpu_ctx, b, 9, cut, cl, cp, 8, True, n_alloc=cut)
        exp, epv = L3.root_step(P, materials, off, mv, flags, cl[:cut], cp[:cut], 8, total=cut)
        _diff(got, exp, fens, cut), _diff(gpv, epv, fens, cut)
    d_ln = gpu_ctx.alloc(9 * 3 * 20)
    d_ln.upload(np.full(9 * 3 * 10, SENTINEL16, dtype=np.uint16))
    gpu_ctx.rank_lines3_device(None, 9, None, None, None, 0, None, None, 3, d_ln)
    gpu_ctx.synchronize()
    empty = d_ln.download(G.LINE3_DTYPE, 27)
    d_ln.free()
    assert all(tuple(x) == L3.EMPTY3 for x in empty.tolist())
    gpu_ctx.rank_lines3_device(None, 0, None, None, None, 0, None, None, 3, None)


# ---- the device chain ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_device_chain_vs_rule(gpu_ctx, expected, mode):
    """gn_expand_device, the children as parents through gn_expand2_device + gn_rank_lines2_device at
    K = 1 (+ gn_line2_pvs_device), then gn_rank_lines3_device."""
    from fishnet_amd import gpu_nnue as G
    from test_gpu_parity import _expand2
    ctx = gpu_ctx
    fens = L3.static_fens()
    boards = G.pack_fens(fens)[0]
    n = len(boards)
    b, total, off, mv, flags = _expand(ctx, boards, mode)
    t, g, out = _expand2(ctx, b["ch"], total, mode)
    assert t > total and g > t
    d_cl, d_cp = ctx.alloc(total * 16), ctx.alloc(total * 16)
    ctx.rank_lines2_device(b["ch"], total, out, 1, d_cl)
    ctx.line2_pvs_device(total, out, None, d_cl, 1, d_cp)
    exp, epv = expected("static", mode)
    d_ln, d_pv = ctx.alloc(n * 8 * 20), ctx.alloc(n * 8 * 16)
    for K in KS:
        ctx.rank_lines3_device(b["b"], n, b["off"], b["mv"], b["co"], total, d_cl, d_cp, K, d_ln, d_pv)
        ctx.synchronize()
        _diff(d_ln.download(G.LINE3_DTYPE, n * K).reshape(n, K), exp[:, :K], fens, (mode, K))
        _diff(d_pv.download(G.PV_DTYPE, n * K).reshape(n, K), epv[:, :K], fens, (mode, K, "pvs"))
    for x in list(b.values()) + list(out.values()) + [d_cl, d_cp, d_ln, d_pv]:
        if hasattr(x, "free"):
            x.free()


SIBLINGS = ("k7/8/2K5/8/8/8/7Q/8 b - - 1 1", "k7/2K5/8/8/8/8/7Q/8 b - - 1 1")


@pytest.mark.parametrize("mode", MODES)
def test_expand2_over_siblings_whose_children_meet(gpu_ctx, oracle_lib, oracle_nets, mode):
    """Two siblings as parents of gn_expand2_device: the only child of the second, 8/k1K5/8/8/8/8/7Q/8 w,
    has the placement of a child of the first one's only child (c6c7) with the same side to move.  As
    consecutive parents of level 2 the two are not a game's consecutive positions: the chained walk must
    not link them, and the depth-2 consistency check must pass with the oracle's values."""
    from fishnet_amd import gpu_nnue as G
    from test_gpu_parity import _expand2
    big, small = oracle_nets
    boards = G.pack_fens(list(SIBLINGS))[0]
    d_b = gpu_ctx.alloc(2 * 32)
    d_b.upload(boards)
    t, g, out = _expand2(gpu_ctx, d_b, 2, mode)
    assert t == 2
    kids = G.boards_to_fens(out["ch"].download(G.BOARD_DTYPE, t))
    assert kids[1].startswith("8/k1K5/8/8/8/8/7Q/8 w") and oracle_lib.child_fen(kids[0], R2.uci_move("c6c7")).split()[0] == kids[1].split()[0]
    got = out["co"].download(G.EVAL_DTYPE, t)
    exp = oracle_lib.eval_fens(big, small, kids, mode)
    for f in ("psqt", "positional", "final_v", "final_cp"):
        assert got[f].tolist() == exp[f].tolist(), f
    for x in list(out.values()) + [d_b]:
        if hasattr(x, "free"):
            x.free()


# ---- gn_evaluate_lines3 -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_got(gpu_ctx, see_ctx):
    """got(name, mode) -> (out, lines[n, 8], pvs[n, 8]) of gn_evaluate_lines3 on the configuration's set."""
    memo = {}

    def got(name, mode=0):
        if (name, mode) not in memo:
            leaf, depth, _, section = CONFIGS[name]
            memo[(name, mode)] = _ctx_of(name, gpu_ctx, see_ctx).evaluate_lines3(_fens(section), 8, leaf, depth, mode)
        return memo[(name, mode)]
    return got


@pytest.mark.parametrize("name", list(CONFIGS))
def test_evaluate_lines3_vs_rule(gpu_ctx, see_ctx, host_got, expected, name):
    from fishnet_amd import gpu_nnue as G
    leaf, depth, _, section = CONFIGS[name]
    fens = _fens(section)
    ctx = _ctx_of(name, gpu_ctx, see_ctx)
    exp, epv = expected(name)
    out, lines, pvs = host_got(name)
    assert lines.dtype == G.LINE3_DTYPE and lines.shape == (len(fens), 8)
    _diff(lines, exp, fens, name), _diff(pvs, epv, fens, (name, "pvs"))
    assert out.tobytes() == ctx.evaluate_lines2(fens, 8, 0)[0].tobytes()
    for K in (1, 3):
        o, l, p = ctx.evaluate_lines3(fens, K, leaf, depth, 0)
        assert o.tobytes() == out.tobytes()
        _diff(l, exp[:, :K], fens, (name, K)), _diff(p, epv[:, :K], fens, (name, K, "pvs"))
    o, l, p = ctx.evaluate_lines3(fens, 3, leaf, depth, 0, pvs=False)
    assert p is None and l.tobytes() == exp[:, :3].tobytes()
    if leaf == L3.LEAF_QUIESCE:
        assert (lines["flags"] & L3.FLAG_SEARCHED).any() and int(pvs["len"].max()) > 3


def test_evaluate_lines3_mode_big(host_got, expected):
    fens = L3.quiesce_fens(1)
    _diff(host_got("q1", 1)[1], expected("q1", 1)[0], fens, "BIG")
    _diff(host_got("q1", 1)[2], expected("q1", 1)[1], fens, "BIG pvs")


def test_known_answers(host_got):
    from fishnet_amd import gpu_nnue as G
    fens = L3.static_fens()
    out, lines, pvs = host_got("static")
    a, b = lines[fens.index(L3.MATE_IN_2)][:2]
    mv = R2.uci_move
    assert a.tolist() == (31997, 2, mv("b5b7"), mv("e8d8"), mv("a6a8"), G.FLAG_MATE, 3, 0)
    assert b.tolist() == (31997, 2, mv("a6a7"), mv("e8d8"), mv("b5b8"), G.FLAG_MATE, 3, 0)
    d = lines[fens.index(L3.MATED_IN_2)]
    assert d[0].tolist() == (-31998, -1, mv("e8d8"), mv("a6a8"), 0, G.FLAG_MATE | G.FLAG_NO_MOVES, 2, 0)
    assert d[1]["reply"] == mv("a6a8") and d[1]["plies"] == 2 and d[2].tolist() == L3.EMPTY3
    q = host_got("q1")[1][0][0]
    assert (int(q["value"]), int(q["score"]), int(q["plies"])) == (-31996, -2, 3) and int(q["flags"]) & G.FLAG_MATE
    for i in (fens.index(L3.BAD_FEN), fens.index(L3.MATED)):
        assert all(x == L3.EMPTY3 for x in lines[i].tolist()) and not pvs[i].view(np.uint16).any()
    assert int(out["flags"][fens.index(L3.BAD_FEN)]) & G.FLAG_BAD_FEN


# ---- oracle-free: every PV replayed -------------------------------------------------------------

@pytest.mark.parametrize("name,mode", [(n, 0) for n in CONFIGS] + [("q1", 1)])
def test_pvs_replayed_without_the_rule(gpu_ctx, host_got, oracle_lib, name, mode):
    """Every PV played out with the oracle's child_fen alone: each move legal where it is played, and the
    end position's own value -- mate, stalemate, else the static final_v of gn_evaluate_batch_mode --
    carried back by negate_ply once per move is the line's value.  (A line the check extension valued
    ends above the extension's own replies, which are not reported: its moves are checked, not its value.)"""
    from fishnet_amd import gpu_nnue as G
    O = oracle_lib
    leaf, depth, _, section = CONFIGS[name]
    fens = _fens(section)
    _, lines, pvs = host_got(name, mode)
    ends, items = [], []
    for i, fen in enumerate(fens):
        for ln, pv in zip(lines[i], pvs[i]):
            k = int(pv["len"])
            if not k:
                assert int(ln["flags"]) & G.FLAG_NO_SCORE
                continue
            f = fen
            for m in pv["moves"][:k].tolist():
                assert m in O.legal_moves(f), (fen, pv)
                f = O.child_fen(f, m)
            assert not pv["moves"][k:].any() and not pv["reserved"] and not ln["reserved"]
            assert pv["moves"][:int(ln["plies"])].tolist() == [int(ln["move"]), int(ln["reply"]), int(ln["reply2"])][:int(ln["plies"])]
            assert k == int(ln["plies"]) or (leaf == L3.LEAF_QUIESCE and int(ln["plies"]) == 3 and int(ln["flags"]) & G.FLAG_SEARCHED)
            if not (leaf == L3.LEAF_CHECKS and int(ln["flags"]) & G.FLAG_SEARCHED):
                items.append((fen, ln, k, len(ends)))
                ends.append(f)
    rec = gpu_ctx.evaluate_batch(ends, mode)
    for fen, ln, k, e in items:
        if int(rec["flags"][e]) & G.FLAG_NO_MOVES:
            v = -R.VALUE_MATE if int(rec["flags"][e]) & G.FLAG_IN_CHECK else 0
        else:
            v = int(rec["final_v"][e])
        for _ in range(k):
            v = R.negate_ply(v)
        assert v == int(ln["value"]), (fen, ln, k, ends[e])
    assert len(items) >= 10


# ---- the library against itself on a wider set --------------------------------------------------

@pytest.mark.parametrize("name", ("static", "q1"))
def test_wide_vs_two_ply_calls_over_the_children(gpu_ctx, oracle_lib, name):
    """48 seeded positions: every root's lines composed on the host (the numpy root step) from
    gn_evaluate_lines2 / gn_evaluate_lines2_quiescent_pv at K = 1 over its children's FENs."""
    from fishnet_amd import gpu_nnue as G
    ctx = gpu_ctx
    leaf, depth = CONFIGS[name][:2]
    boards = G.random_positions(L3.SEED, 0, L3.N_WIDE, 160)
    fens = G.boards_to_fens(boards)
    n = len(boards)
    b, total, off, mv, flags = _expand(ctx, boards)
    kids = G.boards_to_fens(b["ch"].download(G.BOARD_DTYPE, total))
    for x in b.values():
        x.free()
    clen = np.diff(off.astype(np.int64))
    assert total > 20 * n and (clen > 32).any() and (clen < 32).any()
    if leaf == L3.LEAF_STATIC:
        _, cl = ctx.evaluate_lines2(kids, 1, 0)
        cl = cl[:, 0]
        cp = np.zeros(total, dtype=G.PV_DTYPE)
        for j in range(total):
            cp[j] = L3._pv([int(cl[j]["move"]), int(cl[j]["reply"])][:int(cl[j]["plies"])])
    else:
        _, cl, cp = ctx.evaluate_lines2_quiescent_pv(kids, 1, depth, 0)
        cl, cp = cl[:, 0], cp[:, 0]
    P = oracle_lib.eval_params()
    materials = [R.wdl_material(f, P) for f in fens]
    exp, epv = L3.root_step(P, materials, off, mv, flags, cl, cp, 8)
    out, lines, pvs = ctx.evaluate_lines3(fens, 8, leaf, depth, 0)
    _diff(lines, exp, fens, name), _diff(pvs, epv, fens, (name, "pvs"))
    assert (lines["plies"] == 3).sum() > 6 * n
    if leaf == L3.LEAF_QUIESCE:
        assert (pvs["len"] == 4).sum() >= 5 and (lines["flags"] & G.FLAG_SEARCHED).sum() >= 20


# ---- the same bytes from every path -------------------------------------------------------------

@pytest.mark.parametrize("name", ("static", "q1"))
def test_same_bytes_from_every_path(gpu_ctx, host_got, synth_big_path, synth_small_path, name):
    """GN_OPT_CHUNK_PARENTS 1, 7 (a cut inside one root's children) and the default, GN_OPT_EXPAND_PIPELINE
    0 and 2, and a two-shard context."""
    from fishnet_amd import gpu_nnue as G
    leaf, depth, _, section = CONFIGS[name]
    fens = _fens(section)
    base = host_got(name)
    others = []
    try:
        for pipeline, chunk in ((2, 1), (2, 7), (0, 7), (0, 0)):
            gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, pipeline)
            gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, chunk)
            others.append(gpu_ctx.evaluate_lines3(fens, 8, leaf, depth, 0))
            assert gpu_ctx.get_option(G.STAT_RANK3_NS) > 0
    finally:
        gpu_ctx.set_option(G.OPT_EXPAND_PIPELINE, 2)
        gpu_ctx.set_option(G.OPT_CHUNK_PARENTS, 0)
    two = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    try:
        others.append(two.evaluate_lines3(fens, 8, leaf, depth, 0))
        two.set_option(G.OPT_CHUNK_PARENTS, 7)
        others.append(two.evaluate_lines3(fens, 8, leaf, depth, 0))
    finally:
        two.close()
    for o in others:
        assert _same(base, o)


# ---- the games call -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def games():
    """Single positions, a game with moves and a skipped position, and a game that fails."""
    return [(f, "", ()) for f in L3.quiesce_fens(1)[:4]] + \
        [(L3.MATE_IN_2, "b5b7 e8d8 a6a8", (1,)), (R.START, "e2e5", ()), (L3.PLY1_ENDS, "h2h1 a8b8", ())]


@pytest.mark.parametrize("name", ("static", "q1"))
def test_games_call(gpu_ctx, games, oracle_lib, oracle_nets, name):
    from fishnet_amd import gpu_nnue as G
    import guarded_buffers as GB
    big, small = oracle_nets
    leaf, depth = CONFIGS[name][:2]
    K = 3
    offs, status, pos, lines, pvs = gpu_ctx.evaluate_games_lines3(games, K, leaf, depth, 0)
    assert gpu_ctx.get_option(G.STAT_RANK3_NS) > 0
    two = gpu_ctx.evaluate_games_lines2(games, K, 0)
    assert gpu_ctx.get_option(G.STAT_RANK3_NS) == 0
    assert _same((offs, status, pos), two[:3])
    assert status.tolist() == [0, 0, 0, 0, 0, G.E_ILLEGAL_MOVE, 0] and offs[6] == offs[5]  # the failed game has no positions
    fens, skip = [], set()
    for gi, (root, moves, sk) in enumerate(games):
        if status[gi]:
            continue
        fs = oracle_lib.replay_game(root, moves)[0]
        skip |= {len(fens) + k for k in sk}
        fens += fs
    assert len(fens) == len(pos) == int(offs[-1]) and len(skip) == 1
    exp, epv = L3.lines3(oracle_lib, big, small, fens, leaf, depth, 0, K, skip=skip)
    _diff(lines, exp, fens, name), _diff(pvs, epv, fens, (name, "pvs"))
    s = next(iter(skip))
    assert int(pos["flags"][s]) & G.FLAG_SKIPPED and all(x == L3.EMPTY3 for x in lines[s].tolist()) and not pvs[s].view(np.uint16).any()
    # equal to the FEN call on the replayed positions
    keep = [i for i in range(len(fens)) if i not in skip]
    fo, fl, fp = gpu_ctx.evaluate_lines3([fens[i] for i in keep], K, leaf, depth, 0)
    assert fl.tobytes() == lines[keep].tobytes() and fp.tobytes() == pvs[keep].tobytes() and fo.tobytes() == pos[keep].tobytes()
    # outputs of exactly the sizes told, and one position too few
    L = G.lib()
    garr, _keep = G._games_array(games)
    ng, p = len(games), len(pos)
    g = GB.GuardedSet()
    rc = L.gn_evaluate_games_lines3(gpu_ctx.h, garr, ng, 0, K, leaf, depth, g.add("offs", ng + 1, np.uint32),
                                    g.add("status", ng, np.int32), g.add("pos", p, G.EVAL_DTYPE), p,
                                    g.add("lines", p * K, G.LINE3_DTYPE), g.add("pvs", p * K, G.PV_DTYPE))
    assert rc == 0
    g.check()
    assert (g["offs"].bytes(), g["status"].bytes(), g["pos"].bytes(), g["lines"].bytes(), g["pvs"].bytes()) == \
        (offs.tobytes(), status.tobytes(), pos.tobytes(), lines.tobytes(), pvs.tobytes())
    g = GB.GuardedSet()
    rc = L.gn_evaluate_games_lines3(gpu_ctx.h, garr, ng, 0, K, leaf, depth, g.add("offs", ng + 1, np.uint32),
                                    g.add("status", ng, np.int32), g.add("pos", p - 1, G.EVAL_DTYPE), p - 1,
                                    g.add("lines", (p - 1) * K, G.LINE3_DTYPE), g.add("pvs", (p - 1) * K, G.PV_DTYPE))
    assert rc == G.E_CAPACITY
    g.check()
    assert g["offs"].bytes() == offs.tobytes() and g["pos"].untouched() and g["lines"].untouched() and g["pvs"].untouched()
    # without PVs; and without the game that skips a position (every shard in place, nothing gathered)
    o2 = gpu_ctx.evaluate_games_lines3(games, K, leaf, depth, 0, pvs=False)
    assert o2[4] is None and _same(o2[:4], (offs, status, pos, lines))
    o3 = gpu_ctx.evaluate_games_lines3(games[:4] + games[6:], K, leaf, depth, 0)
    rows = list(range(int(offs[4]))) + list(range(int(offs[6]), int(offs[7])))
    assert o3[3].tobytes() == lines[rows].tobytes() and o3[4].tobytes() == pvs[rows].tobytes()


def test_exact_size_fen_call_outputs(gpu_ctx, host_got):
    import guarded_buffers as GB
    from fishnet_amd import gpu_nnue as G
    fens = L3.quiesce_fens(1)
    farr, _keep = G._fen_array(fens)
    want = gpu_ctx.evaluate_lines3(fens, 3, L3.LEAF_QUIESCE, 1, 0)
    g = GB.GuardedSet()
    rc = G.lib().gn_evaluate_lines3(gpu_ctx.h, farr, len(fens), 0, 3, L3.LEAF_QUIESCE, 1, g.add("out", len(fens), G.EVAL_DTYPE),
                                    g.add("lines", len(fens) * 3, G.LINE3_DTYPE), g.add("pvs", len(fens) * 3, G.PV_DTYPE))
    assert rc == 0
    g.check()
    assert (g["out"].bytes(), g["lines"].bytes(), g["pvs"].bytes()) == tuple(x.tobytes() for x in want)


# ---- errors, statistics, and the existing calls -------------------------------------------------

def test_argument_checks(gpu_ctx, games):
    """Every GN_E_INVALID of the three calls; after each failure a valid call on the same context succeeds."""
    from fishnet_amd import gpu_nnue as G
    L = G.lib()
    ctx = gpu_ctx
    want = ctx.evaluate_lines3([L3.MATED_IN_2], 3)

    def still_works():
        assert _same(ctx.evaluate_lines3([L3.MATED_IN_2], 3), want)

    def invalid(f):
        with pytest.raises(G.GnError) as e:
            f()
        assert e.value.code == G.E_INVALID
        still_works()

    d = ctx.alloc(4096)
    for k in (0, 9):
        invalid(lambda: ctx.evaluate_lines3([R.START], k))
        invalid(lambda: ctx.evaluate_games_lines3(games[:2], k))
        invalid(lambda: ctx.rank_lines3_device(d, 1, d, d, d, 1, d, d, k, d, d))
    for leaf, depth in ((-1, 0), (3, 0), (L3.LEAF_QUIESCE, 0), (L3.LEAF_QUIESCE, 4), (L3.LEAF_STATIC, 1), (L3.LEAF_CHECKS, 2)):
        invalid(lambda: ctx.evaluate_lines3([R.START], 3, leaf, depth))
        invalid(lambda: ctx.evaluate_games_lines3(games[:2], 3, leaf, depth))
    # NULL lines with positions
    farr, _keep = G._fen_array([R.START])
    out = np.zeros(1, dtype=G.EVAL_DTYPE)
    assert L.gn_evaluate_lines3(ctx.h, farr, 1, 0, 3, 0, 0, out.ctypes.data, None, None) == G.E_INVALID
    still_works()
    garr, _keep2 = G._games_array(games[:2])
    offs, status, pos = np.zeros(3, dtype=np.uint32), np.zeros(2, dtype=np.int32), np.zeros(64, dtype=G.EVAL_DTYPE)
    assert L.gn_evaluate_games_lines3(ctx.h, garr, 2, 0, 3, 0, 0, offs.ctypes.data, status.ctypes.data, pos.ctypes.data, 64,
                                      None, None) == G.E_INVALID
    still_works()
    # the device call: d_pvs without d_child_pvs, NULL buffers
    invalid(lambda: ctx.rank_lines3_device(d, 1, d, d, d, 1, d, None, 3, d, d))
    invalid(lambda: ctx.rank_lines3_device(d, 1, d, d, d, 1, d, None, 3, None))
    invalid(lambda: ctx.rank_lines3_device(d, 1, d, d, d, 1, None, None, 3, d))
    invalid(lambda: ctx.rank_lines3_device(None, 1, d, d, d, 1, d, None, 3, d))
    d.free()
    # nothing to do
    out, lines, pvs = ctx.evaluate_lines3([], 3)
    assert len(out) == 0 and lines.shape == pvs.shape == (0, 3)
    offs, status, pos, lines, pvs = ctx.evaluate_games_lines3([], 3)
    assert list(offs) == [0] and len(pos) == 0 and len(lines) == 0


def test_stats(gpu_ctx):
    from fishnet_amd import gpu_nnue as G
    fens = L3.quiesce_fens(1)
    gpu_ctx.evaluate_lines3(fens, 3, L3.LEAF_QUIESCE, 1, 0)
    st = {k: gpu_ctx.get_option(getattr(G, k)) for k in ("STAT_RANK3_NS", "STAT_RANK2_NS", "STAT_QUIESCE_NS",
                                                           "STAT_QUIESCE_LEAVES", "STAT_PV_NS", "STAT_EXTEND_NS")}
    assert st["STAT_RANK3_NS"] > 0 and st["STAT_RANK2_NS"] > 0 and st["STAT_QUIESCE_NS"] > 0 and st["STAT_QUIESCE_LEAVES"] > 0
    assert st["STAT_PV_NS"] > 0 and st["STAT_EXTEND_NS"] == 0
    assert gpu_ctx.host_stages()["total"] > 0 and gpu_ctx.host_stages()["compute"] > 0
    gpu_ctx.evaluate_lines3(fens, 3, L3.LEAF_CHECKS, 0, 0, pvs=False)
    assert gpu_ctx.get_option(G.STAT_EXTEND_NS) > 0 and gpu_ctx.get_option(G.STAT_QUIESCE_NS) == 0
    assert gpu_ctx.get_option(G.STAT_RANK3_NS) > 0
    gpu_ctx.evaluate_lines2(fens, 3, 0)
    assert gpu_ctx.get_option(G.STAT_RANK3_NS) == 0 and gpu_ctx.get_option(G.STAT_RANK2_NS) > 0


def test_existing_calls_untouched(gpu_ctx):
    """gn_evaluate_lines2_quiescent_pv gives the same bytes before and after a three-ply call."""
    from fishnet_amd import gpu_nnue as G
    fens = L3.quiesce_fens(1) + [R.START]
    before = gpu_ctx.evaluate_lines2_quiescent_pv(fens, 8, 2, 0)
    games = [(f, "", ()) for f in fens[:3]]
    gbefore = gpu_ctx.evaluate_games_lines2(games, 3, 0)
    gpu_ctx.evaluate_lines3(fens, 8, L3.LEAF_QUIESCE, 1, 0)
    gpu_ctx.evaluate_lines3(fens, 3, L3.LEAF_CHECKS, 0, 0)
    assert _same(before, gpu_ctx.evaluate_lines2_quiescent_pv(fens, 8, 2, 0))
    assert _same(gbefore, gpu_ctx.evaluate_games_lines2(games, 3, 0))
