"""The colour flip F and the file mirror M (tests/symmetry.py) on the GPU.  No oracle judges this
file: a position and its image go through the same call, and the records, node counts, children
and lines must be equal through the move map.  A defect made alike in oracle/oracle.c and in the
kernels (black's rank flip, the side-to-move sign, black's castling or en-passant, the a-d file
mirror of HalfKAv2_hm) passes every parity test and fails here.  tests/test_symmetry.py holds the
same relations for the oracle and the host code: it tells whose defect a failure here is."""
import numpy as np
import pytest

import lines2_history_rule as H2
import lines_rule as R
import symmetry as S

pytestmark = pytest.mark.gpu
MAPS = {"F": (S.flip_fen, S.flip_move), "M": (S.mirror_fen, S.mirror_move)}
FIELDS = ["psqt", "positional", "final_v", "final_cp", "score", "flags"]
NODE_CAP = 2_000_000
N_TWO_PLY = 48   # positions of the two-ply calls: about 45 k grandchildren, as tests/test_gpu_lines_extended.py
N_PERFT_SUM = 60


@pytest.fixture(scope="module")
def G():
    from fishnet_amd import gpu_nnue
    return gpu_nnue


@pytest.fixture(scope="module")
def pairs():
    """{T: (canonical FENs, their images, the move map, the FEN map)}: F on every input, M on those
    without castling rights."""
    fens = S.input_fens()[1]
    out = {}
    for t, (map_fen, map_move) in MAPS.items():
        at = list(range(len(fens))) if t == "F" else S.mirror_subset(fens)
        out[t] = ([fens[i] for i in at], [map_fen(fens[i]) for i in at], map_move, map_fen)
    return out


def test_input_conditions(pairs):
    def king_on_files_a_to_d(fen):
        return any("k" in "".join("." * int(c) if c.isdigit() else c for c in r)[:4].lower()
                   for r in fen.split()[0].split("/"))
    fens, m = pairs["F"][0], pairs["M"][0]
    assert len(fens) >= 200 and len(m) >= 120
    assert sum(1 for f in m if f.split()[3] != "-" or king_on_files_a_to_d(f)) >= 10
    assert sum(1 for f in m if f.split()[3] != "-") >= 2
    assert sum(1 for f in fens if f.split()[1] == "b") >= 40 and sum(1 for f in fens if f.split()[2] != "-") >= 30


def _after(G, fen, *moves):
    """The FEN after the moves, by the library's own replay (host code)."""
    return G.board_to_fen(G.replay_game(fen, [G.move_to_uci(m) for m in moves])[0][-1])


def _same_records(ctx, G, a, b, fens, map_move, mode, exact):
    """gn_eval records of positions and of their images: every field equal, best_move through the
    map.  exact: no best_move may differ; else one may where the two replies tie
    (symmetry.best_move_tie on the children's records), at no more than a tenth of the searched
    positions.  Returns the number of such positions."""
    assert len(a) == len(b) == len(fens)
    fa, fb = a[FIELDS].tolist(), b[FIELDS].tolist()
    for k in [k for k in range(len(fens)) if fa[k] != fb[k]][:5]:
        assert fa[k] == fb[k], fens[k]
    assert fa == fb
    differ = [k for k in range(len(fens)) if map_move(a["best_move"][k]) != int(b["best_move"][k])]
    if exact:
        assert not differ, [(fens[k], int(a["best_move"][k]), int(b["best_move"][k])) for k in differ[:5]]
    for k in differ:
        assert a["best_move"][k] and b["best_move"][k], fens[k]
        kids = [_after(G, fens[k], int(a["best_move"][k])), _after(G, fens[k], map_move(b["best_move"][k]))]
        ca, cb = ctx.evaluate_batch(kids, mode)
        assert S.best_move_tie(ca, cb), (fens[k], kids)
    assert len(differ) <= 0.1 * int((a["flags"] & G.FLAG_SEARCHED != 0).sum())
    return len(differ)


# ---- evaluation ----------------------------------------------------------------------------------

def _evaluate_both_ways(ctx, G, fens, images, mode):
    """((records, the images' records) from one interleaved batch, ... from two batches with
    GN_OPT_FAST_BATCH 0)."""
    both = ctx.evaluate_batch([x for pair in zip(fens, images) for x in pair], mode)
    old = ctx.get_option(G.OPT_FAST_BATCH)
    try:
        ctx.set_option(G.OPT_FAST_BATCH, 0)
        apart = ctx.evaluate_batch(fens, mode), ctx.evaluate_batch(images, mode)
    finally:
        ctx.set_option(G.OPT_FAST_BATCH, old)
    return (both[0::2], both[1::2]), apart


@pytest.mark.parametrize("t", MAPS)
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_evaluation(gpu_ctx, G, pairs, t, mode):
    """F: best_move exact.  M: the reference differs at one position of these inputs, whose two mating
    pawn captures tie (tests/test_symmetry.py::test_oracle_evaluation); only such ties may differ."""
    fens, images, map_move, _ = pairs[t]
    one, apart = _evaluate_both_ways(gpu_ctx, G, fens, images, mode)
    assert one[0].tobytes() == apart[0].tobytes() and one[1].tobytes() == apart[1].tobytes()
    assert (one[0]["flags"] & G.FLAG_SEARCHED != 0).sum() >= 30
    ties = _same_records(gpu_ctx, G, one[0], one[1], fens, map_move, mode, exact=t == "F")
    assert ties <= 1


@pytest.mark.parametrize("t", MAPS)
@pytest.mark.parametrize("l1,seed,mode", [(3072, 11, 1), (128, 7, 2)])
def test_evaluation_on_the_int16_wrap_nets(G, pairs, t, l1, seed, mode):
    from fishnet_amd import synthnet
    path = synthnet.cached_synth_net(l1, seed, stress=True)
    ctx = G.GpuNnue(path, None) if mode == 1 else G.GpuNnue(None, path)
    try:
        fens, images, map_move, _ = pairs[t]
        one, apart = _evaluate_both_ways(ctx, G, fens, images, mode)
        assert one[0].tobytes() == apart[0].tobytes() and one[1].tobytes() == apart[1].tobytes()
        assert _same_records(ctx, G, one[0], one[1], fens, map_move, mode, exact=t == "F") <= 1
    finally:
        ctx.close()


# ---- perft ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", MAPS)
def test_perft(gpu_ctx, pairs, t):
    fens, images, _, _ = pairs[t]
    deep = 0
    for f, g in zip(fens, images):
        for d in (1, 2, 3, 4):
            n = gpu_ctx.perft(f, d)
            assert n == gpu_ctx.perft(g, d), (f, d)
            if n > NODE_CAP:
                break
            deep += d == 4
    assert deep >= 100  # (depth 4 stays within the cap at 210 of the inputs)


# ---- expansion, and the one-ply lines ranked from it --------------------------------------------

def _expand(ctx, G, fens, mode, rank=False):
    """gn_expand_device over the FENs: offsets, moves, child records and child FENs; rank: also
    gn_rank_children_device, gn_extend_checks_device and gn_rank_children_extended_device, K = 8."""
    boards, ok = G.pack_fens(fens)
    assert ok.all()
    n = len(boards)
    cap = 256 * n
    b = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                       ("mv", cap * 2), ("co", cap * G.EVAL_SIZE), ("ln", n * 8 * 12),
                                       ("ext", cap * 4))}
    try:
        b["b"].upload(boards)
        total = ctx.expand_device(b["b"], n, mode, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
        assert total <= cap
        r = {"total": total, "po": b["po"].download(G.EVAL_DTYPE, n), "off": b["off"].download(np.uint32, n + 1),
             "mv": b["mv"].download(np.uint16, total), "co": b["co"].download(G.EVAL_DTYPE, total),
             "ch": G.boards_to_fens(b["ch"].download(G.BOARD_DTYPE, total))}
        if rank:
            ctx.rank_children_device(b["b"], n, b["off"], b["mv"], b["co"], 8, b["ln"])
            ctx.synchronize()
            r["lines"] = b["ln"].download(G.LINE_DTYPE, n * 8).reshape(n, 8)
            r["extended"] = ctx.extend_checks_device(b["b"], n, b["off"], b["mv"], b["co"], total, mode, b["ext"])
            r["ext"] = b["ext"].download(np.int32, total)
            ctx.rank_children_extended_device(b["b"], n, b["off"], b["mv"], b["co"], b["ext"], 8, b["ln"])
            ctx.synchronize()
            r["ext_lines"] = b["ln"].download(G.LINE_DTYPE, n * 8).reshape(n, 8)
    finally:
        for x in b.values():
            x.free()
    return r


def _same_expansion(ctx, G, ra, rb, fens, map_move, map_fen, mode, t):
    assert ra["off"].tolist() == rb["off"].tolist()
    _same_records(ctx, G, ra["po"], rb["po"], fens, map_move, mode, exact=False)
    for i, fen in enumerate(fens):
        lo, hi = int(ra["off"][i]), int(ra["off"][i + 1])
        a = {map_move(m): (tuple(k[FIELDS]), map_move(k["best_move"]), map_fen(c))
             for m, k, c in zip(ra["mv"][lo:hi], ra["co"][lo:hi], ra["ch"][lo:hi])}
        b = {int(m): (tuple(k[FIELDS]), int(k["best_move"]), c)
             for m, k, c in zip(rb["mv"][lo:hi], rb["co"][lo:hi], rb["ch"][lo:hi])}
        assert len(a) == len(b) == hi - lo and a.keys() == b.keys(), fen
        for m in a:
            assert a[m][:2] == b[m][:2], (fen, m)
            # F keeps the parent's fullmove number and black's move advances it: symmetry.without_fullmove
            assert S.without_fullmove(a[m][2]) == S.without_fullmove(b[m][2]), (fen, m)
            assert t == "F" or a[m][2] == b[m][2], (fen, m)


@pytest.fixture(scope="module")
def ranked(gpu_ctx, G, pairs):
    """{T: (mode 0 expansion and one-ply lines of the positions, of their images)}"""
    return {t: (_expand(gpu_ctx, G, pairs[t][0], 0, rank=True), _expand(gpu_ctx, G, pairs[t][1], 0, rank=True))
            for t in MAPS}


@pytest.mark.parametrize("t", MAPS)
@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("options", ("default", "chain 1, king cache 0"))
def test_expansion(gpu_ctx, G, pairs, ranked, t, mode, options):
    fens, images, map_move, map_fen = pairs[t]
    old = gpu_ctx.get_option(G.OPT_CHAIN), gpu_ctx.get_option(G.OPT_KING_CACHE)
    try:
        if options != "default":
            gpu_ctx.set_option(G.OPT_CHAIN, 1)
            gpu_ctx.set_option(G.OPT_KING_CACHE, 0)
        if options == "default" and mode == 0:
            ra, rb = ranked[t]
        else:
            ra, rb = _expand(gpu_ctx, G, fens, mode), _expand(gpu_ctx, G, images, mode)
    finally:
        gpu_ctx.set_option(G.OPT_CHAIN, old[0])
        gpu_ctx.set_option(G.OPT_KING_CACHE, old[1])
    assert ra["total"] >= 3000
    _same_expansion(gpu_ctx, G, ra, rb, fens, map_move, map_fen, mode, t)


def test_perft_is_the_sum_over_the_written_children(gpu_ctx, pairs, ranked):
    """The breadth-first perft and the expansion's child generator, without any reference."""
    fens, r = pairs["F"][0][:N_PERFT_SUM], ranked["F"][0]
    checked = 0
    for i, fen in enumerate(fens):
        kids = r["ch"][int(r["off"][i]):int(r["off"][i + 1])]
        for d in (2, 3):
            n = gpu_ctx.perft(fen, d)
            assert n == sum(gpu_ctx.perft(c, d - 1) for c in kids), (fen, d)
            checked += 1
            if n > NODE_CAP:
                break
    assert checked >= 2 * N_PERFT_SUM - 5


def _share(name, full, live):
    print(f"{name}: {full} of {live} non-empty lines compared in full ({100.0 * full / live:.1f} %)")
    assert full >= 0.7 * live


@pytest.mark.parametrize("t", MAPS)
def test_one_ply_lines(pairs, ranked, t):
    """gn_rank_children_device, gn_extend_checks_device and gn_rank_children_extended_device."""
    fens, _, map_move, _ = pairs[t]
    ra, rb = ranked[t]
    full, live, _ = S.compare_line_tables(ra["lines"], rb["lines"], map_move, fens)
    _share(f"{t} gn_rank_children_device", full, live)
    assert ra["extended"] == rb["extended"] >= 100  # (the rule extends 286 leaves of the inputs, 258 of the M subset)
    for i, fen in enumerate(fens):
        lo, hi = int(ra["off"][i]), int(ra["off"][i + 1])
        assert ({map_move(m): int(e) for m, e in zip(ra["mv"][lo:hi], ra["ext"][lo:hi])}
                == {int(m): int(e) for m, e in zip(rb["mv"][lo:hi], rb["ext"][lo:hi])}), fen
    full, live, at = S.compare_line_tables(ra["ext_lines"], rb["ext_lines"], map_move, fens)
    _share(f"{t} gn_rank_children_extended_device", full, live)
    assert sum(1 for i, j in at if ra["ext_lines"][i, j]["flags"] & 128) >= 1  # a GN_FLAG_SEARCHED line among them


# ---- two-ply lines -------------------------------------------------------------------------------

def _reply_tie(ctx, G, fens, mode=0):
    """compare_line_tables' reply_tie from gn_evaluate_batch_mode on the two grandchildren."""
    def tie(i, move, reply_a, reply_b, flags):
        ga, gb = ctx.evaluate_batch([_after(G, fens[i], move, reply_a), _after(G, fens[i], move, reply_b)], mode)
        return S.replies_tie(ga, gb, flags)
    return tie


@pytest.mark.parametrize("t", MAPS)
@pytest.mark.parametrize("call", ("evaluate_lines2", "evaluate_lines2_extended"))
def test_two_ply_lines(gpu_ctx, G, pairs, t, call):
    fens, images, map_move = pairs[t][0][:N_TWO_PLY], pairs[t][1][:N_TWO_PLY], pairs[t][2]
    pa, la = getattr(gpu_ctx, call)(fens, 8, 0)
    pb, lb = getattr(gpu_ctx, call)(images, 8, 0)
    _same_records(gpu_ctx, G, pa, pb, fens, map_move, 0, exact=False)
    full, live, _ = S.compare_line_tables(la, lb, map_move, fens, _reply_tie(gpu_ctx, G, fens))
    _share(f"{t} gn_{call}", full, live)
    assert (la["plies"] == 2).sum() >= 100


# ---- games (F) -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def games(G):
    """The history fixtures and 16 seeded random games of 80 plies; each with its replayed FENs."""
    gs = H2.both_fixtures() + [(R.START, u, ()) for u in G.random_games_uci(0x5EED5A12, 0, 16, 80)]
    return gs, [S.flip_game(g) for g in gs], [G.boards_to_fens(G.replay_game(*g)[0]) for g in gs]


def test_games(gpu_ctx, G, games):
    gs, flipped, fens = games
    ra = gpu_ctx.evaluate_games(gs, 0, children=True)
    rb = gpu_ctx.evaluate_games(flipped, 0, children=True)
    assert [r["status"] for r in ra] == [r["status"] for r in rb] == [0] * len(gs)
    assert [len(r["evals"]) for r in ra] == [len(r["evals"]) for r in rb] == [len(f) for f in fens]  # position_offsets
    _same_records(gpu_ctx, G, np.concatenate([r["evals"] for r in ra]), np.concatenate([r["evals"] for r in rb]),
                  [f for game in fens for f in game], S.flip_move, 0, exact=False)
    for a, b, f in zip(ra, rb, fens):
        for (ma, ka), (mb, kb), fen in zip(a["children"], b["children"], f):
            assert ({S.flip_move(m): k.tobytes() for m, k in zip(ma, ka)}
                    == {int(m): k.tobytes() for m, k in zip(mb, kb)}), fen
    assert sum(len(m) for r in ra for m, _ in r["children"]) >= 20000


@pytest.mark.parametrize("call", ("evaluate_games_lines_history", "evaluate_games_lines2_history"))
def test_games_history_lines(gpu_ctx, G, games, call):
    gs, flipped, fens = games
    flat = [f for game in fens for f in game]
    oa, sa, pa, la = getattr(gpu_ctx, call)(gs, 8, 0)
    ob, sb, pb, lb = getattr(gpu_ctx, call)(flipped, 8, 0)
    assert oa.tolist() == ob.tolist() and sa.tolist() == sb.tolist() and not sa.any() and len(pa) == len(flat)
    _same_records(gpu_ctx, G, pa, pb, flat, S.flip_move, 0, exact=False)
    full, live, at = S.compare_line_tables(la, lb, S.flip_move, flat, _reply_tie(gpu_ctx, G, flat))
    drawn = sum(1 for i, j in at if la[i, j]["flags"] & G.FLAG_DRAW)
    print(f"F gn_{call}: {full} of {live} non-empty lines compared in full, {drawn} of them drawn by rule")
    # where a line was compared in full its flags were, GN_FLAG_DRAW among them
    assert drawn >= 1
