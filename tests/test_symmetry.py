"""The colour flip F and the file mirror M (tests/symmetry.py) without a GPU: the maps themselves,
and every relation of tests/test_gpu_symmetry.py that the CPU oracle and the library's host code
can express.  No oracle judges these tests: a position and its image must give the same records,
node counts, keys and lines.  Where the GPU test fails and this file passes, the kernel is wrong;
where both fail, the oracle and the library share the defect."""
import numpy as np
import pytest

import history_rule as H
import lines2_history_rule as H2
import lines2_rule as R2
import lines_extended_rule as X
import lines_rule as R
import symmetry as S

AFTER_E4 = "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq e3 0 1"
C960_1 = "bqnb1rkr/pp3ppp/3ppn2/2p5/5P2/P2P4/NPP1P1PP/BQ1BNRKR w HFhf - 2 9"
EN_PASSANT = "8/8/8/8/k2Pp2Q/8/8/3K4 b - d3 0 1"
TWO_MATING_CAPTURES = "5rB1/1n6/2p5/p1bb4/P4pkp/6R1/3N3K/5R2 b - - 3 93"  # of score_fens.json: f4g3# and h4g3#
MAPS = {"F": (S.flip_fen, S.flip_move), "M": (S.mirror_fen, S.mirror_move)}
FIELDS = ["psqt", "positional", "final_v", "final_cp", "score", "flags"]
N_LINES1, N_LINES2 = None, 48  # positions whose one-ply (all) / two-ply lines the Python rules rank here


@pytest.fixture(scope="module")
def G():
    from fishnet_amd import build, gpu_nnue
    build.build()
    return gpu_nnue


@pytest.fixture(scope="module")
def inputs(G):
    return S.input_fens()


@pytest.fixture(scope="module")
def pairs(inputs):
    """{T: (indices, canonical FENs, their images, the move map)}"""
    fens = inputs[1]
    out = {}
    for t, (map_fen, map_move) in MAPS.items():
        at = list(range(len(fens))) if t == "F" else S.mirror_subset(fens)
        out[t] = (at, [fens[i] for i in at], [map_fen(fens[i]) for i in at], map_move)
    return out


# ---- the maps ------------------------------------------------------------------------------------

def test_hand_written_pairs(G):
    assert S.flip_fen(AFTER_E4) == "rnbqkbnr/pppp1ppp/8/4p3/8/8/PPPPPPPP/RNBQKBNR w KQkq e6 0 1"
    assert S.flip_fen(C960_1) == "bq1bnrkr/npp1p1pp/p2p4/5p2/2P5/3PPN2/PP3PPP/BQNB1RKR b HFhf - 2 9"
    assert S.flip_fen(EN_PASSANT) == "3k4/8/8/K2pP2q/8/8/8/8 w - d6 0 1"
    assert S.mirror_fen(EN_PASSANT) == "8/8/8/8/Q2pP2k/8/8/4K3 b - e3 0 1"
    assert S.flip_fen("4k2r/8/8/8/8/8/8/R3K3 w Qk - 5 9") == "r3k3/8/8/8/8/8/8/4K2R b Kq - 5 9"  # white's letters first
    with pytest.raises(ValueError):
        S.mirror_fen(AFTER_E4)
    e2e4, e7e5, d2d4 = R2.uci_move("e2e4"), R2.uci_move("e7e5"), R2.uci_move("d2d4")
    assert (S.flip_move(e2e4), S.mirror_move(e2e4)) == (e7e5, d2d4)
    a7a8q = 1 << 14 | 3 << 12 | R2.uci_move("a7a8")
    assert S.flip_move(a7a8q) == 1 << 14 | 3 << 12 | R2.uci_move("a2a1")
    assert S.mirror_move(a7a8q) == 1 << 14 | 3 << 12 | R2.uci_move("h7h8")
    assert S.flip_move(0) == S.mirror_move(0) == 0
    assert [S.flip_uci(u) for u in ("e2e4", "e1g1", "a7a8q", "h2h1n")] == ["e7e5", "e8g8", "a2a1q", "h7h8n"]
    assert [S.mirror_uci(u) for u in ("e2e4", "a7a8q", "h2h1n")] == ["d2d4", "h7h8q", "a2a1n"]
    assert S.flip_game((AFTER_E4, "e7e5 g1f3", (1,))) == (S.flip_fen(AFTER_E4), "e2e4 g8f6", (1,))
    assert S.flip_game((AFTER_E4, ["e7e5"], ()))[1] == ["e2e4"]
    assert all(G.move_to_uci(t(m)) == u(G.move_to_uci(m)) for m in (e2e4, a7a8q, 3 << 14 | R2.uci_move("e1h1"))
               for t, u in ((S.flip_move, S.flip_uci), (S.mirror_move, S.mirror_uci)))


def test_the_maps_are_involutions(inputs, oracle_lib):
    raw, fens = inputs
    for f in fens + raw:
        assert S.flip_fen(S.flip_fen(f)) == f
    for i in S.mirror_subset(fens):
        assert S.mirror_fen(S.mirror_fen(fens[i])) == fens[i]
        assert S.flip_fen(S.mirror_fen(fens[i])) == S.mirror_fen(S.flip_fen(fens[i]))
    for f in fens[:40]:
        for m in oracle_lib.legal_moves(f):
            assert S.flip_move(S.flip_move(m)) == m == S.mirror_move(S.mirror_move(m))
            u = oracle_lib.move_to_uci(m)
            assert S.flip_uci(S.flip_uci(u)) == u == S.mirror_uci(S.mirror_uci(u))
    for g in H2.both_fixtures():
        assert S.flip_game(S.flip_game(g)) == g


def test_input_conditions(inputs):
    """What the GPU test asserts of the same inputs: the M subset and what it holds."""
    fens = inputs[1]
    at = S.mirror_subset(fens)

    def king_on_files_a_to_d(fen):
        return any("k" in "".join("." * int(c) if c.isdigit() else c for c in r)[:4].lower()
                   for r in fen.split()[0].split("/"))
    assert len(fens) >= 200 and len(at) >= 120
    assert sum(1 for i in at if fens[i].split()[3] != "-" or king_on_files_a_to_d(fens[i])) >= 10
    assert sum(1 for i in at if fens[i].split()[3] != "-") >= 2
    assert sum(1 for f in fens if f.split()[1] == "b") >= 40 and sum(1 for f in fens if f.split()[2] != "-") >= 30


def test_parser_and_printer_commute_with_the_flip(G, inputs, oracle_lib):
    """gn_pack_fens / gn_board_to_fen and the oracle's normalisation: the canonical form of F(raw)
    is F of the canonical form (castling letters, the en-passant gate, either side to move)."""
    raw, fens = inputs
    flipped = [S.flip_fen(r) for r in raw]
    boards, ok = G.pack_fens(flipped)
    assert ok.all()
    assert G.boards_to_fens(boards) == [S.flip_fen(f) for f in fens]
    assert [oracle_lib.normalize_fen(r) for r in flipped] == [S.flip_fen(oracle_lib.normalize_fen(r)) for r in raw]
    at = S.mirror_subset(fens)
    mirrored = [S.mirror_fen(fens[i]) for i in at]
    boards, ok = G.pack_fens(mirrored)
    assert ok.all() and G.boards_to_fens(boards) == mirrored == [oracle_lib.normalize_fen(m) for m in mirrored]


# ---- the oracle ----------------------------------------------------------------------------------

@pytest.mark.parametrize("t", MAPS)
@pytest.mark.parametrize("nets,mode", [("synthetic", 0), ("synthetic", 1), ("synthetic", 2), ("int16 wrap", 1),
                                       ("int16 wrap", 2)])
def test_oracle_evaluation(oracle_lib, oracle_nets, pairs, t, nets, mode):
    big, small = oracle_nets
    if nets == "int16 wrap":  # the stress nets of tests/test_gpu_parity.py
        from fishnet_amd import synthnet
        big = oracle_lib.Net(synthnet.cached_synth_net(3072, 11, stress=True)) if mode == 1 else None
        small = oracle_lib.Net(synthnet.cached_synth_net(128, 7, stress=True)) if mode == 2 else None
    _, fens, images, map_move = pairs[t]
    a = oracle_lib.eval_fens(big, small, fens, mode, threads=8)
    b = oracle_lib.eval_fens(big, small, images, mode, threads=8)
    assert a[FIELDS].tolist() == b[FIELDS].tolist()
    searched = int((a["flags"] & oracle_lib.FLAG_SEARCHED != 0).sum())
    assert searched >= 30 and ((a["best_move"] != 0) == (a["flags"] & oracle_lib.FLAG_SEARCHED != 0)).all()
    # best_move: equal through the move map, but for replies that tie (symmetry.best_move_tie).  On
    # these inputs the oracle differs nowhere under F and at one position under M, whose two pawn
    # captures f4g3 and h4g3 both mate: the smaller encoding is chosen, and M swaps their order.
    differ = [k for k in range(len(fens)) if map_move(a["best_move"][k]) != int(b["best_move"][k])]
    assert differ == ([] if t == "F" else [fens.index(TWO_MATING_CAPTURES)])
    for k in differ:
        kids = [oracle_lib.child_fen(fens[k], m) for m in (int(a["best_move"][k]), map_move(b["best_move"][k]))]
        ca, cb = oracle_lib.eval_fens(big, small, kids, mode)
        assert S.best_move_tie(ca, cb), fens[k]
    assert len(differ) <= 0.1 * searched


@pytest.mark.parametrize("t", MAPS)
def test_oracle_moves_children_and_perft(oracle_lib, pairs, t):
    _, fens, images, map_move = pairs[t]
    map_fen = MAPS[t][0]
    for f, g in zip(fens, images):
        moves = oracle_lib.legal_moves(f)
        assert {map_move(m) for m in moves} == set(oracle_lib.legal_moves(g)), f
        assert len(moves) == 0 or 0 not in moves
        for m in moves:
            got, want = oracle_lib.child_fen(g, map_move(m)), map_fen(oracle_lib.child_fen(f, m))
            assert S.without_fullmove(got) == S.without_fullmove(want), (f, m)
            if t == "M":
                assert got == want, (f, m)
        for d in (1, 2, 3):
            assert oracle_lib.perft(f, d) == oracle_lib.perft(g, d), (f, d)


@pytest.mark.parametrize("t", MAPS)
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_oracle_expansion(oracle_lib, oracle_nets, pairs, t, mode):
    """Per parent, {mapped move: child record}; a child record carries no best_move."""
    big, small = oracle_nets
    _, fens, images, map_move = pairs[t]
    for f, g in zip(fens[:100], images[:100]):
        pa, ma, ka = oracle_lib.expand_eval(big, small, f, mode)
        pb, mb, kb = oracle_lib.expand_eval(big, small, g, mode)
        assert pa[:6] == pb[:6] and not ka["best_move"].any() and not kb["best_move"].any()
        assert {map_move(m): k.tobytes() for m, k in zip(ma, ka)} == {m: k.tobytes() for m, k in zip(mb, kb)}, f


def test_oracle_replays_a_flipped_game(oracle_lib):
    for g in H2.both_fixtures():
        fens, played = oracle_lib.replay_game(g[0], g[1])
        f_fens, f_played = oracle_lib.replay_game(*S.flip_game(g)[:2])
        assert [S.without_fullmove(f) for f in f_fens] == [S.without_fullmove(S.flip_fen(f)) for f in fens]
        assert f_played == [S.flip_move(m) for m in played]


def _share(name, full, live):
    print(f"{name}: {full} of {live} non-empty lines compared in full ({100.0 * full / live:.1f} %)")
    assert full >= 0.7 * live
    return full


def _reply_tie(O, big, small, fens, mode=0):
    """compare_line_tables' reply_tie from the oracle's records of the two grandchildren."""
    def tie(i, move, reply_a, reply_b, flags):
        c = O.child_fen(fens[i], move)
        ga, gb = O.eval_fens(big, small, [O.child_fen(c, reply_a), O.child_fen(c, reply_b)], mode)
        return S.replies_tie(ga, gb, flags)
    return tie


@pytest.mark.parametrize("t", MAPS)
def test_oracle_ranked_lines(oracle_lib, oracle_nets, pairs, t):
    """The four Python rules over the oracle, K = 8, mode 0, through compare_lines."""
    big, small = oracle_nets
    _, fens, images, map_move = pairs[t]
    for name, rule, n in (("lines", R.lines, N_LINES1), ("extended lines", X.lines, N_LINES1),
                          ("lines2", R2.lines2, N_LINES2), ("extended lines2", X.lines2, N_LINES2)):
        a = rule(oracle_lib, big, small, fens[:n], 0, 8)
        b = rule(oracle_lib, big, small, images[:n], 0, 8)
        full, live, _ = S.compare_line_tables(a, b, map_move, fens, _reply_tie(oracle_lib, big, small, fens))
        _share(f"{t} {name}", full, live)


def test_oracle_history_lines_of_flipped_games(oracle_lib, oracle_nets):
    big, small = oracle_nets
    full = live = drawn = 0
    for g in H2.both_fixtures():
        fens = oracle_lib.replay_game(g[0], g[1])[0]
        images = [S.flip_fen(f) for f in fens]
        for rule in (H.game_lines, H2.game_lines2):
            a = rule(oracle_lib, big, small, fens, g[2], 0, 8)
            b = rule(oracle_lib, big, small, images, g[2], 0, 8)
            f, n, at = S.compare_line_tables(a, b, S.flip_move, fens, _reply_tie(oracle_lib, big, small, fens))
            full, live = full + f, live + n
            drawn += sum(1 for i, j in at if a[i, j]["flags"] & H2.FLAG_DRAW)
    # (no share is asked of the games: the fixtures shuffle pieces in endgames where many values tie)
    print(f"F history lines: {full} of {live} non-empty lines compared in full, {drawn} of them drawn")
    assert drawn >= 1


# ---- the library's host code ---------------------------------------------------------------------

def test_position_keys_of_flipped_games(G):
    """gn_position_keys: two positions of a game have equal keys exactly when their images have."""
    pairs_equal = 0
    for g in H2.both_fixtures():
        boards = G.replay_game(*g)[0]
        images = G.replay_game(*S.flip_game(g))[0]
        ka, kb = G.position_keys(boards), G.position_keys(images)
        assert ka.all() and kb.all()
        ea, eb = ka[:, None] == ka[None, :], kb[:, None] == kb[None, :]
        assert np.array_equal(ea, eb)
        pairs_equal += int(ea.sum() - len(ka)) // 2
    assert pairs_equal >= 10  # the fixtures repeat positions


def test_replay_of_a_flipped_game(G):
    """gn_replay_game: F of the game gives F of every board and of every played move."""
    games = H2.both_fixtures() + [(R.START, u, ()) for u in G.random_games_uci(0x5EED5A12, 0, 16, 80)]
    castled = promoted = 0
    for g in games:
        boards, skipped, moves = G.replay_game(*g)
        f_boards, f_skipped, f_moves = G.replay_game(*S.flip_game(g))
        assert ([S.without_fullmove(f) for f in G.boards_to_fens(f_boards)]
                == [S.without_fullmove(S.flip_fen(f)) for f in G.boards_to_fens(boards)])
        assert f_moves.tolist() == [S.flip_move(m) for m in moves] and f_skipped.tolist() == skipped.tolist()
        castled += int((moves >> 14 == 3).sum())
        promoted += int((moves >> 14 == 1).sum())
    assert castled >= 1 and promoted >= 1
