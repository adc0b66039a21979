"""Lichess analysis batches: root FEN + UCI moves + skipPositions -> positions
(IncomingBatch::from_acquired, /root/reference/src/queue.rs:548-700) -> evaluations.

CPU tests check the library's host replay (gn_replay_game needs no GPU) against
public known answers and against the oracle's restatement of shakmaty 0.27.3's
UciMove::to_move; the GPU tests check gn_evaluate_games against the oracle.
The reference's own replay (shakmaty) is a Rust crate absent from the container,
so the move-resolution rule is "parity unpinned" beyond the known answers below.
"""
import random

import numpy as np
import pytest

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
# Morphy - Duke of Brunswick & Count Isouard, Paris 1858 ("Opera game"); the final
# position is a public known answer.
OPERA = ("e2e4 e7e5 g1f3 d7d6 d2d4 c8g4 d4e5 g4f3 d1f3 d6e5 f1c4 g8f6 f3b3 d8e7 b1c3 c7c6 c1g5 b7b5 "
         "c3b5 c6b5 c4b5 b8d7 e1c1 a8d8 d1d7 d8d7 h1d1 e7e6 b5d7 f6d7 b3b8 d7b8 d1d8")
OPERA_FINAL = "1n1Rkb1r/p4ppp/4q3/4p1B1/4P3/8/PPP2PPP/2K5 b k - 1 17"
C960 = "bqnb1rkr/pp3ppp/3ppn2/2p5/5P2/P2P4/NPP1P1PP/BQ1BNRKR w HFhf - 2 9"
# rooks on b and g: "e1g1" is castling (king onto a castling-rights rook), "e1c1" is not
C960_CASTLE = "1r2k1r1/pppppppp/8/8/8/8/PPPPPPPP/1R2K1R1 w GBgb - 0 1"


@pytest.fixture(scope="module")
def G():
    from fishnet_amd import build, gpu_nnue
    build.build()
    return gpu_nnue


def fens_of(G, boards):
    return [G.board_to_fen(b) for b in boards]


def test_opera_game_known_answer(G, oracle_lib):
    boards, skipped, moves = G.replay_game(START, OPERA, skip=[0, 3, 33])
    assert len(boards) == 34 and len(moves) == 33
    assert G.board_to_fen(boards[-1]) == OPERA_FINAL
    assert G.board_to_fen(boards[1]) == "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1"
    assert [int(i) for i in np.nonzero(skipped)[0]] == [0, 3, 33]
    # the Chess960 UCI the reference forwards to the engine (queue.rs:577): O-O-O = king takes rook
    assert G.move_to_uci(int(moves[22])) == "e1a1"
    fens, played = oracle_lib.replay_game(START, OPERA)
    assert fens_of(G, boards) == fens and [int(m) for m in moves] == played


def test_castling_notations_agree(G):
    pre = "e2e4 e7e5 g1f3 b8c6 f1c4 g8f6 "
    a = G.replay_game(START, pre + "e1g1")
    b = G.replay_game(START, pre + "e1h1")
    assert fens_of(G, a[0]) == fens_of(G, b[0]) and list(a[2]) == list(b[2])
    assert G.board_to_fen(a[0][-1]).startswith("r1bqkb1r/pppp1ppp/2n2n2/4p3/2B1P3/5N2/PPPP1PPP/RNBQ1RK1 b kq")


@pytest.mark.parametrize("moves,bad", [
    ("e2e4 e7e5 e1g1", 3),          # standard castling notation without the right to castle
    ("e2e5", 1),                    # not a legal pawn move
    ("e2e4 0000", 2),               # null move: UciMove::Null never resolves
    ("e2e4 e7e5 d1h5 e8e7 h5e8", 5),  # a queen cannot take the king (not a legal move)
    ("e2e4 e7e5 g1f3 k9a1", 4),     # malformed
    ("e2e4 e7e5 e2e4", 3),          # empty from-square
    ("e2e4 d7d5 e4d5 e7e5 d5e6q", 5),  # promotion letter on a non-promoting move
    ("e2e4 e7e5 g1f3 g8f6 f1e2 f8e7 e1g1 e8g8 g1h1 g8h8 f1g1k", 11),  # promotion letter k
    ("C960 e1c1", 1),               # standard O-O-O notation needs the a-rook
])
def test_illegal_moves_fail_the_game(G, moves, bad):
    root = START
    if moves.startswith("C960 "):
        root, moves = C960_CASTLE, moves[5:]
    with pytest.raises(G.GnError) as e:
        G.replay_game(root, moves)
    assert e.value.code == G.E_ILLEGAL_MOVE and f"move {bad} " in str(e.value)


def test_bad_root_and_empty_game(G):
    with pytest.raises(G.GnError) as e:
        G.replay_game("8/8/8/8/8/8/8/8 w - - 0 1", "")
    assert e.value.code == G.E_INVALID
    boards, skipped, moves = G.replay_game(C960, "", skip=[5])  # out-of-range skip index is ignored
    assert len(boards) == 1 and len(moves) == 0 and not skipped.any()


def test_en_passant_promotion_and_chess960(G, oracle_lib):
    games = [
        (START, "e2e4 a7a6 e4e5 d7d5 e5d6 c7d6 g2g4 h7h5 g4h5 g7g5 h5g6 a6a5 g6g7 a5a4 g7h8n"),
        (START, "b2b4 a7a5 b4a5 b7b5 a5b6 c7c5 b6b7 c5c4 b7a8r c4c3 a8b8 d8a5 b8c8 a5d8"),
        (C960, "e2e4 e6e5 g2g3 f6e4"),
        (C960_CASTLE, "e1g1 e8b8"),               # king takes its own rook: O-O then O-O-O
        (C960_CASTLE, "e1b1 e8g8"),
        ("r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", "e1c1 e8g8"),
        ("r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", "e1a1 e8h8"),
    ]
    for root, moves in games:
        boards, _, played = G.replay_game(root, moves)
        fens, exp = oracle_lib.replay_game(root, moves)
        assert fens_of(G, boards) == fens, (root, moves)
        assert [int(m) for m in played] == exp


def _random_game(oracle_lib, rng, root, plies):
    """Random legal line from the oracle; castling written in either notation."""
    fen, out = oracle_lib.normalize_fen(root), []
    for _ in range(plies):
        ms = oracle_lib.legal_moves(fen)
        if not ms:
            break
        m = rng.choice(ms)
        u = oracle_lib.move_to_uci(m)
        frm, to = (m >> 6) & 63, m & 63
        if m >> 14 == 3 and frm in (4, 60) and to % 8 in (0, 7) and rng.random() < 0.5:
            u = u[:2] + ("c" if to % 8 == 0 else "g") + u[3]  # standard notation
        out.append(u)
        fen = oracle_lib.child_fen(fen, m)
    return " ".join(out)


def test_random_games_match_oracle(G, oracle_lib):
    rng = random.Random(1234)
    roots = [START, C960, "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"]
    for g in range(60):
        root = roots[g % 3]
        moves = _random_game(oracle_lib, rng, root, 60)
        boards, _, played = G.replay_game(root, moves)
        fens, exp = oracle_lib.replay_game(root, moves)
        assert fens_of(G, boards) == fens and [int(m) for m in played] == exp


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_evaluate_games_vs_oracle(gpu_ctx, oracle_nets, oracle_lib, mode):
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    rng = random.Random(99 + mode)
    games = [(START, OPERA, [0, 7]), (C960, _random_game(oracle_lib, rng, C960, 40), []),
             (START, "e2e4 e7e5 e1g1", []),  # fails: illegal move
             (START, "", [0]),                # everything skipped
             (START, _random_game(oracle_lib, rng, START, 80), list(range(0, 81, 5)))]
    out = gpu_ctx.evaluate_games(games, mode)
    assert [o["status"] for o in out] == [0, 0, G.E_ILLEGAL_MOVE, 0, 0]
    for (root, moves, skip), o in zip(games, out):
        if o["status"]:
            assert len(o["evals"]) == 0
            continue
        fens, _ = oracle_lib.replay_game(root, moves)
        exp = oracle_lib.eval_fens(big, small, fens, mode)
        got = o["evals"]
        for i in range(len(fens)):
            if i in skip:
                assert tuple(got[i]) == (0, 0, 0, 0, 0, G.FLAG_SKIPPED | G.FLAG_NO_SCORE, 0)
            else:
                assert tuple(got[i]) == tuple(exp[i]), (fens[i], got[i], exp[i])


@pytest.mark.gpu
def test_evaluate_games_with_children_vs_oracle(gpu_ctx, oracle_nets, oracle_lib):
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    rng = random.Random(5)
    many = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"  # 218 legal moves: multi-pass plan
    games = [(START, OPERA, [1, 2]), (C960, _random_game(oracle_lib, rng, C960, 30), [30]),
             (many, _random_game(oracle_lib, rng, many, 12), [])]
    out = gpu_ctx.evaluate_games(games, 0, children=True)
    for (root, moves, skip), o in zip(games, out):
        assert o["status"] == 0
        fens, _ = oracle_lib.replay_game(root, moves)
        for i, fen in enumerate(fens):
            cm, ce = o["children"][i]
            if i in skip:
                assert len(cm) == 0
                continue
            p_exp, m_exp, k_exp = oracle_lib.expand_eval(big, small, fen, 0)
            assert tuple(o["evals"][i]) == tuple(p_exp)
            assert dict(zip(cm.tolist(), map(tuple, ce.tolist()))) == \
                dict(zip(m_exp, map(tuple, G.children_from_evals(k_exp).tolist())))


# games whose lines run into check, checkmate and stalemate
FOOLS_MATE = "f2f3 e7e5 g2g4 d8h4"
LOYD_STALEMATE = "e2e3 a7a5 d1h5 a8a6 h5a5 h7h5 h2h4 a6h6 a5c7 f7f6 c7d7 e8f7 d7b7 d8d3 b7b8 d3h7 b8c8 f7g6 c8e6"


def uci_score(G, rec):
    """The score GpuEvalStub posts for a record (rust/fishnet-gpu/src/gpu_eval_stub.rs): None
    only for a record without one (skipped / bad position)."""
    if rec["flags"] & G.FLAG_NO_SCORE:
        return None
    return ("mate" if rec["flags"] & G.FLAG_MATE else "cp", int(rec["score"]))


@pytest.mark.gpu
@pytest.mark.parametrize("children", [False, True])
def test_every_game_position_scored(gpu_ctx, oracle_nets, oracle_lib, children):
    """a8: every non-skipped position of a lichess batch gets the score fishnet
    posts, checkmate -> mate 0, stalemate -> cp 0, checks by the in-check rule; equal to the
    oracle's records, with and without children."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    rng = random.Random(2024)
    games = [(START, FOOLS_MATE, []), (START, OPERA, [5]), (START, LOYD_STALEMATE, [0]),
             (START, _random_game(oracle_lib, rng, START, 120), [])]
    out = gpu_ctx.evaluate_games(games, 0, children=children)
    seen = set()
    for (root, moves, skip), o in zip(games, out):
        assert o["status"] == 0
        fens, _ = oracle_lib.replay_game(root, moves)
        exp = oracle_lib.eval_fens(big, small, fens, 0)
        for i, fen in enumerate(fens):
            got = o["evals"][i]
            if i in skip:
                assert uci_score(G, got) is None
                continue
            assert tuple(got) == tuple(exp[i]), fen
            s = uci_score(G, got)
            assert s is not None, fen
            if got["flags"] & G.FLAG_NO_MOVES:
                seen.add("mate0" if s == ("mate", 0) else "stalemate" if s == ("cp", 0) else "?")
            elif got["flags"] & G.FLAG_IN_CHECK:
                assert got["flags"] & G.FLAG_SEARCHED and got["best_move"]
                seen.add("check")
    assert seen == {"mate0", "stalemate", "check"}


def test_random_games_uci_replay(G, oracle_lib):
    """gn_random_games_uci: the bench's games in the lichess wire form (standard castling
    notation) replay legally, through the library's host replay and the oracle's."""
    ucis = G.random_games_uci(0x5EED0003, 0, 24, 80)
    assert len(ucis) == 24 and all(ucis)
    for u in ucis:
        boards, _, played = G.replay_game(START, u)
        fens, exp = oracle_lib.replay_game(START, u)
        assert fens_of(G, boards) == fens and [int(m) for m in played] == exp
        assert len(boards) == len(u.split()) + 1


@pytest.mark.gpu
def test_gpu_replay_equals_device_games_and_host_replay(gpu_ctx, oracle_lib):
    """gn_evaluate_games replays the moves on the GPU (replay_games_kernel): its positions are
    the ones gn_random_games_device plays for the same seeds (full-length games), and the host
    replay's (gn_replay_game) for all; a game with an illegal move fails with its message."""
    from fishnet_amd import gpu_nnue as G
    n, plies, seed = 64, 80, 0x5EED0003
    ucis = G.random_games_uci(seed, 0, n, plies)
    games = [(START, u, []) for u in ucis] + [(START, "e2e4 e7e5 e1g1", [])]
    arr, keep = G._games_array(games)
    offs, status, pos, coffs, cmv, cev, _ = gpu_ctx.evaluate_games_arrays(arr, len(games), 1, children=True)
    assert list(status[:n]) == [0] * n and status[n] == G.E_ILLEGAL_MOVE
    assert "move 3 (e1g1) is not legal" in (G.lib().gn_last_error() or b"").decode()
    d_b = gpu_ctx.alloc(n * (plies + 1) * 32)
    gpu_ctx.random_games_device(seed, 0, n, plies, d_b)
    gpu_ctx.synchronize()
    dev = d_b.download(G.BOARD_DTYPE, n * (plies + 1)).reshape(n, plies + 1)
    full = [g for g in range(n) if offs[g + 1] - offs[g] == plies + 1]
    assert len(full) > n // 2
    sel = np.concatenate([dev[g] for g in full])
    m, cap = len(sel), int(60 * len(sel))
    bufs = {k: gpu_ctx.alloc(sz) for k, sz in (("b", m * 32), ("po", m * G.EVAL_SIZE), ("off", (m + 1) * 4),
                                                  ("ch", cap * 32), ("mv", cap * 2), ("co", cap * G.EVAL_SIZE))}
    bufs["b"].upload(sel)
    t = gpu_ctx.expand_device(bufs["b"], m, 1, bufs["po"], bufs["off"], bufs["ch"], bufs["mv"], bufs["co"], cap)
    po, doff = bufs["po"].download(G.EVAL_DTYPE, m), bufs["off"].download(np.uint32, m + 1)
    dmv, dco = bufs["mv"].download(np.uint16, t), G.children_from_evals(bufs["co"].download(G.EVAL_DTYPE, t))
    cev = G.decode_children(cev)
    i = 0
    for g in full:
        for k in range(plies + 1):
            at = int(offs[g]) + k
            assert pos[at] == po[i], (g, k)
            a, b = int(coffs[at]), int(coffs[at + 1])
            c, d = int(doff[i]), int(doff[i + 1])
            assert np.array_equal(cmv[a:b], dmv[c:d]) and np.array_equal(cev[a:b], dco[c:d]), (g, k)
            i += 1
    for g in range(0, n, 7):  # the host replay
        boards, _, _ = G.replay_game(START, ucis[g])
        got = gpu_ctx.evaluate_batch([G.board_to_fen(b) for b in boards], 1)
        assert np.array_equal(got, pos[int(offs[g]):int(offs[g + 1])]), g


@pytest.mark.gpu
def test_king_walk_games_vs_oracle(gpu_ctx, oracle_nets, oracle_lib):
    """Games in which most children are king moves: kings alone (every child refreshes the
    mover's perspective from the king cache), and kings with both rooks and castling rights.
    A parent then has more than four king-move jobs, so the plan takes its second job path
    (PSQT rows loaded four jobs at a time, the job rows recomputed in the job loop), and
    castling children skip the cache; every position and child vs the oracle."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    rng = random.Random(11)
    roots = ["8/8/3k4/8/8/4K3/8/8 w - - 0 1", "r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1",
             "8/2k5/8/8/8/8/5K2/8 b - - 0 1"]
    games = [(r, _random_game(oracle_lib, rng, r, 40), []) for r in roots]
    out = gpu_ctx.evaluate_games(games, 0, children=True)
    most = 0  # most children of a kings-only parent (every child there a king move)
    for g, ((root, moves, _), o) in enumerate(zip(games, out)):
        assert o["status"] == 0
        fens, _ = oracle_lib.replay_game(root, moves)
        for i, fen in enumerate(fens):
            cm, ce = o["children"][i]
            p_exp, m_exp, k_exp = oracle_lib.expand_eval(big, small, fen, 0)
            assert tuple(o["evals"][i]) == tuple(p_exp), fen
            assert dict(zip(cm.tolist(), map(tuple, ce.tolist()))) == \
                dict(zip(m_exp, map(tuple, G.children_from_evals(k_exp).tolist()))), fen
            if g == 0:
                most = max(most, len(cm))
    assert most > 4  # (a parent with more than four king-move jobs)


# (root, moves) of test_chained_links_of_special_moves_vs_oracle; the castling games from index
# CASTLING_GAMES_FROM on (tests/test_gpu_plan_replay.py replays their plans)
SPECIAL_MOVE_GAMES = [(START, "e2e4 a7a6 e4e5 d7d5 e5d6 c7d6 g2g4 h7h5 g4h5 g7g5 h5g6 a6a5 g6g7 a5a4 g7h8n"),
                      (START, "b2b4 a7a5 b4a5 b7b5 a5b6 c7c5 b6b7 c5c4 b7a8r c4c3 a8b8 d8a5 b8c8 a5d8"),
                      ("8/P6k/8/8/8/8/p6K/8 w - - 0 1", "a7a8b a2a1n a8b7 a1b3"),
                      (C960_CASTLE, "e1g1 e8b8"), (C960_CASTLE, "e1b1 e8g8"),
                      ("6kr/8/8/8/8/8/8/6KR w Hh - 0 1", "g1h1 g8h8"),       # the king stays
                      ("k7/8/8/8/8/8/8/4KR2 w F - 0 1", "e1f1 a8b8"),        # the rook stays
                      ("k7/8/8/8/8/8/8/5KR1 w G - 0 1", "f1g1 a8a7"),        # king and rook swap
                      ("r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", "e1c1 e8g8"),
                      ("r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", "e1a1 e8h8")]
CASTLING_GAMES_FROM = 3


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [-81, -2])
def test_chained_links_of_special_moves_vs_oracle(gpu_ctx, oracle_nets, oracle_lib, chain):
    """The chained walk's link -- the child of position i whose placement is position i + 1's,
    found in child_moves_kernel from the squares the two placements differ on -- across every
    move kind: under-promotions with and without capture (four children change the same
    squares), en passant, castling in both notations, and Chess960 castling where the king
    stays, where the rook stays and where king and rook swap squares.  Exact chain lengths
    (GN_OPT_CHAIN < 0): one chain over whole games, and pairs; every position and child vs
    the oracle (a wrong link starts the next position from the wrong accumulators)."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    games = SPECIAL_MOVE_GAMES
    gpu_ctx.set_option(G.OPT_CHAIN, chain)
    try:
        out = gpu_ctx.evaluate_games([(r, m, []) for r, m in games], 0, children=True)
    finally:
        gpu_ctx.set_option(G.OPT_CHAIN, 81)
    for (root, moves), o in zip(games, out):
        assert o["status"] == 0, (root, moves)
        fens, _ = oracle_lib.replay_game(root, moves)
        for i, fen in enumerate(fens):
            cm, ce = o["children"][i]
            p_exp, m_exp, k_exp = oracle_lib.expand_eval(big, small, fen, 0)
            assert tuple(o["evals"][i]) == tuple(p_exp), fen
            assert dict(zip(cm.tolist(), map(tuple, ce.tolist()))) == \
                dict(zip(m_exp, map(tuple, G.children_from_evals(k_exp).tolist()))), fen


# ---- the move string's tokens (whitespace-separated; tabs, CR LF and runs of spaces included) ----
LONG_TOKEN = "e2e4 e2e4e2e4e2e4e2e4e2e4"  # move 2: 24 characters, 16 of them in the message
PROMO_ROOT = "8/4P2k/8/8/8/8/8/K7 w - - 0 1"  # e7e8q is legal here
# (root, moves) of games that fail at a token longer than a move
LONG_TOKEN_GAMES = ((START, LONG_TOKEN), (PROMO_ROOT, "e7e8qq"), (PROMO_ROOT, "e7e8q  h7g7\te7e8qqq"))


def _mixed_whitespace(moves):
    seps = ["\t", "\r\n", "   ", " \t ", "\n", "\r", " "]
    return " \t" + "".join(t + seps[i % len(seps)] for i, t in enumerate(moves.split())) + "\r\n "


def _replay_error(G, root, moves):
    """(code, gn_last_error's message) of a game gn_replay_game fails."""
    with pytest.raises(G.GnError) as e:
        G.replay_game(root, moves)
    return e.value.code, (G.lib().gn_last_error() or b"").decode()


def test_mixed_whitespace_replays_as_single_spaces(G):
    a, b = G.replay_game(START, OPERA, skip=[2]), G.replay_game(START, _mixed_whitespace(OPERA), skip=[2])
    assert len(a[0]) == 34
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for blank in (" \t\r\n  ", ""):
        boards, skipped, moves = G.replay_game(START, blank)
        assert len(boards) == 1 and len(moves) == 0 and G.board_to_fen(boards[0]) == START


def test_long_tokens_fail_at_their_index_with_16_characters(G):
    code, msg = _replay_error(G, START, LONG_TOKEN)
    assert code == G.E_ILLEGAL_MOVE and "move 2 (e2e4e2e4e2e4e2e4) " in msg
    assert len(G.replay_game(PROMO_ROOT, "e7e8q h7g7")[0]) == 3
    for tok, shown in (("e7e8qq", "e7e8qq"), ("e7e8qqq", "e7e8qqq"), ("e7e8q\x0b", "e7e8q\x0b")):
        code, msg = _replay_error(G, PROMO_ROOT, tok)
        assert code == G.E_ILLEGAL_MOVE and f"move 1 ({shown}) " in msg
        code, msg = _replay_error(G, PROMO_ROOT, "e7e8q h7g7 \t" + tok)
        assert code == G.E_ILLEGAL_MOVE and f"move 3 ({shown}) " in msg


@pytest.mark.gpu
def test_evaluate_games_tokens_equal_host_replay(gpu_ctx):
    """gn_evaluate_games splits the move string as gn_replay_game does: the same bytes for mixed
    whitespace, and for a failing game (one per call) the host replay's status and message."""
    from fishnet_amd import gpu_nnue as G

    def run(games, children):
        arr, _keep = G._games_array(games)
        r = gpu_ctx.evaluate_games_arrays(arr, len(games), 0, children=children)
        return [x.tobytes() for x in (r[:6] if children else r[:3])], r[1]

    for children in (False, True):
        plain, status = run([(START, OPERA, [3]), (C960, "e2e4 e6e5", [])], children)
        mixed, _ = run([(START, _mixed_whitespace(OPERA), [3]), (C960, "\te2e4\r\ne6e5\n", [])], children)
        assert not status.any() and plain == mixed
    for root, moves in LONG_TOKEN_GAMES:
        code, msg = _replay_error(G, root, moves)
        _, status = run([(START, OPERA, []), (root, moves, []), (START, "e2e4", [])], False)
        assert list(status) == [0, code, 0] and code == G.E_ILLEGAL_MOVE
        assert (G.lib().gn_last_error() or b"").decode() == msg


# ---- a shard that reads the replay's boards in place beside one that gathers ----
K_MIXED = 3


def _all_arrays(ctx, games):
    """Every array gn_evaluate_games (without and with children) and gn_evaluate_games_lines return."""
    from fishnet_amd import gpu_nnue as G
    arr, _keep = G._games_array(games)
    out = []
    for children in (False, True):
        r = ctx.evaluate_games_arrays(arr, len(games), 0, children=children)
        out += [x.tobytes() for x in (r[:6] if children else r[:3])]
    return out + [x.tobytes() for x in ctx.evaluate_games_lines(games, K_MIXED, 0)]


@pytest.fixture(scope="module")
def two_slots(synth_big_path, synth_small_path):
    from fishnet_amd import gpu_nnue as G
    ctx = G.GpuNnue(synth_big_path, synth_small_path, devices=[0, 0])
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_mixed_shards_equal_one_slot(gpu_ctx, two_slots):
    from fishnet_amd import gpu_nnue as G
    ucis = G.random_games_uci(0x5EED5A4D, 0, 6, 40)
    skips = [(), (1000,), (), (), (0, 7, 40), (3, 4, 5, 999)]  # 1000 / 999: beyond the game, ignored
    games = [(START, u, s) for u, s in zip(ucis, skips)]
    npos = [len(u.split()) + 1 for u in ucis]
    assert npos == [41] * 6

    def skipped_shards(gs):  # per shard of the two-slot context: does it hold a skipped position?
        w = [len(u.split()) + 1 for _, u, _ in gs]
        b = G.partition(len(gs), 2, w)
        return [any(p < w[g] for g in range(b[k], b[k + 1]) for p in gs[g][2]) for k in range(2)], b

    assert skipped_shards(games)[0] == [False, True]
    assert skipped_shards(games[::-1])[0] == [True, False]
    assert skipped_shards(games[1:2])[1] == [0, 1, 1]  # the second shard is empty
    ref = _all_arrays(gpu_ctx, games)
    assert _all_arrays(two_slots, games) == ref
    assert _all_arrays(two_slots, games[::-1]) == _all_arrays(gpu_ctx, games[::-1])
    for g in (1, 4):  # in place alone, gathered alone
        assert _all_arrays(two_slots, games[g:g + 1]) == _all_arrays(gpu_ctx, games[g:g + 1])
    # an out-of-range skip index changes nothing
    plain = [(r, u, () if s == (1000,) else s) for r, u, s in games]
    assert _all_arrays(two_slots, plain) == ref
    assert _all_arrays(gpu_ctx, plain[1:2]) == _all_arrays(gpu_ctx, games[1:2])
