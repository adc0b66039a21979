"""Quiescent ranked lines (include/gpu_nnue.h at gn_line, "quiescent") without a GPU: the rule's Python
restatement (tests/quiesce_rule.py) on the hand-made positions of tests/golden/quiesce_fens.txt, the
structural cases the rule must meet (each found by the rule's own tree walk over the test inputs), its
consequences, the binding, and the conditions on the inputs the GPU tests (tests/test_gpu_quiesce.py)
use."""
import os

import pytest

import lines2_rule as R2
import lines_extended_rule as X
import lines_rule as R
import quiesce_rule as Q

FX = Q.fixture_fens()
mv = R2.uci_move
MODE = 0  # FULL: both nets


@pytest.fixture(scope="module")
def nets(oracle_lib, oracle_nets):
    return (oracle_lib,) + tuple(oracle_nets)


def inputs(n_random=Q.N_RANDOM):
    from fishnet_amd import gpu_nnue as G
    return FX + R.fixture_fens() + G.boards_to_fens(G.random_positions(Q.SEED, 0, n_random, 160))


def inputs3():
    from fishnet_amd import gpu_nnue as G
    return FX + G.boards_to_fens(G.random_positions(Q.SEED, 0, Q.N_RANDOM3, 160))


def test_fixture_file():
    assert FX == [f for _, f, _ in Q.FIXTURES]


def _walk(O, big, small, fen, d, check, static, seen):
    """Every node the rule visits below (and including) the searched leaf fen at depth d, as
    (fen, d, in check, its legal entries of Q.node, the searched ones); dead nodes and d == 0 have none."""
    if not Q.alive(O, fen) or d == 0:
        seen.append((fen, d, check, (), ()))
        return
    kids, srch = Q.node(O, big, small, fen, MODE), Q.searched_moves(O, big, small, fen, MODE, check)
    seen.append((fen, d, check, kids, srch))
    for _, c, kcheck, kstatic, _ in srch:
        _walk(O, big, small, c, d - 1, kcheck, kstatic, seen)


def _leaf(O, big, small, name):
    """(leaf FEN, in check, alive, static, searched) of the named fixture's leaf."""
    fen, u = next((f, u) for n, f, u in Q.FIXTURES if n == name)
    return next(l[1:] for l in Q.leaves(O, big, small, fen, MODE) if l[0] == mv(u))


def _attacks(board, sq):
    """The squares the piece on sq attacks on the placement `board` ({square: letter}): pseudo-legal
    geometry only, restated here so that the walk can tell an illegal capture from an absent one."""
    pc = board[sq]
    f, r = sq & 7, sq >> 3
    out = set()

    def step(df, dr, slide):
        x, y = f + df, r + dr
        while 0 <= x < 8 and 0 <= y < 8:
            out.add(y * 8 + x)
            if not slide or y * 8 + x in board:
                break
            x, y = x + df, y + dr

    t = pc.lower()
    if t == "p":
        for df in (-1, 1):
            step(df, 1 if pc == "P" else -1, False)
    elif t == "n":
        for df, dr in ((1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1), (-2, 1), (-1, 2)):
            step(df, dr, False)
    else:
        for df, dr in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
            if t in ("k", "q") or (t == "r") == (df == 0 or dr == 0):
                step(df, dr, t != "k")
    return out


def _illegal_captures(O, fen, kids):
    """(from, to, mover) of the captures that the geometry allows and the legal moves lack: a pinned
    piece's, or the king's of a defended piece."""
    board, white = O._placement(fen), fen.split()[1] == "w"
    legal = {((k[0] >> 6) & 63, k[0] & 63) for k in kids if k[0] >> 14 != 3}
    return [(a, b, board[a].lower()) for a, pc in board.items() if pc.isupper() == white
            for b in _attacks(board, a) if b in board and board[b].isupper() != white and (a, b) not in legal]


def _checkers(O, fen):
    board, white = O._placement(fen), fen.split()[1] == "w"
    ksq = next(a for a, pc in board.items() if pc == ("K" if white else "k"))
    return [a for a, pc in board.items() if pc.isupper() != white and ksq in _attacks(board, a)]


def test_structural_cases_occur(nets):
    """Each case of the rule occurs in the test inputs (the fixtures' leaves, walked to depth 2), found
    from the rule's own tree walk and the move encodings alone."""
    O, big, small = nets
    typ, to, promo = (lambda m: m >> 14), (lambda m: m & 63), (lambda m: (m >> 12) & 3)
    seen, unsearched = [], []
    for fen in FX:
        for m, c, check, live, static, srch in Q.leaves(O, big, small, fen, MODE):
            if srch:
                _walk(O, big, small, c, 2, check, static, seen)
            elif live:
                unsearched.append((c, check, Q.node(O, big, small, c, MODE)))
    capture = lambda f, k: typ(k[0]) != 3 and to(k[0]) in O._placement(f)
    cases = {
        "en passant as the only noisy move":
            any(len(s) == 1 and typ(s[0][0]) == 2 for _, _, ch, _, s in seen if not ch),
        "a quiet queen promotion":
            any(typ(k[0]) == 1 and promo(k[0]) == 3 and not capture(f, k) and k in s for f, _, ch, _, s in seen
                if not ch for k in s),
        "a capturing underpromotion":
            any(typ(k[0]) == 1 and promo(k[0]) != 3 and capture(f, k) for f, _, ch, _, s in seen if not ch for k in s),
        "a quiet underpromotion that is not searched":
            any(typ(k[0]) == 1 and promo(k[0]) != 3 and not capture(f, k) and k not in s
                for f, _, ch, ks, s in seen if not ch for k in ks),
        "a capture that gives check, the child searched through all its evasions":
            any(capture(f, k) and k[2] and Q.alive(O, k[1]) and
                any(g[0] == k[1] and g[1] == d - 1 >= 1 and g[2] and len(g[4]) == len(g[3]) > 0 for g in seen)
                for f, d, ch, _, s in seen if not ch for k in s),
        "a capture that mates":
            any(capture(f, k) and k[2] and not Q.alive(O, k[1]) for f, _, ch, _, s in seen if not ch for k in s),
        "a capture that stalemates":
            any(capture(f, k) and not k[2] and not Q.alive(O, k[1]) for f, _, ch, _, s in seen if not ch for k in s),
        "a leaf in check with one evasion":
            any(d == 2 and ch and len(ks) == 1 for _, d, ch, ks, _ in seen),
        "a leaf in double check":
            any(d == 2 and ch and len(_checkers(O, f)) == 2 and ks and len(s) == len(ks) for f, d, ch, ks, s in seen),
        "a pinned piece whose capture is illegal and not counted":
            any(any(t != "k" for _, _, t in _illegal_captures(O, f, ks)) and not any(k[4] for k in ks)
                for f, ch, ks in unsearched if not ch),
        "a king capture of a defended piece, not counted":
            any(any(t == "k" for _, _, t in _illegal_captures(O, f, ks)) and not any(k[4] for k in ks)
                for f, ch, ks in unsearched if not ch),
        "a Chess960 castling that is not noisy":
            any(any(typ(k[0]) == 3 for k in ks) and not any(k[4] for k in ks) for _, ch, ks in unsearched if not ch),
        "a leaf with legal moves and no noisy move":
            any(ks and not ch and not any(k[4] for k in ks) for _, ch, ks in unsearched),
    }
    assert all(cases.values()), [c for c, ok in cases.items() if not ok]


def test_fixture_leaves(nets):
    """What each hand-made leaf is there for, and the values that do not depend on the net."""
    O, big, small = nets
    # double check: only king moves are legal, and two pieces give check (neither alone would allow only those)
    c, check, live, static, srch = _leaf(O, big, small, "double_check")
    kids = Q.node(O, big, small, c, MODE)
    assert check and srch and kids and all(O._placement(c)[(k[0] >> 6) & 63] == "k" for k in kids)
    assert O._placement(c)[43] == "N" and O._placement(c)[4] == "R"  # d6 attacks e8, e1 sees e8: two checkers
    # a pinned piece's capture and a king's capture of a defended piece are illegal: not counted, not searched
    c, check, live, static, srch = _leaf(O, big, small, "pinned_capture")
    assert live and not check and not srch and mv("e2d4") not in [k[0] for k in Q.node(O, big, small, c, MODE)]
    assert O._placement(c)[12] == "N" and O._placement(c)[27] == "p"  # the knight on e2 attacks the pawn on d4
    c, check, live, static, srch = _leaf(O, big, small, "defended_piece")
    assert live and not check and not srch and mv("e1d2") not in [k[0] for k in Q.node(O, big, small, c, MODE)]
    assert O._placement(c)[11] == "n"  # next to the king on e1
    # the castling is legal, king takes own rook, and the leaf is not searched
    c, check, live, static, srch = _leaf(O, big, small, "chess960_castling")
    castle = [k for k in Q.node(O, big, small, c, MODE) if k[0] >> 14 == 3]
    assert len(castle) == 1 and O._placement(c)[castle[0][0] & 63] == "R" and not castle[0][4] and not srch
    # en passant only
    c, check, live, static, srch = _leaf(O, big, small, "en_passant_only")
    assert [k[0] >> 14 for k in Q.searched_moves(O, big, small, c, MODE, check)] == [2] and srch
    # mate and stalemate through a capture, at every depth and in every mode
    for mode in (0, 1, 2):
        for d in range(1, Q.MAX_DEPTH + 1):
            fen, u = next((f, u) for n, f, u in Q.FIXTURES if n == "capture_mates")
            by = {l[2]: l for l in Q.all_lines(O, big, small, fen, d, mode)}
            assert by[mv(u)] == (-31998, -1, mv(u), R.FLAG_MATE | Q.FLAG_SEARCHED)  # the leaf: mate 1, the line: mate -1
            fen, u = next((f, u) for n, f, u in Q.FIXTURES if n == "capture_stalemates")
            c = O.child_fen(fen, mv(u))
            l = next(l for l in Q.leaves(O, big, small, fen, mode) if l[0] == mv(u))
            assert Q.Q(O, big, small, c, d, mode, l[2], l[4])[0] == max(l[4], 0)  # stand pat, or the stalemate's 0
    # the history forms' draw comes before the quiescence
    import history_rule as H
    fen = next(f for n, f, _ in Q.FIXTURES if n == "fifty_before_searched")
    drawn = H.drawn_moves(O, [fen], 0)
    assert len(drawn) == 3 and all(l[5] for l in Q.leaves(O, big, small, fen, MODE))
    assert all(l[3] == Q.FLAG_DRAW and l[0] == 0 for l in Q.all_lines(O, big, small, fen, 2, MODE, drawn))
    assert all(l[3] & Q.FLAG_SEARCHED and not l[3] & Q.FLAG_DRAW for l in Q.all_lines(O, big, small, fen, 2, MODE))
    # today's lines value the mating capture's leaf statically
    fen, u = next((f, u) for n, f, u in Q.FIXTURES if n == "capture_mates")
    plain = {l[2]: l for l in R.all_lines(O, big, small, fen, MODE)}
    assert not plain[mv(u)][3] & (R.FLAG_MATE | Q.FLAG_SEARCHED)


def test_in_check_depth_1_is_the_score_rule(nets):
    """Q(x, 1) == value(x, 1) of the score rule for every leaf in check of the inputs."""
    O, big, small = nets
    n = 0
    for fen in inputs():
        for m, c, check, live, static, srch in Q.leaves(O, big, small, fen, MODE) or []:
            if check and live:
                assert srch
                assert Q.Q(O, big, small, c, 1, MODE, check, static)[0] == X.value(O, big, small, c, 1, MODE)[0], (fen, m)
                n += 1
    assert n >= 50


def test_stand_pat_bound(nets):
    """Q(x, d) >= final_v(x) for every searched leaf that is not in check, at depth 1 and 2; depth 2
    changes some values."""
    O, big, small = nets
    n = above = deeper = 0
    for fen in inputs():
        for m, c, check, live, static, srch in Q.leaves(O, big, small, fen, MODE) or []:
            if srch and not check:
                q1, q2 = (Q.Q(O, big, small, c, d, MODE, check, static)[0] for d in (1, 2))
                assert q1 >= static and q2 >= static, (fen, m)
                n, above, deeper = n + 1, above + (q1 > static), deeper + (q1 != q2)
    assert n >= 1000 and above >= 100 and deeper >= 100


def test_equal_to_the_plain_rule_where_nothing_is_searched(nets):
    O, big, small = nets
    same = differ = 0
    for fen in inputs():
        ls = Q.all_lines(O, big, small, fen, 2, MODE)
        if any(l[3] & Q.FLAG_SEARCHED for l in ls):
            differ += 1
        else:
            assert ls == R.all_lines(O, big, small, fen, MODE), fen
            same += 1
    assert same >= 1 and differ >= 50


@pytest.mark.parametrize("mode", (0, 1))
def test_conditions_on_the_gpu_inputs(nets, mode):
    """What tests/test_gpu_quiesce.py asserts of its inputs, met by the reference alone: at least 100
    searched and 20 unsearched leaves per set, trees of at most about 150 k nodes, a top-8 that differs
    from the plain ranking, a mate line."""
    O, big, small = nets
    for depth, fens in ((1, inputs()), (2, inputs()), (3, inputs3())):
        ns = nn = total = 0
        for fen in fens:
            ext, a, b = Q.extensions(O, big, small, fen, depth, mode)
            ns, nn, total = ns + a, nn + b, total + len(ext)
        assert ns >= 100 and total - ns >= 20 and nn <= 150000, (depth, ns, total, nn)
    differ = mates = 0
    for fen in inputs():
        q, plain = Q.all_lines(O, big, small, fen, 2, mode)[:8], R.all_lines(O, big, small, fen, mode)[:8]
        differ += [l[:3] for l in q] != [l[:3] for l in plain]
        mates += sum(1 for l in q if l[3] & Q.FLAG_SEARCHED and l[3] & R.FLAG_MATE)
    assert differ >= 20 and mates >= 1


def test_binding_has_the_quiescent_calls():
    """The four exports, the depth limit, the three statistics and the library's symbols (absent before
    this feature)."""
    from fishnet_amd import build, gpu_nnue as G
    names = ("gn_quiesce_device", "gn_evaluate_lines2_quiescent", "gn_evaluate_games_lines2_quiescent",
             "gn_evaluate_games_lines_quiescent")
    assert all(n in G.EXPORTS for n in names)
    assert (G.STAT_QUIESCE_NS, G.STAT_QUIESCE_LEAVES, G.STAT_QUIESCE_NODES) == (126, 127, 128)
    assert G.MAX_QUIESCE_DEPTH == Q.MAX_DEPTH == 4 and G.NOT_EXTENDED == Q.NOT_EXTENDED
    build.build()
    L = G.lib()
    assert all(hasattr(L, n) for n in G.EXPORTS)
    hdr = open(os.path.join(os.path.dirname(R.HERE), "include", "gpu_nnue.h")).read()
    assert "#define GN_MAX_QUIESCE_DEPTH 4" in hdr and "#define GN_ABI_VERSION 4" in hdr
    assert all(f"#define {n} {v}" in hdr for n, v in (("GN_STAT_QUIESCE_NS", 126), ("GN_STAT_QUIESCE_LEAVES", 127),
                                                     ("GN_STAT_QUIESCE_NODES", 128)))
