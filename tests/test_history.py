"""CPU-only checks of the game-history draws (include/gpu_nnue.h at gn_history): the position
key of gn_position_keys against the first four FEN fields, the properties of the fixture
tests/golden/history_games.txt from the CPU oracle alone, and the C-ABI surface."""
import numpy as np
import pytest

import history_rule as H
import raw_boards as RB


@pytest.fixture(scope="module")
def G():
    from fishnet_amd import build, gpu_nnue
    build.build()
    return gpu_nnue


@pytest.fixture(scope="module")
def replayed(oracle_lib):
    """[(fens of positions 0..=moves, skip)] of the fixture's games."""
    return [(oracle_lib.replay_game(root, moves)[0], skip) for root, moves, skip in H.fixture_games()]


def _identities(G, boards):
    return [H.identity(f) for f in G.boards_to_fens(boards)]


def _assert_keys_are_identities(keys, ids):
    """Equal key <=> equal first four FEN fields; no key is 0."""
    assert len(keys) == len(ids) and (keys != 0).all()
    by_key, by_id = {}, {}
    for k, i in zip(keys.tolist(), ids):
        assert by_key.setdefault(k, i) == i, (k, i, by_key[k])
        assert by_id.setdefault(i, k) == k, (i, k, by_id[i])
    return by_id


def test_position_keys_fixture_and_random(G):
    boards = [G.replay_game(root, moves)[0] for root, moves, _ in H.fixture_games()]
    boards = np.concatenate(boards + [G.random_positions(0x5EED4157, 0, 20000, 160)])
    assert len(boards) >= 20150
    by_id = _assert_keys_are_identities(G.position_keys(boards), _identities(G, boards))
    assert 5000 < len(by_id) < len(boards)  # distinct identities, and repeated ones


def test_position_keys_hand_made_variants(G):
    base = "r3k2r/8/8/3Pp3/8/8/8/R3K2R w KQkq e6 0 1"
    variants = [base,
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R b KQkq - 0 1",    # the other side to move
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w KQkq - 0 1",    # no en-passant square
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w Qkq e6 0 1",    # one castling right fewer, each one
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w Kkq e6 0 1",
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w KQq e6 0 1",
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w KQk e6 0 1",
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w - e6 0 1",
                "r3k2r/8/8/3Pp3/8/8/8/R3K1R1 w Qkq e6 0 1",   # another placement
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w KQkq e6 57 1",  # rule50, fullmove: not in the identity
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w KQkq e6 0 77",
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w KQkq e6 99 300",
                "r3k2r/8/8/3Pp3/8/8/8/R3K2R w KQkq d6 0 1"]   # an en-passant square nothing can capture on
    boards, ok = G.pack_fens(variants)
    assert ok.all()
    junk = boards[:3].copy()
    junk["reserved"] = (1, 0x80, 0xFF)  # `reserved` is not read
    boards = np.concatenate([boards, junk])
    keys = G.position_keys(boards)
    by_id = _assert_keys_are_identities(keys, _identities(G, boards))
    assert len(by_id) == 9  # base, stm, no ep (also the d6 text), 5 sets of rights, the other placement
    assert keys[0] == keys[9] == keys[10] == keys[11] == keys[13] and keys[2] == keys[12]
    assert len({int(k) for k in keys[:9]}) == 9


def test_position_keys_rejected_boards_are_zero(G):
    cat = RB.catalogue()
    boards = np.array([b for _, b, _ in cat], dtype=G.BOARD_DTYPE).reshape(-1)
    keys = G.position_keys(boards)
    bad = np.array([isinstance(canon, str) and canon == "bad" for _, _, canon in cat])
    assert bad.sum() >= 20 and (~bad).sum() >= 20
    assert (keys[bad] == 0).all() and (keys[~bad] != 0).all()
    # an accepted board's key is its canonical form's: that of the FEN gn_board_to_fen writes
    good = boards[~bad]
    again, ok = G.pack_fens(G.boards_to_fens(good))
    assert ok.all() and np.array_equal(G.position_keys(again), keys[~bad])


def test_exports(G):
    lib = G.lib()
    for s in ("gn_position_keys", "gn_position_keys_device", "gn_rank_children_history_device",
              "gn_evaluate_games_lines_history"):
        assert s in G.EXPORTS and hasattr(lib, s), s
    assert G.FLAG_DRAW == 512 and G.STAT_KEYS_NS == 123 and G.HISTORY_DTYPE.itemsize == 8
    assert lib.gn_abi_version() == 4


# ---- the fixture shows what it is there to show (from the oracle alone) ----------------------

def test_fixture_size(replayed):
    assert len(replayed) <= 16 and sum(len(f) for f, _ in replayed) <= 600


def test_fixture_threefold(oracle_lib, replayed):
    O = oracle_lib
    third, second_only, few = [], [], []
    for g, (fens, _) in enumerate(replayed):
        for k in range(len(fens)):
            drawn = H.drawn_moves(O, fens, k)
            occ = H.occurrences(O, fens, k)
            if any(why == "threefold" for why in drawn.values()):
                third.append((g, k))
                if len(occ) <= 8:
                    few.append((g, k))
            if any(n == 1 and m not in drawn for m, n in occ.items()):
                second_only.append((g, k))
    assert len(third) >= 6 and len(second_only) >= 6 and len(few) >= 3
    # the start-position knight shuffle
    root, moves, _ = H.fixture_games()[0]
    assert root == H.R.START and moves.split()[:7] == "g1f3 g8f6 f3g1 f6g8 g1f3 g8f6 f3g1".split()
    fens = replayed[0][0]
    f6g8, f3g1 = O.uci_to_move(fens[7], "f6g8"), O.uci_to_move(fens[6], "f3g1")
    assert H.drawn_moves(O, fens, 7).get(f6g8) == "threefold" and H.occurrences(O, fens, 7)[f6g8] == 2
    assert f3g1 not in H.drawn_moves(O, fens, 6) and H.occurrences(O, fens, 6)[f3g1] == 1


def _placement_twins(fens, field):
    """(i, j): positions i < j with equal placement and side to move that differ in FEN field `field`."""
    for i in range(len(fens)):
        for j in range(i + 1, len(fens)):
            a, b = fens[i].split(), fens[j].split()
            if a[:2] == b[:2] and a[field] != b[field]:
                yield i, j


def test_fixture_castling_rights(oracle_lib, replayed):
    """Equal placement and side to move, different castling rights (a rook went out and came
    back): a move into that placement a third time is the identity's second occurrence."""
    O = oracle_lib
    found = 0
    for fens, _ in replayed:
        for i, j in _placement_twins(fens, 2):
            assert fens[i].split()[3] == fens[j].split()[3]
            for k in range(j + 1, len(fens)):
                for m, c, alive in H._children(O, fens[k]):
                    if H.identity(c) == H.identity(fens[j]) and alive:
                        placements = [f.split()[:2] for f in fens[:k + 1]].count(c.split()[:2])
                        if placements >= 2 and H.occurrences(O, fens, k)[m] == 1:
                            assert m not in H.drawn_moves(O, fens, k)
                            found += 1
    assert found >= 1


def test_fixture_en_passant(oracle_lib, replayed):
    """Equal placement, one position with a capturable en-passant square: not a repetition."""
    O = oracle_lib
    found = 0
    for fens, _ in replayed:
        for i, j in _placement_twins(fens, 3):
            assert fens[i].split()[2] == fens[j].split()[2] and "-" in (fens[i].split()[3], fens[j].split()[3])
            for k in range(j + 1, len(fens)):
                for m, c, alive in H._children(O, fens[k]):
                    if H.identity(c) == H.identity(fens[j]) and alive:
                        placements = [f.split()[:2] for f in fens[:k + 1]].count(c.split()[:2])
                        if placements >= 2 and H.occurrences(O, fens, k)[m] == 1:
                            assert m not in H.drawn_moves(O, fens, k)
                            found += 1
    assert found >= 1


def test_fixture_fifty_move_rule(oracle_lib, oracle_nets, replayed):
    O = oracle_lib
    big, small = oracle_nets
    roots = {int(fens[0].split()[4]) for fens, _ in replayed}
    assert {98, 99, 100, 150} <= roots
    wide = mate = stalemate = 0
    for fens, _ in replayed:
        for k, fen in enumerate(fens):
            r50 = int(fen.split()[4])
            kids = H._children(O, fen)
            drawn = H.drawn_moves(O, fens, k)
            if r50 >= 99:
                quiet = [m for m, c, alive in kids if alive and int(c.split()[4]) == r50 + 1]
                zeroing = [m for m, c, alive in kids if alive and int(c.split()[4]) == 0]
                assert all(drawn.get(m) == "fifty" for m in quiet)
                assert not any(m in drawn for m in zeroing)  # captures and pawn moves
                if r50 == 99 and len(kids) >= 40:
                    # the draws reach the second 32-lane segment of the parent's children
                    order = [m for m, _, _ in kids]
                    assert zeroing and any(order.index(m) >= 32 for m in quiet)
                    wide += 1
                for m, c, alive in kids:
                    if not alive and int(c.split()[4]) >= 100:
                        in_check = bool(O.eval_fens(big, small, [c], 0)[0]["flags"] & H.R.FLAG_IN_CHECK)
                        mate += in_check
                        stalemate += not in_check
                        assert m not in drawn
            elif r50 < 98:
                assert "fifty" not in drawn.values()
    assert wide >= 1 and mate >= 1 and stalemate >= 1
    # the example the rule names
    fens = [f for f, _ in replayed if f[0].startswith("7k/8/5K2/6Q1/8/8/8/8 w")][0]
    g5g7 = O.uci_to_move(fens[0], "g5g7")
    assert g5g7 not in H.drawn_moves(O, fens, 0) and not O.legal_moves(O.child_fen(fens[0], g5g7))


def test_fixture_skipped_positions(oracle_lib, replayed):
    """A game with skipPositions whose earlier occurrences are skipped positions."""
    O = oracle_lib
    found = 0
    for fens, skip in replayed:
        if not skip:
            continue
        for k in range(len(fens)):
            if k in skip:
                continue
            for m, why in H.drawn_moves(O, fens, k).items():
                c = H.identity(O.child_fen(fens[k], m))
                earlier = [i for i in range(k + 1) if H.identity(fens[i]) == c]
                if why == "threefold" and len(earlier) >= 2 and all(i in skip for i in earlier):
                    found += 1
    assert found >= 1


def test_fixture_long_game(oracle_lib, replayed):
    O = oracle_lib
    long = [fens for fens, _ in replayed if len(fens) > 120]
    assert long
    fens = long[0]
    why = [set(H.drawn_moves(O, fens, k).values()) for k in range(len(fens))]
    assert sum("threefold" in w for w in why) >= 20 and sum("fifty" in w for w in why) >= 20
    # a long window: a threefold whose earlier occurrences lie at least 16 and 32 plies back
    k = max(i for i, w in enumerate(why) if "threefold" in w)
    m = [m for m, w in H.drawn_moves(O, fens, k).items() if w == "threefold"][0]
    c = H.identity(O.child_fen(fens[k], m))
    assert sorted(k + 1 - i for i in range(k + 1) if H.identity(fens[i]) == c)[:2] == [16, 32]


def test_library_replay_agrees_with_the_oracle(G, replayed):
    """The fixture's positions as the library replays them are the oracle's (the GPU tests feed
    the library's boards to the device calls and the oracle's FENs to the rule)."""
    for (root, moves, skip), (fens, _) in zip(H.fixture_games(), replayed):
        assert G.boards_to_fens(G.replay_game(root, moves, skip)[0]) == fens
