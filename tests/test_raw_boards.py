"""The gn_board contract (include/gpu_nnue.h at gn_board) on the host: hand-made records
(tests/raw_boards.py) through gn_board_to_fen, the host FEN parser and the CPU oracle.

A raw record behaves exactly like the FEN text that spells its fields.  The one gate
(position_ok, fishnet_amd/csrc/chess.h) is what gn_board_to_fen, the FEN parser and the device
kernels share, so what holds here is what tests/test_gpu_raw_boards.py then uploads.

Finding while writing these (oracle and host parser agree, so neither changed): both read a FEN
text's fullmove 0 as 1 (Stockfish's Position::set computes gamePly from max(2 * (fullmove - 1), 0),
the same game ply for 0 and 1), while a raw record's fullmove 0 is kept; the C6 entries with
fullmove 0 therefore differ from their text in `fullmove` alone.
"""
import os

import numpy as np
import pytest

import raw_boards as R

HERE = os.path.dirname(os.path.abspath(__file__))
CATALOGUE = R.catalogue()
IDS = [n for n, _, _ in CATALOGUE]


def _fens(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return [l.strip() for l in f if l.strip() and not l.startswith("#")]


@pytest.fixture(scope="module")
def G():
    from fishnet_amd import build, gpu_nnue
    build.build()
    return gpu_nnue


def _bad(exp):
    return isinstance(exp, str)


def test_dtype_is_the_librarys(G):
    assert R.BOARD_DTYPE == G.BOARD_DTYPE


def test_catalogue_is_complete():
    names = set(IDS)
    assert not [n for n in R.REQUIRED if n not in names]
    for cls, least in (("R1", 4), ("R2", 16), ("R3", 4), ("R4", 4), ("R5", 2), ("R6", 14), ("C1", 1), ("C2", 2),
                       ("C3", 4), ("C4", 12), ("C5", 9), ("C6", 21)):
        assert sum(n.startswith(cls + "/") for n in IDS) >= least, cls


@pytest.mark.parametrize("name", ["special_fens.txt", "row_cover_fens.txt"])
def test_make_reproduces_pack_fens(G, name):
    fens = _fens(name)
    boards, ok = G.pack_fens(fens)
    assert ok.all()
    for fen, b in zip(fens, boards):
        assert R.from_fen(fen).tobytes() == b.tobytes(), fen


def test_fen_text_round_trips_canonical_boards(G):
    """fen_text of a canonical board, packed by the host, is that board (the writer spells what
    the packer reads)."""
    fens = _fens("special_fens.txt")
    boards, _ = G.pack_fens(fens)
    again, ok = G.pack_fens([R.fen_text(b) for b in boards])
    assert ok.all() and again.tobytes() == boards.tobytes()


@pytest.mark.parametrize("name,board,exp", CATALOGUE, ids=IDS)
def test_board_to_fen_gate(G, name, board, exp):
    one = G.boards_to_fens(np.array([board], dtype=G.BOARD_DTYPE))[0]
    if _bad(exp):
        with pytest.raises(G.GnError) as e:
            G.board_to_fen(board)
        assert e.value.code == G.E_INVALID
        assert one == ""
        return
    fen = G.board_to_fen(board)
    assert one == fen
    assert fen == G.board_to_fen(exp)  # the canonical board's own text
    packed, ok = G.pack_fens([fen])
    assert ok[0]
    want = exp.copy()
    if int(board["fullmove"]) == 0:  # a text's fullmove 0 reads as 1: the only field that differs
        assert fen.endswith(" 0") and int(packed[0]["fullmove"]) == 1
        want["fullmove"] = 1
    assert packed[0].tobytes() == want.tobytes()


@pytest.mark.parametrize("name,board,exp", [c for c in CATALOGUE if c[0] not in R.NO_TEXT],
                         ids=[n for n in IDS if n not in R.NO_TEXT])
def test_host_parser_parity(G, name, board, exp):
    _, ok = G.pack_fens([R.fen_text(board)])
    assert bool(ok[0]) == (not _bad(exp))


def test_no_text_entries_are_the_exempt_ones():
    for name, board, exp in CATALOGUE:
        if name in R.NO_TEXT:
            assert _bad(exp)
            with pytest.raises(ValueError):
                R.fen_text(board)
        else:
            R.fen_text(board)


@pytest.mark.parametrize("name,board,exp", [c for c in CATALOGUE if c[0] not in R.NO_TEXT],
                         ids=[n for n in IDS if n not in R.NO_TEXT])
def test_oracle_parity(G, oracle_lib, name, board, exp):
    text = R.fen_text(board)
    if _bad(exp):
        with pytest.raises(ValueError):
            oracle_lib.normalize_fen(text)
        return
    got, want = oracle_lib.normalize_fen(text), G.board_to_fen(board)
    if name in R.SLOT_NOT_IN_TEXT:
        # the text cannot say which slot held the right: it reads as the rook's own side's
        assert got.split()[2] in ("Q", "q") and want.split()[2] == "-"
        got = " ".join(got.split()[:2] + ["-"] + got.split()[3:])
    if int(board["fullmove"]) == 0:
        assert got.split()[5] == "1" and want.split()[5] == "0"
        got, want = got.rsplit(" ", 1)[0], want.rsplit(" ", 1)[0]
    assert got == want


def test_c6_position_is_observable(oracle_lib, oracle_nets):
    """rule50 enters final_v only where final_v is not zero: both nets give a non-zero value on
    the C6 position, and rule50 moves it."""
    big, small = oracle_nets
    fens = [R.fen_text(b) for n, b, _ in CATALOGUE if n.startswith("C6/") and n.endswith("-fullmove-1")]
    for mode in (1, 2):
        v = oracle_lib.eval_fens(big, small, fens, mode)["final_v"]
        assert v[0] != 0, mode  # (rule50 0; at rule50 == rule50_div, 212, the value is 0 by the formula)
        assert len(set(v.tolist())) == len(R.C6_RULE50), mode  # every rule50 gives another value
