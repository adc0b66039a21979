"""The gn_board contract (include/gpu_nnue.h at gn_board) on the device: hand-made records
(tests/raw_boards.py) through gn_evaluate_device, gn_expand_device, gn_rank_children_device and
gn_expand2_device, and every child board the device writes against the CPU oracle's child.

A raw record behaves exactly like the FEN text that spells its fields handed to
gn_evaluate_batch / gn_expand_and_evaluate: rejected records give the exact BAD record, no
children, empty lines and no grandchildren; normalised records give their canonical board's bytes.
Every call is small (<= 512 boards, <= 200 parents): enough for several 16-position evaluation
tiles, 64-lane plan passes and 32-lane rank groups.  King sort 2 sorts below 1,024 boards.

The guard (fixture `uploads`) runs on the CPU before anything is uploaded: gn_boards_to_fens -- the
same gate the kernels call -- must reject exactly the catalogue's rejected records.
"""
import os

import numpy as np
import pytest

import lines_rule
import raw_boards as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K_LINES = 3
N_GOOD = 16 * 20 + 3


def _special_fens():
    with open(os.path.join(HERE, "golden", "special_fens.txt")) as f:
        return [l.strip() for l in f if l.strip() and not l.startswith("#")]


def mv(frm, to, typ=0, promo=0):
    return R.sq(to) | R.sq(frm) << 6 | promo << 12 | typ << 14


# Parents whose children carry the fields do_move changes: (FEN or raw record, the move that must
# be among the oracle's).
def _boards_out_parents():
    kr = {**R.placement(R.KINGS), R.sq("a8"): R.BR}
    return [
        ("r3k2r/8/8/8/8/8/6B1/R3K2R w KQkq - 0 1", mv("g2", "a8")),   # a rook captured on its castling square
        ("r3k2r/6b1/8/8/8/8/8/R3K2R b KQkq - 0 1", mv("g7", "a1")),
        ("r3k2r/8/8/8/8/8/6B1/R3K2R w KQkq - 0 1", mv("e1", "e2")),   # a king move loses both rights
        ("r3k2r/8/8/8/8/8/6B1/R3K2R w KQkq - 0 1", mv("e1", "h1", 3)),  # castling itself
        ("r3k2r/6b1/8/8/8/8/8/R3K2R b KQkq - 0 1", mv("e8", "a8", 3)),
        ("6kr/8/8/8/8/8/8/6KR w Hh - 0 1", mv("g1", "h1", 3)),        # the king stays on g1
        ("k7/8/8/8/8/8/8/5KR1 w G - 0 1", mv("f1", "g1", 3)),         # king and rook swap
        ("4k3/8/8/8/3p4/8/4P3/4K3 w - - 0 1", mv("e2", "e4")),        # double push beside an enemy pawn
        ("4k3/8/8/8/8/8/4P3/4K3 w - - 0 1", mv("e2", "e4")),          # ... and without one
        ("4k3/8/8/3Pp3/8/8/8/4K3 w - e6 0 1", mv("d5", "e6", 2)),     # en passant
        ("r3k3/1P6/8/8/8/8/8/4K3 w q - 0 1", mv("b7", "a8", 1, 3)),   # a promotion captures a castling rook
        ("4k3/8/8/8/8/8/8/4K2R w - - 99 60", mv("h1", "h2")),         # rule50 99 -> 100
        ("4k3/8/8/8/8/8/4p3/4K3 w - - 57 80", mv("e1", "e2")),        # a capture at rule50 57
        (R.make(kr, R.BLACK, rule50=65535, fullmove=65535), mv("a8", "a7")),  # both saturate in do_move
    ]


@pytest.fixture(scope="module")
def uploads():
    """Every board this module uploads, built and checked on the CPU before a context exists:
    gn_boards_to_fens gives "" for exactly the rejected records."""
    from fishnet_amd import build, gpu_nnue as G
    build.build()
    cat = R.catalogue()
    good = np.concatenate([G.pack_fens(_special_fens())[0], G.random_positions(0x5EED0B0A, 0, N_GOOD, 160)])[:N_GOOD]
    # evaluation: a catalogue entry after every second good board (its slot in the 16-position
    # tile moves from tile to tile), the remaining good boards after them
    ev, ev_cat, ev_good = [], {}, []
    it = iter(cat)
    for i, b in enumerate(good):
        ev_good.append(len(ev))
        ev.append(b)
        if i % 2 == 1:
            e = next(it, None)
            if e is not None:
                ev_cat[len(ev)] = e
                ev.append(e[1])
    assert next(it, None) is None and len(ev) <= 512
    # expansion A: every catalogue entry, good boards between them; expansion B: the canonical
    # board of every accepted entry, then the boards-out parents
    xa, xa_cat = [], {}
    for i, e in enumerate(cat):
        xa_cat[len(xa)] = e
        xa.append(e[1])
        if len(cat) + i < 200:
            xa.append(good[i])
    xb, xb_of = [], {}
    for name, _, exp in cat:
        if not isinstance(exp, str):
            xb_of[name] = len(xb)
            xb.append(exp)
    outs = []
    for p, m in _boards_out_parents():
        b = G.pack_fens([p])[0][0] if isinstance(p, str) else p
        outs.append((len(xb), m))
        xb.append(b)
    assert len(xa) <= 200 and len(xb) <= 200
    u = {"cat": cat, "good": np.array(good, dtype=G.BOARD_DTYPE), "ev": np.array(ev, dtype=G.BOARD_DTYPE),
         "ev_cat": ev_cat, "ev_good": ev_good, "xa": np.array(xa, dtype=G.BOARD_DTYPE), "xa_cat": xa_cat,
         "xb": np.array(xb, dtype=G.BOARD_DTYPE), "xb_of": xb_of, "outs": outs}
    # ---- the guard
    for key, where in (("ev", ev_cat), ("xa", xa_cat)):
        fens = G.boards_to_fens(u[key])
        rejected = {i for i, (_, _, exp) in where.items() if isinstance(exp, str)}
        assert {i for i, f in enumerate(fens) if f == ""} == rejected, key
        u[key + "_fens"] = fens
    u["xb_fens"] = G.boards_to_fens(u["xb"])
    assert all(u["xb_fens"])
    assert all(G.boards_to_fens(u["good"]))
    return u


@pytest.fixture(scope="module")
def ctx(uploads, request):
    """The shared context, asked for only after the guard passed."""
    return request.getfixturevalue("gpu_ctx")


def _text(name, board, exp):
    """The FEN text a record behaves like (a right in the other side's slot has no spelling: the
    canonical board's text stands in, raw_boards.SLOT_NOT_IN_TEXT)."""
    return R.fen_text(exp if name in R.SLOT_NOT_IN_TEXT or name in R.NO_TEXT else board)


@pytest.fixture(scope="module")
def eval_expected(uploads, oracle_lib, oracle_nets):
    """Per mode the oracle's records of the evaluation mix's texts (rejected: None), once."""
    big, small = oracle_nets
    texts = list(uploads["ev_fens"])
    for i, (name, board, exp) in uploads["ev_cat"].items():
        texts[i] = None if isinstance(exp, str) else _text(name, board, exp)
    live = [i for i, t in enumerate(texts) if t is not None]
    return texts, live, {mode: oracle_lib.eval_fens(big, small, [texts[i] for i in live], mode, threads=8)
                         for mode in (0, 1, 2)}


@pytest.mark.parametrize("ksort", [2, 0])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_evaluate_device_raw_boards(ctx, uploads, eval_expected, mode, ksort):
    from fishnet_amd import gpu_nnue as G
    texts, live, oracle = eval_expected
    boards, good = uploads["ev"], uploads["good"]
    n = len(boards)
    d_b, d_o = ctx.alloc(n * 32), ctx.alloc(n * G.EVAL_SIZE)
    try:
        ctx.set_option(G.OPT_KING_SORT, ksort)
        d_b.upload(boards)
        ctx.evaluate_device(d_b, n, mode, d_o)
        got = d_o.download(G.EVAL_DTYPE, n)
        d_b.upload(good)
        ctx.evaluate_device(d_b, len(good), mode, d_o)
        alone = d_o.download(G.EVAL_DTYPE, len(good))
        host = ctx.evaluate_batch([texts[i] for i in live], mode)
    finally:
        ctx.set_option(G.OPT_KING_SORT, 1)
    bad = (0, 0, 0, 0, 0, G.FLAG_BAD_FEN | G.FLAG_NO_SCORE, 0)
    for i, (name, _, exp) in uploads["ev_cat"].items():
        if isinstance(exp, str):
            assert tuple(got[i]) == bad, name
    names = {i: e[0] for i, e in uploads["ev_cat"].items()}
    for k, i in enumerate(live):
        assert tuple(got[i]) == tuple(oracle[mode][k]), (names.get(i), texts[i], "oracle")
        assert tuple(got[i]) == tuple(host[k]), (names.get(i), texts[i], "gn_evaluate_batch")
    assert got[uploads["ev_good"]].tobytes() == alone.tobytes()  # the neighbours are not disturbed


def _run_expansion(ctx, boards, mode):
    """gn_expand_device + gn_rank_children_device (K_LINES), then gn_expand2_device, all outputs."""
    from fishnet_amd import gpu_nnue as G
    from test_gpu_parity import _expand2
    n = len(boards)
    cap = 220 * n  # (218 is the most legal moves of any position)
    b = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                       ("mv", cap * 2), ("co", cap * G.EVAL_SIZE), ("ln", n * K_LINES * 12))}
    b["b"].upload(boards)
    t = ctx.expand_device(b["b"], n, mode, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
    ctx.rank_children_device(b["b"], n, b["off"], b["mv"], b["co"], K_LINES, b["ln"])
    ctx.synchronize()
    r = {"t": t, "po": b["po"].download(G.EVAL_DTYPE, n), "off": b["off"].download(np.uint32, n + 1),
         "mv": b["mv"].download(np.uint16, t), "co": b["co"].download(G.EVAL_DTYPE, t),
         "ch": b["ch"].download(G.BOARD_DTYPE, t), "ln": b["ln"].download(G.LINE_DTYPE, n * K_LINES).reshape(n, K_LINES)}
    t2, g, out = _expand2(ctx, b["b"], n, mode)
    r.update(t2=t2, g=g, po2=out["po"].download(G.EVAL_DTYPE, n), off2=out["off"].download(np.uint32, n + 1),
             mv2=out["mv"].download(np.uint16, t2), co2=out["co"].download(G.EVAL_DTYPE, t2),
             ch2=out["ch"].download(G.BOARD_DTYPE, t2), goff=out["goff"].download(np.uint32, t2 + 1),
             gmv=out["gmv"].download(np.uint16, g), gco=out["gco"].download(G.EVAL_DTYPE, g))
    for x in list(b.values()) + [v for v in out.values() if hasattr(v, "free")]:
        x.free()
    return r


def _parent_view(r, i):
    """Everything the expansion returned for parent i, as bytes: parent record, moves, child
    records, lines, child boards, grandchild moves and records (both calls)."""
    lo, hi = int(r["off"][i]), int(r["off"][i + 1])
    lo2, hi2 = int(r["off2"][i]), int(r["off2"][i + 1])
    glo, ghi = int(r["goff"][lo2]), int(r["goff"][hi2])
    counts = np.diff(r["goff"][lo2:hi2 + 1].astype(np.int64))
    return (r["po"][i].tobytes(), r["mv"][lo:hi].tobytes(), r["co"][lo:hi].tobytes(), r["ln"][i].tobytes(),
            r["ch"][lo:hi].tobytes(), r["po2"][i].tobytes(), r["mv2"][lo2:hi2].tobytes(), r["co2"][lo2:hi2].tobytes(),
            r["ch2"][lo2:hi2].tobytes(), counts.tobytes(), r["gmv"][glo:ghi].tobytes(), r["gco"][glo:ghi].tobytes())


def check_boards_out(G, oracle_lib, parents, offsets, moves, children):
    """Every child board against the oracle's child of (the parent's FEN, the move): as a FEN, and
    all 32 bytes against gn_pack_fens of that FEN (reserved 0, unused nibbles 0).  A parent with
    fullmove 0 has no text of its own (a text's 0 reads as 1): its children keep 0 (white moved)
    or count from it, and are compared with the fullmove field put aside."""
    pfens = G.boards_to_fens(parents)
    cfens = G.boards_to_fens(children)
    want, who = [], []
    for i, pf in enumerate(pfens):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        if not pf:
            assert lo == hi, i
            continue
        assert sorted(int(m) for m in moves[lo:hi]) == sorted(oracle_lib.legal_moves(pf)), pf
        for j in range(lo, hi):
            want.append(oracle_lib.child_fen(pf, int(moves[j])))
            who.append((i, j))
    packed, ok = G.pack_fens(want)
    assert ok.all()
    for (i, j), w, p in zip(who, want, packed):
        got = children[j].copy()
        if int(parents[i]["fullmove"]) == 0:
            stm_black = int(parents[i]["stm_ep"]) >> 7
            assert int(got["fullmove"]) == stm_black, (pfens[i], j)
            assert cfens[j].rsplit(" ", 1)[0] == w.rsplit(" ", 1)[0], (pfens[i], G.move_to_uci(int(moves[j])))
            got["fullmove"] = p["fullmove"]
        else:
            assert cfens[j] == w, (pfens[i], G.move_to_uci(int(moves[j])))
        assert got.tobytes() == p.tobytes(), (pfens[i], G.move_to_uci(int(moves[j])), cfens[j])
    return len(want)


@pytest.fixture(scope="module")
def expansions(ctx, uploads):
    return {mode: (_run_expansion(ctx, uploads["xa"], mode), _run_expansion(ctx, uploads["xb"], mode))
            for mode in (1, 0)}


@pytest.mark.parametrize("mode", [1, 0])
def test_rejected_and_normalised_parents(expansions, uploads, mode):
    from fishnet_amd import gpu_nnue as G
    ra, rb = expansions[mode]
    bad = (0, 0, 0, 0, 0, G.FLAG_BAD_FEN | G.FLAG_NO_SCORE, 0)
    empty = np.array([lines_rule.EMPTY] * K_LINES, dtype=G.LINE_DTYPE)
    assert ra["t"] == ra["t2"] and np.array_equal(ra["off"], ra["off2"]) and np.array_equal(ra["mv"], ra["mv2"])
    assert np.array_equal(ra["po"], ra["po2"]) and np.array_equal(ra["co"], ra["co2"])
    assert ra["ch"].tobytes() == ra["ch2"].tobytes()
    seen = 0
    for i, (name, _, exp) in uploads["xa_cat"].items():
        if isinstance(exp, str):
            assert tuple(ra["po"][i]) == bad and tuple(ra["po2"][i]) == bad, name
            assert ra["off"][i] == ra["off"][i + 1] and ra["off2"][i] == ra["off2"][i + 1], name  # no children,
            assert np.array_equal(ra["ln"][i], empty), name  # only empty lines, and so no grandchildren
        else:
            assert _parent_view(ra, i) == _parent_view(rb, uploads["xb_of"][name]), name
            seen += int(ra["off"][i + 1] > ra["off"][i])
    assert seen > 40  # the normalised parents have children to compare


@pytest.mark.parametrize("mode", [1, 0])
def test_canonical_parents_vs_oracle(expansions, uploads, oracle_lib, oracle_nets, mode):
    """As test_expand_vs_oracle: parent record, move set and child records of every canonical
    parent (the good boards of expansion A, all of expansion B), and their K lines."""
    from fishnet_amd import gpu_nnue as G
    big, small = oracle_nets
    for r, fens, skip in ((expansions[mode][0], uploads["xa_fens"], set(uploads["xa_cat"])),
                          (expansions[mode][1], uploads["xb_fens"], set())):
        idx = [i for i in range(len(fens)) if i not in skip]
        exp_lines = lines_rule.lines(oracle_lib, big, small, [fens[i] for i in idx], mode, K_LINES)
        for k, i in enumerate(idx):
            fen = fens[i]
            p_exp, m_exp, k_exp = oracle_lib.expand_eval(big, small, fen, mode)
            assert tuple(r["po"][i]) == p_exp, fen
            lo, hi = int(r["off"][i]), int(r["off"][i + 1])
            got = {int(m): tuple(c) for m, c in zip(r["mv"][lo:hi], r["co"][lo:hi])}
            want = {int(m): tuple(c) for m, c in zip(m_exp, k_exp)}
            assert set(got) == set(want), (fen, sorted(map(G.move_to_uci, set(got) ^ set(want))))
            assert got == want, fen
            assert r["ln"][i].tolist() == exp_lines[k].tolist(), fen


@pytest.mark.parametrize("mode", [1, 0])
def test_boards_out(expansions, uploads, oracle_lib, mode):
    """Every child board gn_expand_device and gn_expand2_device wrote, of every valid parent."""
    from fishnet_amd import gpu_nnue as G
    ra, rb = expansions[mode]
    for p, m in _boards_out_parents():  # the list does what it says
        fen = p if isinstance(p, str) else G.board_to_fen(p)
        assert m in oracle_lib.legal_moves(fen), (fen, G.move_to_uci(m))
    for i, m in uploads["outs"]:
        assert m in rb["mv"][int(rb["off"][i]):int(rb["off"][i + 1])].tolist()
    for r, boards in ((ra, uploads["xa"]), (rb, uploads["xb"])):
        assert check_boards_out(G, oracle_lib, boards, r["off"], r["mv"], r["ch"]) == r["t"] > 0
        assert check_boards_out(G, oracle_lib, boards, r["off2"], r["mv2"], r["ch2"]) == r["t2"] > 0
