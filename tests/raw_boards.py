"""Raw gn_board records made by hand, for tests/test_raw_boards.py and tests/test_gpu_raw_boards.py.

Pure numpy and Python: nothing here calls the library, so the 32-byte format (include/gpu_nnue.h at
gn_board) is pinned against a second, independent packer, and the device can be fed boards the
host FEN parser never saw.

  make(...)          a BOARD_DTYPE record from a {square: piece code} dict, nothing validated
  fen_text(board)    the FEN text that spells a record's fields, nothing validated either
  from_fen(fen)      a valid FEN -> make() arguments -> record (X-FEN / Shredder castling; the
                     en-passant square and the castling rights kept by the contract's C4 / C5 rules,
                     restated here on the piece dict)
  catalogue()        [(name, board, expected)]: expected is "bad" or the canonical board
"""
import numpy as np

BOARD_DTYPE = np.dtype([("occ", "<u8"), ("pc", "u1", (16,)), ("stm_ep", "u1"), ("reserved", "u1"),
                        ("castle", "<u2"), ("rule50", "<u2"), ("fullmove", "<u2")])
assert BOARD_DTYPE.itemsize == 32

WP, WN, WB, WR, WQ, WK = 1, 2, 3, 4, 5, 6
BP, BN, BB, BR, BQ, BK = 9, 10, 11, 12, 13, 14
WHITE, BLACK = 0, 1
NO_EP = 64
_CHARS = {c: i + 1 for i, c in enumerate("PNBRQK")}
_CHARS.update({c: i + 9 for i, c in enumerate("pnbrqk")})
_LETTER = {v: k for k, v in _CHARS.items()}


def sq(name):
    return (ord(name[1]) - ord("1")) * 8 + ord(name[0]) - ord("a")


def sq_name(s):
    return "abcdefgh"[s & 7] + str((s >> 3) + 1)


def placement(text):
    """'4k3/8/...' -> {square: code}."""
    out, rank, file = {}, 7, 0
    for ch in text:
        if ch == "/":
            rank, file = rank - 1, 0
        elif ch.isdigit():
            file += int(ch)
        else:
            out[rank * 8 + file] = _CHARS[ch]
            file += 1
    assert rank == 0 and file == 8, text
    return out


def make(pieces, stm, ep=NO_EP, castle=(None,) * 4, rule50=0, fullmove=1, reserved=0, junk=0, castle_low=(0,) * 4):
    """A BOARD_DTYPE record.  pieces: {square: code 0..15}, written as they are (squares past the
    32nd have no nibble); castle[i]: the rook's file or None; castle_low[i]: the low bits of a
    nibble without a right; junk: the value of every unused nibble."""
    b = np.zeros((), dtype=BOARD_DTYPE)
    occ, nib = 0, [junk & 15] * 32
    for k, s in enumerate(sorted(pieces)):
        occ |= 1 << s
        if k < 32:
            nib[k] = pieces[s] & 15
    b["occ"] = occ
    b["pc"] = [nib[2 * i] | nib[2 * i + 1] << 4 for i in range(16)]
    b["stm_ep"] = (stm << 7) | (ep & 0x7F)
    b["reserved"] = reserved
    c = 0
    for i in range(4):
        c |= ((8 | castle[i]) if castle[i] is not None else (castle_low[i] & 7)) << (4 * i)
    b["castle"] = c
    b["rule50"], b["fullmove"] = rule50, fullmove
    return b


def fields(board):
    """(pieces, stm, ep, castle nibbles[4], rule50, fullmove) of a record; pieces past the 32nd
    nibble read as None."""
    occ = int(board["occ"])
    pc = [int(x) for x in board["pc"]]
    pieces, k = {}, 0
    for s in range(64):
        if occ >> s & 1:
            pieces[s] = (pc[k >> 1] >> (4 * (k & 1))) & 15 if k < 32 else None
            k += 1
    se = int(board["stm_ep"])
    nibs = [(int(board["castle"]) >> (4 * i)) & 15 for i in range(4)]
    return pieces, se >> 7, se & 0x7F, nibs, int(board["rule50"]), int(board["fullmove"])


def fen_text(board):
    """The FEN text that spells the record's fields: castle nibbles with bit 3 set as Shredder
    file letters, ep as its square name, rule50 and fullmove as numbers.  Nothing is validated;
    a piece nibble that is no piece or an ep field above 64 has no spelling (ValueError)."""
    pieces, stm, ep, nibs, rule50, fullmove = fields(board)
    rows = []
    for r in range(7, -1, -1):
        row, empty = "", 0
        for f in range(8):
            s = r * 8 + f
            if s not in pieces:
                empty += 1
                continue
            if empty:
                row, empty = row + str(empty), 0
            code = pieces[s]
            if code is None:  # past the 32nd piece: any piece keeps the count
                code = WN
            if code not in _LETTER:
                raise ValueError(f"piece code {code} has no FEN letter")
            row += _LETTER[code]
        rows.append(row + (str(empty) if empty else ""))
    if ep > 64:
        raise ValueError(f"en-passant field {ep} has no square name")
    rights = "".join(("ABCDEFGH" if i < 2 else "abcdefgh")[n & 7] for i, n in enumerate(nibs) if n & 8)
    return f"{'/'.join(rows)} {'wb'[stm]} {rights or '-'} {sq_name(ep) if ep < 64 else '-'} {rule50} {fullmove}"


# ---- the contract's C4 / C5 restated on the piece dict (for from_fen and the catalogue's self-check)
def keep_right(pieces, slot, file):
    c = slot >> 1
    back = 7 if c else 0
    kings = [s for s, p in pieces.items() if p == (BK if c else WK)]
    if len(kings) != 1 or kings[0] >> 3 != back:
        return False
    r = back * 8 + file
    if pieces.get(r) != (BR if c else WR):
        return False
    return r > kings[0] if slot & 1 == 0 else r < kings[0]


def keep_ep(pieces, stm, ep):
    if ep >= 64 or ep >> 3 != (5 if stm == WHITE else 2):
        return False
    up = 8 if stm == WHITE else -8
    own, enemy = (WP, BP) if stm == WHITE else (BP, WP)
    f = ep & 7
    capturer = any(0 <= f + df < 8 and pieces.get(ep - up + df) == own for df in (-1, 1))
    return capturer and pieces.get(ep - up) == enemy and ep not in pieces and ep + up not in pieces


def from_fen(fen):
    """A valid FEN -> record, through make()."""
    parts = fen.split() + ["w", "-", "-", "0", "1"][len(fen.split()) - 1:]
    pieces = placement(parts[0])
    stm = BLACK if parts[1] == "b" else WHITE
    castle = [None] * 4
    for ch in parts[2]:
        if ch == "-":
            continue
        c = BLACK if ch.islower() else WHITE
        back, rook, king = (7, BR, BK) if c else (0, WR, WK)
        ksq = next(s for s, p in pieces.items() if p == king)
        rooks = [s for s in range(back * 8, back * 8 + 8) if pieces.get(s) == rook]
        u = ch.upper()
        if u == "K":
            r = max(rooks, default=None)
        elif u == "Q":
            r = min(rooks, default=None)
        else:
            r = back * 8 + ord(u) - ord("A")
        if r is None:
            continue
        slot = 2 * c + (0 if r > ksq else 1)
        if keep_right(pieces, slot, r & 7):
            castle[slot] = r & 7
    ep = sq(parts[3]) if parts[3] != "-" else NO_EP
    if not keep_ep(pieces, stm, ep):
        ep = NO_EP
    return make(pieces, stm, ep, tuple(castle), int(parts[4]), int(parts[5]))


def canonical_fields(board):
    """The record with C1..C5 applied (not the rejection rules): what an accepted board equals."""
    pieces, stm, ep, nibs, rule50, fullmove = fields(board)
    castle = tuple((n & 7) if n & 8 and keep_right(pieces, i, n & 7) else None for i, n in enumerate(nibs))
    return make(pieces, stm, ep if keep_ep(pieces, stm, ep) else NO_EP, castle, rule50, fullmove)


# ---- the catalogue ------------------------------------------------------------------------------
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR"
KINGS = "4k3/8/8/8/8/8/8/4K3"
# white is a queen up (the small net's side of the FULL selection), no castling, no pawn captures
C6_PLACEMENT = "r4rk1/pp3ppp/2n5/8/8/2N5/PPPQ1PPP/R4RK1"
C6_RULE50 = (0, 99, 100, 211, 212, 1000, 65535)
C6_FULLMOVE = (0, 1, 65535)
R2_CODES, R2_INDEX = (0, 7, 8, 15), (0, 15, 16, 31)

REQUIRED = (
    ["R1/count%d" % n for n in (0, 1, 33, 64)]
    + ["R2/code%d-nibble%d" % (c, k) for c in R2_CODES for k in R2_INDEX]
    + ["R3/no-white-king", "R3/no-black-king", "R3/two-white-kings", "R3/two-black-kings"]
    + ["R4/%s-pawn-rank%d" % (c, r) for c in ("white", "black") for r in (1, 8)]
    + ["R5/ep65", "R5/ep127"]
    + ["R6/%s-to-move-%s" % (c, p) for c in ("white", "black") for p in "PNBRQ"]
    + ["R6/adjacent-kings-white-to-move", "R6/adjacent-kings-black-to-move", "R6/pinned-capturer",
       "R6/mover-in-check-too"]
    + ["C1/reserved-ff", "C2/junk-2-pieces", "C2/junk-31-pieces"]
    + ["C3/slot%d" % i for i in range(4)]
    + ["C4/%s-%s" % (c, k) for c in ("white", "black")
       for k in ("no-rook", "enemy-rook", "knight", "rook-rank2", "king-off-rank", "slot0-left-rook",
                 "slot0-left-rook-and-slot1")]
    + ["C5/no-capturer", "C5/no-pawn-to-capture", "C5/ep-square-occupied", "C5/origin-occupied",
       "C5/wrong-rank", "C5/ep0", "C5/ep63", "C5/consistent-white", "C5/consistent-black"]
    + ["C6/rule50-%d-fullmove-%d" % (r, f) for r in C6_RULE50 for f in C6_FULLMOVE]
)
# no FEN text spells these (fen_text raises): the text-based parities skip them by name
NO_TEXT = frozenset(n for n in REQUIRED if n.startswith(("R2/", "R5/")))
# a text names a right by its file alone and the parser files it under the side the rook is on, so
# a right in the other side's slot (dropped, C4) reads as that side's right in the text
SLOT_NOT_IN_TEXT = frozenset(["C4/white-slot0-left-rook", "C4/black-slot0-left-rook"])


def _mirror(pieces):
    """Colours swapped, ranks flipped."""
    return {s ^ 56: p ^ 8 for s, p in pieces.items()}


def catalogue():
    out = []

    def bad(name, board):
        out.append((name, board, "bad"))

    def good(name, board, canon):
        out.append((name, board, canon))

    # R1: popcount(occ) of 0, 1, 33, 64
    bad("R1/count0", make({}, WHITE))
    bad("R1/count1", make({sq("e1"): WK}, WHITE))
    p33 = {s: WN for s in range(8, 39)}
    p33.update({sq("a1"): WK, sq("h8"): BK})
    assert len(p33) == 33
    bad("R1/count33", make(p33, WHITE))
    p64 = {s: WN for s in range(64)}
    p64.update({sq("a1"): WK, sq("h8"): BK})
    bad("R1/count64", make(p64, WHITE))
    # R2: a piece nibble that is no piece, at both ends of both 64-bit words of pc
    start = placement(START)
    order = sorted(start)
    for code in R2_CODES:
        for k in R2_INDEX:
            p = dict(start)
            p[order[k]] = code
            bad("R2/code%d-nibble%d" % (code, k), make(p, WHITE))
    # R3
    bad("R3/no-white-king", make({sq("e8"): BK, sq("a1"): WR}, WHITE))
    bad("R3/no-black-king", make({sq("e1"): WK, sq("a8"): BR}, WHITE))
    bad("R3/two-white-kings", make({sq("a1"): WK, sq("h1"): WK, sq("e8"): BK}, WHITE))
    bad("R3/two-black-kings", make({sq("a8"): BK, sq("h8"): BK, sq("e1"): WK}, BLACK))
    # R4: the pawn stands where it attacks nothing
    kings = placement(KINGS)
    for colour, code in (("white", WP), ("black", BP)):
        for rank, s in ((1, "a1"), (8, "a8")):
            bad("R4/%s-pawn-rank%d" % (colour, rank), make({**kings, sq(s): code}, WHITE))
    # R5
    ep_ok = placement("4k3/8/8/3Pp3/8/8/8/4K3")
    bad("R5/ep65", make(ep_ok, WHITE, ep=65))
    bad("R5/ep127", make(ep_ok, WHITE, ep=127))
    # R6: the side not to move is in check.  White to move and the black king on e8 attacked; the
    # mirror for black to move.
    attackers = {"P": ("d7", WP), "N": ("f6", WN), "B": ("b5", WB), "R": ("e2", WR), "Q": ("h5", WQ)}
    for letter, (s, code) in attackers.items():
        p = {**kings, sq(s): code}
        bad("R6/white-to-move-" + letter, make(p, WHITE))
        bad("R6/black-to-move-" + letter, make(_mirror(p), BLACK))
    adj = {sq("e1"): WK, sq("e2"): BK, sq("a8"): WR}
    bad("R6/adjacent-kings-white-to-move", make(adj, WHITE))
    bad("R6/adjacent-kings-black-to-move", make(adj, BLACK))
    # the knight d1 is pinned to a1 by the rook h1 and still attacks e3
    bad("R6/pinned-capturer", make({sq("a1"): WK, sq("d1"): WN, sq("h1"): BR, sq("e3"): BK}, WHITE))
    # white to move is in check from e5 and attacks e8 from b5
    bad("R6/mover-in-check-too", make({**kings, sq("e5"): BR, sq("b5"): WB}, WHITE))

    # C1, C2
    full = (7, 0, 7, 0)
    good("C1/reserved-ff", make(start, WHITE, castle=full, reserved=0xFF), make(start, WHITE, castle=full))
    good("C2/junk-2-pieces", make(kings, BLACK, junk=15, rule50=3, fullmove=40), make(kings, BLACK, rule50=3, fullmove=40))
    p31 = {s: c for s, c in start.items() if s != sq("h7")}
    good("C2/junk-31-pieces", make(p31, BLACK, castle=full, junk=15), make(p31, BLACK, castle=full))
    # C3: rooks on b and g, every castling move playable; the low bits name the slot's rook
    rooks = placement("1r2k1r1/8/8/8/8/8/8/1R2K1R1")
    for i in range(4):
        low = [0] * 4
        low[i] = 6 if i % 2 == 0 else 1
        good("C3/slot%d" % i, make(rooks, i >> 1, castle_low=tuple(low)), make(rooks, i >> 1))
    # C4: slot 0 (slot 2 for black, mirrored), the side with the right to move
    c4 = {
        "no-rook": ({**kings, sq("a8"): BR}, (7, None)),
        "enemy-rook": ({**kings, sq("h1"): BR}, (7, None)),  # (white to move is in check: a valid position)
        "knight": ({**kings, sq("h1"): WN}, (7, None)),
        "rook-rank2": ({**kings, sq("h2"): WR}, (7, None)),
        "king-off-rank": ({sq("e2"): WK, sq("e8"): BK, sq("h1"): WR}, (7, None)),
        "slot0-left-rook": ({**kings, sq("a1"): WR}, (0, None)),
    }
    for colour in ("white", "black"):
        for key, (p, (s0, s1)) in c4.items():
            if colour == "white":
                good("C4/white-" + key, make(p, WHITE, castle=(s0, s1, None, None)), make(p, WHITE))
            else:
                good("C4/black-" + key, make(_mirror(p), BLACK, castle=(None, None, s0, s1)), make(_mirror(p), BLACK))
        p = {**kings, sq("a1"): WR}
        if colour == "white":
            good("C4/white-slot0-left-rook-and-slot1", make(p, WHITE, castle=(0, 0, None, None)),
                 make(p, WHITE, castle=(None, 0, None, None)))
        else:
            good("C4/black-slot0-left-rook-and-slot1", make(_mirror(p), BLACK, castle=(None, None, 0, 0)),
                 make(_mirror(p), BLACK, castle=(None, None, None, 0)))
    # C5 (white to move, ep e6, unless said)
    e6 = sq("e6")

    def c5(name, text, stm=WHITE, ep=e6, keep=False):
        p = placement(text)
        good("C5/" + name, make(p, stm, ep=ep), make(p, stm, ep=ep if keep else NO_EP))

    c5("no-capturer", "4k3/8/8/4p3/8/8/8/4K3")
    c5("no-pawn-to-capture", "4k3/8/8/3P4/8/8/8/4K3")
    c5("ep-square-occupied", "4k3/8/4n3/3Pp3/8/8/8/4K3")
    c5("origin-occupied", "4k3/4n3/8/3Pp3/8/8/8/4K3")
    c5("wrong-rank", "4k3/8/8/8/3pP3/8/8/4K3", ep=sq("e3"))  # black's capture, white to move
    c5("ep0", "4k3/8/8/3Pp3/8/8/8/4K3", ep=0)
    c5("ep63", "4k3/8/8/3Pp3/8/8/8/4K3", ep=63)
    c5("consistent-white", "4k3/8/8/3Pp3/8/8/8/4K3", keep=True)
    c5("consistent-black", "4k3/8/8/8/3pP3/8/8/4K3", stm=BLACK, ep=sq("e3"), keep=True)
    # C6: taken as they are
    p6 = placement(C6_PLACEMENT)
    for r in C6_RULE50:
        for f in C6_FULLMOVE:
            b = make(p6, WHITE, rule50=r, fullmove=f)
            good("C6/rule50-%d-fullmove-%d" % (r, f), b, b.copy())

    names = [n for n, _, _ in out]
    assert len(set(names)) == len(names), "duplicate catalogue names"
    missing = [n for n in REQUIRED if n not in names]
    assert not missing, f"catalogue entries missing: {missing}"
    # the hand-written expectations agree with the contract's C rules restated above
    for name, board, exp in out:
        if not isinstance(exp, str):
            assert canonical_fields(board).tobytes() == exp.tobytes(), name
            assert canonical_fields(exp).tobytes() == exp.tobytes(), name
    return out
