"""Regenerates tests/golden/row_cover_fens.txt: positions that together read every reachable row of
the HalfKAv2_hm feature-transformer table (22528 rows = 32 king buckets x 11 planes x 64 squares).

Playouts from the start position touch well under half of the table, so a wrong row in the device
copy (LEB128 decode, doubling, padded stride, per-bucket PSQT copy) would go unseen.  This file is
built the other way round: seeded random placements, chosen greedily for the rows they add.

  * A row is reachable when, for some own-king square, it is a non-king plane on another square
    (pawn planes on ranks 2-7 only) or the king plane on the own king's square or on an enemy-king
    square that is not adjacent.
  * Every position has one king each, at most 32 pieces, no pawn on a back rank, the side not to
    move not in check (what `oracle.normalize_fen` and the product's parser accept), at most
    3 queens, 4 rooks, 4 bishops, 4 knights and 8 pawns a side, and at most MAX_MOVES legal moves.
    A piece that attacks a king is placed only where the row needs it (an enemy piece next to the
    own king is a reachable row), in one position of CHECK_EVERY and in the finishing phase; the
    attacked side is then the one to move.  Most positions have no check, so the score rule's
    search stays cheap.
  * Piece counts cycle over the eight piece-count buckets (count - 1) // 4 until each holds PER_BUCKET
    positions; what is still uncovered then is finished with 32-piece positions.
  * King squares are the pair that adds most king-plane rows, then most uncovered piece rows; each
    further square takes the piece that adds most rows over both perspectives.

The rows of every written FEN are `oracle.features` of it (the Python index below only steers the
search; every oracle row is asserted to lie in the reachable set).  Run from the repo root:  python tests/golden/make_row_cover.py
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402

SEED = 20240607
PER_BUCKET = 150
MAX_FENS = 2500
MAX_MOVES = 120
CHECK_EVERY = 16
LIMIT = {"p": 8, "n": 4, "b": 4, "r": 4, "q": 3}
PT = {"p": 0, "n": 1, "b": 2, "r": 3, "q": 4}


def row(persp, ksq, sq, plane):
    """HalfKAv2_hm row of `plane` on `sq` for perspective `persp` (0 white) with its king on ksq."""
    orient = (7 if (ksq & 7) < 4 else 0) ^ (56 if persp else 0)
    rel_rank = (ksq >> 3) if persp == 0 else 7 - (ksq >> 3)
    f = ksq & 7
    bucket = 4 * (7 - rel_rank) + min(f, 7 - f)
    return (sq ^ orient) + plane * 64 + bucket * 704


def adjacent(a, b):
    return max(abs((a & 7) - (b & 7)), abs((a >> 3) - (b >> 3))) <= 1


def reachable_rows():
    out = set()
    for k in range(64):
        for sq in range(64):
            if sq == k:
                out.add(row(0, k, sq, 10))
                continue
            for plane in range(10):
                if plane < 2 and not 1 <= (sq >> 3) <= 6:
                    continue
                out.add(row(0, k, sq, plane))
            if not adjacent(k, sq):
                out.add(row(0, k, sq, 10))
    return out


def piece_rows(kw, kb, sq, colour, letter):
    """The two rows (white's and black's perspective) of a non-king piece."""
    pt = PT[letter]
    return row(0, kw, sq, 2 * pt + (colour != 0)), row(1, kb, sq, 2 * pt + (colour != 1))


def fen_of(board, stm, rule50):
    ranks = []
    for r in range(7, -1, -1):
        s, gap = "", 0
        for f in range(8):
            c = board.get(r * 8 + f)
            if c is None:
                gap += 1
            else:
                s += (str(gap) if gap else "") + c
                gap = 0
        ranks.append(s + (str(gap) if gap else ""))
    return f"{'/'.join(ranks)} {'wb'[stm]} - - {rule50} 1"


def safe(board, colour):
    """True when `colour`'s king is not attacked (normalize_fen rejects a position whose side not
    to move is in check)."""
    try:
        O.normalize_fen(fen_of(board, 1 - colour, 0))
        return True
    except ValueError:
        return False


def rows_of(fen):
    return set(O.features(fen, 0)) | set(O.features(fen, 1))


def build_position(rng, todo, count, checks):
    pairs = [(kw, kb) for kw in range(64) for kb in range(64) if not adjacent(kw, kb)]
    per_king = [[0, 0] for _ in range(64)]  # uncovered piece rows by (king square, perspective)
    for k in range(64):
        for persp in (0, 1):
            per_king[k][persp] = sum(row(persp, k, sq, pl) in todo for sq in range(64) for pl in range(10))

    def pair_score(p):
        kw, kb = p
        kings = (row(0, kw, kb, 10) in todo) + (row(1, kb, kw, 10) in todo) + \
                (row(0, kw, kw, 10) in todo) + (row(1, kb, kb, 10) in todo)
        return kings * 100000 + per_king[kw][0] + per_king[kb][1] + rng.random()

    kw, kb = max(pairs, key=pair_score)
    board = {kw: "K", kb: "k"}
    left = [dict(LIMIT), dict(LIMIT)]
    squares = [s for s in range(64) if s not in board]
    rng.shuffle(squares)
    got, forced = set(), None
    for sq in squares:
        if len(board) >= count:
            break
        cand = []
        for colour in (0, 1):
            for letter in "pnbrq":
                if not left[colour][letter] or (letter == "p" and not 1 <= (sq >> 3) <= 6):
                    continue
                a, b = piece_rows(kw, kb, sq, colour, letter)
                gain = (a in todo and a not in got) + (b in todo and b not in got)
                cand.append((gain + rng.random() * 0.5, colour, letter))
        for g, colour, letter in sorted(cand, reverse=True)[:6]:
            board[sq] = letter.upper() if colour == 0 else letter
            hit = None if safe(board, 0) else 0
            if not safe(board, 1):
                hit = 1 if hit is None else 2
            # a piece that attacks a king is kept only for the rows it adds, and only that king's
            # side may then be the one to move
            if hit == forced or (checks and g >= 1 and hit in (0, 1) and forced is None):
                forced = hit
                left[colour][letter] -= 1
                got.update(piece_rows(kw, kb, sq, colour, letter))
                break
            del board[sq]
    if len(board) != count:
        return None
    stm = rng.randrange(2) if forced is None else forced
    fen = O.normalize_fen(fen_of(board, stm, rng.choice([0, 0, rng.randrange(100)])))
    if len(O.legal_moves(fen)) > MAX_MOVES:
        return None
    return fen


def main():
    rng = random.Random(SEED)
    reach = reachable_rows()
    todo = set(reach)
    fens, per_bucket = [], [0] * 8
    while todo or min(per_bucket) < PER_BUCKET:
        short = [b for b in range(8) if per_bucket[b] < PER_BUCKET]
        if short:
            b = short[len(fens) % len(short)]
            count = rng.randrange(max(4 * b + 1, 2), 4 * b + 5)
        else:
            count = 32
        fen = build_position(rng, todo, count, checks=not short or len(fens) % CHECK_EVERY == CHECK_EVERY - 1)
        if fen is None:
            continue
        rows = rows_of(fen)
        assert rows <= reach, fen
        fens.append(fen)
        per_bucket[(sum(c.isalpha() for c in fen.split()[0]) - 1) // 4] += 1
        todo -= rows
        if len(fens) % 100 == 0:
            print(len(fens), len(todo), per_bucket, file=sys.stderr)
        assert len(fens) <= MAX_FENS
    with open(os.path.join(ROOT, "tests", "golden", "row_cover_fens.txt"), "w") as f:
        f.write("# Row-cover positions (tests/golden/make_row_cover.py, seed %d): %d FENs that together read all\n"
                "# %d reachable rows of the 22528-row feature-transformer table; piece-count buckets hold %s.\n"
                % (SEED, len(fens), len(reach), " ".join(map(str, per_bucket))))
        f.write("\n".join(fens) + "\n")
    print(len(fens), "fens,", len(reach), "reachable rows, buckets", per_bucket)


if __name__ == "__main__":
    main()
