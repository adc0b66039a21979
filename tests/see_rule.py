"""The exchange evaluation and the pruned quiescence (include/gpu_nnue.h at gn_line, "exchange
evaluation") restated in Python, for tests/test_see.py and tests/test_gpu_see.py.

`see(O, fen, m, values)` is the rule as the header writes it -- the recursion R(P, occ, s) over the
attackers of the destination square -- on the oracle's placement `O._placement(fen)` alone: the oracle
has no attack function, so the geometry (pawn capture directions, knight and king steps, slider lines
with `occ` as the blockers) is restated here.  Nothing of the library's own SEE is read.

Qs, the searched set, d_ext, the lines and PVQs are tests/quiesce_rule.py's and tests/quiesce_pv_rule.py's
own functions with the rule's filter exchanged: `pruned()` swaps quiesce_rule's `searched_moves` and
`is_searched` (every other function of the two modules reaches the moves through them) for the kept
moves -- all legal moves in check, else the noisy ones with see >= 0 under the oracle's current
piece values -- and gives the memo of Q a dictionary of its own, so pruned and unpruned values never
mix.  The functions below named like quiesce_rule's run under it.
"""
import contextlib
import functools
import os

import lines2_rule as R2
import lines_rule as R
import quiesce_pv_rule as PV
import quiesce_rule as Q

DEFAULT_VALUES = (208, 781, 825, 1276, 2538)
REVERSED_VALUES = (900, 781, 825, 1276, 300)  # a second set that reverses an order: a pawn above a queen
ORDER = "pnbrqk"
KNIGHT_STEPS = ((1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1), (-2, 1), (-1, 2))
KING_STEPS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1))


def fixture_rows():
    """tests/golden/see_fens.txt: [(name, FEN, UCI move, see or None)]."""
    rows = []
    with open(os.path.join(R.HERE, "golden", "see_fens.txt")) as f:
        for l in f:
            if l.strip() and not l.startswith("#"):
                name, fen, uci, val = (x.strip() for x in l.split("|"))
                rows.append((name, fen, uci, None if val == "-" else int(val)))
    return rows


def find_move(O, fen, uci):
    """The legal move of fen a UCI text names (castling as king takes rook), in the 16-bit encoding."""
    code = R2.uci_move(uci)
    promo = "nbrq".index(uci[4]) if len(uci) == 5 else None
    for m in O.legal_moves(fen):
        if m & 0xFFF == code and ((m >> 14 == 1 and (m >> 12) & 3 == promo) if promo is not None else m >> 14 != 1):
            return m
    raise ValueError((fen, uci))


def _attacks(board, occ, sq, to):
    """The piece on sq attacks `to` with the blockers occ."""
    pc, t = board[sq], board[sq].lower()
    df, dr = (to & 7) - (sq & 7), (to >> 3) - (sq >> 3)
    if t == "p":
        return abs(df) == 1 and dr == (1 if pc == "P" else -1)
    if t == "n":
        return (df, dr) in KNIGHT_STEPS
    if t == "k":
        return (df, dr) in KING_STEPS
    straight, diagonal = (df == 0) != (dr == 0), abs(df) == abs(dr) and df != 0
    if not ((straight and t in "rq") or (diagonal and t in "bq")):
        return False
    sf, sr = (df > 0) - (df < 0), (dr > 0) - (dr < 0)
    x, y = (sq & 7) + sf, (sq >> 3) + sr
    while y * 8 + x != to:
        if y * 8 + x in occ:
            return False
        x, y = x + sf, y + sr
    return True


def _R(board, to, P, occ, white, v):
    A = [sq for sq in occ if sq != to and _attacks(board, occ, sq, to)]
    mine = [(ORDER.index(board[sq].lower()), sq) for sq in A if board[sq].isupper() == white]
    if not mine:
        return 0
    t, a = min(mine)
    others = any(board[sq].isupper() != white for sq in A)
    if ORDER[t] == "k":
        return 0 if others else max(0, v(P))
    return max(0, v(P) - _R(board, to, ORDER[t], occ - {a}, not white, v))


def see(O, fen, m, values=DEFAULT_VALUES):
    """see(fen, m) of the rule for a legal move m of fen, with v(P N B R Q) = values."""
    if m >> 14 != 0:
        return 0
    board = O._placement(fen)
    frm, to = (m >> 6) & 63, m & 63
    v = lambda ch: 0 if ch.lower() == "k" else values[ORDER.index(ch.lower())]
    c = v(board[to]) if to in board else 0
    return c - _R(board, to, board[frm], frozenset(board) - {frm}, not board[frm].isupper(), v)


# ---- the pruned quiescence: quiesce_rule / quiesce_pv_rule with the filter exchanged ----

def _values(O):
    return tuple(int(x) for x in O.eval_params().piece_value)


@functools.lru_cache(maxsize=None)
def _see_cached(O, fen, m, values):
    return see(O, fen, m, values)


def kept(O, fen, m, values=None):
    """A kept move: noisy with see >= 0."""
    return Q.noisy(O, fen, m) and _see_cached(O, fen, m, values or _values(O)) >= 0


def kept_moves(O, big, small, fen, mode, check):
    """The entries of Q.node(fen) the pruned quiescence searches: all in check, the kept ones otherwise."""
    values = _values(O)
    return [k for k in Q.node(O, big, small, fen, mode) if check or (k[4] and kept(O, fen, k[0], values))]


def is_searched(O, big, small, fen, mode, check):
    """A leaf is searched under pruning: it has a legal move and is in check, or it has a kept move."""
    return Q.alive(O, fen) and (check or bool(kept_moves(O, big, small, fen, mode, False)))


_qs = {}


@contextlib.contextmanager
def pruned():
    saved = Q.searched_moves, Q.is_searched, Q._q
    Q.searched_moves, Q.is_searched, Q._q = kept_moves, is_searched, _qs
    try:
        yield
    finally:
        Q.searched_moves, Q.is_searched, Q._q = saved


def _under_pruning(fn):
    @functools.wraps(fn)
    def run(*a, **k):
        with pruned():
            return fn(*a, **k)
    return run


Qs = _under_pruning(Q.Q)
leaves = _under_pruning(Q.leaves)
extensions = _under_pruning(Q.extensions)
all_lines = _under_pruning(Q.all_lines)
all_lines2 = _under_pruning(Q.all_lines2)
lines = _under_pruning(Q.lines)
lines2 = _under_pruning(Q.lines2)
game_lines = _under_pruning(Q.game_lines)
game_lines2 = _under_pruning(Q.game_lines2)
pvqs = _under_pruning(PV.pvq)
tails = _under_pruning(PV.tails)
line_pvs = _under_pruning(PV.line_pvs)
line2_pvs = _under_pruning(PV.line2_pvs)


def losing_below(O, big, small, fen, depth, mode):
    """(noisy legal moves with see < 0 at fen's searched leaves that are not in check, the same at the
    nodes the UNPRUNED search visits below them down to `depth`): what the pruning would remove."""
    at0 = below = 0

    def walk(f, d, check, level):
        nonlocal at0, below
        if d == 0 or not Q.alive(O, f):
            return
        if not check:
            n = sum(1 for k in Q.node(O, big, small, f, mode) if k[4] and not kept(O, f, k[0]))
            if level:
                below += n
            else:
                at0 += n
        for _, c, kcheck, _, _ in Q.searched_moves(O, big, small, f, mode, check):
            walk(c, d - 1, kcheck, level + 1)

    for _, c, check, live, _, srch in Q.leaves(O, big, small, fen, mode) or []:
        if srch:
            walk(c, depth, check, 0)
    return at0, below
