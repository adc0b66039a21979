"""Parameter sets, the input list and a Python restatement for the gn_eval_params tests (test
infrastructure only): tests/test_eval_params.py checks the oracle's parameterised epilogue with
them on the CPU, tests/test_gpu_eval_params.py the GPU against that oracle.

The restatement (`restate`) is written from the field comments of gn_eval_params and the mode /
flag comments in include/gpu_nnue.h, not from oracle/oracle.c: int32 wrap arithmetic, C's
truncating division, IEEE doubles without contraction (Python floats) and std::round's
half-away-from-zero.  It takes a position's net outputs from the oracle (`net_output`) and
everything else from the FEN.
"""
import ctypes as C
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))
INT32_MAX = 2**31 - 1
FLAG_SMALLNET, FLAG_REEVAL = 2, 8
THREADS = 16

# the 28 scalars of gn_eval_params in declaration order: (field, index or None)
SCALARS = ([(n, None) for n in (
    "small_net_threshold", "psqt_weight", "positional_weight", "reeval_threshold", "complexity_div_small",
    "complexity_div_big", "material_pawn_small", "material_pawn_big", "material_base", "rule50_div", "value_clamp")]
    + [("piece_value", i) for i in range(5)] + [("wdl_a", i) for i in range(4)]
    + [("wdl_material_min", None), ("wdl_material_max", None), ("wdl_material_anchor", None)]
    + [("wdl_piece_weight", i) for i in range(5)])
assert len(SCALARS) == 28

# ---- the named sets (ISSUE: each changes few fields, so that a failure points at one) --------
NAMED = {
    "weights": dict(psqt_weight=111, positional_weight=143, reeval_threshold=150),
    "small-vs-big": dict(complexity_div_small=9000, complexity_div_big=27000, material_pawn_small=400,
                         material_pawn_big=700),
    "material": dict(material_base=50000, piece_value=(180, 700, 900, 1400, 2300), small_net_threshold=600),
    "rule50/clamp": dict(rule50_div=100, value_clamp=300),
    "negative divisor": dict(rule50_div=-212),
    "ties": dict(wdl_a=(0.0, 0.0, 0.0, 200.0)),
    "ties-poly": dict(wdl_a=(-20.5, 80.25, -90.125, 300.0625), wdl_piece_weight=(2, 3, 4, 6, 10),
                      wdl_material_min=10, wdl_material_max=60, wdl_material_anchor=40),
    # a(material) = 194 * m + a3 with m = 31 / 58 for every position: the rounded product plus a3 is
    # exactly half way between 200 and the next double, so unfused arithmetic gives a = 200 (ties to
    # even) and every odd final_v an exact tie, while a fused multiply-add gives the next double
    # above 200 and every odd final_v the other rounding (fma_a below; test_eval_params.py)
    "ties-fma": dict(wdl_a=(0.0, 0.0, 194.0, float.fromhex("0x1.813dcb08d3dcdp+6")), wdl_material_min=31,
                     wdl_material_max=31, wdl_material_anchor=58),
    "all small": dict(small_net_threshold=-1, reeval_threshold=0),
    "never small": dict(small_net_threshold=INT32_MAX),
    "always re-evaluated": dict(reeval_threshold=INT32_MAX),
    "wrap": dict(psqt_weight=2_000_003, positional_weight=-1_999_993, material_base=7),
}
# oracle/sanitize_main.c's PARAMS (the sanitizer driver's non-default pass)
SANITIZE_SET = dict(small_net_threshold=700, psqt_weight=2_000_003, positional_weight=-1_999_993, reeval_threshold=150,
                    complexity_div_small=9000, complexity_div_big=27000, material_pawn_small=400,
                    material_pawn_big=700, material_base=50000, rule50_div=-212, value_clamp=300,
                    piece_value=(180, 700, 900, 1400, 2300), wdl_a=(-20.5, 80.25, -90.125, 300.0625),
                    wdl_material_min=10, wdl_material_max=60, wdl_material_anchor=40,
                    wdl_piece_weight=(2, 3, 4, 6, 10))
EXTREMES = ("all small", "never small", "always re-evaluated")
TIES = ("ties", "ties-poly", "ties-fma")

# one scalar moved off its default, everything else at the defaults: (field, index) -> value
SINGLE = {
    ("small_net_threshold", None): 700, ("psqt_weight", None): 126, ("positional_weight", None): 130,
    ("reeval_threshold", None): 300, ("complexity_div_small", None): 9000, ("complexity_div_big", None): 12000,
    ("material_pawn_small", None): 600, ("material_pawn_big", None): 500, ("material_base", None): 60000,
    ("rule50_div", None): 200, ("value_clamp", None): 150,
    ("piece_value", 0): 245, ("piece_value", 1): 818, ("piece_value", 2): 862, ("piece_value", 3): 1313,
    ("piece_value", 4): 2575,
    ("wdl_a", 0): -30.0, ("wdl_a", 1): 125.0, ("wdl_a", 2): -128.0, ("wdl_a", 3): 400.0,
    ("wdl_material_min", None): 30, ("wdl_material_max", None): 60, ("wdl_material_anchor", None): 50,
    ("wdl_piece_weight", 0): 2, ("wdl_piece_weight", 1): 4, ("wdl_piece_weight", 2): 4, ("wdl_piece_weight", 3): 6,
    ("wdl_piece_weight", 4): 10,
}
assert list(SINGLE) == SCALARS


def single_name(key):
    return key[0] if key[1] is None else f"{key[0]}[{key[1]}]"


def make(oracle_lib, overrides=None, single=None):
    """The oracle's defaults with `overrides` (field -> value or tuple) or one `single` key applied."""
    oracle_lib.set_eval_params(None)
    p = oracle_lib.eval_params()
    for k, v in (overrides or {}).items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(p, k)[i] = x
        else:
            setattr(p, k, v)
    if single is not None:
        if single[1] is None:
            setattr(p, single[0], SINGLE[single])
        else:
            getattr(p, single[0])[single[1]] = SINGLE[single]
    return p


def all_sets(oracle_lib):
    """[(name, params)]: the named sets, then the 28 single-field sets."""
    return ([(n, make(oracle_lib, o)) for n, o in NAMED.items()]
            + [(single_name(k), make(oracle_lib, single=k)) for k in SINGLE])


def as_gpu(p):
    """An oracle parameter structure as the GPU wrapper's (same layout: test_eval_params.py)."""
    from fishnet_amd import gpu_nnue as G
    return G.EvalParams.from_buffer_copy(bytes(p))


# ---- the input list ---------------------------------------------------------------------------
def _lines(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]


def score_fixture_fens():
    with open(os.path.join(HERE, "golden", "score_fens.json")) as f:
        return [r[0] for r in json.load(f)["results"]["full"]]


def input_fens():
    """About 600 fixed positions: the special positions (bare kings, nine queens, rule50 99 and
    150), the score fixture (mates, stalemates, searched in-check positions) and 500 seeded
    random playouts of up to 160 plies."""
    from fishnet_amd import gpu_nnue as G
    rnd = [G.board_to_fen(b) for b in G.random_positions(0x5EED0E50, 0, 500, 160)]
    return _lines("special_fens.txt") + score_fixture_fens() + rnd


_RECORDS = {}
STATIC = ["psqt", "positional", "final_v", "final_cp"]


def oracle_records(oracle_lib, nets, fens, p, mode):
    """The oracle's records of `fens` under the parameters p (None: the defaults), computed once per
    (nets, positions, parameters, mode) and shared read-only; the defaults are restored."""
    key = (id(nets[0]), id(nets[1]), hash(tuple(fens)), None if p is None else bytes(p), mode)
    if key not in _RECORDS:
        with oracle_lib.eval_params_set(p):
            rec = oracle_lib.eval_fens(nets[0], nets[1], fens, mode, threads=THREADS)
        rec.setflags(write=False)
        _RECORDS[key] = (nets, rec)  # (the nets are kept alive: their ids stay theirs)
    return _RECORDS[key][1]


# ---- the restatement --------------------------------------------------------------------------
def wrap32(x):
    return (x + 2**31) % 2**32 - 2**31


def tdiv(a, b):
    """C's a / b: the quotient truncated toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def round_half_away(x):
    """std::round of a double."""
    ax = abs(x)
    f = math.floor(ax)
    r = f + 1 if ax - f >= 0.5 else f  # (ax - f is exact)
    return int(r) if x >= 0 else -int(r)


def fen_counts(fen):
    """(counts[colour][P N B R Q], side to move, rule50) of a FEN."""
    parts = fen.split()
    cnt = [[0] * 5, [0] * 5]
    for ch in parts[0]:
        k = "pnbrq".find(ch.lower())
        if ch.isalpha() and k >= 0:
            cnt[0 if ch.isupper() else 1][k] += 1
    rule50 = min(int(parts[4]), 65535) if len(parts) > 4 else 0
    return cnt, (1 if parts[1] == "b" else 0), rule50


def to_cp(p, v, cnt):
    """UCIEngine::to_cp as the comment in gn_eval_params gives it."""
    material = sum(p.wdl_piece_weight[k] * (cnt[0][k] + cnt[1][k]) for k in range(5))
    m = min(max(material, p.wdl_material_min), p.wdl_material_max) / float(p.wdl_material_anchor)
    a = ((p.wdl_a[0] * m + p.wdl_a[1]) * m + p.wdl_a[2]) * m + p.wdl_a[3]
    return round_half_away(float(100 * v) / a)


def fma_a(p, material):
    """a(material) as a compiler that contracts to_cp's multiply-adds would compute it (what the
    device code and the oracle must NOT do): each a * m + b rounded once."""
    from fractions import Fraction as F
    m = min(max(material, p.wdl_material_min), p.wdl_material_max) / float(p.wdl_material_anchor)
    a = p.wdl_a[0]
    for k in (1, 2, 3):
        a = float(F(a) * F(m) + F(p.wdl_a[k]))
    return a


def restate(p, fen, big_out, small_out, mode, detail=None):
    """-> (psqt, positional, final_v, final_cp, flags & (SMALLNET | REEVAL)) of one position under
    the parameters p in `mode`; big_out / small_out: the nets' (psqt, positional).  `detail`
    (a dict) receives whether a product left int32 and whether the clamp bit."""
    cnt, us, rule50 = fen_counts(fen)
    pawns = [cnt[0][0], cnt[1][0]]
    npm = [sum(p.piece_value[k] * c[k] for k in range(1, 5)) for c in cnt]
    simple = p.piece_value[0] * (pawns[us] - pawns[us ^ 1]) + (npm[us] - npm[us ^ 1])
    small = mode == 2 or (mode == 0 and abs(simple) > p.small_net_threshold)
    wrapped = False

    def mul(a, b):
        nonlocal wrapped
        wrapped |= not -2**31 <= a * b < 2**31
        return wrap32(a * b)

    def blend(o):
        return tdiv(wrap32(mul(p.psqt_weight, o[0]) + mul(p.positional_weight, o[1])), 128)

    flags = 0
    o = small_out if small else big_out
    nnue = blend(o)
    if mode == 0 and small and abs(nnue) < p.reeval_threshold:
        o, small, flags = big_out, False, FLAG_REEVAL
        nnue = blend(o)
    complexity = abs(o[0] - o[1])
    nnue = wrap32(nnue - tdiv(mul(nnue, complexity), p.complexity_div_small if small else p.complexity_div_big))
    material = (p.material_pawn_small if small else p.material_pawn_big) * (pawns[0] + pawns[1]) + npm[0] + npm[1]
    v = tdiv(mul(nnue, p.material_base + material), p.material_base)
    v = wrap32(v - tdiv(mul(v, rule50), p.rule50_div))
    clamped = abs(v) > p.value_clamp
    v = max(-p.value_clamp, min(p.value_clamp, v))
    if small:
        flags |= FLAG_SMALLNET
    if detail is not None:
        detail["wrapped"], detail["clamped"] = wrapped, clamped
    return o[0], o[1], v, to_cp(p, v, cnt), flags


assert C.sizeof(C.c_double) == 8 and tdiv(-7, 2) == -3 and tdiv(7, -2) == -3 and round_half_away(-2.5) == -3
