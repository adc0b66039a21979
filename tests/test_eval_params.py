"""The oracle's parameterised epilogue (or_set_eval_params) pinned before the GPU is compared with
it (CPU only): the parameter structure's layout and defaults against gn_eval_params, a Python
restatement written from include/gpu_nnue.h's field comments (tests/eval_param_sets.py) against
the oracle under every parameter set in every mode, the properties each set is there for, and
the observability of each of the 28 scalars on the input list.
"""
import ctypes as C

import numpy as np
import pytest

import eval_param_sets as S

MODES = (0, 1, 2)
NAMES = list(S.NAMED) + [S.single_name(k) for k in S.SINGLE]


@pytest.fixture(scope="module")
def G():
    from fishnet_amd import build, gpu_nnue
    build.build()
    return gpu_nnue


@pytest.fixture(scope="module")
def fens(G):
    return S.input_fens()


@pytest.fixture(scope="module")
def sets(oracle_lib):
    return dict(S.all_sets(oracle_lib))


@pytest.fixture(scope="module")
def outs(oracle_lib, oracle_nets, fens):
    """Every position's (psqt, positional) of the big and of the small net."""
    return [[oracle_lib.net_output(net, f) for f in fens] for net in oracle_nets]


@pytest.fixture(scope="module")
def default_records(oracle_lib, oracle_nets, fens):
    oracle_lib.set_eval_params(None)
    return [S.oracle_records(oracle_lib, oracle_nets, fens, None, m) for m in MODES]


@pytest.fixture(scope="module")
def records(oracle_lib, oracle_nets, fens, sets):
    """name -> the oracle's records of the input list in modes 0, 1, 2 under that set."""
    return {n: [S.oracle_records(oracle_lib, oracle_nets, fens, p, m) for m in MODES] for n, p in sets.items()}


def test_layout_and_defaults_match_gn_eval_params(oracle_lib, G):
    a, b = oracle_lib.OrEvalParams, G.EvalParams
    assert C.sizeof(a) == C.sizeof(b) == 128
    assert [f[0] for f in a._fields_] == [f[0] for f in b._fields_]
    for name, _ in a._fields_:
        fa, fb = getattr(a, name), getattr(b, name)
        assert (fa.offset, fa.size) == (fb.offset, fb.size), name
    assert sum(getattr(a, n).size // (8 if n == "wdl_a" else 4) for n, _ in a._fields_) == 28 == len(S.SCALARS)
    oracle_lib.set_eval_params(None)
    assert bytes(oracle_lib.eval_params()) == bytes(G.default_eval_params())


def test_set_get_restore(oracle_lib, oracle_nets, sets):
    O = oracle_lib
    fen = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
    O.set_eval_params(None)
    d, e0 = bytes(O.eval_params()), O.eval_fen(*oracle_nets, fen, 0)
    p = sets["weights"]
    with O.eval_params_set(p):
        assert bytes(O.eval_params()) == bytes(p) != d
        assert O.eval_fen(*oracle_nets, fen, 0) != e0
        bad = S.make(O, S.NAMED["weights"])
        for f in ("material_base", "rule50_div", "complexity_div_small", "complexity_div_big", "wdl_material_anchor"):
            setattr(bad, f, 0)
            with pytest.raises(ValueError):
                O.set_eval_params(bad)
            setattr(bad, f, 5)
            O.set_eval_params(p)  # (S.make went through the defaults)
        assert bytes(O.eval_params()) == bytes(p)  # a refused set changes nothing
    assert bytes(O.eval_params()) == d and O.eval_fen(*oracle_nets, fen, 0) == e0
    with pytest.raises(RuntimeError):
        with O.eval_params_set(p):
            raise RuntimeError
    assert bytes(O.eval_params()) == d


def test_input_list(fens, default_records, oracle_lib):
    """About 600 fixed positions; under the defaults mode FULL selects the small net, re-evaluates
    and selects the big net, and the list reaches the edges the sets rely on."""
    assert 550 <= len(fens) <= 650 and fens == S.input_fens()
    fl = default_records[0]["flags"]
    assert not (fl & oracle_lib.FLAG_BAD_FEN).any()
    small, reeval, big = (fl & 2) != 0, (fl & 8) != 0, (fl & 10) == 0
    assert min(small.sum(), reeval.sum(), big.sum()) >= 50 and not (small & reeval).any()
    cnt = [S.fen_counts(f) for f in fens]
    wdl = [c[0][0] + c[1][0] + 3 * (c[0][1] + c[1][1] + c[0][2] + c[1][2]) + 5 * (c[0][3] + c[1][3])
           + 9 * (c[0][4] + c[1][4]) for c, _, _ in cnt]
    assert min(wdl) < 17 and max(wdl) > 78 and sum(17 < w < 78 for w in wdl) >= 100
    assert {99, 150} <= {r for _, _, r in cnt}
    assert (fl & oracle_lib.FLAG_SEARCHED).sum() >= 30 and (fl & oracle_lib.FLAG_MATE).sum() >= 20


def _check_restatement(p, fens, outs, recs, default_recs, name):
    """Flags, final_v and final_cp (and the outputs) of every position in every mode."""
    any_wrap = any_clamp = False
    for mode in MODES:
        rec, drec = recs[mode], default_recs[mode]
        # what the parameters cannot change: in check, no moves, searched, mate
        assert np.array_equal(rec["flags"] & ~np.uint16(10), drec["flags"] & ~np.uint16(10)), (name, mode)
        for i, fen in enumerate(fens):
            d = {}
            exp = S.restate(p, fen, outs[0][i], outs[1][i], mode, d)
            got = (int(rec["psqt"][i]), int(rec["positional"][i]), int(rec["final_v"][i]), int(rec["final_cp"][i]),
                   int(rec["flags"][i]) & 10)
            assert got == exp, (name, mode, fen)
            any_wrap |= d["wrapped"]
            any_clamp |= d["clamped"]
    return any_wrap, any_clamp


def test_restatement_equals_oracle_at_defaults(oracle_lib, fens, outs, default_records):
    oracle_lib.set_eval_params(None)
    _check_restatement(oracle_lib.eval_params(), fens, outs, default_records, default_records, "defaults")


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_oracle(name, sets, fens, outs, records, default_records):
    wrapped, clamped = _check_restatement(sets[name], fens, outs, records[name], default_records, name)
    rec, p = records[name], sets[name]
    if name == "small-vs-big":  # re-evaluated positions must take the big variants
        assert ((rec[0]["flags"] & 8) != 0).sum() >= 50
    if name == "rule50/clamp":
        assert clamped and (np.abs(rec[0]["final_v"]) == 300).any() and np.abs(rec[0]["final_v"]).max() == 300
        at150 = [i for i, f in enumerate(fens) if S.fen_counts(f)[2] == 150 and default_records[1]["final_v"][i]]
        assert at150  # v - v * 150 / 100: the sign flips
        assert all(int(default_records[1]["final_v"][i]) * int(rec[1]["final_v"][i]) < 0 for i in at150)
    if name == "negative divisor":
        with50 = [i for i, f in enumerate(fens) if S.fen_counts(f)[2] > 0 and default_records[1]["final_v"][i] != 0]
        assert len(with50) >= 100  # v + v * rule50 / 212: |v| grows
        assert all(abs(rec[1]["final_v"][i]) >= abs(default_records[1]["final_v"][i]) for i in with50)
    if name == "ties":
        v, cp = rec[0]["final_v"].astype(np.int64), rec[0]["final_cp"].astype(np.int64)
        odd = v % 2 != 0
        assert (odd & (v > 0)).sum() >= 10 and (odd & (v < 0)).sum() >= 10
        assert np.array_equal(cp[odd], (v[odd] + np.sign(v[odd])) // 2)  # exact ties go away from zero
        assert np.array_equal(cp[~odd], v[~odd] // 2)
    if name == "ties-fma":  # exact ties only without contraction
        v, cp = rec[1]["final_v"].astype(np.int64), rec[1]["final_cp"].astype(np.int64)
        odd = v % 2 != 0
        assert odd.sum() >= 100 and np.array_equal(cp[odd], (v[odd] + np.sign(v[odd])) // 2)
        a = S.fma_a(p, 40)
        assert a > 200.0 and all(S.round_half_away(float(100 * int(x)) / a) != int(c) for x, c in zip(v[odd], cp[odd]))
    if name == "wrap":
        assert wrapped and p.rule50_div > 0 and p.material_base > 0 and p.complexity_div_small > 0
    if name == "all small":
        assert np.array_equal(rec[0], rec[2])
    if name == "never small":
        assert np.array_equal(rec[0], rec[1])
    if name == "always re-evaluated":
        was_small = (default_records[0]["flags"] & 10) != 0  # selected small under the defaults
        assert not (rec[0]["flags"] & 2).any() and np.array_equal((rec[0]["flags"] & 8) != 0, was_small)
        assert np.array_equal(rec[0][S.STATIC], rec[1][S.STATIC])  # (the big net's numbers everywhere)


@pytest.mark.parametrize("key", list(S.SINGLE), ids=S.single_name)
def test_every_scalar_is_observable(key, sets, records, default_records, oracle_lib):
    """One scalar moved off its default changes at least one record of the input list."""
    oracle_lib.set_eval_params(None)
    p, d = sets[S.single_name(key)], oracle_lib.eval_params()
    diff = [i for i, (x, y) in enumerate(zip(bytes(p), bytes(d))) if x != y]
    field = getattr(type(p), key[0])
    lo = field.offset + (key[1] or 0) * (8 if key[0] == "wdl_a" else 4)
    assert diff and lo <= min(diff) and max(diff) < lo + (8 if key[0] == "wdl_a" else 4)  # that scalar alone
    assert any((records[S.single_name(key)][m] != default_records[m]).any() for m in MODES), key
