"""The stage times of gn_time_expand_device and gn_time_evaluate_device, which bench.py reports and
every optimisation is judged by: the eight (four) stages are disjoint parts of an iteration, the
three GN_STAT_*_NS intervals tile the big-net stage serial and pipelined, and the timed call
computes what gn_expand_device computes.

Shape: two 80-ply games (162 parents, a few thousand children): two games' blocks, a chained walk
and, over three pipelined iterations, both buffer sets in use."""
import types

import numpy as np
import pytest

from fishnet_amd import gpu_nnue as G

pytestmark = pytest.mark.gpu

GAMES, PLIES, ITERS = 2, 80, 3
N = GAMES * (PLIES + 1)
# Slack of the two identities below, ms.  Consecutive event intervals need not telescope exactly (a
# marker has a duration of its own; the stages are float32 sums, the statistics whole nanoseconds).
# Measured on the library as it was before the stage events got names (three runs of every case
# below, MI355X): the stages never summed to more than an iteration (they fell short of it by at
# least 0.0074 ms in the serial expansions and 0.17 ms in the evaluations: deviation 0), and the
# three statistics missed the big-net stage by at most 0.000002678 ms (2.7 ns: each is cut to whole
# nanoseconds).  DELTA_MS is twice that largest deviation.
DELTA_MS = 2 * 0.000002678
# (mode, GN_OPT_EXPAND_PIPELINE, GN_OPT_STREAM_SLICES)
CASES = [(mode, pipe, 3) for mode in (G.MODE_FULL, G.MODE_BIG, G.MODE_SMALL) for pipe in (0, 2)]
CASES += [(G.MODE_BIG, pipe, 1) for pipe in (0, 2)]


def make_shape(gpu_ctx):
    """The parents on the device, and two sets of output buffers (the timed call's, gn_expand_device's)."""
    d_b = gpu_ctx.alloc(N * G.BOARD_SIZE)
    gpu_ctx.random_games_device(0x5EED57A6, 0, GAMES, PLIES, d_b)
    gpu_ctx.synchronize()
    _, total, _, _ = gpu_ctx.time_expand_device(d_b, N, G.MODE_BIG, 1)
    assert 2000 < total < 10000
    bufs = lambda: {"po": gpu_ctx.alloc(N * G.EVAL_SIZE), "off": gpu_ctx.alloc((N + 1) * 4),
                    "mv": gpu_ctx.alloc(total * 2), "co": gpu_ctx.alloc(total * G.EVAL_SIZE), "cap": total}
    return types.SimpleNamespace(d_b=d_b, total=total, timed=bufs(), plain=bufs(),
                                 ch=gpu_ctx.alloc(total * G.BOARD_SIZE), ev=gpu_ctx.alloc(N * G.EVAL_SIZE))


@pytest.fixture(scope="module")
def shape(gpu_ctx):
    return make_shape(gpu_ctx)


def checksums(ctx, s, out):
    return tuple(ctx.checksum_device(out[b], nb) for b, nb in
                 (("po", N * G.EVAL_SIZE), ("off", (N + 1) * 4), ("mv", s.total * 2), ("co", s.total * G.EVAL_SIZE)))


def timed_expand(ctx, s, mode, pipe, slices):
    """(ms_total, the stages by name, [plan, stream, finish] in ms) of ITERS timed expansions."""
    ctx.set_option(G.OPT_EXPAND_PIPELINE, pipe)
    ctx.set_option(G.OPT_STREAM_SLICES, slices)
    try:
        ms, total, st, _ = ctx.time_expand_device(s.d_b, N, mode, ITERS, outputs=s.timed)
        stats = [ctx.get_option(o) / 1e6 for o in (G.STAT_PLAN_NS, G.STAT_STREAM_NS, G.STAT_FINISH_NS)]
    finally:
        ctx.set_option(G.OPT_EXPAND_PIPELINE, 2)
        ctx.set_option(G.OPT_STREAM_SLICES, 3)
    assert total == s.total
    return ms, dict(zip(G.EXPAND_STAGES, st)), stats


def sum_excess(ms, stages):
    """By how much the stages of one iteration exceed an iteration, ms (negative: they fit)."""
    return float(sum(stages)) - ms / ITERS


def tiling_gap(stage, stats):
    """By how much plan + stream + finish miss the big-net stage, ms."""
    return abs(float(sum(stats)) - stage["big_net"])


@pytest.mark.parametrize("mode,pipe,slices", CASES)
def test_expand_stage_times(gpu_ctx, shape, mode, pipe, slices):
    ms, stage, stats = timed_expand(gpu_ctx, shape, mode, pipe, slices)
    print(f"mode {mode} pipe {pipe} slices {slices}: ms {ms:.6f} stages {stage} stats {stats} "
          f"excess {sum_excess(ms, stage.values()):.7f} gap {tiling_gap(stage, stats):.7f}")
    assert len(stage) == 8 and all(np.isfinite(v) and v >= 0 for v in stage.values()), stage
    if pipe == 0 or mode == G.MODE_SMALL:  # serial (the small net alone is never pipelined)
        assert sum_excess(ms, stage.values()) <= DELTA_MS
    if mode != G.MODE_SMALL:
        assert tiling_gap(stage, stats) <= DELTA_MS
        assert stats[0] > 0 and stats[1] > 0
    if mode != G.MODE_BIG:
        assert stage["small_net"] > 0


@pytest.mark.parametrize("mode", [G.MODE_FULL, G.MODE_BIG, G.MODE_SMALL])
def test_timed_expansion_equals_expand_device(gpu_ctx, shape, mode):
    s = shape
    for out in (s.timed, s.plain):
        for b in ("po", "off", "mv", "co"):
            out[b].upload(np.zeros(out[b].nbytes, np.uint8))
    gpu_ctx.time_expand_device(s.d_b, N, mode, ITERS, outputs=s.timed)
    p = s.plain
    assert gpu_ctx.expand_device(s.d_b, N, mode, p["po"], p["off"], s.ch, p["mv"], p["co"], s.total) == s.total
    assert checksums(gpu_ctx, s, s.timed) == checksums(gpu_ctx, s, s.plain)


def timed_evaluate(ctx, s, mode):
    """(ms_total, the four stages by bench.py's names, FT rows) of ITERS timed evaluations."""
    ms, per, rows = ctx.time_evaluate_device(s.d_b, N, mode, s.ev, ITERS, rows=True)
    return ms, dict(zip(("classify_sort", "small_net", "big_net", "finalize"), per)), rows


@pytest.mark.parametrize("mode", [G.MODE_FULL, G.MODE_BIG, G.MODE_SMALL])
def test_evaluate_stage_times(gpu_ctx, shape, mode):
    ms, stage, rows = timed_evaluate(gpu_ctx, shape, mode)
    print(f"mode {mode}: ms {ms:.6f} stages {stage} rows {rows} excess {sum_excess(ms, stage.values()):.7f}")
    assert len(stage) == 4 and all(np.isfinite(v) and v >= 0 for v in stage.values()), stage
    assert sum_excess(ms, stage.values()) <= DELTA_MS
    if mode != G.MODE_SMALL:
        assert stage["big_net"] > 0
    if mode != G.MODE_BIG:
        assert stage["small_net"] > 0
    assert rows > 0


def test_time_evaluate_bad_mode_then_valid(gpu_ctx, shape):
    with pytest.raises(G.GnError) as e:
        gpu_ctx.time_evaluate_device(shape.d_b, N, 7, shape.ev, ITERS)
    assert e.value.code == G.E_INVALID
    ms, per = gpu_ctx.time_evaluate_device(shape.d_b, N, G.MODE_FULL, shape.ev, ITERS)
    assert ms > 0 and len(per) == 4
