"""A context gives back the device memory it took: three cycles of load, one call of every buffer
family, close, with the device's free memory read after each close.

A coarse check.  The fine one is the library's types: every device buffer, event and stream of a
context is freed by its owner's destructor (gpu_nnue.hip)."""
import numpy as np
import pytest
import torch  # (before libgpu_nnue, as in bench.py)

from fishnet_amd import gpu_nnue as G

pytestmark = pytest.mark.gpu

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
# Slack of the free-memory comparison, bytes: twice the largest drop of the free memory from the
# first close to the third, measured over three runs of this test's cycles on the library as it was
# when it freed its buffers by hand-written lists (MI355X).  That drop was 0 bytes in every run (each
# close returned 1,858,076,672 bytes), so the comparisons below are exact.
B = 2 * 0


def free_memory():
    return torch.cuda.mem_get_info(0)[0]


def cycle(big_path, small_path):
    """One context's life; (free memory just before its close, just after)."""
    fens = G.boards_to_fens(G.random_positions(0x5EED11FE, 0, 80, 160))
    games = [(START, u, ()) for u in G.random_games_uci(0x5EED11FE, 0, 3, 40)]
    ctx = G.GpuNnue(big_path, small_path)
    bufs = []

    def alloc(nbytes):
        bufs.append(ctx.alloc(nbytes))
        return bufs[-1]

    try:
        n = len(fens)
        assert len(ctx.evaluate_batch(fens)) == n  # one game's worth: the captured graph
        assert ctx.get_option(G.STAT_FAST_BATCHES) == 1
        d_b, d_o = alloc(n * G.BOARD_SIZE), alloc(n * G.EVAL_SIZE)
        d_b.upload(G.pack_fens(fens)[0])
        ctx.evaluate_device(d_b, n, G.MODE_FULL, d_o)
        assert ctx.get_option(G.OPT_EXPAND_PIPELINE) == 2
        _, total, _, _ = ctx.time_expand_device(d_b, n, G.MODE_FULL, 2)
        d_off, d_ch = alloc((n + 1) * 4), alloc(total * G.BOARD_SIZE)
        d_mv, d_co = alloc(total * 2), alloc(total * G.EVAL_SIZE)
        assert ctx.expand_device(d_b, n, G.MODE_FULL, d_o, d_off, d_ch, d_mv, d_co, total) == total
        assert all(g["status"] == 0 for g in ctx.evaluate_games(games, children=True))
        ctx.evaluate_games_lines_history(games, 3)
        ctx.evaluate_lines2(fens[:8], 2)
        assert ctx.perft(START, 2) == 400
        for b in bufs:
            b.free()
        before = free_memory()
    finally:
        for b in bufs:
            b.free()
        ctx.close()
    return before, free_memory()


def test_three_context_lives_return_their_memory(synth_big_path, synth_small_path):
    from fishnet_amd import build
    build.build()
    lives = [cycle(synth_big_path, synth_small_path) for _ in range(3)]
    print("free memory (before close, after close) per cycle:", lives, "first -> third drop:",
          lives[0][1] - lives[2][1])
    assert lives[2][1] >= lives[0][1] - B
    for before, after in lives:  # (a leak of a quarter of a context cannot hide under B)
        assert after - before > 4 * B
