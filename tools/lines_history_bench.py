#!/usr/bin/env python3
"""gn_evaluate_games_lines_history against gn_evaluate_games_lines on the same games (DESIGN.md
§1.5), mode FULL, K lines, on two workloads:

  random   G random 80-ply games in the lichess wire form (tools/lines_bench.py's workload);
  shuffle  G games of a 120-ply king shuffle with a 16-ply cycle behind a locked pawn pair: the
           worst case for the history lookup, every window is long (the half-move clock never
           resets) and most children match nothing, so their walk runs to the window's end.

Both calls run in one process on one context with preallocated output buffers: one warm-up call
each, then `--reps` calls each, alternating; per call the median wall time with its minimum and
maximum, and the median call's stage statistics (GN_STAT_HOST_*, GN_STAT_RANK_NS,
GN_STAT_KEYS_NS, read after every call).  GPU_NNUE_LIB selects another build of the library.
Prints one JSON line.  Usage: python tools/lines_history_bench.py [--games G] [--lines K] [--reps R]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
SHUFFLE_ROOT = "k7/8/8/7p/7P/8/8/K7 w - - 0 1"
SHUFFLE_CYCLE = ("a1b1 a8b8 b1c1 b8c8 c1d1 c8d8 d1d2 d8d7 d2c2 d7c7 c2b2 c7b7 b2a2 b7a7 a2a1 a7a8").split()


def shuffle_games(n, plies=120):
    moves = " ".join((SHUFFLE_CYCLE * (plies // len(SHUFFLE_CYCLE) + 1))[:plies])
    return [(SHUFFLE_ROOT, moves, ())] * n


def measure(nn, games, K, reps):
    import numpy as np
    from fishnet_amd import gpu_nnue as G
    arr, _keep = G._games_array(games)
    ng = len(games)
    pcap = len(nn.evaluate_games_lines(games, K, G.MODE_FULL)[2])  # the size, from a first call
    offs, status = np.zeros(ng + 1, dtype=np.uint32), np.zeros(ng, dtype=np.int32)
    pos = np.zeros(pcap, dtype=G.EVAL_DTYPE)
    lines = np.zeros((pcap, K), dtype=G.LINE_DTYPE)
    L = G.lib()

    def call(f):
        G._check(f(nn.h, arr, ng, G.MODE_FULL, K, offs.ctypes.data, status.ctypes.data, pos.ctypes.data, pcap,
                   lines.ctypes.data))

    def stats():
        st = {k: round(v, 3) for k, v in nn.host_stages().items()}
        st["rank"] = round(nn.get_option(G.STAT_RANK_NS) / 1e6, 3)
        st["keys"] = round(nn.get_option(G.STAT_KEYS_NS) / 1e6, 3)
        return st

    calls = (("plain", L.gn_evaluate_games_lines), ("history", L.gn_evaluate_games_lines_history))
    runs = {name: [] for name, _ in calls}
    draws = 0
    for name, f in calls:  # warm-up of the preallocated host buffers' pages
        call(f)
        if name == "history":
            draws = int(((lines["flags"] & G.FLAG_DRAW) != 0).sum())
    for _ in range(reps):
        for name, f in calls:
            t = time.perf_counter()
            call(f)
            runs[name].append((time.perf_counter() - t, stats()))
    out = {"games": ng, "n_positions": pcap, "draw_lines": draws}
    for name, rs in runs.items():
        rs.sort(key=lambda r: r[0])
        med = rs[len(rs) // 2]
        out[name] = {"wall_ms_median": round(med[0] * 1e3, 2), "wall_ms_min": round(rs[0][0] * 1e3, 2),
                     "wall_ms_max": round(rs[-1][0] * 1e3, 2), "stages_ms": med[1],
                     "rank_ms_all": sorted(r[1]["rank"] for r in rs)}
    out["history_over_plain"] = round(out["history"]["wall_ms_median"] / out["plain"]["wall_ms_median"], 4)
    out["rank_history_over_plain"] = round(out["history"]["stages_ms"]["rank"] /
                                           max(out["plain"]["stages_ms"]["rank"], 1e-9), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--lines", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    from fishnet_amd import gpu_nnue as G, synthnet
    big, small, label = synthnet.net_paths()
    nn = G.GpuNnue(big, small, devices=[0])
    out = {"nets": label, "n_lines": args.lines, "reps": args.reps}
    out["random"] = measure(nn, [(START, u, ()) for u in G.random_games_uci(0x5EED0000, 0, args.games, 80)],
                            args.lines, args.reps)
    out["shuffle"] = measure(nn, shuffle_games(args.games), args.lines, args.reps)
    print(json.dumps(out), flush=True)
    nn.close()


if __name__ == "__main__":
    main()
