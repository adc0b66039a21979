#!/usr/bin/env python3
"""gn_evaluate_games_lines against gn_evaluate_games(with_children = 1) on the same games
(DESIGN.md §1.3): G random 80-ply games in the lichess wire form, mode FULL, K lines.

Both calls run in one process on one context with preallocated output buffers: one warm-up call
each, then `--reps` calls each, alternating; the median call's wall time is reported with its
stage statistics (GN_STAT_HOST_*, GN_STAT_RANK_NS, read after every call) and the bytes each call
downloads.  GPU_NNUE_LIB selects another build of the library for an A/B.
Prints one JSON line.  Usage: python tools/lines_bench.py [--games G] [--lines K] [--reps R]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--lines", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    from fishnet_amd import gpu_nnue as G, synthnet
    big, small, label = synthnet.net_paths()
    nn = G.GpuNnue(big, small, devices=[0])
    games = [(START, u, ()) for u in G.random_games_uci(0x5EED0000, 0, args.games, 80)]
    arr, _keep = G._games_array(games)
    ng, K = len(games), args.lines
    # the sizes, from a first call (which also warms the device buffers)
    offs, status, pos, coffs, cmv, cev, caps = nn.evaluate_games_arrays(arr, ng, G.MODE_FULL, children=True)
    pcap, ccap = len(pos), len(cev)
    offs = np.zeros(ng + 1, dtype=np.uint32)
    status = np.zeros(ng, dtype=np.int32)
    pos = np.zeros(pcap, dtype=G.EVAL_DTYPE)
    coffs, cmv = np.zeros(pcap + 1, dtype=np.uint32), np.zeros(ccap, dtype=np.uint16)
    cev = np.zeros(ccap, dtype=G.CHILD_DTYPE)
    lines = np.zeros((pcap, K), dtype=G.LINE_DTYPE)
    L = G.lib()

    def with_children():
        G._check(L.gn_evaluate_games(nn.h, arr, ng, G.MODE_FULL, 1, offs.ctypes.data, status.ctypes.data,
                                     pos.ctypes.data, pcap, coffs.ctypes.data, cmv.ctypes.data, cev.ctypes.data, ccap))

    def with_lines():
        G._check(L.gn_evaluate_games_lines(nn.h, arr, ng, G.MODE_FULL, K, offs.ctypes.data, status.ctypes.data,
                                           pos.ctypes.data, pcap, lines.ctypes.data))

    def stats():
        st = {k: round(v, 3) for k, v in nn.host_stages().items()}
        st["rank"] = round(nn.get_option(G.STAT_RANK_NS) / 1e6, 3)
        return st

    runs = {"children": [], "lines": []}
    for f in (with_children, with_lines):  # warm-up of the preallocated host buffers' pages
        f()
    for _ in range(args.reps):
        for name, f in (("children", with_children), ("lines", with_lines)):
            t = time.perf_counter()
            f()
            runs[name].append((time.perf_counter() - t, stats()))
    out = {"nets": label, "games": ng, "n_positions": pcap, "n_children": ccap, "n_lines": K, "reps": args.reps}
    for name, rs in runs.items():
        rs.sort(key=lambda r: r[0])
        med = rs[len(rs) // 2]
        out[name] = {"wall_ms_median": round(med[0] * 1e3, 2), "wall_ms_min": round(rs[0][0] * 1e3, 2),
                     "wall_ms_max": round(rs[-1][0] * 1e3, 2), "stages_ms": med[1]}
    out["children"]["bytes_downloaded"] = pcap * G.EVAL_SIZE + ccap * (G.CHILD_SIZE + 2)
    out["lines"]["bytes_downloaded"] = pcap * G.EVAL_SIZE + pcap * K * G.LINE_DTYPE.itemsize
    out["lines"]["rank_share_of_compute"] = round(out["lines"]["stages_ms"]["rank"] /
                                                  max(out["lines"]["stages_ms"]["compute"], 1e-9), 4)
    out["lines_over_children"] = round(statistics.median(r[0] for r in runs["lines"]) /
                                       statistics.median(r[0] for r in runs["children"]), 4)
    print(json.dumps(out), flush=True)
    nn.close()


if __name__ == "__main__":
    main()
