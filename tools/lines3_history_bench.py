#!/usr/bin/env python3
"""gn_evaluate_games_lines3_history against gn_evaluate_games_lines3 on the same games (DESIGN.md
§1.12), mode FULL, static leaves, K lines.

`--games` seeded random games (gn_random_games_uci) of `--plies` plies from the start position.  The
two calls alternate in one process on one context, one warm-up each and then `--reps` calls each; per
call the stage statistics GN_STAT_RANK2_NS, GN_STAT_RANK3_NS, GN_STAT_KEYS_NS and GN_STAT_HOST_TOTAL_NS
are read, and the median of each over the calls is reported (ms), with the wall time's median, the
number of positions and how many lines of the history call carry GN_FLAG_DRAW or differ from the plain
call's.  Prints one JSON line.
Usage: python tools/lines3_history_bench.py [--games N] [--plies P] [--lines K] [--reps R]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--lines", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    from fishnet_amd import gpu_nnue as G, synthnet
    big, small, label = synthnet.net_paths()
    nn = G.GpuNnue(big, small, devices=[0])
    L = G.lib()
    K = args.lines
    games = [(START, u, ()) for u in G.random_games_uci(0x5EED44E8, 0, args.games, args.plies)]
    arr, _keep = G._games_array(games)
    ng = len(games)
    cap = ng * (args.plies + 1)
    offs, status = np.zeros(ng + 1, dtype=np.uint32), np.zeros(ng, dtype=np.int32)
    pos = np.zeros(cap, dtype=G.EVAL_DTYPE)
    out = {name: (np.zeros((cap, K), dtype=G.LINE3_DTYPE), np.zeros((cap, K), dtype=G.PV_DTYPE)) for name in ("history", "plain")}
    fn = {"history": L.gn_evaluate_games_lines3_history, "plain": L.gn_evaluate_games_lines3}
    stat = {"rank2_ms": G.STAT_RANK2_NS, "rank3_ms": G.STAT_RANK3_NS, "keys_ms": G.STAT_KEYS_NS,
            "host_total_ms": G.HOST_STAGES["total"]}

    def timed(name):
        lines, pvs = out[name]
        t = time.perf_counter()
        G._check(fn[name](nn.h, arr, ng, G.MODE_FULL, K, G.LEAF_STATIC, 0, offs.ctypes.data, status.ctypes.data,
                          pos.ctypes.data, cap, lines.ctypes.data, pvs.ctypes.data))
        t = time.perf_counter() - t
        return dict({k: nn.get_option(v) / 1e6 for k, v in stat.items()}, wall_ms=t * 1e3)

    runs = {"history": [], "plain": []}
    timed("history"), timed("plain")  # warm-up: device buffers grown, host pages touched
    for _ in range(args.reps):
        for name in runs:
            runs[name].append(timed(name))
    n = int(offs[-1])
    h, p = out["history"][0][:n], out["plain"][0][:n]
    res = {"nets": label, "n_lines": K, "reps": args.reps, "n_games": ng, "plies": args.plies, "n_positions": n,
           "failed_games": int((status != 0).sum()),
           "lines_with_draw": int(((h["flags"] & G.FLAG_DRAW) != 0).sum()), "lines_that_differ": int((h != p).sum())}
    for name, rs in runs.items():
        res[name] = {k: round(float(np.median([r[k] for r in rs])), 3) for k in rs[0]}
    print(json.dumps(res), flush=True)
    nn.close()


if __name__ == "__main__":
    main()
