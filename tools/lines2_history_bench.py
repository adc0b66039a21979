#!/usr/bin/env python3
"""The games front of the two-ply lines and its history form, mode FULL, K lines,
on two workloads:

  random   G random 80-ply games in the lichess wire form;
  shuffle  G games of a 120-ply king shuffle with a 16-ply cycle behind a locked pawn pair
           (tools/lines_history_bench.py's): the worst case for the history lookup, every window
           is long and most children and grandchildren match nothing.

Three calls on the same positions: `fens`, gn_evaluate_lines2 over every position as a FEN (what a
caller had to do before the games front; its lines must equal the plain games call's, which is
checked); `plain`, gn_evaluate_games_lines2; `history`, gn_evaluate_games_lines2_history.  All run
in one process on one context with preallocated output buffers: one warm-up call each, then
`--reps` calls each, alternating; per call the median wall time with its minimum and maximum, and
the median call's stage statistics (GN_STAT_HOST_*, GN_STAT_RANK2_NS, GN_STAT_KEYS_NS, read after
every call).  GPU_NNUE_LIB selects another build of the library.
Prints one JSON line.  Usage: python tools/lines2_history_bench.py [--games G] [--lines K] [--reps R]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lines_history_bench import START, shuffle_games  # noqa: E402


def measure(nn, games, K, reps):
    import numpy as np
    from fishnet_amd import gpu_nnue as G
    arr, _keep = G._games_array(games)
    ng = len(games)
    fens = [f for root, moves, _ in games for f in G.boards_to_fens(G.replay_game(root, moves)[0])]
    farr, _fkeep = G._fen_array(fens)
    pcap = len(fens)
    offs, status = np.zeros(ng + 1, dtype=np.uint32), np.zeros(ng, dtype=np.int32)
    pos = np.zeros(pcap, dtype=G.EVAL_DTYPE)
    lines = np.zeros((pcap, K), dtype=G.LINE2_DTYPE)
    L = G.lib()

    def games_call(f):
        return lambda: G._check(f(nn.h, arr, ng, G.MODE_FULL, K, offs.ctypes.data, status.ctypes.data,
                                  pos.ctypes.data, pcap, lines.ctypes.data))

    def fens_call():
        G._check(L.gn_evaluate_lines2(nn.h, farr, pcap, G.MODE_FULL, K, pos.ctypes.data, lines.ctypes.data))

    def stats():
        st = {k: round(v, 3) for k, v in nn.host_stages().items()}
        st["rank2"] = round(nn.get_option(G.STAT_RANK2_NS) / 1e6, 3)
        st["keys"] = round(nn.get_option(G.STAT_KEYS_NS) / 1e6, 3)
        return st

    calls = (("fens", fens_call), ("plain", games_call(L.gn_evaluate_games_lines2)),
             ("history", games_call(L.gn_evaluate_games_lines2_history)))
    runs = {name: [] for name, _ in calls}
    first = {}
    for name, f in calls:  # warm-up: device buffers grown, host pages touched
        f()
        first[name] = (pos.tobytes(), lines.copy())
    assert int(offs[-1]) == pcap and not status.any()
    assert first["fens"][0] == first["plain"][0] == first["history"][0]  # the records
    assert first["fens"][1].tobytes() == first["plain"][1].tobytes()     # the plain lines
    hl = first["history"][1]
    draw = (hl["flags"] & G.FLAG_DRAW) != 0
    for _ in range(reps):
        for name, f in calls:
            t = time.perf_counter()
            f()
            runs[name].append((time.perf_counter() - t, stats()))
    out = {"games": ng, "n_positions": pcap, "draw_lines_plies1": int((draw & (hl["plies"] == 1)).sum()),
           "draw_lines_plies2": int((draw & (hl["plies"] == 2)).sum()),
           "positions_differing": int((hl != first["plain"][1]).any(axis=1).sum())}
    for name, rs in runs.items():
        rs.sort(key=lambda r: r[0])
        med = rs[len(rs) // 2]
        out[name] = {"wall_ms_median": round(med[0] * 1e3, 2), "wall_ms_min": round(rs[0][0] * 1e3, 2),
                     "wall_ms_max": round(rs[-1][0] * 1e3, 2), "stages_ms": med[1],
                     "rank2_ms_all": sorted(r[1]["rank2"] for r in rs)}
    out["plain_over_fens"] = round(out["plain"]["wall_ms_median"] / out["fens"]["wall_ms_median"], 4)
    out["history_over_plain"] = round(out["history"]["wall_ms_median"] / out["plain"]["wall_ms_median"], 4)
    out["rank2_history_over_plain"] = round(out["history"]["stages_ms"]["rank2"] /
                                            max(out["plain"]["stages_ms"]["rank2"], 1e-9), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
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
