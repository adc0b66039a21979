#!/usr/bin/env python3
"""The check-extended lines calls against the plain calls of the same build, mode
FULL, K lines.

Two pairs, each alternating in one process on one context, one warm-up each and then `--reps`
calls each; the median, the fastest and the slowest call's wall time are reported with the median
call's stage statistics (GN_STAT_HOST_*, GN_STAT_RANK_NS / GN_STAT_RANK2_NS, GN_STAT_EXTEND_NS,
GN_STAT_EXTENDED_LEAVES):
  two_ply   gn_evaluate_lines2 / gn_evaluate_lines2_extended over `--positions` seeded random
            positions (gn_random_positions);
  one_ply   gn_evaluate_games_lines / gn_evaluate_games_lines_extended (history 0) over `--games`
            seeded random games of `--plies` plies (gn_random_games_uci).  The extended call runs
            its chunks unpipelined; GN_OPT_CHUNK_PARENTS is `--chunk` (0: the default).
The plain paths are the parent commit's code, so the plain numbers also serve as the parent's; run
with GPU_NNUE_LIB set to another build of the library to measure that build's plain calls
(`--plain-only`).  Prints one JSON line.
Usage: python tools/lines_extended_bench.py [--positions N] [--games G] [--lines K] [--reps R]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=1024)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--plies", type=int, default=80)
    ap.add_argument("--lines", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    from fishnet_amd import gpu_nnue as G, synthnet
    big, small, label = synthnet.net_paths()
    nn = G.GpuNnue(big, small, devices=[0])
    nn.set_option(G.OPT_CHUNK_PARENTS, args.chunk)
    L = G.lib()
    K = args.lines

    fens = G.boards_to_fens(G.random_positions(0x5EED2222, 0, args.positions, 160))
    n = len(fens)
    arr, _keep = G._fen_array(fens)
    out = np.zeros(n, dtype=G.EVAL_DTYPE)
    lines2 = np.zeros((n, K), dtype=G.LINE2_DTYPE)

    def two_ply(name):
        return lambda: G._check(getattr(L, name)(nn.h, arr, n, G.MODE_FULL, K, out.ctypes.data, lines2.ctypes.data))

    start = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
    games = [(start, u, ()) for u in G.random_games_uci(0x5EED3333, 0, args.games, args.plies)]
    garr, _gkeep = G._games_array(games)
    ng = len(games)
    pcap = ng * (args.plies + 1)
    offs, status = np.zeros(ng + 1, dtype=np.uint32), np.zeros(ng, dtype=np.int32)
    pos = np.zeros(pcap, dtype=G.EVAL_DTYPE)
    lines1 = np.zeros((pcap, K), dtype=G.LINE_DTYPE)

    def one_ply(extended):
        tail = (offs.ctypes.data, status.ctypes.data, pos.ctypes.data, pcap, lines1.ctypes.data)
        if extended:
            return lambda: G._check(L.gn_evaluate_games_lines_extended(nn.h, garr, ng, G.MODE_FULL, K, 0, *tail))
        return lambda: G._check(L.gn_evaluate_games_lines(nn.h, garr, ng, G.MODE_FULL, K, *tail))

    def stats():
        st = {k: round(v, 3) for k, v in nn.host_stages().items()}
        st["rank"] = round(nn.get_option(G.STAT_RANK_NS) / 1e6, 3)
        st["rank2"] = round(nn.get_option(G.STAT_RANK2_NS) / 1e6, 3)
        if hasattr(G, "STAT_EXTEND_NS") and not args.plain_only:
            st["extend"] = round(nn.get_option(G.STAT_EXTEND_NS) / 1e6, 3)
            st["extended_leaves"] = nn.get_option(G.STAT_EXTENDED_LEAVES)
        return st

    def measure(pair):
        runs = {name: [] for name, _ in pair}
        for _, f in pair:  # warm-up: device buffers grown, host pages touched
            f()
        for _ in range(args.reps):
            for name, f in pair:
                t = time.perf_counter()
                f()
                runs[name].append((time.perf_counter() - t, stats()))
        res = {}
        for name, rs in runs.items():
            rs.sort(key=lambda r: r[0])
            med = rs[len(rs) // 2]
            res[name] = {"wall_ms_median": round(med[0] * 1e3, 2), "wall_ms_min": round(rs[0][0] * 1e3, 2),
                         "wall_ms_max": round(rs[-1][0] * 1e3, 2), "stages_ms": med[1]}
        if "extended" in res:
            e = res["extended"]
            res["extended_over_plain"] = round(e["wall_ms_median"] / res["plain"]["wall_ms_median"], 4)
            e["extend_share_of_compute"] = round(e["stages_ms"]["extend"] / max(e["stages_ms"]["compute"], 1e-9), 4)
        return res

    ext = not args.plain_only
    res = {"nets": label, "n_lines": K, "reps": args.reps, "chunk_parents": args.chunk,
           "two_ply": {"n_positions": n}, "one_ply": {"n_games": ng, "plies": args.plies}}
    res["two_ply"].update(measure([("plain", two_ply("gn_evaluate_lines2"))] +
                                  ([("extended", two_ply("gn_evaluate_lines2_extended"))] if ext else [])))
    res["one_ply"].update(measure([("plain", one_ply(False))] + ([("extended", one_ply(True))] if ext else [])))
    res["one_ply"]["n_positions"] = int(offs[-1])
    print(json.dumps(res), flush=True)
    nn.close()


if __name__ == "__main__":
    main()
