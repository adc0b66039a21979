#!/usr/bin/env python3
"""The quiescent lines calls against the plain and the check-extended calls of the same build
(DESIGN.md §1.8), mode FULL, K lines.

Two workloads, the variants of each alternating in one process on one context, one warm-up each and
then `--reps` calls each; the median, the fastest and the slowest call's wall time are reported with
the median call's stage statistics (GN_STAT_HOST_*, GN_STAT_RANK_NS / GN_STAT_RANK2_NS,
GN_STAT_EXTEND_NS, GN_STAT_QUIESCE_NS, GN_STAT_QUIESCE_LEAVES, GN_STAT_QUIESCE_NODES):
  two_ply   gn_evaluate_lines2 / _extended / _quiescent over `--positions` seeded random positions
            (gn_random_positions);
  one_ply   gn_evaluate_games_lines / _extended / _quiescent (history 0) over `--games` seeded random
            games of `--plies` plies (gn_random_games_uci).  The extended and quiescent calls run their
            chunks unpipelined; GN_OPT_CHUNK_PARENTS is `--chunk` (0: the default).
The variants are plain, extended and q<d> for every depth of `--depths`; a depth written <d>pv adds
q<d>pv, the quiescent call that also returns each line's whole variation (gn_evaluate_lines2_quiescent_pv,
gn_evaluate_games_lines_quiescent_pv; GN_STAT_PV_NS is then reported as "pv"); a depth written <d>see
adds q<d>see, the same call under GN_OPT_QUIESCE_SEE = 1 (the losing captures pruned; the option is set
around that call alone, outside the timed region).  The plain and extended
paths are the parent commit's code; run with GPU_NNUE_LIB set to another build of the library and
`--depths ""` to measure that build's calls.  Prints one JSON line.
Usage: python tools/quiesce_bench.py [--positions N] [--games G] [--lines K] [--reps R] [--depths 1,1see,1pv,2,2see,2pv,3,3see]
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
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--plies", type=int, default=80)
    ap.add_argument("--lines", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--depths", default="1,2,3")
    ap.add_argument("--skip", default="", help="two_ply or one_ply: leave that workload out")
    args = ap.parse_args()
    import numpy as np
    from fishnet_amd import gpu_nnue as G, synthnet
    big, small, label = synthnet.net_paths()
    nn = G.GpuNnue(big, small, devices=[0])
    nn.set_option(G.OPT_CHUNK_PARENTS, args.chunk)
    L = G.lib()
    K = args.lines
    depths = [d for d in args.depths.split(",") if d]  # "2": q2, "2pv": q2pv
    with_pv = any(d.endswith("pv") for d in depths)

    fens = G.boards_to_fens(G.random_positions(0x5EED2222, 0, args.positions, 160))
    n = len(fens)
    arr, _keep = G._fen_array(fens)
    out = np.zeros(n, dtype=G.EVAL_DTYPE)
    lines2 = np.zeros((n, K), dtype=G.LINE2_DTYPE)
    ends = (out.ctypes.data, lines2.ctypes.data)
    pvs2 = np.zeros((n, K), dtype=G.PV_DTYPE)

    def two_ply(variant):
        if variant == "plain":
            return lambda: G._check(L.gn_evaluate_lines2(nn.h, arr, n, G.MODE_FULL, K, *ends))
        if variant == "extended":
            return lambda: G._check(L.gn_evaluate_lines2_extended(nn.h, arr, n, G.MODE_FULL, K, *ends))
        if variant.endswith("pv"):
            return lambda: G._check(L.gn_evaluate_lines2_quiescent_pv(nn.h, arr, n, G.MODE_FULL, K, int(variant[1:-2]), *ends,
                                                                      pvs2.ctypes.data))
        return lambda: G._check(L.gn_evaluate_lines2_quiescent(nn.h, arr, n, G.MODE_FULL, K, int(variant[1:]), *ends))

    start = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
    games = [(start, u, ()) for u in G.random_games_uci(0x5EED3333, 0, args.games, args.plies)]
    garr, _gkeep = G._games_array(games)
    ng = len(games)
    pcap = ng * (args.plies + 1)
    offs, status = np.zeros(ng + 1, dtype=np.uint32), np.zeros(ng, dtype=np.int32)
    pos = np.zeros(pcap, dtype=G.EVAL_DTYPE)
    lines1 = np.zeros((pcap, K), dtype=G.LINE_DTYPE)
    tail = (offs.ctypes.data, status.ctypes.data, pos.ctypes.data, pcap, lines1.ctypes.data)
    pvs1 = np.zeros((pcap, K), dtype=G.PV_DTYPE)

    def one_ply(variant):
        if variant == "plain":
            return lambda: G._check(L.gn_evaluate_games_lines(nn.h, garr, ng, G.MODE_FULL, K, *tail))
        if variant == "extended":
            return lambda: G._check(L.gn_evaluate_games_lines_extended(nn.h, garr, ng, G.MODE_FULL, K, 0, *tail))
        if variant.endswith("pv"):
            return lambda: G._check(L.gn_evaluate_games_lines_quiescent_pv(nn.h, garr, ng, G.MODE_FULL, K, 0,
                                                                           int(variant[1:-2]), *tail, pvs1.ctypes.data))
        return lambda: G._check(L.gn_evaluate_games_lines_quiescent(nn.h, garr, ng, G.MODE_FULL, K, 0, int(variant[1:]),
                                                                    *tail))

    def pruned(make):
        """make(variant), with a trailing "see" taken off the variant and the option set around the call."""
        def made(variant):
            if not variant.endswith("see"):
                return make(variant), None
            return make(variant[:-3]), G.OPT_QUIESCE_SEE
        return made

    def stats():
        st = {k: round(v, 3) for k, v in nn.host_stages().items()}
        st["rank"] = round(nn.get_option(G.STAT_RANK_NS) / 1e6, 3)
        st["rank2"] = round(nn.get_option(G.STAT_RANK2_NS) / 1e6, 3)
        st["extend"] = round(nn.get_option(G.STAT_EXTEND_NS) / 1e6, 3)
        if hasattr(G, "STAT_QUIESCE_NS"):
            st["quiesce"] = round(nn.get_option(G.STAT_QUIESCE_NS) / 1e6, 3)
            st["quiesce_leaves"] = nn.get_option(G.STAT_QUIESCE_LEAVES)
            st["quiesce_nodes"] = nn.get_option(G.STAT_QUIESCE_NODES)
        if with_pv:
            st["pv"] = round(nn.get_option(G.STAT_PV_NS) / 1e6, 3)
        return st

    def measure(make):
        variants = ["plain", "extended"] + [f"q{d}" for d in depths]
        calls = [(v, *pruned(make)(v)) for v in variants]
        runs = {v: [] for v in variants}

        def timed(f, opt):
            if opt is not None:
                nn.set_option(opt, 1)
            t = time.perf_counter()
            f()
            t = time.perf_counter() - t
            st = stats()
            if opt is not None:
                nn.set_option(opt, 0)
            return t, st

        for _, f, opt in calls:  # warm-up: device buffers grown, host pages touched
            timed(f, opt)
        for _ in range(args.reps):
            for v, f, opt in calls:
                runs[v].append(timed(f, opt))
        res = {}
        for v, rs in runs.items():
            rs.sort(key=lambda r: r[0])
            med = rs[len(rs) // 2]
            res[v] = {"wall_ms_median": round(med[0] * 1e3, 2), "wall_ms_min": round(rs[0][0] * 1e3, 2),
                      "wall_ms_max": round(rs[-1][0] * 1e3, 2), "stages_ms": med[1]}
        return res

    res = {"nets": label, "n_lines": K, "reps": args.reps, "chunk_parents": args.chunk, "depths": depths}
    if args.skip != "two_ply":
        res["two_ply"] = {"n_positions": n, **measure(two_ply)}
    if args.skip != "one_ply":
        res["one_ply"] = {"n_games": ng, "plies": args.plies, **measure(one_ply)}
        res["one_ply"]["n_positions"] = int(offs[-1])
    print(json.dumps(res), flush=True)
    nn.close()


if __name__ == "__main__":
    main()
