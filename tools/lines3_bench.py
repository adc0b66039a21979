#!/usr/bin/env python3
"""The three-ply lines calls against the two-ply calls over the same positions' children
(DESIGN.md §1.11), mode FULL, K lines.

`--positions` seeded random positions (gn_random_positions).  Per leaf rule two calls alternate in one
process on one context, one warm-up each and then `--reps` calls each:
  lines3_<rule>    gn_evaluate_lines3 over the positions, K lines, with PVs;
  children_<rule>  the two-ply call of the same rule (gn_evaluate_lines2, _extended, _quiescent_pv) at
                   K = 1 over exactly those positions' children as FENs (gn_expand_device +
                   gn_boards_to_fens, made once outside the timed region): the same leaf work, so the
                   difference is the price of the root level and of keeping the children's lines on
                   the device.
The rules are static, checks, q1 and q1see (q1 under GN_OPT_QUIESCE_SEE = 1, the option set around
those calls alone, outside the timed region).  The median, the fastest and the slowest call's wall
time are reported with the median call's stage statistics (GN_STAT_HOST_*, GN_STAT_RANK3_NS,
GN_STAT_RANK2_NS, GN_STAT_EXTEND_NS, GN_STAT_QUIESCE_NS / _LEAVES / _NODES, GN_STAT_PV_NS) and the ratio
of the two medians.  Prints one JSON line.
Usage: python tools/lines3_bench.py [--positions N] [--lines K] [--reps R] [--rules static,checks,q1,q1see]
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
    ap.add_argument("--positions", type=int, default=256)
    ap.add_argument("--lines", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--rules", default="static,checks,q1,q1see")
    args = ap.parse_args()
    import numpy as np
    from fishnet_amd import gpu_nnue as G, synthnet
    big, small, label = synthnet.net_paths()
    nn = G.GpuNnue(big, small, devices=[0])
    nn.set_option(G.OPT_CHUNK_PARENTS, args.chunk)
    L = G.lib()
    K = args.lines

    boards = G.random_positions(0x5EED2222, 0, args.positions, 160)
    fens = G.boards_to_fens(boards)
    n = len(fens)
    cap = 256 * n
    b = {k: nn.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4), ("ch", cap * 32),
                                      ("mv", cap * 2), ("co", cap * G.EVAL_SIZE))}
    b["b"].upload(boards)
    total = nn.expand_device(b["b"], n, G.MODE_FULL, b["po"], b["off"], b["ch"], b["mv"], b["co"], cap)
    kids = G.boards_to_fens(b["ch"].download(G.BOARD_DTYPE, total))
    for x in b.values():
        x.free()

    arr, _keep = G._fen_array(fens)
    out = np.zeros(n, dtype=G.EVAL_DTYPE)
    lines3 = np.zeros((n, K), dtype=G.LINE3_DTYPE)
    pvs3 = np.zeros((n, K), dtype=G.PV_DTYPE)
    karr, _kkeep = G._fen_array(kids)
    kout = np.zeros(total, dtype=G.EVAL_DTYPE)
    klines = np.zeros((total, 1), dtype=G.LINE2_DTYPE)
    kpvs = np.zeros((total, 1), dtype=G.PV_DTYPE)
    kends = (kout.ctypes.data, klines.ctypes.data)
    leaf_of = {"static": (G.LEAF_STATIC, 0), "checks": (G.LEAF_CHECKS, 0), "q1": (G.LEAF_QUIESCE, 1), "q2": (G.LEAF_QUIESCE, 2)}

    def calls(rule):
        base = rule[:-3] if rule.endswith("see") else rule
        leaf, depth = leaf_of[base]
        three = lambda: G._check(L.gn_evaluate_lines3(nn.h, arr, n, G.MODE_FULL, K, leaf, depth, out.ctypes.data,
                                                      lines3.ctypes.data, pvs3.ctypes.data))
        if base == "static":
            two = lambda: G._check(L.gn_evaluate_lines2(nn.h, karr, total, G.MODE_FULL, 1, *kends))
        elif base == "checks":
            two = lambda: G._check(L.gn_evaluate_lines2_extended(nn.h, karr, total, G.MODE_FULL, 1, *kends))
        else:
            two = lambda: G._check(L.gn_evaluate_lines2_quiescent_pv(nn.h, karr, total, G.MODE_FULL, 1, depth, *kends,
                                                                     kpvs.ctypes.data))
        return three, two, (G.OPT_QUIESCE_SEE if rule.endswith("see") else None)

    def stats():
        st = {k: round(v, 3) for k, v in nn.host_stages().items()}
        for name, opt in (("rank3", G.STAT_RANK3_NS), ("rank2", G.STAT_RANK2_NS), ("extend", G.STAT_EXTEND_NS),
                          ("quiesce", G.STAT_QUIESCE_NS), ("pv", G.STAT_PV_NS)):
            st[name] = round(nn.get_option(opt) / 1e6, 3)
        st["quiesce_leaves"] = nn.get_option(G.STAT_QUIESCE_LEAVES)
        st["quiesce_nodes"] = nn.get_option(G.STAT_QUIESCE_NODES)
        return st

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

    def summary(rs):
        rs.sort(key=lambda r: r[0])
        med = rs[len(rs) // 2]
        return {"wall_ms_median": round(med[0] * 1e3, 2), "wall_ms_min": round(rs[0][0] * 1e3, 2),
                "wall_ms_max": round(rs[-1][0] * 1e3, 2), "stages_ms": med[1]}

    res = {"nets": label, "n_lines": K, "reps": args.reps, "chunk_parents": args.chunk, "n_positions": n,
           "n_children": total, "rules": {}}
    for rule in [r for r in args.rules.split(",") if r]:
        three, two, opt = calls(rule)
        runs = {"lines3": [], "children": []}
        timed(three, opt), timed(two, opt)  # warm-up: device buffers grown, host pages touched
        for _ in range(args.reps):
            runs["lines3"].append(timed(three, opt))
            runs["children"].append(timed(two, opt))
        r = {k: summary(v) for k, v in runs.items()}
        r["ratio"] = round(r["lines3"]["wall_ms_median"] / r["children"]["wall_ms_median"], 4)
        res["rules"][rule] = r
    print(json.dumps(res), flush=True)
    nn.close()


if __name__ == "__main__":
    main()
