#!/usr/bin/env python3
"""gn_evaluate_lines2 against what a caller had to do before it: N seeded random
positions (gn_random_positions), mode FULL, K two-ply lines.

`lines2`: one gn_evaluate_lines2 call over the N FENs (depth-2 expansion in chunks, ranked on the
GPU, 24 + 16 K bytes per position downloaded).  `download`: the same positions through
gn_expand2_device into caller-owned device buffers (one call over all N parents by default;
`--block B`: B parents per call) and a full download of the
parent records, child offsets / moves / records and grandchild offsets / moves / records: the
input of a minimax on the CPU, which is not run here.  Both run in one process on one context:
one warm-up each, then `--reps` calls each, alternating; the median call's wall time is reported,
for lines2 with its stage statistics (GN_STAT_HOST_*, GN_STAT_RANK2_NS).  GPU_NNUE_LIB selects
another build of the library.  GN_OPT_CHUNK_PARENTS is `--chunk` (0: the default).
Prints one JSON line.  Usage: python tools/lines2_bench.py [--positions N] [--lines K] [--reps R]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--lines", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--block", type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    from fishnet_amd import gpu_nnue as G, synthnet
    big, small, label = synthnet.net_paths()
    nn = G.GpuNnue(big, small, devices=[0])
    nn.set_option(G.OPT_CHUNK_PARENTS, args.chunk)
    boards = G.random_positions(0x5EED2222, 0, args.positions, 160)
    fens = G.boards_to_fens(boards)
    n, K = len(fens), args.lines
    arr, _keep = G._fen_array(fens)
    out = np.zeros(n, dtype=G.EVAL_DTYPE)
    lines = np.zeros((n, K), dtype=G.LINE2_DTYPE)
    L = G.lib()

    def lines2():
        G._check(L.gn_evaluate_lines2(nn.h, arr, n, G.MODE_FULL, K, out.ctypes.data, lines.ctypes.data))
        return 0

    # the download path: the parents of each block on the device, and output buffers sized once for
    # the largest block by the call's own GN_E_CAPACITY replies
    block = args.block or n
    parts = []
    for a in range(0, n, block):
        m = min(block, n - a)
        d = nn.alloc(m * 32)
        d.upload(boards[a:a + m])
        parts.append([d, m, 0, 0])

    def need(d, m, bufs):
        try:
            return nn.expand2_device(d, m, G.MODE_FULL, bufs)
        except G.GnError as e:
            if e.code != G.E_CAPACITY:
                raise
            return e.need

    bufs = {"po": nn.alloc(block * G.EVAL_SIZE), "off": nn.alloc((block + 1) * 4), "cap": 0, "gcap": 0}
    for p in parts:
        p[2] = need(p[0], p[1], bufs)[0]
    cap = max(max(p[2] for p in parts), 1)
    bufs.update(cap=cap, ch=nn.alloc(cap * 32), mv=nn.alloc(cap * 2), co=nn.alloc(cap * G.EVAL_SIZE),
                goff=nn.alloc((cap + 1) * 4))
    for p in parts:
        p[3] = need(p[0], p[1], bufs)[1]
    gcap = max(max(p[3] for p in parts), 1)
    bufs.update(gcap=gcap, gmv=nn.alloc(gcap * 2), gco=nn.alloc(gcap * G.EVAL_SIZE))

    def download():
        total = 0
        for d, m, _, _ in parts:
            t, g = nn.expand2_device(d, m, G.MODE_FULL, bufs)
            got = [bufs["po"].download(G.EVAL_DTYPE, m), bufs["off"].download(np.uint32, m + 1),
                   bufs["mv"].download(np.uint16, t), bufs["co"].download(G.EVAL_DTYPE, t),
                   bufs["goff"].download(np.uint32, t + 1), bufs["gmv"].download(np.uint16, g),
                   bufs["gco"].download(G.EVAL_DTYPE, g)]
            total += sum(x.nbytes for x in got)
        return total

    def stats():
        st = {k: round(v, 3) for k, v in nn.host_stages().items()}
        st["rank2"] = round(nn.get_option(G.STAT_RANK2_NS) / 1e6, 3)
        return st

    runs = {"lines2": [], "download": []}
    for f in (lines2, download):  # warm-up: device buffers grown, host pages touched
        f()
    for _ in range(args.reps):
        for name, f in (("lines2", lines2), ("download", download)):
            t = time.perf_counter()
            nbytes = f()
            runs[name].append((time.perf_counter() - t, stats() if name == "lines2" else None, nbytes))
    res = {"nets": label, "n_positions": n, "n_children": sum(p[2] for p in parts),
           "n_grandchildren": sum(p[3] for p in parts), "n_lines": K, "reps": args.reps,
           "chunk_parents": args.chunk or 1024, "download_block": block}
    for name, rs in runs.items():
        rs.sort(key=lambda r: r[0])
        med = rs[len(rs) // 2]
        res[name] = {"wall_ms_median": round(med[0] * 1e3, 2), "wall_ms_min": round(rs[0][0] * 1e3, 2),
                     "wall_ms_max": round(rs[-1][0] * 1e3, 2)}
        if med[1]:
            res[name]["stages_ms"] = med[1]
    res["lines2"]["bytes_downloaded"] = n * G.EVAL_SIZE + n * K * G.LINE2_DTYPE.itemsize
    res["download"]["bytes_downloaded"] = runs["download"][0][2]
    res["lines2"]["rank2_share_of_compute"] = round(res["lines2"]["stages_ms"]["rank2"] /
                                                    max(res["lines2"]["stages_ms"]["compute"], 1e-9), 4)
    res["lines2"]["grandchildren_per_s"] = round(res["n_grandchildren"] / (res["lines2"]["wall_ms_median"] / 1e3))
    res["lines2_over_download"] = round(statistics.median(r[0] for r in runs["lines2"]) /
                                        statistics.median(r[0] for r in runs["download"]), 4)
    print(json.dumps(res), flush=True)
    nn.close()


if __name__ == "__main__":
    main()
