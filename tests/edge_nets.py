"""Edge nets for the tests (test infrastructure only): synthetic nets whose layer stacks
keep fc_0 and fc_1 in the range where every weight is observable.

`synthnet.synth_net_arrays` leaves fc_0's rows with a sum of about +3000 at L1 = 3072
(its `// l1` recentring subtracts 0 or -1), so with inputs of about 30 the outputs 0-14 sit
far above the 8160 clip and fc_1 sees the constant 127.  An edge net keeps the feature
transformer, the PSQT table and every bias of the synthetic net of the same (l1, seed,
stress) and replaces, per layer stack b:

  w0[b]  rows drawn with sigma = SIGMA0 / sqrt(l1) at 1/16 resolution, recentred to an exact
         zero mean, rounded; row 15 (the skip term) divided by 4; clipped to int8; then 127
         and -128 planted in rows 0, 1, 2;
  w1[b]  [0, 5] = 127, [1, 20] = -128;
  w2[b]  [3] = 127, [7] = -128;

and, with loud = k, multiplies the PSQT table by k so that final_v and final_cp leave the
few-hundred range (k = 48 reaches |final_v| of about 25,000).
"""
import os
import struct

import numpy as np

from fishnet_amd import synthnet

SIGMA0 = 140.0  # (120 left fc_1 above its clip only 4 times in the 128-wide net's bucket 0)
LOUD = 48


def edge_net_arrays(l1, seed, stress=False, loud=0, with_ft=True):
    a = synthnet.synth_net_arrays(l1, seed, stress, with_ft=with_ft)
    for b in range(synthnet.LAYER_STACKS):
        w0 = synthnet._normal(seed, 100 + 10 * b + 1, 16 * l1, 16 * SIGMA0 / np.sqrt(l1)).astype(np.float64) / 16
        w0 = w0.reshape(16, l1)
        w0 = np.rint(w0 - w0.mean(axis=1, keepdims=True))
        w0[15] = np.rint(w0[15] / 4)
        w0 = np.clip(w0, -128, 127).astype(np.int8)
        for r in range(3):
            w0[r, (37 * r + 11 * b + 5) % l1] = 127
            w0[r, (53 * r + 7 * b + 64) % l1] = -128
        a["w0"][b] = w0
        w1 = a["w1"][b].copy()
        w1[0, 5], w1[1, 20] = 127, -128
        a["w1"][b] = w1
        w2 = a["w2"][b].copy()
        w2[3], w2[7] = 127, -128
        a["w2"][b] = w2
    if loud:
        a["psqt"] = (a["psqt"].astype(np.int64) * loud).astype(np.int32)
    return a


def _description(l1, seed, stress, loud):
    return f"fishnet_amd edge net L1={l1} seed={seed} stress={int(stress)} loud={loud}"


def edge_net_bytes(l1, seed, stress=False, loud=0, base=None):
    """The .nnue image.  With `base` (the image of the synthetic net of the same l1, seed
    and stress) the feature-transformer section is copied from it and not regenerated: only
    the description, the PSQT block and the layer stacks differ."""
    desc = _description(l1, seed, stress, loud)
    if base is None:
        return synthnet.net_bytes(edge_net_arrays(l1, seed, stress, loud), l1, desc)
    old_tail = synthnet.tail_bytes(synthnet.synth_net_arrays(l1, seed, stress, with_ft=False), l1)
    (dlen,) = struct.unpack_from("<I", base, 8)
    assert base.endswith(old_tail) and struct.unpack_from("<I", base, 0)[0] == synthnet.VERSION
    new_tail = synthnet.tail_bytes(edge_net_arrays(l1, seed, stress, loud, with_ft=False), l1)
    d = desc.encode()
    return base[:8] + struct.pack("<I", len(d)) + d + base[12 + dlen:len(base) - len(old_tail)] + new_tail


def edge_net(l1, seed, stress=False, loud=0, cache_dir=None):
    """Path of an edge net, generated once into the cache directory of cached_synth_net."""
    cache_dir = cache_dir or os.environ.get("GPU_NNUE_CACHE") or os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), ".cache")
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, f"edge_L{l1}_s{seed}{'_stress' if stress else ''}{f'_loud{loud}' if loud else ''}.nnue")
    if not os.path.exists(path):
        base = None
        if l1 >= 1024:
            with open(synthnet.cached_synth_net(l1, seed, stress, cache_dir), "rb") as f:
                base = f.read()
        data = edge_net_bytes(l1, seed, stress, loud, base)
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, path)
    return path


def stack_bytes(l1):
    """Size of one layer stack in the file (hash, b0, w0, b1, w1, b2, w2)."""
    return 4 + 16 * 4 + 16 * l1 + 32 * 4 + 32 * 32 + 4 + 32


def zero_w0_columns(data, l1, start, width=16, rows=15):
    """The image with columns [start, start + width) of fc_0 rows 0..rows-1 zeroed in every layer
    stack (a mutation the fixtures must notice)."""
    out = bytearray(data)
    first = len(data) - synthnet.LAYER_STACKS * stack_bytes(l1)
    for b in range(synthnet.LAYER_STACKS):
        w0 = first + b * stack_bytes(l1) + 4 + 16 * 4
        for r in range(rows):
            out[w0 + r * l1 + start:w0 + r * l1 + start + width] = bytes(width)
    return bytes(out)


def golden_path(name):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)


def _fen_file(name):
    with open(golden_path(name)) as f:
        return [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]


def row_cover_fens():
    return _fen_file("row_cover_fens.txt")


def fixture_fens():
    """F: the row-cover positions, then the hand-picked special positions."""
    return row_cover_fens() + _fen_file("special_fens.txt")
