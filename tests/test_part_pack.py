"""The column slices' packed fc_0 partial sums (fishnet_amd/csrc/kernels.h, GN_PART_DWORDS): a numpy
model of the offset rule and of the 48-byte record, written from the rule's statement and not from
the kernels, driven to both ends of a slice's range; the library's own tables against the model.

The rule.  Slice s of a 3072-wide net covers, for each perspective h, the fc_0 inputs
1536 h + 512 s .. + 511 (1,024 inputs, each an activation in [0, 127]).  For bucket b and output o,
    part_off[b][s][o] = 127 * sum(max(-w, 0)) over the slice's weights of row (b, o),
    b0p[b][o]         = b0[b][o] - sum over s of part_off[b][s][o],
and a slice stores sum + part_off, which lies in [0, 127 * sum|w|] and so below 2^24 (127 * 128 * 1024
= 16,646,144).  Four such values a, b, c, d go into three dwords: a | b << 24, b >> 8 | c << 16,
c >> 16 | d << 8; a position's record is four of those groups (outputs 4 j .. 4 j + 3 in dwords 3 j ..
3 j + 2).  finalize adds the three slices' values and b0p.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1, HALF, COLS, SLICES = 3072, 1536, 512, 3
M32 = (1 << 32) - 1


def slice_columns(s):
    """The 1,024 fc_0 inputs slice s covers (both perspectives)."""
    return np.concatenate([np.arange(h * HALF + s * COLS, h * HALF + (s + 1) * COLS) for h in range(2)])


def model_tables(w0, b0):
    """(part_off [B][3][16], b0p [B][16]) as int64 / int32 from w0 [B][16][3072] int8, b0 [B][16] int32."""
    w = np.asarray(w0).astype(np.int64)
    off = np.stack([127 * np.maximum(-w[:, :, slice_columns(s)], 0).sum(axis=2) for s in range(SLICES)], axis=1)
    b0p = (np.asarray(b0).astype(np.int64) - off.sum(axis=1)) & M32
    return off, b0p.astype(np.uint32).view(np.int32).reshape(np.asarray(b0).shape)


def pack(vals):
    """[..., 16] values in [0, 2^24) -> [..., 12] dwords."""
    v = np.asarray(vals).astype(np.uint64).reshape(vals.shape[:-1] + (4, 4))
    a, b, c, d = (v[..., k] for k in range(4))
    out = np.stack([(a | b << 24) & M32, (b >> 8 | c << 16) & M32, (c >> 16 | d << 8) & M32], axis=-1)
    return out.reshape(vals.shape[:-1] + (12,)).astype(np.uint32)


def unpack(rec):
    r = np.asarray(rec).astype(np.uint64).reshape(rec.shape[:-1] + (4, 3))
    x, y, z = (r[..., k] for k in range(3))
    out = np.stack([x & 0xFFFFFF, x >> 24 | (y & 0xFFFF) << 8, y >> 16 | (z & 0xFF) << 16, z >> 8], axis=-1)
    return out.reshape(rec.shape[:-1] + (16,)).astype(np.int64)


def _rows():
    """fc_0 rows [16][3072] per kind: every output's row of the kind (random: 16 seeded rows)."""
    alt = np.where(np.arange(L1) % 2 == 0, -128, 127).astype(np.int8)
    rng = np.random.default_rng(0x24B175)
    return {"all -128": np.full((16, L1), -128, np.int8), "all +127": np.full((16, L1), 127, np.int8),
            "alternating": np.tile(alt, (16, 1)), "alternating, shifted": np.tile(-1 - alt, (16, 1)),
            "random": rng.integers(-128, 128, (16, L1), dtype=np.int8)}


@pytest.mark.parametrize("kind", list(_rows()))
def test_extreme_slices_fit_24_bits_and_finalize_sum_is_exact(kind):
    """Each slice driven with the activations that minimise and maximise its sums (127 on the
    negative or the positive weights, 0 elsewhere), in every combination over the three slices:
    the biased values stay in [0, 2^24), the record round-trips, and the three unpacked values + b0p
    equal the three sums + b0 as wrapping int32."""
    w0 = _rows()[kind][None]  # one bucket
    b0 = np.array([[-(1 << 31), (1 << 31) - 1, 0, -1, 1000, -1000, 77, 5, 1 << 24, -(1 << 24), 3, 4, 5, 6, 7, 8]], np.int32)
    off, b0p = model_tables(w0, b0)
    w = w0[0].astype(np.int64)
    sums = np.zeros((2, SLICES, 16), np.int64)  # [min / max][slice][output]
    for s in range(SLICES):
        ws = w[:, slice_columns(s)]
        sums[0, s] = (127 * np.minimum(ws, 0)).sum(axis=1)
        sums[1, s] = (127 * np.maximum(ws, 0)).sum(axis=1)
    assert sums.min() >= -(1 << 31) and sums.max() < (1 << 31)
    if kind == "all -128":
        assert sums[0].min() == -127 * 128 * 1024 and (off[0] == 127 * 128 * 1024).all()
    if kind == "all +127":
        assert sums[1].max() == 127 * 127 * 1024 and (off[0] == 0).all()
    biased = sums + off[0][None]
    assert biased.min() >= 0 and biased.max() < (1 << 24), (kind, int(biased.min()), int(biased.max()))
    assert (biased[0] == 0).all()  # the minimum is the offset's negative exactly
    rec = pack(biased)
    assert rec.shape == (2, SLICES, 12) and np.array_equal(unpack(rec), biased)
    for pick in range(8):  # which end each slice is at
        ends = [(pick >> s) & 1 for s in range(SLICES)]
        raw = sum(sums[e, s] for s, e in enumerate(ends))
        got = (sum(unpack(rec[e, s]) for s, e in enumerate(ends)) + b0p[0].astype(np.int64)) & M32
        assert np.array_equal(got, (raw + b0[0].astype(np.int64)) & M32), (kind, ends)


def test_pack_layout_and_roundtrip_of_random_records():
    """The dword layout stated above, on a record of distinct bytes, and a seeded round trip."""
    v = np.array([0x030201, 0x060504, 0x090807, 0x0C0B0A] * 4, np.int64)
    rec = pack(v[None])[0]
    assert rec[:3].tobytes() == bytes(range(1, 13))  # little-endian: the four values' 12 bytes in order
    assert np.array_equal(rec.reshape(4, 3), np.tile(rec[:3], (4, 1)))
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 24, (1000, 16))
    x[0], x[1] = 0, (1 << 24) - 1
    assert np.array_equal(unpack(pack(x)), x)


def test_plain_signed_24_bits_would_not_do():
    """Why the offset: the unbiased sums of an all -128 and an all +127 row span more than 2^24."""
    assert 127 * 127 * 1024 - (-127 * 128 * 1024) >= 1 << 24
    assert 127 * 128 * 1024 < 1 << 24


def _net_arrays(kind):
    from fishnet_amd import synthnet
    import edge_nets
    a = synthnet.synth_net_arrays(L1, 1, with_ft=False) if kind == "synthetic" else \
        edge_nets.edge_net_arrays(L1, 1, with_ft=False)
    return np.stack(a["w0"]), np.stack(a["b0"])


HOST_MAIN = r"""
#include <stdio.h>
#include <vector>
#include "nnue.h"
int main(int argc, char **argv) {
  std::vector<int8_t> w0(8 * 16 * 3072);
  std::vector<int32_t> b0(8 * 16), off(8 * 3 * 16), b0p(8 * 16);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(w0.data(), 1, w0.size(), f) != w0.size() || fread(b0.data(), 4, b0.size(), f) != b0.size()) return 2;
  fclose(f);
  if (!gn::part_offsets(w0.data(), b0.data(), 3072, off.data(), b0p.data())) return 3;
  f = fopen(argv[2], "wb");
  fwrite(off.data(), 4, off.size(), f), fwrite(b0p.data(), 4, b0p.size(), f);
  return fclose(f) ? 4 : 0;
}
"""


def test_host_offset_rule_equals_the_model(tmp_path):
    """nnue.h's part_offsets (what the library computes when it loads a big net), compiled into a
    stand-alone host program, on the bench's synthetic net, the edge net and the extreme rows."""
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    (tmp_path / "main.hip").write_text(HOST_MAIN)
    exe = tmp_path / "part_offsets"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "fishnet_amd", "csrc"),
                    str(tmp_path / "main.hip"), "-o", str(exe)], check=True, capture_output=True)
    rows = _rows()
    extreme = np.stack([rows[k] for k in list(rows)[:4]] * 2)
    cases = [_net_arrays("synthetic"), _net_arrays("edge"),
             (extreme, np.arange(-64, 64, dtype=np.int32).reshape(8, 16) * 16777213)]
    for i, (w0, b0) in enumerate(cases):
        src, dst = tmp_path / f"in{i}.bin", tmp_path / f"out{i}.bin"
        src.write_bytes(w0.astype(np.int8).tobytes() + b0.astype("<i4").tobytes())
        subprocess.run([str(exe), str(src), str(dst)], check=True)
        got = np.fromfile(dst, "<i4")
        off, b0p = model_tables(w0, b0)
        assert np.array_equal(got[:8 * 3 * 16].reshape(8, 3, 16), off), i
        assert np.array_equal(got[8 * 3 * 16:].reshape(8, 16), b0p), i


def test_range_net_drives_single_slices_to_both_ends(oracle_lib):
    """tests/part_pack_nets.py: on the hand-picked parents and their children the oracle's fc_0 sums
    are b0 + w * 126 * 1024 * (slices alive), w the bucket's weight: every slice's activations are all
    126 or all 0.  Both states occur in a NEG and in a POS bucket, children cross buckets, and the
    stored value reaches the largest offset there is, 127 * 128 * 1024 (a dead slice in a NEG bucket)."""
    import part_pack_nets as N
    O = oracle_lib
    net = O.Net(N.range_net())
    a = N.range_net_arrays()
    fens = [O.normalize_fen(f) for f in N.PICKED]
    kids = [O.child_fen(f, m) for f in fens for m in O.legal_moves(f)]
    seen, crossed = set(), set()
    for f in fens:
        crossed |= {(N.bucket(f), N.bucket(O.child_fen(f, m))) for m in O.legal_moves(f)}
    assert {(1, 0), (7, 6), (2, 1)} <= crossed, crossed
    tr = O.trace_fens(net, fens + kids)
    off, _ = model_tables(np.stack(a["w0"]), np.stack(a["b0"]))
    for f, t in zip(fens + kids, tr):
        b = N.bucket(f)
        assert int(t["bucket"]) == b
        if b not in N.NEG + N.POS:
            continue
        w, alive = (-128 if b in N.NEG else 127), N.alive_slices(f)
        want = a["b0"][b].astype(np.int64) + w * N.ACT * 1024 * sum(alive)
        assert np.array_equal(t["fc0"].astype(np.int64), want), f
        for s, al in enumerate(alive):
            stored = off[b, s] + (w * N.ACT * 1024 if al else 0)
            assert (0 <= stored).all() and (stored < 1 << 24).all()
            seen.add((b in N.NEG, al, int(stored[0])))
    assert {(neg, al) for neg, al, _ in seen} == {(True, True), (True, False), (False, True), (False, False)}
    assert max(v for _, _, v in seen) == 127 * 128 * 1024 and min(v for _, _, v in seen) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synthetic", "edge"])
def test_library_tables_equal_the_model(kind):
    """gn_debug_part_offsets (fishnet_amd/csrc/plan_snapshot.h, internal) of a loaded big net of the
    bench's shape -- the bench's own synthetic net and the edge net -- equals the model's tables."""
    from fishnet_amd import build, gpu_nnue as G, synthnet
    import edge_nets
    build.build()
    path = synthnet.cached_synth_net(L1, 1) if kind == "synthetic" else edge_nets.edge_net(L1, 1)
    ctx = G.GpuNnue(path, None)
    try:
        off, b0p = np.zeros((8, 3, 16), np.int32), np.zeros((8, 16), np.int32)
        f = G.lib().gn_debug_part_offsets
        f.argtypes, f.restype = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p], C.c_int
        G._check(f(ctx.h, 0, off.ctypes.data, b0p.ctypes.data))
        want_off, want_b0p = model_tables(*_net_arrays(kind))
        assert np.array_equal(off, want_off) and np.array_equal(b0p, want_b0p)
        assert off.min() >= 0 and off.max() < (1 << 24)
    finally:
        ctx.close()
