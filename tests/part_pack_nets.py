"""A purpose-made big net for the packed partial sums (test infrastructure only): single column
slices of fc_0 reach both ends of their range.

  fc_0   buckets NEG: every weight -128; buckets POS: every weight +127; the other buckets, fc_1,
         fc_2, the biases and the PSQT table are the (3072, 1) edge net's (tests/edge_nets.py).
  FT     bias 1000 in every column (2000 doubled: both halves of every pair clamp to 254, and the
         transform's largest output is 254 * 254 >> 9 = 126); every weight 0, except KILL on the
         columns of slice s (both halves, columns 1536 h + 512 s .. + 511) in the rows of the piece
         types KILL_PLANES[s] of either colour: slice 0 dies with a queen on the board, slice 1
         with a rook, slice 2 with a knight (accumulator 2000 - 5000 k < 0, activation 0; in int16
         up to k = 6 such pieces).

So a slice's 1,024 activations are all 126 or all 0, by position, and a slice's sum in a NEG bucket
is -126 * 128 * 1024 or 0 (stored as 131,072 or 16,646,144, the largest offset there is), in a POS
bucket 126 * 127 * 1024 = 16,386,048 or 0.  127 itself is not reachable: the transform ends at 126.
"""
import os
import struct

import numpy as np

import edge_nets
from fishnet_amd import synthnet

L1 = 3072
NEG, POS = (0, 7), (1, 6)
BIAS, KILL = 1000, -2500
KILL_PLANES = ((8, 9), (6, 7), (2, 3))  # (own, their) queen / rook / knight planes of HalfKAv2_hm
KILL_LETTERS = ("Qq", "Rr", "Nn")
ACT = 126


def range_net_arrays():
    a = edge_nets.edge_net_arrays(L1, 1, with_ft=False)
    for b in NEG:
        a["w0"][b] = np.full((16, L1), -128, np.int8)
    for b in POS:
        a["w0"][b] = np.full((16, L1), 127, np.int8)
    a["ft_bias"] = np.full(L1, BIAS, np.int16)
    return a


def _ft_weight_block():
    """The LEB128 block of the FT weights [22528][3072]: 0 (one byte) or KILL (two bytes)."""
    plane = (np.arange(synthnet.FT_INPUTS) % 704) // 64
    col_slice = (np.arange(L1) % (L1 // 2)) // (L1 // 6)
    kill = np.zeros((synthnet.FT_INPUTS, L1), bool)
    for s, planes in enumerate(KILL_PLANES):
        kill |= np.isin(plane, planes)[:, None] & (col_slice == s)[None, :]
    two = synthnet.leb128_encode(np.array([KILL]))[21:]
    assert len(two) == 2
    buf = np.zeros((synthnet.FT_INPUTS, L1, 2), np.uint8)
    buf[..., 0][kill] = two[0]
    buf[..., 1] = two[1]
    keep = np.ones(buf.shape, bool)
    keep[..., 1] = kill
    payload = buf[keep].tobytes()
    return synthnet.LEB_MAGIC + struct.pack("<I", len(payload)) + payload


def range_net_bytes():
    a = range_net_arrays()
    net_hash, ft_hash, _ = synthnet.hashes(L1)
    desc = b"fishnet_amd range net for the packed partial sums"
    return b"".join([struct.pack("<III", synthnet.VERSION, net_hash, len(desc)), desc, struct.pack("<I", ft_hash),
                     synthnet.leb128_encode(a["ft_bias"]), _ft_weight_block(), synthnet.tail_bytes(a, L1)])


def range_net(cache_dir=None):
    """Path of the net, generated once into the cache directory of cached_synth_net."""
    cache_dir = cache_dir or os.environ.get("GPU_NNUE_CACHE") or os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), ".cache")
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, "range_L3072.nnue")
    if not os.path.exists(path):
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(range_net_bytes())
        os.replace(tmp, path)
    return path


# Hand-picked parents (white to move, a capture on d5 available): the piece count drops across a
# layer-stack bucket, (count - 1) // 4: 5 -> 4 pieces is POS bucket 1 -> NEG bucket 0, 29 -> 28 is NEG
# bucket 7 -> POS bucket 6, 9 -> 8 is bucket 2 -> POS bucket 1; with queens, rooks, knights or none of
# them, so that the slices die one at a time.
PICKED = ("4k3/8/8/3b4/4P3/8/8/3BK3 w - - 0 1",      # no queen, rook or knight: every slice at 126
          "4k3/8/8/3q4/4P3/8/8/3QK3 w - - 0 1",      # queens: slice 0 at 0
          "4k3/8/8/3r4/4P3/8/8/3RK3 w - - 0 1",      # rooks: slice 1 at 0
          "4k3/8/8/3n4/4P3/8/8/3NK3 w - - 0 1",      # knights: slice 2 at 0
          "4k3/8/8/3q4/4P3/8/8/3BK3 w - - 0 1",      # the capture removes the only queen: slice 0 comes alive
          "4k3/pp6/8/3r4/4P3/8/PP6/3RK3 w - - 0 1",  # 9 -> 8 pieces
          "rnbqkb1r/ppp1pppp/8/3p4/4P3/8/PPPP1PPP/R1BQKBN1 w Qkq - 0 1",  # 29 -> 28 pieces
          "4k3/8/8/3b4/4P3/8/8/3BK3 b - - 0 1")      # black to move


def alive_slices(fen):
    """Per slice: no piece of its killing type is on the board (its activations are all 126)."""
    placement = fen.split()[0]
    return [not any(c in placement for c in letters) for letters in KILL_LETTERS]


def bucket(fen):
    return (sum(c.isalpha() for c in fen.split()[0]) - 1) // 4
