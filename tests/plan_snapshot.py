"""gn_debug_plan_snapshot (fishnet_amd/csrc/plan_snapshot.h, internal) for the tests: the last
planned expansion's plan as a plan_replay.Snapshot.  The entry point is not part of the public
header, so it is bound here and not in fishnet_amd.gpu_nnue."""
import ctypes as C

import numpy as np

import plan_replay

U32_FIELDS = ("header_bytes", "tile_bytes", "l1", "row_stride", "ft_rows", "ft_bias_row", "zero_row", "scr_rows",
              "ent_spare", "scr_gap", "ring", "slice_ring", "np", "k", "nblk", "slices", "xu", "hu", "kc", "ordered")
U64_FIELDS = ("npos", "n_ent", "n_tiles", "n_pinfo", "pads", "zero_row_entries", "rows")


class Header(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in U32_FIELDS] + [(n, C.c_uint64) for n in U64_FIELDS]


class Bufs(C.Structure):
    _fields_ = [(n, t) for name in ("eoff", "ent", "tiles", "btiles", "order", "pinfo", "offsets")
                for n, t in ((name, C.c_void_p), (name + "_cap", C.c_size_t))]


def _fn(G):
    f = G.lib().gn_debug_plan_snapshot
    f.argtypes = [C.c_void_p, C.c_int, C.POINTER(Header), C.POINTER(Bufs)]
    f.restype = C.c_int
    return f


def header(G, ctx, slot=0):
    """The sizes and constants alone (raises G.GnError when the last expansion was not planned)."""
    h = Header()
    G._check(_fn(G)(ctx.h, slot, C.byref(h), None))
    assert h.header_bytes == C.sizeof(Header) and h.tile_bytes == plan_replay.TILE_DTYPE.itemsize
    return h


def take(G, ctx, slot=0, shrink=None):
    """The snapshot of ctx's device slot.  shrink: the name of one buffer to pass one element too
    small (the call must then fail)."""
    h = header(G, ctx, slot)
    arrays = {"eoff": np.zeros(h.np + 1, np.uint64), "ent": np.zeros(h.n_ent, np.uint64),
              "tiles": np.zeros(h.n_tiles, plan_replay.TILE_DTYPE), "btiles": np.zeros(h.nblk, np.uint32),
              "order": np.zeros(h.nblk, np.uint32), "pinfo": np.zeros((h.n_pinfo, 2), np.int32),
              "offsets": np.zeros(h.np + 1, np.uint64)}
    b = Bufs()
    for name, a in arrays.items():
        setattr(b, name, a.ctypes.data)
        setattr(b, name + "_cap", len(a) - (1 if name == shrink else 0))
    G._check(_fn(G)(ctx.h, slot, C.byref(h), C.byref(b)))
    hdr = {n: int(getattr(h, n)) for n in U32_FIELDS + U64_FIELDS}
    return plan_replay.Snapshot(hdr, arrays["eoff"], arrays["ent"], arrays["tiles"], arrays["btiles"], arrays["order"],
                                arrays["pinfo"] if h.n_pinfo else None, arrays["offsets"])
