"""The row stream's lists hold no entry on the all-zero row: a chained parent takes the result
of the child that is its position, and a king-cache store rides on its slot's last row entry
(stream.hip).  Every case runs one input through the planned expansion and

  - compares every parent record, child record, move and offset byte for byte with the plain
    path (GN_OPT_CHAIN 1, GN_OPT_KING_CACHE 0: one refresh-started parent per workgroup),
  - compares sampled parents with all their children with the oracle,
  - relies on the plan's error word being clear (the library reads it after every planned
    expansion and fails the call on any bit: entry overflow, no scratch slot, a king-cache reload
    closer than GN_SCR_GAP to its store),
  - asserts GN_STAT_ZERO_ROW_ENTRIES == 0,

at GN_OPT_STREAM_SLICES 3 and 1, modes BIG and FULL, and exact chain lengths 2, 3 and 81.  The
plain path's results and the oracle's are computed once per input and mode.
"""
import numpy as np
import pytest

import edge_nets

pytestmark = pytest.mark.gpu

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
KP_ENDING = "8/8/4k3/8/8/4K3/4P3/8 w - - 0 1"
KP_SEED = 6  # (_playout: a seed whose game lasts the 80 plies)
PLIES, COPIES = 80, 24
MODE_BIG, MODE_FULL = 1, 0
THREADS = 16


def _playout(oracle_lib, fen, plies, seed):
    """The positions of a seeded random game from fen: plies + 1 FENs (the game must last)."""
    rng = np.random.default_rng(seed)
    fens = [oracle_lib.normalize_fen(fen)]
    for _ in range(plies):
        moves = oracle_lib.legal_moves(fens[-1])
        assert moves, "the playout ended early: choose another seed"
        fens.append(oracle_lib.child_fen(fens[-1], moves[int(rng.integers(len(moves)))]))
    return fens


def _boards(name, ctx, oracle_lib):
    """(boards, the FENs of the sampled parents, their indices)."""
    from fishnet_amd import gpu_nnue as G
    if name == "king_shuffle":  # every king-move child hits the cache; the position repeats every 4 plies
        shuffle = "e2e4 e7e5 " + " ".join(["e1e2 e8e7 e2e1 e7e8"] * 19) + " e1e2 e8e7"
        fens, _ = oracle_lib.replay_game(START, shuffle)
    elif name == "kp_ending":  # nearly every child a king move, refreshes of 3 rows, parents of few children
        fens = _playout(oracle_lib, KP_ENDING, PLIES, KP_SEED)
    else:  # the general mix: castling, promotions, captures that change the bucket
        d = ctx.alloc(COPIES * (PLIES + 1) * 32)
        ctx.random_games_device(0x5EED0E17, 0, COPIES, PLIES, d)
        ctx.synchronize()
        boards = d.download(G.BOARD_DTYPE, COPIES * (PLIES + 1))
        d.free()
        idx = np.concatenate([np.arange(PLIES + 1), 81 * 7 + np.arange(0, 81, 2)])  # a whole game and half of another
        return boards, G.boards_to_fens(boards[idx]), idx
    assert len(fens) == PLIES + 1
    one, ok = G.pack_fens(fens)
    assert ok.all()
    return np.tile(one, COPIES), fens, np.arange(PLIES + 1)


class _Input:
    """One input on the device with its output buffers; the plain path's results and the oracle's
    sampled expansions per mode, each computed once."""

    def __init__(self, ctx, oracle_lib, nets, name):
        from fishnet_amd import gpu_nnue as G
        self.ctx, self.O, self.nets = ctx, oracle_lib, nets
        self.boards, self.fens, self.idx = _boards(name, ctx, oracle_lib)
        n = self.n = len(self.boards)
        self.cap = 48 * n
        self.bufs = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4),
                                                    ("ch", self.cap * 32), ("mv", self.cap * 2),
                                                    ("co", self.cap * G.EVAL_SIZE))}
        self.bufs["b"].upload(self.boards)
        self._plain, self._oracle = {}, {}

    def run(self, mode, slices, chain, kc):
        from fishnet_amd import gpu_nnue as G
        ctx, b = self.ctx, self.bufs
        ctx.set_option(G.OPT_STREAM_SLICES, slices)
        ctx.set_option(G.OPT_CHAIN, chain)
        ctx.set_option(G.OPT_KING_CACHE, kc)
        try:
            t = ctx.expand_device(b["b"], self.n, mode, b["po"], b["off"], b["ch"], b["mv"], b["co"], self.cap)
            zero_row = ctx.get_option(G.STAT_ZERO_ROW_ENTRIES)
        finally:
            ctx.set_option(G.OPT_STREAM_SLICES, 3)
            ctx.set_option(G.OPT_CHAIN, 81)
            ctx.set_option(G.OPT_KING_CACHE, 1)
        return (b["po"].download(G.EVAL_DTYPE, self.n), b["off"].download(np.uint32, self.n + 1),
                b["mv"].download(np.uint16, t), b["co"].download(G.EVAL_DTYPE, t)), zero_row

    def plain(self, mode):
        if mode not in self._plain:
            self._plain[mode] = self.run(mode, 3, 1, 0)[0]
        return self._plain[mode]

    def oracle(self, mode):
        if mode not in self._oracle:
            big, small = self.nets
            par, cnt, kids = self.O.expand_eval_batch(big, small if mode == MODE_FULL else None, self.fens, mode, True,
                                                      threads=THREADS, keep_children=True)
            self._oracle[mode] = (par, cnt, kids, [self.O.legal_moves(f) for f in self.fens])
        return self._oracle[mode]

    def check(self, mode, slices, chain):
        what = f"mode {mode} slices {slices} chain {chain}"
        got, zero_row = self.run(mode, slices, chain, 1)
        for name, a, b in zip(("parents", "offsets", "moves", "children"), self.plain(mode), got):
            assert a.tobytes() == b.tobytes(), (what, name, int(np.flatnonzero(a != b)[0]) if a.shape == b.shape else -1)
        po, off, mv, co = got
        par, cnt, kids, moves = self.oracle(mode)
        for j, i in enumerate(self.idx):
            assert tuple(po[i]) == tuple(par[j]), (what, self.fens[j])
            lo, hi = int(off[i]), int(off[i + 1])
            assert hi - lo == cnt[j] == len(moves[j]), (what, self.fens[j])
            assert {int(m): tuple(x) for m, x in zip(mv[lo:hi], co[lo:hi])} == \
                   {int(m): tuple(x) for m, x in zip(moves[j], kids[j, :cnt[j]])}, (what, self.fens[j])
        assert zero_row == 0, what

    def free(self):
        for b in self.bufs.values():
            b.free()


@pytest.fixture(scope="module")
def inputs(gpu_ctx, oracle_lib, oracle_nets):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Input(gpu_ctx, oracle_lib, oracle_nets, name)
        return made[name]
    yield get
    for x in made.values():
        x.free()


@pytest.mark.parametrize("chain", [-2, -3, -81])
@pytest.mark.parametrize("mode", [MODE_BIG, MODE_FULL])
@pytest.mark.parametrize("slices", [3, 1])
@pytest.mark.parametrize("name", ["king_shuffle", "kp_ending", "random_games"])
def test_no_zero_row_entries(inputs, name, slices, mode, chain):
    """king_shuffle: the game of test_king_cache_reload_at_minimum_gap, 24 copies -- every king-move
    child hits the cache, hits without a difference (the load entry alone, carrying the store) occur,
    and a store merged into a row entry is reloaded at the minimum gap.  kp_ending: a king-and-pawn ending
    played 80 plies -- the non-hit paths, slots of one or two row entries (two stores inside one
    ring window), chained parents alone at a tile's start and tiles without an evaluated slot.
    random_games: 24 seeded 80-ply games."""
    inputs(name).check(mode, slices, chain)


def test_no_zero_row_entries_1024_wide_net(oracle_lib):
    """stream_eval_kernel<1024, 1> (one launch over whole rows; its writer stores a chained
    parent's output with the child's) on the 1,024-wide edge net: the three inputs above, chain
    lengths 2, 3 and 81."""
    from fishnet_amd import build, gpu_nnue as G
    build.build()
    path = edge_nets.edge_net(1024, 5)
    ctx = G.GpuNnue(path, None)
    made = []
    try:
        assert ctx.net_info()["big_l1"] == 1024
        nets = (oracle_lib.Net(path), None)
        for name in ("king_shuffle", "kp_ending", "random_games"):
            x = _Input(ctx, oracle_lib, nets, name)
            made.append(x)
            for chain in (-2, -3, -81):
                x.check(MODE_BIG, 3, chain)
    finally:
        for x in made:
            x.free()
        ctx.close()
