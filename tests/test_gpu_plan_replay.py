"""The plan of the planned expansion, replayed on the CPU (tests/plan_replay.py).

Every case runs one input through gn_expand_device, copies the plan plan_kernel wrote
(gn_debug_plan_snapshot, fishnet_amd/csrc/plan_snapshot.h), executes its lists in list order and
expects no finding: every evaluated slot's two half accumulators equal the oracle's or_accumulate
(rows from the net file's arrays, not from the device), every scratch load sits GN_SCR_GAP entries
behind its row's store in its own list, a scratch row belongs to one list, and the descriptors,
regions, counters and pinfo are what kernels.h says.  The records of the same run equal the plain
path's (GN_OPT_CHAIN 1, GN_OPT_KING_CACHE 0) byte for byte, so a plan the checker passes is also a
plan the stream evaluates correctly.

Inputs (built with the helpers of tests/test_stream_entries.py): king_shuffle and kp_ending, one game
each; four seeded random 80-ply games; special_fens.txt as unrelated consecutive parents; the
castling games of test_chained_links_of_special_moves_vs_oracle.  Options: the rows of CONFIGS.
The oracle's accumulators are computed once per input and net.

Wall time of the file's CPU work and the counted situations: see test_input_conditions.
"""
import numpy as np
import pytest

import edge_nets
import plan_replay as R
import plan_snapshot
import test_games
import test_stream_entries as SE

pytestmark = pytest.mark.gpu

MODE_BIG, MODE_FULL = SE.MODE_BIG, SE.MODE_FULL
INPUTS = ("king_shuffle", "kp_ending", "random_games", "special_fens", "castling_games")
# (net, mode, GN_OPT_STREAM_SLICES, GN_OPT_CHAIN, GN_OPT_KING_CACHE): every chain length of the issue
# (-2, -3, -81 exact; 81 shortened to fill the device; 1 unchained), the king cache on and off, both
# modes (FULL: the need masks leave slots unevaluated), the 3072-wide net sliced and whole-row, and
# the 1,024-wide edge net (its tile field counts 16-byte units as the sliced stream's does)
CONFIGS = ((3072, MODE_BIG, 3, 81, 1), (3072, MODE_BIG, 1, -3, 1), (3072, MODE_FULL, 3, -2, 1),
           (3072, MODE_FULL, 3, -81, 1), (3072, MODE_BIG, 3, -81, 0), (3072, MODE_FULL, 1, 1, 1),
           (3072, MODE_BIG, 1, -81, 1), (1024, MODE_BIG, 3, -81, 1), (1024, MODE_BIG, 3, -2, 1))
CONDITIONS = ("reload_at_gap", "reload_at_list_gap", "pads", "kst_hit_without_difference", "third_bucket_cuts", "multi_pass_parents",
              "chained_parent_first_in_tile", "king_child_in_other_list")


class _Input(SE._Input):
    """test_stream_entries' input (device buffers, run(), the plain path once per mode) over this
    file's boards."""

    def __init__(self, ctx, oracle_lib, nets, boards, fens):
        from fishnet_amd import gpu_nnue as G
        self.ctx, self.O, self.nets = ctx, oracle_lib, nets
        self.boards, self.fens, self.idx = boards, fens, np.arange(len(boards))
        n = self.n = len(boards)
        self.cap = 64 * n + 256
        self.bufs = {k: ctx.alloc(sz) for k, sz in (("b", n * 32), ("po", n * G.EVAL_SIZE), ("off", (n + 1) * 4),
                                                    ("ch", self.cap * 32), ("mv", self.cap * 2),
                                                    ("co", self.cap * G.EVAL_SIZE))}
        self.bufs["b"].upload(self.boards)
        self._plain, self._oracle = {}, {}
        self._positions = None

    def positions(self, off, mv, mode):
        """The reference of every parent and child (plan_replay.Positions): or_accumulate of both
        perspectives, once; evaluated: what the oracle's evaluation takes the big net for."""
        O, big = self.O, self.nets[0]
        if self._positions is None:
            fens = list(self.fens)
            for i, f in enumerate(self.fens):
                fens += [O.child_fen(f, int(m)) for m in mv[int(off[i]):int(off[i + 1])]]
            acc = np.zeros((len(fens), 2, big.l1), np.uint16)
            psqt = np.zeros((len(fens), 2, 8), np.int32)
            for q, f in enumerate(fens):
                for h in range(2):
                    a, psqt[q, h] = O.accumulate(big, f, h)
                    acc[q, h] = a.view(np.uint16)
            stm = np.array([f.split()[1] == "b" for f in fens], np.uint8)
            pieces = np.array([sum(ch.isalpha() for ch in f.split()[0]) for f in fens], np.int32)
            self._positions = (fens, stm, pieces, acc, psqt, {})
        fens, stm, pieces, acc, psqt, ev = self._positions
        if mode not in ev:
            if mode == MODE_BIG:
                ev[mode] = np.ones(len(fens), bool)
            else:
                rec = O.eval_fens(big, self.nets[1], fens, mode, threads=SE.THREADS)
                ev[mode] = (rec["flags"] & O.FLAG_SMALLNET) == 0
        return R.Positions(stm, pieces, acc, psqt, ev[mode])


def _make_boards(name, ctx, O):
    from fishnet_amd import gpu_nnue as G
    if name in ("king_shuffle", "kp_ending"):  # one game of the 24 copies
        boards, fens, _ = SE._boards(name, ctx, O)
        return boards[:SE.PLIES + 1].copy(), fens
    if name == "random_games":  # four of its seeded games
        boards, _, _ = SE._boards(name, ctx, O)
        boards = boards[:4 * (SE.PLIES + 1)].copy()
        return boards, G.boards_to_fens(boards)
    if name == "special_fens":
        fens = [O.normalize_fen(f) for f in edge_nets._fen_file("special_fens.txt")]
    else:
        fens = []
        for root, moves in test_games.SPECIAL_MOVE_GAMES[test_games.CASTLING_GAMES_FROM:]:
            fens += O.replay_game(root, moves)[0]
    boards, ok = G.pack_fens(fens)
    assert ok.all()
    return boards, fens


class _World:
    """Per net: the context, the oracle's net, the doubled row table from the file's arrays, the
    inputs; per (input, configuration): the run's snapshot, findings and counted situations."""

    def __init__(self, gpu_ctx, oracle_lib, oracle_nets):
        self.O, self.nets, self.ctx = oracle_lib, {3072: oracle_nets}, {3072: gpu_ctx}
        self.tables, self.inputs, self.runs = {}, {}, {}
        self.own = []

    def net(self, l1):
        from fishnet_amd import build, gpu_nnue as G, synthnet
        if l1 not in self.ctx:
            build.build()
            path = edge_nets.edge_net(1024, 5)
            self.ctx[l1] = G.GpuNnue(path, None)
            self.own.append(self.ctx[l1])
            self.nets[l1] = (self.O.Net(path), None)
        if l1 not in self.tables:
            a = synthnet.synth_net_arrays(3072, 1) if l1 == 3072 else edge_nets.edge_net_arrays(1024, 5)
            self.tables[l1] = R.doubled_table(a["ft_w"], a["ft_bias"])
        return self.ctx[l1], self.nets[l1], self.tables[l1]

    def input(self, l1, name):
        if (l1, name) not in self.inputs:
            ctx, nets, _ = self.net(l1)
            self.inputs[(l1, name)] = _Input(ctx, self.O, nets, *_make_boards(name, ctx, self.O))
        return self.inputs[(l1, name)]

    def run(self, name, cfg):
        from fishnet_amd import gpu_nnue as G
        if (name, cfg) not in self.runs:
            l1, mode, slices, chain, kc = cfg
            ctx, _, table = self.net(l1)
            x = self.input(l1, name)
            ctx.set_option(G.OPT_EXPAND_PIPELINE, 0)
            try:
                got, zero_row = x.run(mode, slices, chain, kc)
                snap = plan_snapshot.take(G, ctx)
                plain = x.plain(mode)
            finally:
                ctx.set_option(G.OPT_EXPAND_PIPELINE, 2)
            pos = x.positions(got[1], got[2], mode)
            stats = {}
            findings = R.check_plan(snap, table, pos, stats)
            self.runs[(name, cfg)] = dict(got=got, plain=plain, snap=snap, pos=pos, findings=findings, stats=stats,
                                          zero_row=zero_row, table=table)
        return self.runs[(name, cfg)]

    def close(self):
        for x in self.inputs.values():
            x.free()
        for c in self.own:
            c.close()


@pytest.fixture(scope="module")
def world(gpu_ctx, oracle_lib, oracle_nets):
    w = _World(gpu_ctx, oracle_lib, oracle_nets)
    yield w
    w.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "L%d-mode%d-slices%d-chain%d-kc%d" % c)
@pytest.mark.parametrize("name", INPUTS)
def test_plan_replays_without_findings(world, name, cfg):
    r = world.run(name, cfg)
    h, s = r["snap"].hdr, r["stats"]
    print(f"{name} {cfg}: np {h['np']} k {h['k']} blocks {h['nblk']} xu {h['xu']} hu {h['hu']} entries {s['entries']} "
          f"pads {h['pads']} rows {h['rows']} moving {s['moving_entries']} parent stores {s['parent_stores']} "
          + " ".join(f"{k} {s[k]}" for k in CONDITIONS))
    assert [tuple(f) for f in r["findings"][:20]] == [], len(r["findings"])
    for what, a, b in zip(("parents", "offsets", "moves", "children"), r["plain"], r["got"]):
        assert a.tobytes() == b.tobytes(), (what, int(np.flatnonzero(a != b)[0]) if a.shape == b.shape else -1)
    l1, mode, slices, chain, kc = cfg
    assert h["l1"] == l1 and h["slices"] == (slices if l1 == 3072 else 1) and h["np"] == len(r["plain"][0])
    assert h["k"] == (abs(chain) if chain < 0 else h["k"]) and h["kc"] == (kc if h["k"] > 1 else 0)
    assert (h["xu"], h["hu"]) == ((2, 1) if (l1, slices) == (3072, 1) else (65, 32))
    assert s["evaluated_slots"] > 0 and r["zero_row"] == h["zero_row_entries"] == 0


def test_input_conditions(world):
    """The situations the inputs exist for, counted over the whole matrix on the snapshots: a net,
    seed or fixture change that removes one fails here.

    Counted on the MI355X's plans (45 snapshots): 4 reloads exactly GN_SCR_GAP behind their own row's
    store (random_games, FULL, chain 2) and 1,464 that far behind the list's last store to another
    row; 4,262 no-op pads; 673 stores on a hit without a difference; 12 tile cuts for a third
    bucket; 27 parents of more than one 64-slot pass; 211 chained parents first in their tile; 4,984
    king-move children in the other perspective's list.

    Wall time of this file's CPU work, measured on one core replaying the 45 saved snapshots: 11 s
    for the replays, 17 s for the two row tables, 2 s for the oracle's accumulators (the whole file
    on the MI355X's host: 11 s)."""
    total = dict.fromkeys(CONDITIONS, 0)
    for name in INPUTS:
        for cfg in CONFIGS:
            s = world.run(name, cfg)["stats"]
            for k in CONDITIONS:
                total[k] += s[k]
    print("counted over the matrix:", total)
    for k in CONDITIONS:
        assert total[k] > 0, (k, total)


MUTATE_ON = ("king_shuffle", (3072, MODE_FULL, 3, -81, 1))  # (one of CONFIGS: sliced, chained, king cache)


def _recheck(r, snap):
    return R.names(R.check_plan(snap, r["table"], r["pos"]))


def _swap_reload_with_its_pad(r, per_row):
    """The snapshot with one reload at exactly GN_SCR_GAP (behind its own row's store, or behind the
    list's last store to another row) swapped with the no-op pad before it: the accumulators stay
    what they were, the reload sits one entry too close."""
    snap, gap = r["snap"].copy(), r["snap"].hdr["scr_gap"]
    for blk, g, i, row, j, last_any in r["stats"]["loads"]:
        e = snap.list_entries(blk, g)
        if j is None or i == 0 or int(snap.ent[e[i - 1]]) >> 32 & 0xFFFF != 0:
            continue
        if (i - j == gap) if per_row else (i - last_any == gap and i - j > gap):
            snap.ent[e[i - 1]], snap.ent[e[i]] = snap.ent[e[i]], snap.ent[e[i - 1]]
            return snap
    pytest.fail("no reload at the minimum gap behind a pad")


def test_mutation_reload_closer_than_the_gap(world):
    """A reload one entry closer than GN_SCR_GAP to its row's store: the per-row gap finding and no
    other (random_games, FULL, chain 2: the one configuration with such reloads).  One as close to
    the list's last store, of another row: the plan's declared rule alone.  Nothing doctored goes to
    the GPU."""
    r = world.run("random_games", (3072, MODE_FULL, 3, -2, 1))
    assert _recheck(r, _swap_reload_with_its_pad(r, True)) == [R.F_GAP_ROW]
    r = world.run(*MUTATE_ON)
    assert _recheck(r, _swap_reload_with_its_pad(r, False)) == [R.F_GAP_LIST]


def test_mutation_multiplier(world):
    """One row subtracted where it is added: accumulator findings and no other."""
    r = world.run(*MUTATE_ON)
    snap = r["snap"].copy()
    e = snap.list_entries(0, 1)
    i = next(i for i in range(len(e)) if int(snap.ent[e[i]]) >> 32 & 0x3FFFF == 1)  # a plain add
    snap.ent[e[i]] = int(snap.ent[e[i]]) | 0xFFFF << 32
    assert _recheck(r, snap) == [R.F_ACC]


def test_mutation_store_in_the_other_list(world):
    """The first store of a king-cache row that its list reloads later (a child's), moved to a slot's
    last entry in the other list: the ownership finding and no other."""
    r = world.run(*MUTATE_ON)
    snap = r["snap"].copy()
    reloaded = {(blk, g, j) for blk, g, i, row, j, _ in r["stats"]["loads"] if j is not None}
    for blk, g, i, row, first in r["stats"]["stores"]:
        e, o = snap.list_entries(blk, g), snap.list_entries(blk, 1 - g)
        w = int(snap.ent[e[i]])
        plain_last = [x for x in o if (int(snap.ent[x]) >> 32) & (R.H_LAST | R.H_X) == R.H_LAST]
        # (a child's store: a parent's counts as a row of its own in the plan's row count)
        if first and (blk, g, i) in reloaded and not w & R.L_SCR and not (w >> 32) & R.H_PAR_E and plain_last:
            hi = (w >> 32) & ~(R.H_KST | R.H_X)
            snap.ent[e[i]] = (w & 0xFFFFFFFF & ~R.L_KT) | hi << 32
            snap.ent[plain_last[0]] = int(snap.ent[plain_last[0]]) | (row - 2) | (R.H_X | R.H_KST) << 32
            break
    else:
        pytest.fail("no first store that is reloaded")
    assert _recheck(r, snap) == [R.F_OWNER]


def test_mutation_alias_of_the_wrong_child(world):
    """A chained parent's PINFO_ALIAS pointed at a sibling of the child that is its position."""
    r = world.run(*MUTATE_ON)
    snap = r["snap"].copy()
    off = snap.offsets
    for p in range(1, snap.hdr["np"]):
        y, nch = int(snap.pinfo[p, 1]), int(off[p] - off[p - 1])
        if y >= 0 and y & R.PINFO_ALIAS and nch > 1:
            c = ((y >> R.PINFO_NS_SH) + 1) % nch
            snap.pinfo[p, 1] = (y & (1 << R.PINFO_NS_SH) - 1) | c << R.PINFO_NS_SH
            break
    else:
        pytest.fail("no chained parent")
    assert _recheck(r, snap) == [R.F_PINFO_ALIAS]


def test_snapshot_errors(world):
    """GN_E_INVALID with a message: a buffer one element too small; an expansion that was not planned
    (the small net alone)."""
    from fishnet_amd import gpu_nnue as G
    r = world.run(*MUTATE_ON)
    ctx, _, _ = world.net(3072)
    x = world.input(3072, MUTATE_ON[0])
    x.run(*MUTATE_ON[1][1:])
    for name in ("eoff", "ent", "tiles", "btiles", "order", "pinfo", "offsets"):
        with pytest.raises(G.GnError) as e:
            plan_snapshot.take(G, ctx, shrink=name)
        assert e.value.code == G.E_INVALID and f"buffer {name} holds" in str(e.value), name
    again = plan_snapshot.take(G, ctx)  # (the same input and options: the same plan)
    assert again.hdr == r["snap"].hdr and again.btiles.tobytes() == r["snap"].btiles.tobytes()
    assert R.names(R.check_plan(again, r["table"], r["pos"])) == []
    x.run(2, 3, -81, 1)  # GN_MODE_SMALL
    with pytest.raises(G.GnError) as e:
        plan_snapshot.header(G, ctx)
    assert e.value.code == G.E_INVALID and "not planned" in str(e.value)
