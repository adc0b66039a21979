"""An independent CPU interpreter and checker of the planned expansion's plan (test infrastructure).

plan_kernel (fishnet_amd/csrc/stream.hip) turns every block of consecutive parents into two lists of
row entries and a descriptor per tile of <= 16 slots; stream_eval_kernel walks the lists.  This
module executes the lists in list order from the documented entry format (the head comment of
stream.hip, kernels.h at TileDesc and PINFO_ALIAS), compares what every slot's last entry leaves
in the accumulator with a reference computed elsewhere (the oracle's or_accumulate), and checks
from the entries themselves the ordering rules the stream relies on.  Pure numpy: no GPU, no
library.  It shares nothing with plan_kernel: where the plan tracks "the list's last scratch
store" to keep its own rule, the checker recomputes every distance from the list.

Entry (u64 = lo | hi << 32), as the stream consumes it:
  lo & ~127   the row's byte offset: row * row_stride; with bit 31 (SCR) a row of the block's
              scratch slot, row index ft_rows + r, r = 2 + 64 h + ksq the king-cache row
  lo & 127    at a KST entry: 64 h + ksq of the king-cache row it stores to
  hi[15:0]    multiplier m: 1, 0xFFFF (-1) or 0 (a no-op)
  hi[17:16]   source: 0 the accumulator, 1 ZERO, 2 PACC (the list's parent accumulator; the result
              becomes the sibling base), 3 BASE (the sibling base)      acc = src + m * row  (mod 2^16)
  hi[18]      LAST: the slot's half accumulator is complete; hi[31:22] = slot * xu + side * hu
  hi[19]      X, with hi[20] PAR_E (acc becomes the list's parent accumulator) or hi[21] KST (acc is
              stored to the king-cache row); the stream looks at both at a LAST entry only
The accumulators are compared in the doubled domain: table rows are 2 * the file's weights mod 2^16,
which is what or_accumulate returns (2 * (bias + sum of rows), wrapped).

check_plan() returns a list of Finding(name, where, detail); the names are the module's F_*
constants.  One defect gets one name: an accumulator that depends on a scratch row the list had
not stored is not compared (the load is the finding), and a load that breaks the per-row gap is not
also reported under the plan's stronger per-list rule.
"""
from collections import namedtuple

import numpy as np

TILE_DTYPE = np.dtype([("e_end", "<u4", 2), ("p_first", "<u4"), ("first", "<u4"), ("meta", "u1", 16),
                       ("psq", "<i4", (16, 2)), ("adj", "<i2", 16)])
assert TILE_DTYPE.itemsize == 192

H_LAST, H_X, H_PAR_E, H_KST, H_LDS_SH = 1 << 18, 1 << 19, 1 << 20, 1 << 21, 22
L_SCR, L_KT = 1 << 31, 127
SRC_ACC, SRC_ZERO, SRC_PACC, SRC_BASE = 0, 1, 2, 3
META_EVAL, META_PARENT, META_STM, META_NEXT_PARENT = 1, 16, 32, 64
PINFO_ALIAS, PINFO_NS_SH = 1 << 3, 4

F_ACC = "accumulator"
F_PSQT = "psqt"
F_META_BUCKET, F_META_SIDE, F_META_PARENT, F_META_EVAL = "meta bucket", "meta side", "meta parent", "meta evaluated"
F_GAP_ROW, F_GAP_LIST = "gap per row", "gap per list"
F_NOT_STORED, F_OWNER, F_KST_PLACE = "loaded row was stored", "ownership", "KST placement"
F_TILE_SLOTS, F_TILE_BUCKETS, F_E_END, F_REGION, F_REGIONS, F_BTILES = \
    "tile slots", "tile buckets", "e_end order", "region overflow", "regions overlap", "btiles bound"
F_SLOT_MAP = "slot map"
F_LAST, F_UNEVAL, F_CHAIN = "LAST count", "unevaluated slot has entries", "chain"
F_ZERO_ROW, F_NOOP_ROW, F_ENTRY = "zero row", "no-op row", "entry format"
F_STAT_PADS, F_STAT_ZERO, F_STAT_ROWS = "stat pads", "stat zero rows", "stat rows"
F_PINFO_BUCKET, F_PINFO_ALIAS, F_PINFO_EVAL, F_PINFO_PSQT = "pinfo bucket", "pinfo alias", "pinfo evaluated", "pinfo psqt"

Finding = namedtuple("Finding", "name where detail")


class Snapshot:
    """The plan of one expansion: hdr (the constants of gn_plan_snapshot_header by name) and the
    arrays eoff, ent, tiles (TILE_DTYPE), btiles, order, pinfo ([npos, 2] or None) and offsets."""

    def __init__(self, hdr, eoff, ent, tiles, btiles, order, pinfo, offsets):
        self.hdr = dict(hdr)
        self.eoff, self.ent, self.tiles, self.btiles = eoff, ent, tiles, btiles
        self.order, self.pinfo, self.offsets = order, pinfo, offsets

    def copy(self):
        c = lambda a: None if a is None else a.copy()
        return Snapshot(self.hdr, c(self.eoff), c(self.ent), c(self.tiles), c(self.btiles), c(self.order),
                        c(self.pinfo), c(self.offsets))

    def region(self, blk):
        """(first entry, one past the last) of block blk's entry region."""
        h = self.hdr
        pbeg, pend = blk * h["k"], min(blk * h["k"] + h["k"], h["np"])
        return int(self.eoff[pbeg]) + h["ent_spare"] * blk, int(self.eoff[pend]) + h["ent_spare"] * (blk + 1)

    def tile_base(self, blk):
        h = self.hdr
        pbeg = blk * h["k"]
        return (pbeg + int(self.offsets[pbeg])) // 16 + (h["k"] + 2) * blk

    def list_entries(self, blk, g):
        """Indices into ent of list g of block blk, in list order (list 0 upward from the region's
        start, list 1 downward from its end), as long as the block's last tile says."""
        rbeg, rend = self.region(blk)
        n = int(self.tiles[self.tile_base(blk) + int(self.btiles[blk]) - 1]["e_end"][g]) if self.btiles[blk] else 0
        return rbeg + np.arange(n) if g == 0 else rend - 1 - np.arange(n)


class Positions:
    """The reference, by output index q (parent p: p; child c of the expansion: np + c):
    stm[q] (0 white), pieces[q], acc[q, perspective] (uint16[L1], the doubled accumulators of the
    absolute perspective, 0 white), psqt[q, perspective, bucket] (int32) and evaluated[q] (the big
    net evaluates the position)."""

    def __init__(self, stm, pieces, acc, psqt, evaluated):
        self.stm, self.pieces, self.acc, self.psqt, self.evaluated = stm, pieces, acc, psqt, evaluated


def doubled_table(ft_w, ft_bias):
    """The rows as the stream adds them: 2 * the file's weights mod 2^16, the bias row last."""
    t = np.empty((ft_w.shape[0] + 1, ft_w.shape[1]), dtype=np.uint16)
    np.multiply(ft_w.view(np.uint16), 2, out=t[:-1])
    t[-1] = ft_bias.astype(np.int16).view(np.uint16) * np.uint16(2)
    return t


def psqt_term(a, b):
    """Network::evaluate's PSQT term (a - b) / 2 in wrapping int32, truncated toward zero."""
    d = (int(a) - int(b)) & 0xFFFFFFFF
    d = d - (1 << 32) if d >= 1 << 31 else d
    return -((-d) // 2) if d < 0 else d // 2


def check_plan(snap, table, pos, stats=None):
    """Every check of the module on one snapshot.  stats (optional dict) receives the counted
    situations (reload_at_gap: exactly scr_gap entries behind the row's store; reload_at_list_gap:
    behind the list's last store to any row; pads, kst_hit_without_difference, third_bucket_cuts,
    multi_pass_parents, chained_parent_first_in_tile, king_child_in_other_list), the entry counts, and
    every scratch load (block, list, entry, row, the entry of the row's latest store in the list or
    None, the entry of the list's latest store) and store (block, list, entry, row, the list's first
    store to the row)."""
    h, out = snap.hdr, []
    st = dict(reload_at_gap=0, reload_at_list_gap=0, pads=0, kst_hit_without_difference=0, third_bucket_cuts=0, multi_pass_parents=0,
              chained_parent_first_in_tile=0, king_child_in_other_list=0, zero_row_entries=0, moving_entries=0,
              parent_stores=0, unevaluated_parent_refreshes=0, entries=0, evaluated_slots=0, loads=[], stores=[])
    add = lambda name, where, detail="": out.append(Finding(name, where, detail))
    np_, K, nblk, L1, RS = h["np"], h["k"], h["nblk"], h["l1"], h["row_stride"]
    GAP, SPARE, xu, hu = h["scr_gap"], h["ent_spare"], h["xu"], h["hu"]
    off = snap.offsets.astype(np.int64)
    lo_all = (snap.ent & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hi_all = (snap.ent >> np.uint64(32)).astype(np.int64)
    zeros = np.zeros(L1, dtype=np.uint16)
    prev_rend = skipped = 0
    for blk in range(nblk):
        pbeg, pend = blk * K, min(blk * K + K, np_)
        rbeg, rend = snap.region(blk)
        if rbeg < prev_rend or rend > len(snap.ent) or rend < rbeg:
            add(F_REGIONS, f"block {blk}", f"[{rbeg}, {rend}) after {prev_rend} of {len(snap.ent)}")
            skipped += 1
            continue
        prev_rend = rend
        slots = (pend - pbeg) + int(off[pend] - off[pbeg])
        nt, base = int(snap.btiles[blk]), snap.tile_base(blk)
        next_base = snap.tile_base(blk + 1) if blk + 1 < nblk else len(snap.tiles)
        if nt > (slots + 15) // 16 + (pend - pbeg) or base + nt > next_base or base + nt > len(snap.tiles):
            add(F_BTILES, f"block {blk}", f"{nt} tiles for {slots} slots of {pend - pbeg} parents, base {base}, next {next_base}")
            skipped += 1
            continue
        T = snap.tiles[base:base + nt]
        us = (np.arange(pbeg, pend + 1) - pbeg) + (off[pbeg:pend + 1] - off[pbeg])  # each parent's first slot
        for p in range(pbeg, pend):
            st["multi_pass_parents"] += int(1 + off[p + 1] - off[p] > 64)
        # ---- the tiles: slot ranges, list segments
        firsts = [int(t["first"]) for t in T] + [slots]
        ok = nt > 0 and firsts[0] == 0
        for k in range(nt):
            where = f"block {blk} tile {k}"
            cnt = firsts[k + 1] - firsts[k]
            if cnt < 1 or cnt > 16:
                add(F_TILE_SLOTS, where, f"{cnt} slots")
                ok = ok and cnt >= 1
            if ok:
                own = pbeg + int(np.searchsorted(us, firsts[k], side="right")) - 1
                if int(T[k]["p_first"]) != own:
                    add(F_SLOT_MAP, where, f"p_first {int(T[k]['p_first'])}, slot {firsts[k]} belongs to parent {own}")
                    ok = False
        if nt == 0 and slots:
            add(F_SLOT_MAP, f"block {blk}", "no tiles")
        if not ok:
            if nt:
                add(F_SLOT_MAP, f"block {blk}", f"tile firsts {firsts}")
            skipped += 1
            continue
        e_end = np.zeros((nt + 1, 2), dtype=np.int64)
        for k in range(nt):
            e_end[k + 1] = T[k]["e_end"]
        if (np.diff(e_end, axis=0) < 0).any():
            add(F_E_END, f"block {blk}", str(e_end[1:].tolist()))
            skipped += 1
            continue
        len0, len1 = int(e_end[nt, 0]), int(e_end[nt, 1])
        if len0 + len1 > (rend - rbeg) - SPARE:
            add(F_REGION, f"block {blk}", f"{len0} + {len1} entries in a region of {rend - rbeg} less {SPARE}")
            skipped += 1
            continue
        # ---- slot -> position, the descriptors' fields
        slot_q = {}      # (tile, t) -> output index
        slot_par = {}    # (tile, t) -> (parent, processing position q: 0 the parent)
        for k in range(nt):
            cnt = min(firsts[k + 1] - firsts[k], 16)
            buckets = set()
            for t in range(cnt):
                u = firsts[k] + t
                p = pbeg + int(np.searchsorted(us, u, side="right")) - 1
                qq = u - int(us[p - pbeg])
                m = int(T[k]["meta"][t])
                where = f"block {blk} tile {k} slot {t} (parent {p} + {qq})"
                if qq == 0:
                    q = p
                else:
                    c = qq - 1 + int(T[k]["adj"][t])
                    if not 0 <= c < off[p + 1] - off[p]:
                        add(F_SLOT_MAP, where, f"adj {int(T[k]['adj'][t])}: child {c} of {int(off[p + 1] - off[p])}")
                        continue
                    q = np_ + int(off[p]) + c
                slot_q[(k, t)], slot_par[(k, t)] = q, (p, qq)
                if bool(m & META_PARENT) != (qq == 0):
                    add(F_META_PARENT, where, f"meta {m:#x}")
                ev = bool(m & META_EVAL)
                if ev:
                    st["evaluated_slots"] += 1
                    b = (m >> 1) & 7
                    buckets.add(b)
                    if b != (int(pos.pieces[q]) - 1) // 4:
                        add(F_META_BUCKET, where, f"bucket {b}, {int(pos.pieces[q])} pieces")
                    if (m >> 5) & 1 != int(pos.stm[q]):
                        add(F_META_SIDE, where, f"meta {m:#x}, side to move {int(pos.stm[q])}")
                    if not pos.evaluated[q]:
                        add(F_META_EVAL, where, "evaluated, but the big net does not evaluate the position")
                    b = (int(pos.pieces[q]) - 1) // 4
                    for side in range(2):
                        if int(T[k]["psq"][t][side]) != int(pos.psqt[q, int(pos.stm[q]) ^ side, b]):
                            add(F_PSQT, where, f"side {side}: {int(T[k]['psq'][t][side])}, oracle {int(pos.psqt[q, int(pos.stm[q]) ^ side, b])}")
                elif pos.evaluated[q] and qq != 0:
                    add(F_META_EVAL, where, "not evaluated, but the big net evaluates the position")
            if len(buckets) > 2:
                add(F_TILE_BUCKETS, f"block {blk} tile {k}", f"buckets {sorted(buckets)}")
            if k + 1 < nt and firsts[k + 1] - firsts[k] < 16 and len(buckets) == 2:
                m = int(T[k + 1]["meta"][0])
                st["third_bucket_cuts"] += int(bool(m & META_EVAL) and ((m >> 1) & 7) not in buckets)
        # ---- replay the two lists
        scratch = {}                  # scratch row -> (value, poisoned)
        touched = {}                  # scratch row -> set of lists
        stored_by = {}                # scratch row -> set of lists that stored it
        emits = {}                    # (tile, t, side) -> [count, list, index, PAR_E]
        loads = []                    # (list, index, row, same-list store index or None, last store any row)
        for g in range(2):
            acc, pacc, base = zeros.copy(), zeros.copy(), zeros.copy()
            bad = {"acc": False, "pacc": False, "base": False}
            last_store, last_any = {}, None
            idx = (rbeg + np.arange(e_end[nt, g])) if g == 0 else (rend - 1 - np.arange(e_end[nt, g]))
            los, his = lo_all[idx], hi_all[idx]
            k = 0
            for i in range(len(idx)):
                while i >= e_end[k + 1, g]:
                    k += 1
                lo, hi = int(los[i]), int(his[i])
                where = f"block {blk} list {g} entry {i} (tile {k})"
                st["entries"] += 1
                m, kind = hi & 0xFFFF, (hi >> 16) & 3
                if m not in (0, 1, 0xFFFF) or bool(hi & H_X) != bool(hi & (H_PAR_E | H_KST)):
                    add(F_ENTRY, where, f"hi {hi:#x}")
                roff = lo & 0x7FFFFFFF & ~L_KT
                r, rem = divmod(roff, RS)
                poisoned = False
                if rem:
                    add(F_ENTRY, where, f"lo {lo:#x} is no row offset")
                    row = zeros
                elif lo & L_SCR:
                    r -= h["ft_rows"]
                    if not 2 <= r < h["scr_rows"]:
                        add(F_ENTRY, where, f"scratch row {r}")
                        row = zeros
                    else:
                        touched.setdefault(r, set()).add(g)
                        j = last_store.get(r)
                        loads.append((g, i, r, j, last_any, where))
                        st["loads"].append((blk, g, i, r, j, last_any))
                        row, poisoned = scratch.get((g, r), (zeros, True))
                elif r == h["zero_row"]:
                    add(F_ZERO_ROW, where, f"hi {hi:#x}")
                    st["zero_row_entries"] += 1
                    row = zeros
                elif r >= h["ft_rows"]:
                    add(F_ENTRY, where, f"row {r}")
                    row = zeros
                else:
                    row = table[r]
                if m == 0:
                    st["pads"] += 1
                    if (r != h["ft_bias_row"] or lo & L_SCR) and r != h["zero_row"]:
                        add(F_NOOP_ROW, where, f"row {r}")
                elif r != h["zero_row"] or lo & L_SCR:
                    st["moving_entries"] += 1
                src, sbad = ((acc, bad["acc"]), (zeros, False), (pacc, bad["pacc"]), (base, bad["base"]))[kind]
                if m == 1:
                    acc = src + row
                elif m == 0xFFFF:
                    acc = src - row
                else:
                    acc = src.copy()
                bad["acc"] = sbad or (poisoned and m != 0)
                if kind == SRC_PACC:
                    base, bad["base"] = acc, bad["acc"]
                if hi & H_KST and not hi & H_LAST:
                    add(F_KST_PLACE, where, f"hi {hi:#x}")
                if not hi & H_LAST:
                    continue
                par_e, kst = bool(hi & H_X and hi & H_PAR_E), bool(hi & H_X and hi & H_KST)
                if par_e:
                    pacc, bad["pacc"] = acc, bad["acc"]
                if kst:
                    sr = 2 + (lo & L_KT)
                    if sr >= h["scr_rows"]:
                        add(F_ENTRY, where, f"store to scratch row {sr}")
                    else:
                        scratch[(g, sr)] = (acc, bad["acc"])
                        st["stores"].append((blk, g, i, sr, sr not in last_store))
                        last_store[sr], last_any = i, i
                        touched.setdefault(sr, set()).add(g)
                        stored_by.setdefault(sr, set()).add(g)
                        if lo & L_SCR and r == sr and kind == SRC_ZERO:
                            st["kst_hit_without_difference"] += 1
                field = hi >> H_LDS_SH
                t, rest = divmod(field, xu)
                side = rest // hu if hu else 0
                if rest not in (0, hu) or t >= min(firsts[k + 1] - firsts[k], 16):
                    add(F_LAST, where, f"tile field {field}: slot {t} of {firsts[k + 1] - firsts[k]}, rest {rest}")
                    continue
                e = emits.setdefault((k, t, side), [0, g, i, par_e, kst])
                e[0] += 1
                if e[0] > 1:
                    continue
                q = slot_q.get((k, t))
                if q is None:
                    continue
                persp = int(pos.stm[q]) ^ side
                if persp != g and slot_par[(k, t)][1] != 0:
                    st["king_child_in_other_list"] += 1
                st["parent_stores"] += int(kst and slot_par[(k, t)][1] == 0)
                if not bad["acc"] and not np.array_equal(acc, pos.acc[q, persp]):
                    d = np.flatnonzero(acc != pos.acc[q, persp])
                    add(F_ACC, where, f"slot {t} side {side} (position {q}, perspective {persp}): {len(d)} columns differ, "
                                      f"first {int(d[0])}: {int(acc[d[0]])} != {int(pos.acc[q, persp][d[0]])}")
        # ---- the ordering rules
        for g, i, r, j, last_any, where in loads:
            if j is None:
                if not stored_by.get(r, set()) - {g}:  # (stored by the other list: the ownership finding below)
                    add(F_NOT_STORED, where, f"scratch row {r}")
                continue
            if i - j < GAP:
                add(F_GAP_ROW, where, f"scratch row {r} stored at entry {j}: distance {i - j} < {GAP}")
            elif i - last_any < GAP:
                add(F_GAP_LIST, where, f"the list's last scratch store at entry {last_any}: distance {i - last_any} < {GAP}")
            st["reload_at_gap"] += int(i - j == GAP)
            st["reload_at_list_gap"] += int(i - last_any == GAP)
        for r, lists in sorted(touched.items()):
            if len(lists) > 1:
                add(F_OWNER, f"block {blk} scratch row {r}", "touched by both lists")
        # ---- every slot's LAST entries, the chain
        for k in range(nt):
            for t in range(min(firsts[k + 1] - firsts[k], 16)):
                if (k, t) not in slot_par:
                    continue
                m = int(T[k]["meta"][t])
                p, qq = slot_par[(k, t)]
                where = f"block {blk} tile {k} slot {t} (parent {p} + {qq})"
                n = [emits.get((k, t, s), [0])[0] for s in range(2)]
                if m & META_EVAL:
                    if n != [1, 1]:
                        add(F_LAST, where, f"{n} last entries for sides 0, 1")
                elif qq != 0:
                    if n != [0, 0]:
                        add(F_UNEVAL, where, f"{n} last entries")
                elif n != [0, 0]:
                    # an unevaluated parent whose children are: a complete refresh into the parent accumulators
                    st["unevaluated_parent_refreshes"] += 1
                    if n != [1, 1] or not all(emits[(k, t, s)][3] for s in range(2)):
                        add(F_UNEVAL, where, f"{n} last entries, not a parent refresh")
                if qq == 0 and not m & META_EVAL and pos.evaluated[p] and n == [0, 0]:
                    # a chained parent: its predecessor's child that is its position carries its result
                    st["chained_parent_first_in_tile"] += int(t == 0)
                    out.extend(_check_chain(snap, pos, blk, p, pbeg, slot_par, slot_q, T, emits, firsts, nt))
    # ---- the counters (of the whole plan: compared when every block was walked)
    if skipped:
        pass
    elif st["pads"] != h["pads"]:
        add(F_STAT_PADS, "header", f"{h['pads']} counted by the plan, {st['pads']} entries with multiplier 0")
    if not skipped and st["zero_row_entries"] != h["zero_row_entries"]:
        add(F_STAT_ZERO, "header", f"{h['zero_row_entries']} counted by the plan, {st['zero_row_entries']} in the lists")
    # (the plan's row count: every row-moving entry, and one more row for each parent slot whose
    # refresh is stored to the king cache -- the store's own entry of earlier plans, still counted)
    if not skipped and st["moving_entries"] + st["parent_stores"] != h["rows"]:
        add(F_STAT_ROWS, "header", f"{h['rows']} counted by the plan, {st['moving_entries']} row-moving entries and "
                                   f"{st['parent_stores']} stores of a parent's refresh")
    out.extend(_check_pinfo(snap, pos))
    if stats is not None:
        stats.update(st)
    return out


def _check_chain(snap, pos, blk, p, pbeg, slot_par, slot_q, T, emits, firsts, nt):
    """Parent p's slot is not evaluated although the big net evaluates p: among its predecessor's
    children there is one marked META_NEXT_PARENT, which is p's position, ends in PAR_E in both
    lists and is the last evaluated of its siblings."""
    where = f"block {blk} chained parent {p}"
    if p == pbeg:
        return [Finding(F_CHAIN, where, "the block's first parent has no entries")]
    sib = sorted((key for key, (pp, qq) in slot_par.items() if pp == p - 1 and qq > 0), key=lambda kt: (kt[0], kt[1]))
    marked = [kt for kt in sib if int(T[kt[0]]["meta"][kt[1]]) & META_NEXT_PARENT]
    if len(marked) != 1:
        return [Finding(F_CHAIN, where, f"{len(marked)} children of parent {p - 1} marked as the next parent")]
    k, t = marked[0]
    q = slot_q[(k, t)]
    out = []
    evaluated = [kt for kt in sib if int(T[kt[0]]["meta"][kt[1]]) & META_EVAL]
    if not evaluated or evaluated[-1] != (k, t):
        out.append(Finding(F_CHAIN, where, "the marked child is not the last evaluated of its siblings"))
    if not all(emits.get((k, t, s), [0, 0, 0, False])[3] for s in range(2)):
        out.append(Finding(F_CHAIN, where, "the marked child does not end in PAR_E in both lists"))
    for s in range(2):
        e = emits.get((k, t, s))
        if e and e[1] != int(pos.stm[q]) ^ s:
            out.append(Finding(F_CHAIN, where, f"the marked child's perspective {int(pos.stm[q]) ^ s} ends in list {e[1]}"))
    if not (np.array_equal(pos.acc[q], pos.acc[p]) and np.array_equal(pos.psqt[q], pos.psqt[p]) and
            pos.stm[q] == pos.stm[p]):
        out.append(Finding(F_CHAIN, where, f"the marked child (position {q}) is not the parent's position"))
    if snap.hdr["slices"] == 3:  # the sliced stream's finish finds the child through pinfo
        y = int(snap.pinfo[p, 1])
        if y < 0 or not y & PINFO_ALIAS or snap.hdr["np"] + int(snap.offsets[p - 1]) + (y >> PINFO_NS_SH) != q:
            out.append(Finding(F_PINFO_ALIAS, f"position {p}", f"pinfo.y {y:#x} does not name the marked child (position {q})"))
    return out


def _check_pinfo(snap, pos):
    """The column-sliced stream's (PSQT term, bucket) pairs by output index."""
    h, out = snap.hdr, []
    if h["slices"] != 3:
        return out
    np_, K = h["np"], h["k"]
    pi = snap.pinfo
    ev = np.asarray(pos.evaluated, dtype=bool)
    for q in np.flatnonzero((pi[:, 1] >= 0) != ev):
        out.append(Finding(F_PINFO_EVAL, f"position {int(q)}", f"pinfo.y {int(pi[q, 1])}, evaluated {bool(ev[q])}"))
    for q in np.flatnonzero((pi[:, 1] >= 0) & ev):
        q, y = int(q), int(pi[q, 1])
        b, s = (int(pos.pieces[q]) - 1) // 4, int(pos.stm[q])
        if y & 7 != b:
            out.append(Finding(F_PINFO_BUCKET, f"position {q}", f"{y & 7}, {int(pos.pieces[q])} pieces"))
        want = psqt_term(pos.psqt[q, s, b], pos.psqt[q, s ^ 1, b])
        if int(pi[q, 0]) != want:
            out.append(Finding(F_PINFO_PSQT, f"position {q}", f"{int(pi[q, 0])}, oracle {want}"))
        if y & PINFO_ALIAS:
            c = y >> PINFO_NS_SH
            good = 0 < q < np_ and q % K != 0 and c < int(snap.offsets[q] - snap.offsets[q - 1])
            if good:
                a = np_ + int(snap.offsets[q - 1]) + c
                good = bool(ev[a]) and np.array_equal(pos.acc[a], pos.acc[q]) and pos.stm[a] == pos.stm[q]
            if not good:
                out.append(Finding(F_PINFO_ALIAS, f"position {q}", f"child {c} of parent {q - 1} is not its position"))
        elif y >> 3:
            out.append(Finding(F_PINFO_ALIAS, f"position {q}", f"pinfo.y {y:#x} without PINFO_ALIAS"))
    return out


def names(findings):
    return sorted({f.name for f in findings})
