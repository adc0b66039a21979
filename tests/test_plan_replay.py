"""plan_replay's own test: hand-written plans of a few entries over a toy table of four feature
rows and a bias row, 32 columns.  The expected accumulators are written out by hand; then one
mutation per check, each of which must produce its named finding and no other."""
import numpy as np
import pytest

import plan_replay as R

L1, RS = 32, 128
BIAS, ZERO_ROW, FT_ROWS, GAP, SPARE = 4, 200, 5, 4, 32
c = np.arange(L1, dtype=np.uint16)
# the doubled rows, chosen so that sums wrap: bias 60000 + c, rows 1 + c, 100 + 2 c, 1000 + 3 c, 7000 + 5 c
TABLE = np.stack([1 + c, 100 + 2 * c, 1000 + 3 * c, 7000 + 5 * c, 60000 + c]).astype(np.uint16)
R0, R1, R2, R3, B = TABLE
ADD, SUB, NOP = 1, 0xFFFF, 0
PLAIN, ZERO, PACC, BASE = 0, 1 << 16, 2 << 16, 3 << 16
LAST, PAR_E, KST = R.H_LAST, R.H_X | R.H_PAR_E, R.H_X | R.H_KST
XU, HU = 2, 1


def E(row, m, flags, slot, side, kt=0, scr=False):
    lo = (FT_ROWS + row if scr else row) * RS | (R.L_SCR if scr else 0) | kt
    return lo | (m | flags | (slot * XU + side * HU) << R.H_LDS_SH) << 32


# One block of two parents.  Slots: P0 (white to move), its children c0, c1, c2 (black to move), P1
# (black to move, no children).  Output indices: P0 0, P1 1, c0 2, c1 3, c2 4.
#   P0   refresh: perspective 0 = bias + R0 + R1, perspective 1 = bias + R2 + R3
#   c0   from the parent: 0: - R0 + R2; 1: - R2 + R0           (PACC; parent - from-row is the base)
#   c1   the same from-rows: 0: base + R3; 1: base + R1       (BASE)
#   c2   a white king move to square 5: 0 refreshed = bias + R3 + R2, stored to king-cache row 2 + 5;
#        1: - R3 + R0
#   P1   0: the king-cache row reloaded at exactly GAP entries behind its store (three no-op pads),
#        + R1; 1 refreshed = bias + R0 + R1
KROW = 2 + 5
LIST0 = [E(BIAS, ADD, ZERO | PAR_E, 0, 0), E(0, ADD, PAR_E, 0, 0), E(1, ADD, LAST | PAR_E, 0, 0),      # 0-2 P0
         E(0, SUB, PACC, 1, 1), E(2, ADD, LAST, 1, 1),                                                  # 3-4 c0
         E(3, ADD, BASE | LAST, 2, 1),                                                                  # 5 c1
         E(BIAS, ADD, ZERO, 3, 1), E(3, ADD, PLAIN, 3, 1), E(2, ADD, LAST | KST, 3, 1, kt=5),           # 6-8 c2
         E(BIAS, NOP, PLAIN, 0, 0), E(BIAS, NOP, PLAIN, 0, 0), E(BIAS, NOP, PLAIN, 0, 0),               # 9-11 pads
         E(KROW, ADD, ZERO | PAR_E, 4, 1, scr=True), E(1, ADD, LAST | PAR_E, 4, 1)]                     # 12-13 P1
LIST1 = [E(BIAS, ADD, ZERO | PAR_E, 0, 1), E(2, ADD, PAR_E, 0, 1), E(3, ADD, LAST | PAR_E, 0, 1),      # 0-2 P0
         E(2, SUB, PACC, 1, 0), E(0, ADD, LAST, 1, 0),                                                  # 3-4 c0
         E(1, ADD, BASE | LAST, 2, 0),                                                                  # 5 c1
         E(3, SUB, PACC, 3, 0), E(0, ADD, LAST, 3, 0),                                                  # 6-7 c2
         E(BIAS, ADD, ZERO | PAR_E, 4, 0), E(0, ADD, PAR_E, 4, 0), E(1, ADD, LAST | PAR_E, 4, 0)]       # 8-10 P1
STORE_AT, RELOAD_AT = 8, 12

# by hand, [position][perspective]
EXPECT = {0: (B + R0 + R1, B + R2 + R3),
          2: (B + R1 + R2, B + R3 + R0),
          3: (B + R1 + R3, B + R3 + R1),
          4: (B + R3 + R2, B + R2 + R0),
          1: (B + R3 + R2 + R1, B + R0 + R1)}


def test_expected_values_wrap():
    """The literal numbers of two of the sums above (mod 2^16): the toy table does wrap."""
    assert int(EXPECT[1][0][0]) == (60000 + 7000 + 1000 + 100) % 65536 == 2564
    assert int(EXPECT[1][0][31]) == (60031 + 7155 + 1093 + 162) % 65536 == 2905
    assert int(EXPECT[3][0][31]) == (60031 + 162 + 7155) % 65536 == 1812
    assert int(EXPECT[0][1][31]) == (60031 + 1093 + 7155) % 65536 == 2743
    assert int(EXPECT[0][0][0]) == 60101  # (and one that does not)


def make(list0=LIST0, list1=LIST1, offsets=(0, 3, 3), pieces=None, pads=3, zero_rows=0, eoff_end=30, acc_of=None):
    """(snapshot, positions) of the toy plan with the given lists."""
    np_, npos = 2, 2 + offsets[-1]
    stm = np.zeros(npos, np.uint8)
    stm[1:5] = 1  # P1 and the children of P0
    pcs = np.full(npos, 3, np.int32)
    for q, v in (pieces or {}).items():
        pcs[q] = v
    acc = np.zeros((npos, 2, L1), np.uint16)
    for q, (a, b) in {**EXPECT, **(acc_of or {})}.items():
        acc[q, 0], acc[q, 1] = a, b
    psqt = (1000 * np.arange(npos)[:, None, None] + 100 * np.arange(2)[None, :, None] - 7 * np.arange(8)[None, None, :]).astype(np.int32)
    ev = np.zeros(npos, bool)
    ev[:5] = True
    pos = R.Positions(stm, pcs, acc, psqt, ev)
    tile = np.zeros(1, R.TILE_DTYPE)
    tile["e_end"][0] = (len(list0), len(list1))
    for t, (q, parent) in enumerate(((0, 1), (2, 0), (3, 0), (4, 0), (1, 1))):
        b = (int(pcs[q]) - 1) // 4
        tile["meta"][0][t] = 1 | b << 1 | parent << 4 | int(stm[q]) << 5
        for side in range(2):
            tile["psq"][0][t][side] = psqt[q, int(stm[q]) ^ side, b]
    eoff = np.array([0, 20, eoff_end], np.uint64)
    ent = np.zeros(eoff_end + SPARE, np.uint64)
    ent[:len(list0)] = list0
    ent[len(ent) - len(list1):] = list1[::-1]
    hdr = dict(l1=L1, row_stride=RS, ft_rows=FT_ROWS, ft_bias_row=BIAS, zero_row=ZERO_ROW, scr_rows=130, ent_spare=SPARE,
               scr_gap=GAP, ring=4, slice_ring=4, np=np_, k=2, nblk=1, slices=1, xu=XU, hu=HU, kc=1, ordered=0,
               npos=npos, n_ent=len(ent), n_tiles=1, n_pinfo=0, pads=pads, zero_row_entries=zero_rows,
               rows=len(list0) + len(list1) - pads)
    snap = R.Snapshot(hdr, eoff, ent, tile, np.array([1], np.uint32), np.array([0], np.uint32), None,
                      np.array(offsets, np.uint64))
    return snap, pos


def check(snap, pos, stats=None):
    return R.check_plan(snap, TABLE, pos, stats)


def test_the_plan_replays_to_the_hand_written_accumulators():
    stats = {}
    assert check(*make(), stats) == []
    assert stats["reload_at_gap"] == 1 and stats["pads"] == 3 and stats["entries"] == 25
    assert stats["evaluated_slots"] == 5 and stats["king_child_in_other_list"] == 0


def test_wrong_reference_is_an_accumulator_finding():
    snap, pos = make()
    pos.acc[3, 1, 17] ^= 1
    f = check(snap, pos)
    assert R.names(f) == [R.F_ACC] and len(f) == 1 and "position 3, perspective 1" in f[0].detail


def set_flags(e, clear=0, setf=0, kt=None):
    lo, hi = e & 0xFFFFFFFF, e >> 32
    hi = (hi & ~clear) | setf
    if kt is not None:
        lo = (lo & ~R.L_KT) | kt
    return lo | hi << 32


def m_reload_closer():  # the reload one entry closer to its store
    l0 = LIST0[:9] + LIST0[10:]
    return make(list0=l0, pads=2)


def m_store_in_other_list():  # c2's store moved to its last entry in list 1
    l0, l1 = list(LIST0), list(LIST1)
    l0[STORE_AT] = set_flags(l0[STORE_AT], clear=KST, kt=0)
    l1[7] = set_flags(l1[7], setf=KST, kt=5)
    return make(list0=l0, list1=l1)


def m_multiplier_flipped():  # c0's added row subtracted
    l0 = list(LIST0)
    l0[4] = (l0[4] & ~(0xFFFF << 32)) | SUB << 32
    return make(list0=l0)


def m_last_dropped():  # c1's entry in list 0 no longer ends its slot
    l0 = list(LIST0)
    l0[5] = set_flags(l0[5], clear=LAST)
    return make(list0=l0)


def m_17_slots():  # P1 gets 12 children the big net does not evaluate: 17 slots in the one tile
    return make(offsets=(0, 3, 15))


def m_third_bucket():  # c0 with 7 pieces, c1 with 11: buckets 0, 1 and 2 in the tile
    return make(pieces={2: 7, 3: 11})


def m_zero_row():  # a pad on the all-zero row (the plan counted it)
    l0 = list(LIST0)
    l0[9] = E(ZERO_ROW, NOP, PLAIN, 0, 0)
    return make(list0=l0, zero_rows=1, pads=3)


def m_kst_without_last():  # the store flag on an entry that does not end its slot
    l0 = list(LIST0)
    l0[7] = set_flags(l0[7], setf=KST, kt=5)
    return make(list0=l0)


def m_load_never_stored():  # P1 reloads a king-cache row nobody stored
    l0 = list(LIST0)
    l0[RELOAD_AT] = E(KROW + 1, ADD, ZERO | PAR_E, 4, 1, scr=True)
    return make(list0=l0)


def m_second_store_closer():  # P1 reloads a row c1 stored long ago, 3 entries behind c2's store: the per-list rule alone
    l0 = LIST0[:9] + LIST0[10:]
    l0[5] = set_flags(l0[5], setf=KST, kt=9)
    l0[RELOAD_AT - 1] = E(2 + 9, ADD, ZERO | PAR_E, 4, 1, scr=True)
    return make(list0=l0, pads=2, acc_of={1: (B + R1 + R3 + R1, B + R0 + R1)})


def m_noop_off_the_bias_row():
    l0 = list(LIST0)
    l0[10] = E(2, NOP, PLAIN, 0, 0)
    return make(list0=l0)


def m_parent_flag_missing():
    snap, pos = make()
    snap.tiles["meta"][0][4] &= 0xFF ^ R.META_PARENT
    return snap, pos


def m_region_overflow():  # the region less its spare entries holds 24 of the 25 entries
    return make(eoff_end=24)


def m_pads_miscounted():
    return make(pads=2)


MUTATIONS = [(m_reload_closer, R.F_GAP_ROW), (m_store_in_other_list, R.F_OWNER), (m_multiplier_flipped, R.F_ACC),
             (m_last_dropped, R.F_LAST), (m_17_slots, R.F_TILE_SLOTS), (m_third_bucket, R.F_TILE_BUCKETS),
             (m_zero_row, R.F_ZERO_ROW), (m_kst_without_last, R.F_KST_PLACE), (m_load_never_stored, R.F_NOT_STORED),
             (m_second_store_closer, R.F_GAP_LIST), (m_noop_off_the_bias_row, R.F_NOOP_ROW),
             (m_parent_flag_missing, R.F_META_PARENT), (m_region_overflow, R.F_REGION)]


@pytest.mark.parametrize("mutate,name", MUTATIONS, ids=[n for _, n in MUTATIONS])
def test_each_mutation_gives_its_finding_and_no_other(mutate, name):
    assert R.names(check(*mutate())) == [name]


def test_miscounted_pads_change_both_counters():
    """The toy header derives the row count from the pad count, so one wrong count shows in both."""
    assert R.names(check(*m_pads_miscounted())) == sorted([R.F_STAT_PADS, R.F_STAT_ROWS])


def test_chained_parent():
    """P1 as a chained parent: no entries of its own, its position is c2 (the marked child, evaluated
    last, ending in PAR_E in the list of each perspective)."""
    def chained():
        l0 = LIST0[:8] + [set_flags(LIST0[8], setf=PAR_E)]
        l1 = LIST1[:7] + [set_flags(LIST1[7], setf=PAR_E)]
        snap, pos = make(list0=l0, list1=l1, pads=0)
        snap.tiles["meta"][0][3] |= R.META_NEXT_PARENT
        snap.tiles["meta"][0][4] &= 0xFF ^ R.META_EVAL
        pos.acc[1], pos.psqt[1], pos.stm[1] = pos.acc[4], pos.psqt[4], pos.stm[4]
        return snap, pos
    stats = {}
    assert check(*chained(), stats) == []
    assert stats["chained_parent_first_in_tile"] == 0
    snap, pos = chained()
    snap.tiles["meta"][0][3] &= 0xFF ^ R.META_NEXT_PARENT
    assert R.names(check(snap, pos)) == [R.F_CHAIN]
    snap, pos = chained()
    snap.ent[8] = set_flags(int(snap.ent[8]), clear=R.H_PAR_E)  # (X stays: the entry still stores)
    assert R.names(check(snap, pos)) == [R.F_CHAIN]
    snap, pos = chained()
    pos.acc[1, 0, 3] += 1  # the parent is another position than the marked child
    assert R.names(check(snap, pos)) == [R.F_CHAIN]


def test_sliced_pinfo():
    """The column-sliced stream's pinfo: bucket, PSQT term, evaluated positions, PINFO_ALIAS."""
    def sliced():
        snap, pos = make()
        snap.hdr["slices"], snap.hdr["n_pinfo"] = 3, 5
        pi = np.zeros((5, 2), np.int32)
        for q in range(5):
            s = int(pos.stm[q])
            pi[q] = (R.psqt_term(pos.psqt[q, s, 0], pos.psqt[q, s ^ 1, 0]), 0)
        snap.pinfo = pi
        return snap, pos
    assert check(*sliced()) == []
    for field, value, name in ((1, 1, R.F_PINFO_BUCKET), (0, 12345, R.F_PINFO_PSQT), (1, -1, R.F_PINFO_EVAL),
                               (1, R.PINFO_ALIAS | 2 << R.PINFO_NS_SH, R.F_PINFO_ALIAS)):
        snap, pos = sliced()
        snap.pinfo[1, field] = value
        assert R.names(check(snap, pos)) == [name], name
    assert R.psqt_term(-7, 0) == -3 and R.psqt_term(7, 0) == 3 and R.psqt_term(-2 ** 31, 1) == (2 ** 31 - 1) // 2
