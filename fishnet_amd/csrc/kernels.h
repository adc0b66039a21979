// kernels.h — host-side launchers for the gfx950 kernels in kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nnue.h"

// Row-ring depth of the planned expansion's stream (stream.hip: entries in flight per wave,
// 4 or 8), and GN_SCR_GAP, the least distance in entries of one list from a king-cache store to
// a later load of that row (the plan pads the lists to keep it and asserts it: error bit 2).
// The store rides on its slot's last row entry (no entry of its own), so the distance counts
// from that entry.  The ring issues an entry's row loads while consuming the entry GN_RING
// before it, and the store happens while consuming its own entry, so at a distance >= GN_RING the load is issued
// after the store, by the same lanes, to the same address.  One work-item's later load of an
// address it stored needs no wait on this hardware: hipcc itself emits `global_store_dword`
// directly followed by `global_load_dword` for C++ `p[i] = x; y = p[i ^ j];`
// (tests/test_host.py::test_same_address_store_then_load_needs_no_wait compiles exactly that
// and checks), i.e. one wave's vector-memory operations reach one address in issue order.
// -DGN_SCR_GAP=7 (2 * GN_RING - 1) is the stricter variant: the ring's vmcnt(2 * GN_RING - 2)
// waits then retire the store before the load issues (vmcnt counts loads and stores together
// in issue order, MI355X_MICROARCH.md "s_waitcnt vmcnt(N)"); measured 2.9 % slower stream.
#ifndef GN_RING
#define GN_RING 4
#endif
// the column-sliced stream's ring (stream_eval_kernel<3072, 3>): 4, 5 or 6 entries per wave
#ifndef GN_SLICE_RING
#define GN_SLICE_RING 4
#endif
#ifndef GN_SCR_GAP // (the plan serves both streams: the deeper ring's distance)
#define GN_SCR_GAP (GN_RING > GN_SLICE_RING ? GN_RING : GN_SLICE_RING)
#endif
// Workgroup size of the expansion's front kernels (count_children, child_moves, child_boards,
// block_keys, plan_kernel).  The expansion pipeline runs them beside the row stream, whose
// 2-wave workgroups hold every wave slot of a CU: a front workgroup is dispatched only where
// enough stream workgroups have ended at once.  2 waves (128): per step 150.8 against 151.9 ms
// with 4 (256) and 153.0 with 1 (64), which runs the front fully beside the stream and slows
// the stream by as much (round 6, profiles/r06/ab_r06p_front_wg.log).
#ifndef GN_FRONT_WG
#define GN_FRONT_WG 128
#endif
static_assert(GN_FRONT_WG == 64 || GN_FRONT_WG == 128 || GN_FRONT_WG == 256, "front workgroups of 1, 2 or 4 waves");

// Spare entries at the end of each block's entry region (plan_kernel, stream_eval_kernel): the
// stream's scalar prefetch of the entries two ring revolutions ahead reads up to 2 * ring + 8 - 1
// entries past its position, so a list ending at the region less the spares never reads past it.
constexpr unsigned ENT_SPARE = 32;

// The column-sliced stream's fc_0 partial sums: one array per slice (default), which
// finalize_kernel adds; or, with -DGN_PART_INPLACE (A/B only), one array that each slice
// s > 0 adds its sums to in place, reading slice s - 1's at the tile's start.  In place measured
// slower (round 5: finish 5.44 -> 2.75 ms, but each later stream launch +2.1 ms: the prefetch
// misses to HBM and, vector-memory completion being in order, holds up the ring's next loads).
// GN_PART_SLICES: the arrays launch_plan_stream's part holds.
// A position's record in a slice's array (GN_PART_DWORDS dwords): its 16 sums as unsigned 24-bit
// numbers, 48 B.  A slice's sum over its 1,024 activations (each in [0, 127], transform8) with int8
// weights lies in [127 N, 127 P], N / P the sums of the row's negative / positive weights, a span
// of 127 sum|w| <= 127 * 128 * 1024 < 2^24: stored as sum + part_off, part_off = -127 N
// (NetDevice), it never needs more, for any net.  Lane wj of the writer packs outputs 4 wj ..
// 4 wj + 3 into dwords 3 wj .. 3 wj + 2 (pack24x4 / unpack24x4, device_util.h); finalize adds the
// slices' values and b0p = b0 - the three offsets: the int32 sum of before, bit for bit.  The
// in-place array keeps int32 sums (its running totals over the slices exceed 24 bits).
#ifdef GN_PART_INPLACE
#define GN_PART_SLICES 1
#define GN_PART_DWORDS 16
#else
#define GN_PART_SLICES 3
#define GN_PART_DWORDS 12
#endif

namespace gn {

// NetworkOutput {psqt / 16, positional / 16} for every position whose
// need[i] != 0 (need == nullptr: all); other entries of out are untouched.
// perm (optional): slot q evaluates boards[perm[q]] and writes out[perm[q]].
// swz: XCD-aware tile order (each XCD gets a contiguous range of tiles).
// rows_out (optional): += FT rows the gather reads (common-row base counted once per tile).
// cls (the small net, mode FULL): the kernel selects the positions itself (classify_kernel's rule:
// need_small / need_big written for every position, need ignored) and applies reeval_kernel's rule to
// the small net's outputs (need_big set where |nnue| < reeval_threshold): one launch for three.
hipError_t launch_eval_net(const NetDevice &net, const gn_board *boards, const uint8_t *need, size_t n,
                           int2 *out, const uint32_t *perm, int swz, hipStream_t s,
                           unsigned long long *rows_out = nullptr, const gn_eval_params *cls = nullptr,
                           uint8_t *need_small = nullptr, uint8_t *need_big = nullptr);
// *out += position-sensitive checksum of bytes at p (caller zeroes *out)
hipError_t launch_checksum(const void *p, size_t bytes, unsigned long long *out, hipStream_t s);
// permutation of [0, n) ordering positions by (white king, black king) square, then
// (placement) by 30 home-square bits, one per square of ranks 1, 2, 7, 8 without
// e1 / e8, set when the start position's piece still stands there
// (king_keys_kernel), which serve the big net's common-row base; kings only
// (16-bit keys) otherwise
// order[]: the nblk blocks (K consecutive parents each) sorted by their middle parent's
// king squares (stream_eval_kernel's XCD-local order); keys / idx / keys_out: nblk scratch.
hipError_t block_order(const gn_board *parents, size_t n, uint32_t K, uint32_t nblk, uint16_t *keys, uint32_t *idx,
                       uint16_t *keys_out, uint32_t *order, void *&temp, size_t &temp_bytes, hipStream_t s);
hipError_t king_sort(const gn_board *boards, size_t n, uint64_t *keys, uint32_t *idx, uint64_t *keys_out,
                     uint32_t *perm, bool placement, void *&temp, size_t &temp_bytes, hipStream_t s);
// Incremental evaluation of parents + all their children with the small net (L1 = 128;
// expand_eval_kernel, one workgroup per parent; children of parent p are
// [offsets[p], offsets[p+1]) with deltas[]); need_* select what this net evaluates
// (nullptr: all).  The big nets always run planned (launch_plan_stream).
hipError_t launch_expand_net(const NetDevice &net, const gn_board *parents, size_t n, const uint64_t *offsets,
                             const gn_board *children, const ChildDelta *deltas, const uint8_t *need_parent,
                             const uint8_t *need_child, int2 *out_parent, int2 *out_child, int swz, hipStream_t s);
// Planned expansion (stream.hip): one descriptor per tile of <= 16 consecutive slots of a
// block (slots = [parent, its children, next parent, ...] of the block's consecutive
// parents) with <= 2 buckets among its evaluated slots.  e_end: list 0 / list 1 entries
// of the block up to the end of this tile (any length: the lists are not padded at a tile's end
// since the stream's ring runs across tiles); p_first: the
// parent owning slot 0; first: the block-relative index of slot 0; meta[t]: bit 0
// evaluated (clear for a chained parent: it has no entries, its result is that of the child
// that is its position; also clear for a parent the big net does not evaluate, which keeps its refresh
// entries, LAST | PAR_E, whenever one of its children is evaluated: they start from it -- no other
// unevaluated slot has entries), bits 1-3 bucket, bit 4 a parent slot, bit 5 the slot's side to move,
// bit 6 (META_NEXT_PARENT) a child that is the next parent's position and whose result is that
// parent's too (the whole-row streams store it to both; the sliced stream's finish: PINFO_ALIAS);
// psq[t][side]: the slot's PSQT accumulators at its bucket (side 0: the perspective to move).
constexpr uint32_t META_NEXT_PARENT = 1u << 6; // (TileDesc.meta)
// pinfo[position].y of the column-sliced stream: < 0 not evaluated by the big net; else bits 0-2 the
// bucket, and for a chained parent (its slot is not evaluated) PINFO_ALIAS and from PINFO_NS_SH the
// child c of its predecessor P - 1 that is its position: its fc_0 sums are those of output index
// np + offsets[P - 1] + c (relative, so that no batch size is too large for the field)
constexpr int PINFO_ALIAS = 1 << 3, PINFO_NS_SH = 4;
struct TileDesc {
  uint32_t e_end[2];
  uint32_t p_first;
  uint32_t first;
  uint8_t meta[16];
  int32_t psq[16][2];
  int16_t adj[16]; // a child slot's output index minus its position (the chained walk's reorder)
};
static_assert(sizeof(TileDesc) == 192, "TileDesc is 192 bytes");
// Tiles of a block start at tiles + (pbeg + offsets[pbeg]) / 16 + (K + 2) * block (btiles[block]
// of them), entries at ent + eoff[pbeg] + ENT_SPARE * block (list 0 upward, list 1 downward from
// the region's end, eoff = exclusive scan of write_children's per-parent entry bounds).
// One call plans and / or evaluates every block of the n parents.
// phases: PLAN_PHASE (the pinfo reset and plan_kernel) and / or STREAM_PHASE (the stream
// launches), so that an expansion's plan can run on another stream than its row stream (the
// expansion pipeline, gpu_nnue.hip): the two calls take the same PlanStreamArgs, and differ in
// phases and swz.
constexpr int PLAN_PHASE = 1, STREAM_PHASE = 2;
struct PlanStreamArgs {
  const gn_board *parents = nullptr;
  size_t n = 0;
  const uint64_t *offsets = nullptr; // the parents' child offsets (n + 1)
  const ChildDelta *deltas = nullptr;
  const uint8_t *need_parent = nullptr, *need_child = nullptr; // what this net evaluates (nullptr: all)
  int2 *out_parent = nullptr, *out_child = nullptr;
  const uint8_t *next_slot = nullptr; // the chained walk's links (chain_k > 1) ...
  int chain_k = 1;                    // ... and its block length
  int kc = 0;                         // king cache on
  const uint64_t *eoff = nullptr;
  uint64_t *ent = nullptr;
  TileDesc *tiles = nullptr;
  uint32_t *btiles = nullptr;
  // 88 words (scratch-slot bits, then 8 block claim counters per stream launch), zeroed by the
  // caller before each STREAM_PHASE call
  uint32_t *pool = nullptr;
  // bit 0 entry overflow, bit 1 no scratch slot, bit 2 a king-cache load closer than GN_SCR_GAP
  // entries to its list's last store to scratch
  uint32_t *err = nullptr;
  // += FT rows the stream gathers: every entry with a multiplier (bias and king-cache loads included),
  // and one more for each parent slot whose refresh is stored to the king cache (a child's store is
  // not counted; tests/plan_replay.py holds the plan to exactly this)
  unsigned long long *rows_out = nullptr;
  // (optional, 2 words) [0] += no-op entries the plan inserted to keep GN_SCR_GAP, [1] += entries put on
  // the zero row (they move no row and add nothing)
  unsigned long long *pads_out = nullptr;
  const uint32_t *order = nullptr;        // block order of the stream (block_order) or NULL
  // slices == 3 (L1 3072; part, pinfo non-null): the stream runs as three launches over 1,024
  // columns each (stream_eval_kernel<3072, 3>); part = GN_PART_SLICES x npos x GN_PART_DWORDS
  // dwords of fc_0 partial sums, pinfo = npos (PSQT value, bucket) pairs (the plan writes every one:
  // (0, -1) for a position the big net does not evaluate), npos = n + the
  // children; out_parent / out_child stay unwritten: the caller's launch_finalize takes the big
  // net's outputs from part and pinfo itself (SlicedOut).  Otherwise one launch over whole rows
  int slices = 1;
  int32_t *part = nullptr;
  size_t npos = 0;
  int2 *pinfo = nullptr;
  int swz = 0;
};
hipError_t launch_plan_stream(const NetDevice &net, const PlanStreamArgs &a, int phases, hipStream_t s);
// What launch_plan_stream derives from its arguments and hands to plan_kernel: the block length and
// count, whether the king cache runs (chained blocks only), whether the stream is column-sliced, and
// the units of an entry's tile field (stream.hip: hi[31:22] = slot * xu + side * hu).  nblk == 0: the
// net has no planned kernels (L1 other than 3072 / 1024) or there are no parents.
struct PlanGeometry {
  uint32_t K = 1, nblk = 0;
  int kc = 0;
  bool sliced = false;
  uint32_t xu = 0, hu = 0;
};
PlanGeometry plan_geometry(const NetDevice &net, const PlanStreamArgs &a);
// GN_MODE_FULL preparation: need_small = valid && |simple_eval| > threshold,
// need_big = valid && !need_small.
hipError_t launch_classify(const gn_board *boards, size_t n, const gn_eval_params &P, uint8_t *need_small,
                           uint8_t *need_big, hipStream_t s);
// GN_MODE_FULL: marks need_big where the small net's |nnue| < reeval_threshold.
hipError_t launch_reeval(const int2 *out_small, const uint8_t *need_small, size_t n, const gn_eval_params &P,
                         uint8_t *need_big, hipStream_t s);
// Eval::evaluate epilogue -> gn_eval (flags incl. IN_CHECK / BAD_FEN).
// score: 0 child records (GN_FLAG_NO_SCORE); 1 positions: the score rule's static part
// (mate 0 / cp 0 without a legal move, from counts[i] when given, else found here; final_cp
// otherwise, which resolve_scores replaces for the in-check ones).
// owner / moves / unpacked (optional, children only): board i is unpacked[owner[i]] after
// moves[i] (the parents write_children unpacked), instead of unpacking boards[i].
// sliced (optional): the column-sliced stream's partial sums of the big net; position i's big-net
// output is then slice_finish_from its slice_sums and pinfo[qoff + i] (out_big[i] where pinfo.y < 0)
struct SlicedOut {
  const NetDevice *net;
  const int32_t *part;
  const int2 *pinfo;
  uint64_t npos, qoff;
  const uint64_t *offsets = nullptr; // the parents' launch (qoff 0): their child offsets, for PINFO_ALIAS
};
hipError_t launch_finalize(const gn_board *boards, size_t n, int mode, const int2 *out_small,
                           const int2 *out_big, const uint8_t *need_small, const uint8_t *need_big,
                           const gn_eval_params &P, const Tables *tables, gn_eval *out, hipStream_t s,
                           int score, const uint64_t *counts = nullptr, const uint32_t *owner = nullptr,
                           const uint16_t *moves = nullptr, const Board *unpacked = nullptr,
                           const SlicedOut *sliced = nullptr);
// The score rule's in-check positions (include/gpu_nnue.h gn_eval.score): select (sel[n + 1],
// 1 for a scored position in check with a legal move), gather (idx / boards of the selected,
// pos = exclusive scan of sel), reduce (max over each selected position's replies
// [off[j], off[j + 1]) of moves / records ce, csv = the replies' own rule values where
// GN_FLAG_SEARCHED; writes score / flags / best_move of out[idx[j]] and sv[idx[j]] if sv).
hipError_t launch_score_select(const gn_eval *out, size_t n, uint64_t *sel, hipStream_t s);
hipError_t launch_score_gather(const gn_board *boards, const uint64_t *sel, const uint64_t *pos, size_t n,
                               const Tables *tables, uint32_t *idx, gn_board *sb, hipStream_t s);
// Replies already evaluated by an expansion (records rec / moves at [off[i], off[i + 1]) of
// parent i, the parents unpacked by write_children): compact offsets coff (m + 1, scan of
// counts; *total_host = coff[m], synchronous), then (_fill) ce / cb / cm = the selected
// parents' replies as positions of the rule (records with their static score part, boards,
// moves).
hipError_t launch_score_replies(const uint32_t *idx, size_t m, const uint64_t *off, uint64_t *counts,
                                uint64_t *coff, void *&temp, size_t &temp_bytes, uint64_t *total_host, hipStream_t s);
hipError_t launch_score_replies_fill(const uint32_t *idx, size_t m, const uint64_t *off, const uint64_t *coff,
                                     const gn_eval *rec, const uint16_t *moves, const Board *unpacked,
                                     const Tables *tables, gn_eval *ce, gn_board *cb, uint16_t *cm, hipStream_t s);
// (idx NULL: position j is sb[j] / out[j], and positions without replies are skipped)
hipError_t launch_score_reduce(const gn_board *sb, size_t m, const uint32_t *idx, const uint64_t *off,
                               const uint16_t *moves, const gn_eval *ce, const int32_t *csv, const gn_eval_params &P,
                               gn_eval *out, int32_t *sv, hipStream_t s);
// The small-batch graph's two reductions in one workgroup (idx NULL for both): level 1's positions
// sb1 [0, m1) from their replies (moves2 / ce2 / csv2 at off1) into out1 / sv1, then level 0's sb0
// [0, m0) from level 1's records and values (moves1 at off0) into out0.
hipError_t launch_score_reduce2(const gn_board *sb1, size_t m1, const uint64_t *off1, const uint16_t *moves2,
                                const gn_eval *ce2, const int32_t *csv2, gn_eval *out1, int32_t *sv1,
                                const gn_board *sb0, size_t m0, const uint64_t *off0, const uint16_t *moves1,
                                const gn_eval_params &P, gn_eval *out0, hipStream_t s);
// One level of the score rule's replies for a small batch in one launch (reply_level_kernel,
// kernels.hip): n <= 16,384 positions, selected from their boards (valid, in check, a legal move);
// replies into rb / rm [0, cap) (empty boards after the last), off = n + 1 offsets; *flag set
// (first) / or'd when the replies exceed cap.
hipError_t launch_reply_level(const gn_board *boards, size_t n, const Tables *tables, uint64_t *off, size_t cap,
                              gn_board *rb, uint16_t *rm, uint32_t *flag, int first, hipStream_t s);
// legal-move counts per board (invalid boards: 0); ebound (optional): per parent an
// upper bound of the planned expansion's list entries (stream.hip).  The boards pass the gate
// (chess.h unpack) unless trusted: the library's own boards (a legal child of a valid parent).
hipError_t launch_count_children(const gn_board *boards, size_t n, const Tables *tables, uint64_t *counts,
                                 hipStream_t s, uint64_t *ebound = nullptr, bool trusted = false);
// children of every board at offsets[i] (exclusive prefix sums of counts): their moves,
// owning board (owner, scratch) and, for children [c0, c0 + nc) (all children of these
// boards), the child boards, deltas and chained-walk links.  moves / owner: required.
// unpacked (optional, n entries): the boards unpacked once by the per-board pass, so that the
// per-child pass reads its parent instead of unpacking it again.  Without it the per-child pass
// reads boards as they are: they must be canonical (trusted, or stored by score_gather_kernel).
hipError_t launch_write_children(const gn_board *boards, size_t n, const Tables *tables, const uint64_t *offsets,
                                 size_t c0, size_t nc, gn_board *children, uint16_t *moves, uint32_t *owner,
                                 ChildDelta *deltas, uint8_t *next_slot, int chain_k, unsigned long long *rows,
                                 hipStream_t s, Board *unpacked = nullptr, bool trusted = false);
// sum of legal-move counts over all boards into *total (added; caller zeroes)
hipError_t launch_count_sum(const gn_board *boards, size_t n, const Tables *tables,
                            unsigned long long *total, hipStream_t s);
// random playouts (chess.h random_playout), one thread per position
hipError_t launch_random_positions(uint64_t seed, size_t first, size_t n, int max_plies, const Tables *tables,
                                   gn_board *out, hipStream_t s);
// random games: out[g * (plies + 1) + k] = position after k plies of game g
hipError_t launch_random_games(uint64_t seed, size_t first_game, size_t n_games, int plies, const Tables *tables,
                               gn_board *out, hipStream_t s);
// lichess batches replayed on the GPU: game g's move codes codes[moff[g], moff[g + 1]) from
// roots[g]; positions at boards[moff[g] + g + k], resolved moves at smoves[moff[g] + k - 1],
// status[g] = 0 or the 1-based index of the first illegal move (replay_games_kernel)
hipError_t launch_replay_games(const gn_board *roots, size_t ng, const uint64_t *moff, const uint16_t *codes,
                               const Tables *tables, gn_board *boards, uint16_t *smoves, int32_t *status, hipStream_t s);
// dst[i] = src[idx[i]]
hipError_t launch_gather_boards(const gn_board *src, const uint32_t *idx, size_t n, gn_board *dst, hipStream_t s);
// gn_eval -> gn_child (ABI v4 child records for the host-buffer calls)
hipError_t launch_pack_children(const gn_eval *in, size_t n, gn_child *out, hipStream_t s);
// Ranked lines (include/gpu_nnue.h gn_line): lines[i * K + k] = line k + 1 of parent i, from its
// children [offsets[i], offsets[i + 1]) (moves, records rec of one expansion), 1 <= K <= GN_MAX_LINES.
// The parents as write_children unpacked them with the pipeline's 64-bit offsets (an entry is
// read only where the parent has children), or packed with the C-ABI's 32-bit offsets.
// With history (include/gpu_nnue.h at gn_history) the game-history draws are applied: hist[i] names
// parent i's game so far in keys[0, n_keys) (position_key of each position).  NULL: the plain ranking.
// With ext (include/gpu_nnue.h, the check-extended calls): ext[c] is child c's check extension, or
// GN_NOT_EXTENDED where it keeps its static value.  NULL: no extension, today's kernels.
// ahead (rank_lines2_kernel alone; 0 or 1): the plies parent i lies after keys[hist[i].self].  1 is the
// three-ply chain, whose parents are the children of a game's position (include/gpu_nnue.h at
// gn_line3, "game history"); every other ranking kernel ignores it.
struct RankHistory {
  const uint64_t *keys;
  size_t n_keys;
  const gn_history *hist;
  uint32_t ahead = 0;
};
hipError_t launch_rank_children(const Board *unpacked, size_t n, const uint64_t *offsets, const uint16_t *moves,
                                const gn_eval *rec, const gn_eval_params &P, const Tables *tables, int K,
                                gn_line *lines, const RankHistory *history, const int32_t *ext, hipStream_t s);
hipError_t launch_rank_children(const gn_board *parents, size_t n, const uint32_t *offsets, const uint16_t *moves,
                                const gn_eval *rec, const gn_eval_params &P, const Tables *tables, int K,
                                gn_line *lines, const RankHistory *history, const int32_t *ext, hipStream_t s);
// keys[i] = position_key of boards[i], a lane per board.  gate: a caller's boards (unpack; a
// rejected board's key is 0); else the library's own canonical boards (unpack_fields)
hipError_t launch_position_keys(const gn_board *boards, size_t n, bool gate, const Tables *tables, uint64_t *keys,
                                hipStream_t s);
// Two-ply ranked lines (include/gpu_nnue.h gn_line2): lines[i * K + k] = line k + 1 of parent i, from
// a depth-2 expansion's outputs: the children [offsets[i], offsets[i + 1]) (boards, records rec,
// moves) and each child c's grandchildren [goffsets[c], goffsets[c + 1]) (gmoves, records grec).
// One launch, no scratch memory; children / grandchild arrays are not read when no parent has a
// child.  (The kernel is templated on the parent form and offset type like rank_children_kernel;
// the host path feeds it the same packed parents and 32-bit offsets as the C-ABI: level 2 of the
// expansion has overwritten the buffer set's unpacked parents and 64-bit offsets by then.)
// history: the game-history draws at both levels (include/gpu_nnue.h at gn_line2 and gn_history),
// hist[i] naming parent i's game so far as above; NULL: the plain ranking.  gext: the grandchildren's
// check extensions (as ext above), NULL: none.
hipError_t launch_rank_lines2(const gn_board *parents, size_t n, const uint32_t *offsets, const gn_board *children,
                              const gn_eval *rec, const uint16_t *moves, const uint32_t *goffsets,
                              const uint16_t *gmoves, const gn_eval *grec, const gn_eval_params &P,
                              const Tables *tables, int K, gn_line2 *lines, const RankHistory *history,
                              const int32_t *gext, hipStream_t s);
// Three-ply ranked lines, the root step (include/gpu_nnue.h gn_line3): lines[i * K + k] = line k + 1 of
// root i, from the root expansion (offsets, moves, the child records rec for GN_FLAG_IN_CHECK) and
// clines[c] = line 1 of the two-ply ranking with child c as the parent (empty: c has no legal move);
// with pvs (NULL: none) pvs[i * K + k] = [move] + cpvs[the line's child].  One launch, no move
// generation, no scratch memory; every child range is clamped to total, and with total == 0 no input
// but n is read.
// history (NULL: the plain kernel, which takes no child board): hist[i] names root i's game so far; a
// child (children[c], the library's own boards) whose line is not empty and that is drawn by rule
// against that window overrides its line (value 0, GN_FLAG_DRAW, plies 1), and a child line's
// GN_FLAG_DRAW passes into the root's.
hipError_t launch_rank_lines3(const gn_board *parents, size_t n, const uint32_t *offsets, const uint16_t *moves,
                              const gn_eval *rec, size_t total, const gn_line2 *clines, const gn_pv *cpvs,
                              const gn_eval_params &P, const Tables *tables, int K, gn_line3 *lines, gn_pv *pvs,
                              hipStream_t s, const gn_board *children = nullptr, const RankHistory *history = nullptr);
// chist[j] = hist[i] for every child j in [offsets[i], offsets[i + 1]) of the n roots, the ranges
// clamped to total as rank_lines3_kernel clamps them (total == 0: nothing is read): the children's
// gn_history entries for the two-ply stage of the three-ply history calls (RankHistory::ahead = 1)
hipError_t launch_spread_history(const gn_history *hist, size_t n, const uint32_t *offsets, size_t total,
                                 gn_history *chist, hipStream_t s);
// Check extension of one expansion level (gpu_nnue.hip extend_checks): select (sel[total + 1] from
// the leaf records' GN_FLAG_IN_CHECK, ext[total] = GN_NOT_EXTENDED), boards (pos = exclusive scan of
// sel: the selected leaves' boards sb, leaf indices idx and sv = GN_NOT_EXTENDED, compacted; the
// parents unpacked with 64-bit offsets, or packed with the C-ABI's 32-bit offsets, as for
// launch_rank_children), scatter (ext[idx[k]] = sv[k], *extended += those that are values).
hipError_t launch_extend_select(const gn_eval *rec, size_t total, uint64_t *sel, int32_t *ext, hipStream_t s);
hipError_t launch_extend_boards(const Board *unpacked, size_t n, const uint64_t *offsets, const uint16_t *moves,
                                const uint64_t *sel, const uint64_t *pos, size_t total, const Tables *tables,
                                uint32_t *idx, gn_board *sb, int32_t *sv, hipStream_t s);
hipError_t launch_extend_boards(const gn_board *parents, size_t n, const uint32_t *offsets, const uint16_t *moves,
                                const uint64_t *sel, const uint64_t *pos, size_t total, const Tables *tables,
                                uint32_t *idx, gn_board *sb, int32_t *sv, hipStream_t s);
hipError_t launch_extend_scatter(const uint32_t *idx, const int32_t *sv, size_t m, int32_t *ext,
                                 unsigned long long *extended, hipStream_t s);
// Capture quiescence of one expansion level (gpu_nnue.hip quiesce; the rule in include/gpu_nnue.h at
// gn_quiesce_device).  select: ext[j] = GN_NOT_EXTENDED for all j < total and sel[c] = 1 where leaf c is searched
// (sel zeroed by the caller, total + 1 entries; parents as for launch_extend_boards, which then makes
// the selected leaves' boards; lcnt[c] = leaf c's searched moves, total entries).  count: counts[i] = the searched moves of node i (all legal moves in
// check, the noisy legal ones otherwise; the library's own boards), counts[n] = 0.  children: those
// moves, their owners and boards at offsets (the scan of counts), at most nc.  reduce: val[i] of the
// m nodes from their records (rec[idx[i]] with idx: level 0's child records) and their children's
// values cval, or with cval NULL the children's static part from their position records crec.
// see (select, count, children; NULL: unpruned): the piece values of the pruned rule Qs
// (GN_OPT_QUIESCE_SEE): a node not in check searches only its noisy moves with see >= 0; the pruned
// forms are kernels of their own.
hipError_t launch_quiesce_select(const Board *unpacked, size_t n, const uint64_t *offsets, const uint16_t *moves,
                                 size_t total, const Tables *tables, uint64_t *sel, uint32_t *lcnt, int32_t *ext,
                                 hipStream_t s, const SeeValues *see);
hipError_t launch_quiesce_select(const gn_board *parents, size_t n, const uint32_t *offsets, const uint16_t *moves,
                                 size_t total, const Tables *tables, uint64_t *sel, uint32_t *lcnt, int32_t *ext,
                                 hipStream_t s, const SeeValues *see);
// gn_see_device: out[j] = see(parent of j, moves[j]) where a valid parent's offsets cover j,
// GN_NOT_EXTENDED for every other j < total (a 32-bit fill, then see_moves_kernel)
hipError_t launch_see_moves(const gn_board *parents, size_t n, const uint32_t *offsets, const uint16_t *moves, size_t total,
                            const Tables *tables, const SeeValues &V, int32_t *out, hipStream_t s);
// level 0's counts (m + 1, m = pos[total]) compacted from the selection pass's per-leaf lcnt
hipError_t launch_quiesce_level0_counts(const uint64_t *sel, const uint64_t *pos, const uint32_t *lcnt, size_t total,
                                        uint64_t *counts, hipStream_t s);
hipError_t launch_quiesce_count(const gn_board *boards, size_t n, const Tables *tables, uint64_t *counts, hipStream_t s,
                                const SeeValues *see);
hipError_t launch_quiesce_children(const gn_board *boards, size_t n, const Tables *tables, const uint64_t *offsets,
                                   size_t nc, uint16_t *moves, uint32_t *owner, gn_board *children, hipStream_t s,
                                   const SeeValues *see);
hipError_t launch_quiesce_reduce(const gn_eval *rec, const uint32_t *idx, size_t m, const uint64_t *off, size_t nc,
                                 const gn_eval *crec, const int32_t *cval, int32_t *val, hipStream_t s);
// The quiescence's own variation (the rule at gn_pv in include/gpu_nnue.h).  reduce_pv: reduce, plus
// best[i] = the chosen child's index in the next level (cmoves: that level's moves, for the tie rule),
// QUIESCE_NO_BEST where the node stands pat or has no child.  walk: a lane per selected leaf follows
// best down L.levels levels and writes the moves it passes to tail[idx[i] * GN_MAX_QUIESCE_DEPTH + k]
// (tail zeroed by the caller, total * GN_MAX_QUIESCE_DEPTH entries).  line_pvs / line2_pvs: pvs[p * K
// + k] = the gn_pv of lines[p * K + k], its tail (NULL: none) found through the position's offsets
// and moves; a lane per (position, line).
constexpr uint32_t QUIESCE_NO_BEST = 0xFFFFFFFFu;
struct QuiescePvLevels {
  const uint32_t *best[GN_MAX_QUIESCE_DEPTH]; // level k's chosen children ...
  const uint16_t *moves[GN_MAX_QUIESCE_DEPTH]; // ... and level k + 1's moves
  uint32_t cnt[GN_MAX_QUIESCE_DEPTH + 1];      // the levels' node counts
  int levels;                                  // the levels that were reduced (best[k] valid for k < levels)
};
hipError_t launch_quiesce_reduce_pv(const gn_eval *rec, const uint32_t *idx, size_t m, const uint64_t *off, size_t nc,
                                    const gn_eval *crec, const int32_t *cval, const uint16_t *cmoves, int32_t *val,
                                    uint32_t *best, hipStream_t s);
hipError_t launch_quiesce_walk(const QuiescePvLevels &L, const uint32_t *idx, size_t m, size_t total, uint16_t *tail,
                               hipStream_t s);
hipError_t launch_line_pvs(size_t n, const uint64_t *off, const uint16_t *moves, const uint16_t *tail,
                           const gn_line *lines, int K, gn_pv *pvs, hipStream_t s);
hipError_t launch_line_pvs(size_t n, const uint32_t *off, const uint16_t *moves, const uint16_t *tail,
                           const gn_line *lines, int K, gn_pv *pvs, hipStream_t s);
hipError_t launch_line2_pvs(size_t n, const uint32_t *off, const uint16_t *moves, const uint32_t *goff,
                            const uint16_t *gmoves, const uint16_t *gtail, const gn_line2 *lines, int K, gn_pv *pvs,
                            hipStream_t s);
// exclusive_scan_u64's / king_sort's temporary storage for n1 counts / n boards grown now, so that
// the call itself does not allocate (a caller that reports a failed allocation as its own)
hipError_t reserve_scan_u64(size_t n1, void *&temp, size_t &temp_bytes);
hipError_t reserve_king_sort(size_t n, bool placement, void *&temp, size_t &temp_bytes);
// narrowing copy of offsets for the C-ABI
hipError_t launch_offsets_u32(const uint64_t *in, size_t n, uint32_t *out, hipStream_t s);
// exclusive scan of n + 1 counts (counts[n] must be 0); temp grows on demand
hipError_t exclusive_scan_u64(const uint64_t *counts, uint64_t *offsets, size_t n1, void *&temp,
                              size_t &temp_bytes, hipStream_t s);

} // namespace gn
