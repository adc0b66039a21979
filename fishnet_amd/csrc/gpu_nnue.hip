// gpu_nnue.hip — C-ABI of libgpu_nnue.so (see include/gpu_nnue.h).
//
// Host side of the boundary that replaces the per-core Stockfish processes'
// static evaluation for batch workloads (/root/reference/src/stockfish.rs:36-47
// is the plugin API it sits beside).  Owns: the .nnue loader, device memory,
// one HIP stream per device, FEN packing, and the launch sequences of the
// kernels in kernels.hip.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "archive.h"
#include "host_board.h"
#include "kernels.h"
#include "plan_snapshot.h"
#include "sha256.h"

using namespace gn;

// ------------------------------------------------------------ errors ------
static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return fail(GN_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                      __FILE__, __LINE__);                                          \
  } while (0)

// The exception fence: f's code, or the code and message of what it threw (nothing is thrown
// across the C-ABI or out of a device's host thread).
template <class F>
static int guarded(F &&f) {
  try {
    return f();
  } catch (const std::bad_alloc &) {
    return fail(GN_E_NOMEM, "host allocation failed");
  } catch (...) {
    return fail(GN_E_INVALID, "unexpected exception");
  }
}

namespace gn {
const Tables &host_tables() {
  static Tables T = [] {
    Tables t;
    init_tables(t);
    return t;
  }();
  return T;
}
} // namespace gn

// ----------------------------------------------------------- net file -----
struct HostNet {
  int L1 = 0;
  uint32_t hash = 0;
  std::vector<uint8_t> ft;    // [22528][ft_row_stride(L1)]
  std::vector<int16_t> bias;  // [L1], doubled
  std::vector<int8_t> w0, w1, w2;
  std::vector<int32_t> b0, b1, b2;
};

struct Reader {
  const uint8_t *p;
  size_t n, off = 0;
  bool take(void *dst, size_t k) {
    if (off + k > n) return false;
    memcpy(dst, p + off, k);
    off += k;
    return true;
  }
  bool u32(uint32_t &v) {
    uint8_t b[4];
    if (!take(b, 4)) return false;
    v = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    return true;
  }
  // signed LEB128 block ("COMPRESSED_LEB128", u32 byte count, payload)
  template <class Emit>
  bool leb(int bits, size_t count, Emit &&emit) {
    char magic[17];
    uint32_t nbytes;
    if (!take(magic, 17) || memcmp(magic, "COMPRESSED_LEB128", 17) || !u32(nbytes) || off + nbytes > n) return false;
    const uint8_t *q = p + off, *end = q + nbytes;
    for (size_t i = 0; i < count; ++i) {
      uint32_t r = 0;
      int shift = 0;
      for (;;) {
        if (q >= end || shift >= bits) return false;
        const uint8_t byte = *q++;
        r |= (uint32_t)(byte & 0x7f) << shift;
        shift += 7;
        if (!(byte & 0x80)) {
          if (shift < 32 && (byte & 0x40)) r |= ~((1u << shift) - 1u);
          break;
        }
      }
      emit(i, bits == 16 ? (int32_t)(int16_t)(uint16_t)r : (int32_t)r);
    }
    if (q != end) return false;
    off += nbytes;
    return true;
  }
};

static int parse_net(const uint8_t *data, size_t len, HostNet &h) {
  Reader r{data, len};
  uint32_t version, hash, dlen, fth;
  if (!r.u32(version) || version != NNUE_VERSION) return fail(GN_E_FORMAT, "not a Stockfish .nnue (version)");
  if (!r.u32(hash) || !r.u32(dlen) || r.off + dlen > len) return fail(GN_E_FORMAT, "bad .nnue header");
  r.off += dlen;
  if (!r.u32(fth)) return fail(GN_E_FORMAT, "truncated .nnue");
  int l1 = 0;
  for (int c = 32; c <= 4096 && !l1; c += 32)
    if (ft_hash(c) == fth && (ft_hash(c) ^ arch_hash(c)) == hash) l1 = c;
  if (!l1) return fail(GN_E_FORMAT, "network hash 0x%08x does not match a HalfKAv2_hm architecture", hash);
  if (l1 != 3072 && l1 != 1024 && l1 != 128) return fail(GN_E_FORMAT, "unsupported L1 width %d", l1);
  h.L1 = l1;
  h.hash = hash;
  const size_t RS = ft_row_stride((uint32_t)l1);
  h.ft.assign((size_t)FT_ROWS * RS, 0);
  h.bias.resize(l1);
  uint8_t *ft = h.ft.data();
  if (!r.leb(16, l1, [&](size_t i, int32_t v) { h.bias[i] = (int16_t)(uint16_t)(v * 2); }))
    return fail(GN_E_FORMAT, "bad feature-transformer biases");
  memcpy(ft + (size_t)FT_BIAS_ROW * RS, h.bias.data(), 2 * (size_t)l1);
  if (!r.leb(16, (size_t)l1 * FT_INPUTS, [&](size_t i, int32_t v) {
        const int16_t d = (int16_t)(uint16_t)(v * 2);
        memcpy(ft + (i / l1) * RS + 2 * (i % l1), &d, 2);
      }))
    return fail(GN_E_FORMAT, "bad feature-transformer weights");
  if (!r.leb(32, (size_t)PSQT_BUCKETS * FT_INPUTS, [&](size_t i, int32_t v) {
        memcpy(ft + (i / PSQT_BUCKETS) * RS + 2 * l1 + 4 * (i % PSQT_BUCKETS), &v, 4);
      }))
    return fail(GN_E_FORMAT, "bad PSQT weights");
  h.w0.resize((size_t)LAYER_STACKS * 16 * l1);
  h.w1.resize(LAYER_STACKS * 32 * 32);
  h.w2.resize(LAYER_STACKS * 32);
  h.b0.resize(LAYER_STACKS * 16);
  h.b1.resize(LAYER_STACKS * 32);
  h.b2.resize(LAYER_STACKS);
  const uint32_t ah = arch_hash(l1);
  for (int s = 0; s < LAYER_STACKS; ++s) {
    uint32_t hs;
    if (!r.u32(hs) || hs != ah) return fail(GN_E_FORMAT, "bad layer-stack hash in stack %d", s);
    bool ok = true;
    for (int i = 0; i < 16 && ok; ++i) ok = r.u32(reinterpret_cast<uint32_t &>(h.b0[s * 16 + i]));
    ok = ok && r.take(&h.w0[(size_t)s * 16 * l1], (size_t)16 * l1);
    for (int i = 0; i < 32 && ok; ++i) ok = r.u32(reinterpret_cast<uint32_t &>(h.b1[s * 32 + i]));
    ok = ok && r.take(&h.w1[s * 1024], 1024);
    ok = ok && r.u32(reinterpret_cast<uint32_t &>(h.b2[s]));
    ok = ok && r.take(&h.w2[s * 32], 32);
    if (!ok) return fail(GN_E_FORMAT, "truncated layer stack %d", s);
  }
  if (r.off != len) return fail(GN_E_FORMAT, "%zu trailing bytes after the network", len - r.off);
  return GN_OK;
}

// ----------------------------------------------------------- context ------
// Device resources are owned by the members that name them: each of the types below frees what it
// holds in its destructor and is move-only, so a context is torn down by its destructors (~Dev
// makes the device current and idle first) and a timing call's events go on every way out.
template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept { return std::swap(p, o.p), std::swap(cap, o.cap), *this; }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    const size_t want = std::max(n, cap + cap / 2);
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    // (whole 16-B units: a kernel may read the aligned word holding a byte array's last byte,
    // plan_kernel's need / next-slot loads)
    hipError_t e = hipMalloc(&p, (std::max<size_t>(want, 1) * sizeof(T) + 15) & ~(size_t)15);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { // (also mid-life: memory given back when an allocation beside it failed)
    if (p) (void)hipFree(p);
    p = nullptr, cap = 0;
  }
};
// A HIP handle (it converts to the handle wherever one is taken; h is set by the hip*Create call).
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(const Handle &) = delete;
  Handle &operator=(const Handle &) = delete;
  Handle(Handle &&o) noexcept : h(o.h) { o.h = nullptr; }
  Handle &operator=(Handle &&o) noexcept { return std::swap(h, o.h), *this; }
  ~Handle() {
    if (h) (void)Destroy(h);
  }
  operator H() const { return h; }
};
static hipError_t idle_then_destroy(hipStream_t s) {
  (void)hipStreamSynchronize(s);
  return hipStreamDestroy(s);
}
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, idle_then_destroy>;
// The events of one timing call: make() creates one for each handle it is given.
struct Events {
  std::vector<Event> v;
  hipError_t make(std::initializer_list<hipEvent_t *> es) {
    for (hipEvent_t *e : es) {
      v.emplace_back();
      if (const hipError_t r = hipEventCreate(&v.back().h); r != hipSuccess) return r;
      *e = v.back();
    }
    return hipSuccess;
  }
};

// The net outputs / selections of one evaluation (evaluate_on)
struct EvalBufs {
  DevBuf<int2> osm, obg;
  DevBuf<uint8_t> nsm, nbg;
};

// How a ranked-lines call values its lines' leaves: by their static records (the plain calls); the
// leaves in check by the score rule (the _extended calls); or the searched leaves by the capture
// quiescence to `depth` plies, 1..GN_MAX_QUIESCE_DEPTH (the _quiescent calls; check_leaf_rule).
struct LeafRule {
  enum Kind { STATIC, CHECKS, QUIESCE } kind = STATIC;
  int depth = 0;       // QUIESCE alone
  bool pruned = false; // QUIESCE alone: Qs, the losing captures pruned (GN_OPT_QUIESCE_SEE, read once per call)
  static LeafRule checks() { return {CHECKS, 0}; }
  static LeafRule quiesce(const gn_ctx *ctx, int depth);
  bool extends() const { return kind != STATIC; } // the call runs the leaf stage, and its ranking takes ext
};
struct LeafCount { // one run of the leaf stage: the leaves it valued, the positions evaluated below them
  size_t leaves = 0, nodes = 0;
  float pv_ms = 0; // with a tail: quiesce_walk_kernel's time
};

// ---- the drop-in's small batches ------------------------------------
// fishnet's GPU backend sends one game per gn_evaluate_batch (/root/reference/src/stockfish.rs:
// 36-47, src/main.rs:306-338: a chunk per worker call), ~80 positions, a few of them in check.
// The general path costs ~20 launches and three host round trips per call (the score rule's
// reply counts); on a one-device context a batch of <= 4,096 positions runs instead as one
// captured HIP graph per (size class, mode): upload from pinned memory, both levels of the
// in-check replies (reply_level_kernel: one workgroup selects from the boards, counts, scans and
// makes a level's replies; the levels are sized by their capacities, unused slots empty boards,
// so nothing waits for a count), one evaluation of the positions and both levels together, the
// two reductions (one workgroup), and the download of the overflow flag and the records.  One
// synchronisation per call.  A level with
// more replies than its capacity (nb / 2 + 256, nb / 4 + 256: beyond a game's) sets the flag and
// the call reruns on the general path.  Positions beyond n are empty boards (BAD_FEN records,
// never read back).
constexpr size_t FAST_NB0 = 128, FAST_MAX = 4096;
struct FastBatch {
  size_t nb = 0, c1 = 0, c2 = 0;
  int mode = -1;
  uint64_t gen = 0;
  Handle<hipGraph_t, hipGraphDestroy> graph;
  Handle<hipGraphExec_t, hipGraphExecDestroy> exec;
  Event done; // recorded behind each launch (the caller waits for it without d.mu)
  bool busy = false;         // a launch of this instance is in flight (d.mu)
  gn_board *h_in = nullptr; // pinned: nb boards
  gn_eval *h_out = nullptr; // pinned: one record holding the overflow flag, then nb records
  // the three levels one after another (in: nb boards, r1: c1 replies, r2: c2 replies of replies)
  // and their records behind the flag record, so that one evaluation covers them all
  DevBuf<gn_board> all;
  DevBuf<gn_eval> rec;
  gn_board *in = nullptr, *r1 = nullptr, *r2 = nullptr;
  gn_eval *out = nullptr, *e1 = nullptr, *e2 = nullptr;
  DevBuf<uint64_t> off0, off1;
  DevBuf<uint16_t> m1, m2;
  DevBuf<int32_t> sv1, sv2;
  EvalBufs eb;
  ~FastBatch() {
    if (h_in) (void)hipHostFree(h_in);
    if (h_out) (void)hipHostFree(h_out);
  }
};

// The buffers one expansion's front half (child generation, classify, small net, plan) writes and
// its back half (row stream, finalize, score rule) reads: the expansion pipeline (run_expansions
// below) runs expansion k + 1's front on the device's second stream while expansion k's back
// runs, in the other set (Dev::cur / Dev::alt, swap_sets).
struct ExpSet {
  DevBuf<uint64_t> counts, offsets;
  DevBuf<uint32_t> owner;                // parent of each child (write_children scratch)
  DevBuf<Board> unpacked;                // the parents unpacked once (write_children scratch)
  DevBuf<uint16_t> moves_tmp;            // when the caller keeps no moves
  const uint16_t *child_moves = nullptr; // the last generate_children's moves (finalize reads them)
  DevBuf<int2> pinfo;                    // sliced stream: each position's (PSQT value, bucket) for the finish
  DevBuf<int2> p_osm, p_obg;             // parent-side net outputs during expansion
  DevBuf<uint8_t> p_nsm, p_nbg;          // parent-side net selection during expansion
  EvalBufs eb;                           // the children's net outputs; evaluate_on's outputs
  DevBuf<gn_board> children;             // library-internal child boards
  int chain_k = 1;      // block length of this expansion (1: no chaining)
  int slices = 1;       // this expansion's stream: column slices (3) or whole rows (1)
  bool planned = false; // this expansion runs the planned kernels (stream.hip; perr is meaningful)
  uint64_t etot = 0;    // eoff[n] of this expansion
  // the scans' / sorts' scratch, which they grow themselves (cap in bytes; the two streams' scans /
  // sorts run at once)
  DevBuf<void> scan_tmp, sort_tmp;
  // recorded on the device stream behind this set's last score rule: a front that does not wait
  // for the row stream (GN_OPT_EXPAND_PIPELINE 2) waits for it before it overwrites the set
  Event scored;
  DevBuf<uint32_t> perr;            // the planned expansion's error word ...
  // ... and its counts: [0] pads, [1] zero-row entries (each expansion of the pipeline its own), [2] the
  // plan's FT rows when no caller counts them (expand_level; gn_debug_plan_snapshot reads all three)
  DevBuf<unsigned long long> pstat;
  // the plan's output the row stream reads (GN_OPT_EXPAND_PIPELINE 2: the next plan runs beside
  // this expansion's row stream)
  DevBuf<uint64_t> ent, eoff;
  DevBuf<TileDesc> tiles;
  DevBuf<uint32_t> btiles, border;
  // what the last plan in this set was launched with (gn_debug_plan_snapshot, plan_snapshot.h);
  // plan_geo.nblk == 0: none since the set's last child generation
  PlanGeometry plan_geo;
  size_t plan_n = 0, plan_total = 0;
  bool plan_ordered = false;
};

struct Dev {
  int id = 0;
  Stream stream; // (the first member: destroyed after everything queued on it is freed)
  DevBuf<uint8_t> net_mem[2];
  NetDevice net[2] = {};
  bool has[2] = {false, false};
  DevBuf<Tables> tables;
  // The current expansion's buffers (generate_children, expand_evaluate, resolve_scores and
  // evaluate_on work in cur) and the other set, in which the pipeline's next front runs.  What an
  // expansion's back half reads belongs in ExpSet.  Here stay only: what the front half that wrote
  // it alone reads (deltas, nslot, ebound, bkeys*, bidx: the fronts run one after another on one
  // stream), and what the back halves share because they run one after another (pool; part, which
  // a front may not reallocate while a pipeline runs: part_locked).
  ExpSet cur, alt;
  DevBuf<gn_board> io_boards, frontier; // frontier: gn_perft's current level
  DevBuf<gn_eval> io_out, io_out2;
  DevBuf<uint32_t> off32;
  DevBuf<uint16_t> moves;
  DevBuf<ChildDelta> deltas;
  DevBuf<uint64_t> kkeys, kkeys2; // king-sort keys
  DevBuf<uint32_t> kidx, kperm;   // king-sort permutation
  DevBuf<unsigned long long> sum;
  DevBuf<uint8_t> nslot; // chained walk: child of parent i that is parent i + 1 (255: none)
  DevBuf<int32_t> part;  // column-sliced stream: fc_0 partial sums of the 3 slices (3 x positions x GN_PART_DWORDS)
  bool part_locked = false; // a pipeline runs: part is in use by a back half (no reallocation)
  DevBuf<uint64_t> ebound;  // planned expansion (stream.hip): per-parent entry bounds
  DevBuf<uint32_t> pool;    // ... and the scratch-slot pool
  DevBuf<uint16_t> bkeys, bkeys2; // block_order scratch
  DevBuf<uint32_t> bidx;          // block_order: identity
  // Cross-stream ordering of the library-owned scratch above: every launch sequence
  // waits for the previous one when it runs on another stream (gn_*_device take a
  // caller stream and return while their kernels are still queued).
  Event done;
  hipStream_t done_on = nullptr;
  float plan_ms = 0, stream_ms = 0, finish_ms = 0; // the last timed planned expansion (GN_STAT_PLAN_NS /
                                                    // _STREAM_NS / _FINISH_NS)
  // the score rule's two levels of in-check replies (resolve_scores): selection, the selected
  // positions, their replies and the replies' records / rule values
  struct ScoreLevel {
    DevBuf<uint64_t> sel, pos, counts, offsets;
    DevBuf<uint32_t> idx, owner;
    DevBuf<gn_board> boards, children;
    DevBuf<uint16_t> moves;
    DevBuf<gn_eval> ce;
    DevBuf<int32_t> sv;
  } lv[2];
  // the host-buffer calls' pipeline (expand_pipelined): per chunk slot the parent / child
  // records and child moves a drain thread downloads on the copy stream while the next chunk
  // computes; the lichess replay's inputs and outputs (replay_games_kernel)
  Stream copy;
  Event cev[2];
  DevBuf<gn_eval> po2[2], co2[2];
  DevBuf<gn_child> cc2[2]; // co2 packed as the host's 12-B child records (ABI v4)
  DevBuf<gn_line> ln2[2];  // or ranked: the chunk's lines (gn_evaluate_games_lines)
  Event rev[2]; // around a chunk's rank_children_kernel (GN_STAT_RANK_NS)
  DevBuf<uint16_t> mv2[2];
  DevBuf<gn_pv> pv2[2]; // the _pv calls: the chunk's PVs, downloaded with its lines
  Event pev[4];         // around quiesce_walk_kernel and around a chunk's PV assembly (GN_STAT_PV_NS)
  // gn_evaluate_lines2: one chunk's depth-2 expansion (gn_expand2_device's outputs, library-owned
  // and grown to the chunk's exact counts) and its lines
  struct Lines2 {
    DevBuf<gn_eval> po, co, gco;
    DevBuf<uint32_t> off, goff;
    DevBuf<gn_board> ch;
    DevBuf<uint16_t> mv, gmv;
    DevBuf<gn_line2> ln;
    DevBuf<int32_t> gext; // a rule that extends: the grandchildren's values from the leaf stage
    DevBuf<uint16_t> gtail; // the _pv calls: the grandchildren's tails from the leaf stage ...
    DevBuf<gn_pv> pv;       // ... and the chunk's PVs
  } l2;
  // gn_evaluate_lines3: one chunk of roots' depth-1 expansion (l2 is in use below it: the children
  // run through the two-ply chunk computation as parents), each child's line 1 and its PV, which
  // never leave the device, and the chunk's lines and PVs
  struct Lines3 {
    DevBuf<gn_eval> po, co;
    DevBuf<uint32_t> off;
    DevBuf<gn_board> ch;
    DevBuf<uint16_t> mv;
    DevBuf<gn_line2> cln;
    DevBuf<gn_pv> cpv;
    DevBuf<gn_history> chist; // the history calls: each child's entry, its root's (launch_spread_history)
    DevBuf<gn_line3> ln;
    DevBuf<gn_pv> pv;
  } l3;
  Event r3ev[2];     // around a chunk's rank_lines3_kernel (GN_STAT_RANK3_NS)
  double t_rank3 = 0; // ... summed over the last three-ply call's chunks, ms
  // the leaf stage of one expansion level (value_leaves).  The selected leaves (level 0): the
  // selection and its scan, their indices, boards and values, the count of valued ones; rec: the
  // check extension's own records of them; ext: the one-ply games calls' per-chunk leaf values.
  // The quiescence's levels: lv[k] holds level k's searched-move counts and their scan and, for
  // k >= 1, its boards, position records and values; moves / owner: the level being made.  With a
  // tail requested (the _pv calls) each level k >= 1 keeps its own moves and each reduced level its
  // chosen children (best), and tail holds the one-ply games calls' per-chunk tails.
  struct LeafStage {
    DevBuf<uint64_t> sel, pos;
    DevBuf<uint32_t> idx;
    DevBuf<gn_board> boards;
    DevBuf<gn_eval> rec;
    DevBuf<int32_t> sv;
    DevBuf<unsigned long long> count;
    DevBuf<int32_t> ext;
    struct Level {
      DevBuf<gn_board> boards;
      DevBuf<gn_eval> rec;
      DevBuf<int32_t> val;
      DevBuf<uint64_t> counts, offsets;
      DevBuf<uint16_t> moves;
      DevBuf<uint32_t> best;
    } lv[GN_MAX_QUIESCE_DEPTH + 1];
    DevBuf<uint16_t> tail;
    DevBuf<uint16_t> moves;
    DevBuf<uint32_t> owner;
    DevBuf<uint32_t> lcnt; // every leaf's searched moves, from the quiescence's selection pass
    void release() { // (a quiescent call's failed allocation: the levels, and what of level 0 grows with the leaves)
      for (Level &l : lv) l.boards.release(), l.rec.release(), l.val.release(), l.counts.release(), l.offsets.release();
      for (Level &l : lv) l.moves.release(), l.best.release();
      moves.release(), owner.release(), lcnt.release();
      sel.release(), pos.release(), idx.release(), boards.release(), rec.release(), sv.release();
    }
    // the stage in the last host-buffer call, by the rule's kind (extend_stage): GN_STAT_EXTEND_NS /
    // _QUIESCE_NS in ms, GN_STAT_EXTENDED_LEAVES / _QUIESCE_LEAVES, GN_STAT_QUIESCE_NODES
    struct Stats {
      double ms = 0;
      uint64_t leaves = 0, nodes = 0;
    } stats[3];
  } leaf;
  DevBuf<gn_board> roots, rboards, par;
  DevBuf<uint64_t> moff;
  DevBuf<uint16_t> codes, smoves;
  DevBuf<int32_t> rstatus;
  DevBuf<uint32_t> gidx;
  // gn_evaluate_games_lines_history: position_key of every board of rboards (n_rkeys of them), and
  // one gn_history per evaluated position of the shard
  DevBuf<uint64_t> rkeys;
  size_t n_rkeys = 0;
  DevBuf<gn_history> hist;
  double t_keys = 0; // position_keys_kernel in that call (GN_STAT_KEYS_NS), ms
  // stage times of the last host-buffer call on this device (GN_STAT_HOST_*), ms
  double t_upload = 0, t_replay = 0, t_compute = 0, t_download = 0, t_tail = 0, t_rank = 0, t_rank2 = 0;
  double t_pv = 0; // the PV kernels in the last _pv call (GN_STAT_PV_NS), ms
  // the drop-in's small-batch graphs (FastBatch): two per size class (128 << k positions) and mode,
  // so that a second call's launch queues on the stream behind a first one in flight
  std::unique_ptr<FastBatch> fast[6][3][2];
  std::condition_variable fast_cv; // an instance's launch completed (its busy flag cleared; d.mu)
  // the expansion pipeline: the front's stream and its two events (the back's row stream done:
  // the front may overwrite the plan's lists; the plan done)
  Stream front;
  Event ev_streamed, ev_planned;
  std::mutex mu;
  // the device current and its streams idle before the members above free what may still be in use
  ~Dev() {
    (void)hipSetDevice(id);
    for (hipStream_t s : {stream.h, front.h, copy.h})
      if (s) (void)hipStreamSynchronize(s);
  }
};

// The Dev's current expansion buffers <-> its other set (host-side pointers only: launches already
// queued keep the buffers they were given).
static void swap_sets(Dev &d) { std::swap(d.cur, d.alt); }

// Called under d.mu before a launch sequence on stream s / after it.
static hipError_t seq_begin(Dev &d, hipStream_t s) {
  if (d.done_on && d.done_on != s) return hipStreamWaitEvent(s, d.done, 0);
  return hipSuccess;
}
static hipError_t seq_end(Dev &d, hipStream_t s) {
  hipError_t e = hipEventRecord(d.done, s);
  if (e == hipSuccess) d.done_on = s;
  return e;
}
// After a synchronised planned expansion: its device error word (entry overflow or no
// scratch slot; neither can happen by construction, but a wrong result must not pass).
static int check_plan(Dev &d, hipStream_t s) {
  if (!d.cur.planned || !d.cur.perr.p) return GN_OK;
  uint32_t e = 0;
  HIP_TRY(hipMemcpyAsync(&e, d.cur.perr.p, sizeof(e), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (e) return fail(GN_E_HIP, "planned expansion failed on the device (error bits 0x%x)", e);
  return GN_OK;
}

struct SeqGuard { // seq_begin now, seq_end when the scope ends (d.mu held throughout)
  Dev &d;
  hipStream_t s;
  hipError_t e;
  bool ended = false;
  SeqGuard(Dev &d_, hipStream_t s_) : d(d_), s(s_) { e = seq_begin(d, s); }
  // the sequence's end marker now, then wait for the stream: the call returns with its stream idle
  hipError_t finish() {
    ended = true;
    hipError_t r = seq_end(d, s);
    return r == hipSuccess ? hipStreamSynchronize(s) : r;
  }
  ~SeqGuard() {
    if (!ended) (void)seq_end(d, s);
  }
};

// A single-device entry point's frame: the device's lock, the device made current, and a launch
// sequence on the caller's stream (NULL: the device's own), for the object's lifetime.  rc is the
// failure that kept the sequence from beginning (its message set), or GN_OK.
struct DevCall {
  std::lock_guard<std::mutex> lk;
  const hipStream_t s;
  std::optional<SeqGuard> sg; // (ends before the lock is released)
  int rc;
  DevCall(Dev &d, void *stream = nullptr) : lk(d.mu), s(stream ? (hipStream_t)stream : d.stream) {
    rc = [&]() -> int {
      HIP_TRY(hipSetDevice(d.id));
      sg.emplace(d, s);
      HIP_TRY(sg->e);
      return GN_OK;
    }();
  }
};

// Merged launches running at once (evaluate_coalesced).  Two (-DGN_MAX_LEADERS=2: a second
// leader's launch queues on the stream behind the first's, the small-batch graphs having two
// instances per class) measured the same 16-caller rate with 50 % more, smaller launches
// (round 6, profiles/r06/dropin_ab_r06w.txt): one at a time.
#ifndef GN_MAX_LEADERS
#define GN_MAX_LEADERS 1
#endif
constexpr int MAX_LEADERS = GN_MAX_LEADERS;
// One gn_evaluate_batch call waiting for, or in, a merged launch (evaluate_coalesced).
struct BatchReq {
  const gn_board *boards;
  size_t n;
  int mode;
  gn_eval *out;
  int rc = GN_OK;
  bool done = false;
  bool taken = false; // in a leader's launch (its thread waits for the result)
  char err[256] = ""; // (fixed size: copied while another caller's launch is marked busy, noexcept)
};

struct gn_ctx {
  std::vector<std::unique_ptr<Dev>> devs;
  // concurrent gn_evaluate_batch callers (fishnet's workers, one chunk per call) are merged
  // into one launch (evaluate_coalesced); GN_OPT_COALESCE
  struct {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<BatchReq *> q; // calls waiting for a launch
    int active = 0;            // launches running (<= MAX_LEADERS)
    uint64_t launches = 0, calls = 0;
  } co;
  bool coalesce = true;
  bool fast_batch = true;                  // GN_OPT_FAST_BATCH
  int pipeline = 2;                        // GN_OPT_EXPAND_PIPELINE (2: the next front beside the stream)
  std::atomic<uint64_t> graph_gen{0};      // bumped by every option / parameter change: the small-
                                           // batch graphs captured before it are rebuilt
  std::atomic<uint64_t> fast_runs{0}, fast_fallbacks{0};
  gn_eval_params P;
  bool incremental = true; // GN_OPT_INCREMENTAL_CHILDREN
  int swizzle = 9;          // GN_OPT_XCD_SWIZZLE bit mask: 1 small-net expansion, 2 batch evaluation,
                            // 4 / 8 big-net expansion (static eighths / XCD-local claiming)
  int king_sort = 1;        // GN_OPT_KING_SORT (1: batches of >= KING_SORT_MIN positions, 2: all)
  int chain = 81;           // GN_OPT_CHAIN (blocks of consecutive parents per workgroup)
  bool king_cache = true;   // GN_OPT_KING_CACHE
  int stream_slices = 3;    // GN_OPT_STREAM_SLICES (3 or 1)
  int64_t chunk_parents = 0; // GN_OPT_CHUNK_PARENTS (0: automatic)
  bool quiesce_see = false;  // GN_OPT_QUIESCE_SEE
  int l1[2] = {0, 0};
  uint32_t hash[2] = {0, 0};
  double t_parse = 0, t_total = 0; // the last host-buffer expansion call (GN_STAT_HOST_*), ms
};

enum { BIG = 0, SMALL = 1 };

static gn_eval_params default_params() {
  gn_eval_params P;
  P.small_net_threshold = 962;
  P.psqt_weight = 125;
  P.positional_weight = 131;
  P.reeval_threshold = 236;
  P.complexity_div_small = 18000;
  P.complexity_div_big = 18000;
  P.material_pawn_small = 535;
  P.material_pawn_big = 535;
  P.material_base = 77777;
  P.rule50_div = 212;
  P.value_clamp = 31506;
  const int32_t pv[5] = {208, 781, 825, 1276, 2538};
  memcpy(P.piece_value, pv, sizeof(pv));
  const double wa[4] = {-37.45051876, 121.19101539, -132.78783573, 420.70576692};
  memcpy(P.wdl_a, wa, sizeof(wa));
  P.wdl_material_min = 17;
  P.wdl_material_max = 78;
  P.wdl_material_anchor = 58;
  const int32_t ww[5] = {1, 3, 3, 5, 9};
  memcpy(P.wdl_piece_weight, ww, sizeof(ww));
  return P;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static int upload_net(Dev &d, int which, const HostNet &h) {
  const size_t RS = ft_row_stride((uint32_t)h.L1);
  size_t off[12], o = 0;
  const int carry = h.L1 == 128 ? 0 : CARRY_SLOTS; // the chained walk's scratch rows
  // the PSQT weights once more as [bucket][row] (721 KB: L2-resident for the plan kernel's
  // scattered 4-byte reads, which would otherwise each touch a 6 KB FT row)
  std::vector<int32_t> psqt((size_t)PSQT_BUCKETS * FT_ROWS);
  for (size_t r = 0; r < (size_t)FT_ROWS; ++r)
    for (int b = 0; b < PSQT_BUCKETS; ++b)
      memcpy(&psqt[(size_t)b * FT_ROWS + r], h.ft.data() + r * RS + 2 * (size_t)h.L1 + 4 * b, 4);
  // fc_0 weights once more in the MFMA's operand order (stream.hip): per bucket and 64-wide
  // k-step, lane ln's 16 bytes (output ln & 15, inputs 16 (ln >> 4) .. + 15) at 16 ln, so a
  // wave's k-step is one contiguous 1 KiB (8 whole lines) instead of 16 pieces of 64 B
  const int KS = h.L1 / 64;
  std::vector<int8_t> w0f(h.w0.size());
  for (int b = 0; b < LAYER_STACKS; ++b)
    for (int ks = 0; ks < KS; ++ks)
      for (int ln = 0; ln < 64; ++ln)
        memcpy(&w0f[(((size_t)b * KS + ks) * 64 + ln) * 16],
               &h.w0[((size_t)b * 16 + (ln & 15)) * h.L1 + 64 * (size_t)ks + 16 * (ln >> 4)], 16);
  // the column-sliced stream's packed partial sums (kernels.h): the slices' offsets, the corrected bias
  std::vector<int32_t> poff(h.L1 == 3072 ? LAYER_STACKS * 3 * 16 : 0), b0p(h.L1 == 3072 ? LAYER_STACKS * 16 : 0);
  if (h.L1 == 3072 && !part_offsets(h.w0.data(), h.b0.data(), h.L1, poff.data(), b0p.data()))
    return fail(GN_E_FORMAT, "fc_0 weights of a column slice span 2^24 or more");
  const size_t sz[12] = {((size_t)FT_ROWS + 4 * (size_t)carry + 128 * (size_t)carry + (carry ? 1 : 0)) * RS, h.bias.size() * 2, h.w0.size(), h.b0.size() * 4,
                         h.w1.size(), h.b1.size() * 4, h.w2.size(), h.b2.size() * 4, psqt.size() * 4, w0f.size(),
                         poff.size() * 4, b0p.size() * 4};
  const void *src[12] = {h.ft.data(), h.bias.data(), h.w0.data(), h.b0.data(),
                         h.w1.data(), h.b1.data(), h.w2.data(), h.b2.data(), psqt.data(), w0f.data(),
                         poff.data(), b0p.data()};
  for (int i = 0; i < 12; ++i) off[i] = o, o += align256(sz[i]);
  if (d.net_mem[which].ensure(o) != hipSuccess) return fail(GN_E_NOMEM, "device allocation of %zu bytes failed", o);
  uint8_t *const m = d.net_mem[which].p;
  for (int i = 0; i < 12; ++i)
    if (sz[i]) HIP_TRY(hipMemcpy(m + off[i], src[i], i == 0 ? (size_t)FT_ROWS * RS : sz[i], hipMemcpyHostToDevice));
  if (carry) HIP_TRY(hipMemset(m + off[0] + (size_t)FT_ROWS * RS, 0, 4 * (size_t)carry * RS));
  if (carry) HIP_TRY(hipMemset(m + off[0] + (size_t)ZERO_ROW * RS, 0, RS)); // the zero row
  NetDevice &n = d.net[which];
  n.L1 = h.L1;
  n.row_stride = (uint32_t)RS;
  n.carry_slots = carry;
  n.kc_slots = carry;
  n.ft = m + off[0];
  n.bias = reinterpret_cast<const int16_t *>(m + off[1]);
  n.w0 = reinterpret_cast<const int8_t *>(m + off[2]);
  n.b0 = reinterpret_cast<const int32_t *>(m + off[3]);
  n.w1 = reinterpret_cast<const int8_t *>(m + off[4]);
  n.b1 = reinterpret_cast<const int32_t *>(m + off[5]);
  n.w2 = reinterpret_cast<const int8_t *>(m + off[6]);
  n.b2 = reinterpret_cast<const int32_t *>(m + off[7]);
  n.psqt = reinterpret_cast<const int32_t *>(m + off[8]);
  n.w0f = reinterpret_cast<const int8_t *>(m + off[9]);
  n.part_off = poff.empty() ? nullptr : reinterpret_cast<const int32_t *>(m + off[10]);
  n.b0p = b0p.empty() ? nullptr : reinterpret_cast<const int32_t *>(m + off[11]);
  d.has[which] = true;
  return GN_OK;
}

static void destroy(gn_ctx *ctx) { delete ctx; }

static int create(const uint8_t *big, size_t big_len, const uint8_t *small, size_t small_len, const int *devices,
                  int n_devices, gn_ctx **out) {
  if (!out) return fail(GN_E_INVALID, "out is NULL");
  *out = nullptr;
  if (!big && !small) return fail(GN_E_INVALID, "no network given");
  HostNet hn[2];
  if (big) {
    int rc = parse_net(big, big_len, hn[BIG]);
    if (rc) return rc;
  }
  if (small) {
    int rc = parse_net(small, small_len, hn[SMALL]);
    if (rc) return rc;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(GN_E_NODEVICE, "no HIP device visible");
  std::vector<int> ids;
  if (devices && n_devices > 0) ids.assign(devices, devices + n_devices);
  else ids.push_back(0);
  std::unique_ptr<gn_ctx> ctx(new gn_ctx());
  ctx->P = default_params();
  for (int w = 0; w < 2; ++w) ctx->l1[w] = hn[w].L1, ctx->hash[w] = hn[w].hash;
  for (int id : ids) {
    if (id < 0 || id >= count) return fail(GN_E_NODEVICE, "device %d out of range (%d visible)", id, count);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, id));
    if (!strstr(prop.gcnArchName, "gfx950"))
      return fail(GN_E_NODEVICE, "device %d is %s; libgpu_nnue is built for gfx950 only", id, prop.gcnArchName);
    ctx->devs.emplace_back(new Dev());
    Dev &d = *ctx->devs.back();
    d.id = id;
    HIP_TRY(hipSetDevice(id));
    for (Stream *s : {&d.stream, &d.copy, &d.front}) HIP_TRY(hipStreamCreateWithFlags(&s->h, hipStreamNonBlocking));
    for (Event *e : {&d.done, &d.ev_streamed, &d.ev_planned, &d.cev[0], &d.cev[1], &d.cur.scored, &d.alt.scored})
      HIP_TRY(hipEventCreateWithFlags(&e->h, hipEventDisableTiming));
    for (Event &e : d.rev) HIP_TRY(hipEventCreate(&e.h));
    for (Event &e : d.pev) HIP_TRY(hipEventCreate(&e.h));
    for (Event &e : d.r3ev) HIP_TRY(hipEventCreate(&e.h));
    HIP_TRY(d.tables.ensure(1));
    for (ExpSet *x : {&d.cur, &d.alt}) { // the planned expansion's error word and pad count
      HIP_TRY(x->perr.ensure(1));
      HIP_TRY(x->pstat.ensure(3));
    }
    HIP_TRY(hipMemset(d.alt.perr.p, 0, sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(d.tables.p, &host_tables(), sizeof(Tables), hipMemcpyHostToDevice));
    for (int w = 0; w < 2; ++w)
      if (hn[w].L1) {
        int rc = upload_net(d, w, hn[w]);
        if (rc) return rc;
      }
  }
  *out = ctx.release();
  return GN_OK;
}

static bool read_file(const char *path, std::vector<uint8_t> &buf) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  buf.resize(n > 0 ? (size_t)n : 0);
  bool ok = n >= 0 && fread(buf.data(), 1, buf.size(), f) == buf.size();
  fclose(f);
  return ok;
}

// ---------------------------------------------------------- launches ------
// The marks of one timed evaluation, in stream order: gn_time_evaluate_device's four stages are
// [begun, sorted] classify (+ the king sort), [sorted, small_done] the small net (+ reeval),
// [small_done, big_done] the big net, [big_done, finalized] finalize.
struct EvalEvents {
  hipEvent_t begun, sorted, small_done, big_done, finalized;
  hipError_t create(Events &from) { return from.make({&begun, &sorted, &small_done, &big_done, &finalized}); }
};
// Every device allocation of one evaluate_on over n positions, in two parts: the net outputs and
// selections of the mode (in B), and the king sort's keys, permutation and temporary storage.
// evaluate_on calls both itself; a caller that has to report a failed allocation as its own (quiesce)
// calls them first, after which evaluate_on allocates nothing.
static hipError_t reserve_eval_outputs(EvalBufs &B, size_t n, int mode) {
  hipError_t e = hipSuccess;
  if (mode != GN_MODE_BIG && (e = B.osm.ensure(n)) != hipSuccess) return e;
  if (mode != GN_MODE_SMALL && (e = B.obg.ensure(n)) != hipSuccess) return e;
  if (mode == GN_MODE_FULL) {
    if ((e = B.nsm.ensure(n)) != hipSuccess) return e;
    if ((e = B.nbg.ensure(n)) != hipSuccess) return e;
  }
  return e;
}
static hipError_t reserve_king_sort_buffers(Dev &d, size_t n, int mode) {
  hipError_t e;
  if ((e = d.kkeys.ensure(n)) != hipSuccess) return e;
  if ((e = d.kkeys2.ensure(n)) != hipSuccess) return e;
  if ((e = d.kidx.ensure(n)) != hipSuccess) return e;
  if ((e = d.kperm.ensure(n)) != hipSuccess) return e;
  return reserve_king_sort(n, mode != GN_MODE_SMALL, d.cur.sort_tmp.p, d.cur.sort_tmp.cap);
}
// evaluate_on sorts by king squares (default options): a small batch gains nothing from the order and
// would pay the sort's launches on its latency (bench.py secondary.dropin)
constexpr size_t KING_SORT_MIN = 1024;
static bool king_sorted(const gn_ctx *ctx, size_t n) {
  return ctx->king_sort == 2 || (ctx->king_sort == 1 && n >= KING_SORT_MIN);
}
// evaluate_on's optional arguments.
struct EvalOnOpts {
  EvalEvents *ev = nullptr;           // recorded between the stages
  unsigned long long *rows = nullptr; // += FT rows the gather reads (the big net's, or the small net's in GN_MODE_SMALL)
  // the records are positions (the score rule's static part; resolve_scores does the in-check
  // ones) rather than child records (0)
  int score = 1;
  const uint64_t *counts = nullptr; // their legal-move counts
  // the net outputs and selections in these buffers instead of the current set's (the drop-in's
  // captured small-batch graphs own theirs, FastBatch)
  EvalBufs *eb = nullptr;
  bool sort = true; // false: no king sort
};
// Launch sequence of one evaluation.
static int evaluate_on(gn_ctx *ctx, Dev &d, const gn_board *b, size_t n, int mode, gn_eval *out, hipStream_t s,
                       const EvalOnOpts &o = {}) {
  if (mode < GN_MODE_FULL || mode > GN_MODE_SMALL) return fail(GN_E_INVALID, "bad mode %d", mode);
  if ((mode != GN_MODE_SMALL && !d.has[BIG]) || (mode != GN_MODE_BIG && !d.has[SMALL]))
    return fail(GN_E_NONET, "mode %d needs a network that is not loaded", mode);
  if (!n) return GN_OK;
  EvalBufs &B = o.eb ? *o.eb : d.cur.eb;
  DevBuf<int2> &osm = B.osm, &obg = B.obg;
  DevBuf<uint8_t> &nsm = B.nsm, &nbg = B.nbg;
  HIP_TRY(reserve_eval_outputs(B, n, mode));
  auto mark = [&](hipEvent_t EvalEvents::*m) { return o.ev ? hipEventRecord(o.ev->*m, s) : hipSuccess; };
  const gn_eval_params &P = ctx->P;
  HIP_TRY(mark(&EvalEvents::begun)); // (mode FULL's selection runs inside the small net's launch: launch_eval_net cls)
  const uint32_t *perm = nullptr;
  if (o.sort && king_sorted(ctx, n)) {
    if (n > 0x7FFFFFFFull) return fail(GN_E_INVALID, "king sort supports < 2^31 positions per call");
    HIP_TRY(reserve_king_sort_buffers(d, n, mode));
    HIP_TRY(king_sort(b, n, d.kkeys.p, d.kidx.p, d.kkeys2.p, d.kperm.p, mode != GN_MODE_SMALL, d.cur.sort_tmp.p,
                      d.cur.sort_tmp.cap, s));
    perm = d.kperm.p;
  }
  const int swz = (ctx->swizzle >> 1) & 1;
  HIP_TRY(mark(&EvalEvents::sorted));
  if (mode == GN_MODE_FULL && d.net[SMALL].L1 != 128) {
    // only the 128-wide kernel selects inside its launch: a wider net in the small slot gets the
    // selection, the selected positions and the re-evaluation marks as launches of their own
    HIP_TRY(launch_classify(b, n, P, nsm.p, nbg.p, s));
    HIP_TRY(launch_eval_net(d.net[SMALL], b, nsm.p, n, osm.p, perm, swz, s, nullptr));
    HIP_TRY(launch_reeval(osm.p, nsm.p, n, P, nbg.p, s));
  } else if (mode != GN_MODE_BIG)
    HIP_TRY(launch_eval_net(d.net[SMALL], b, nullptr, n, osm.p, perm, swz, s, mode == GN_MODE_SMALL ? o.rows : nullptr,
                            mode == GN_MODE_FULL ? &P : nullptr, nsm.p, nbg.p));
  HIP_TRY(mark(&EvalEvents::small_done));
  if (mode != GN_MODE_SMALL)
    HIP_TRY(launch_eval_net(d.net[BIG], b, mode == GN_MODE_FULL ? nbg.p : nullptr, n, obg.p, perm, swz, s, o.rows));
  HIP_TRY(mark(&EvalEvents::big_done));
  HIP_TRY(launch_finalize(b, n, mode, osm.p, obg.p, nsm.p, nbg.p, P, d.tables.p, out, s, o.score, o.counts));
  HIP_TRY(mark(&EvalEvents::finalized));
  return GN_OK;
}

static Dev *slot(gn_ctx *ctx, int s) {
  if (!ctx || s < 0 || s >= (int)ctx->devs.size()) return nullptr;
  return ctx->devs[s].get();
}
// the lines calls' K
static int check_n_lines(int n_lines) {
  if (n_lines < 1 || n_lines > GN_MAX_LINES) return fail(GN_E_INVALID, "n_lines %d outside 1..%d", n_lines, GN_MAX_LINES);
  return GN_OK;
}
// ... and their leaf rule: the quiescent calls' depth
LeafRule LeafRule::quiesce(const gn_ctx *ctx, int depth) { return {QUIESCE, depth, ctx && ctx->quiesce_see}; }
// the context's piece values, as the exchange evaluation takes them
static SeeValues see_values(const gn_ctx *ctx) {
  SeeValues V;
  for (int i = 0; i < 5; ++i) V.v[i] = ctx->P.piece_value[i];
  return V;
}

static int check_leaf_rule(LeafRule rule) {
  if (rule.kind == LeafRule::QUIESCE && (rule.depth < 1 || rule.depth > GN_MAX_QUIESCE_DEPTH))
    return fail(GN_E_INVALID, "quiescence depth %d outside 1..%d", rule.depth, GN_MAX_QUIESCE_DEPTH);
  return GN_OK;
}

template <class F>
static void parallel_for(size_t n, size_t grain, F &&f) {
  unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  size_t chunks = std::min<size_t>(hw, (n + grain - 1) / std::max<size_t>(grain, 1));
  if (chunks <= 1) {
    f(0, n);
    return;
  }
  std::vector<std::thread> th;
  size_t per = (n + chunks - 1) / chunks;
  for (size_t c = 0; c < chunks; ++c) {
    size_t lo = c * per, hi = std::min(n, lo + per);
    if (lo < hi) th.emplace_back([=, &f] { f(lo, hi); });
  }
  for (auto &t : th) t.join();
}

// Block length of the chained walk for an n-parent expansion: GN_OPT_CHAIN, shortened
// (to >= 2) when the blocks would not fill the resident workgroups; 1 = off.
static int chain_len(const gn_ctx *ctx, Dev &d, size_t n) {
  if (!ctx->incremental || (ctx->chain >= -1 && ctx->chain <= 1) || !d.has[BIG] || !d.net[BIG].carry_slots)
    return 1;
  if (ctx->chain < 0) return -ctx->chain; // exact (tests)
  // keep >= 2048 blocks (8 per resident workgroup) when the batch allows
  size_t k = (size_t)ctx->chain;
  if ((n + k - 1) / k < 2048) k = std::max<size_t>(2, std::min(k, n / 2048));
  return (int)k;
}

// The big net's expansion (modes FULL / BIG) runs planned (stream.hip).
// (Round 2's pipeline of block ranges on two streams, range c + 1's child generation and plan
// under range c's row stream, took the same time as the serial order, 296 vs 259 + 19 + 15.5
// + 5 ms: the overlapped kernels slow the row stream by what they add; it was removed.)
static bool plan_path(const gn_ctx *ctx, const Dev &d, int mode) {
  return mode != GN_MODE_SMALL && ctx->incremental && d.has[BIG] &&
         (d.net[BIG].L1 == 3072 || d.net[BIG].L1 == 1024);
}

// finalize of the n parents and total children (their net outputs in the Dev buffers)
// (score_parents: the parents are positions with the score rule; the children are child records)
// (sliced: the big net's outputs are the sliced stream's partial sums, positions = parents then
// children, which finalize finishes itself)
static int finalize_all(gn_ctx *ctx, Dev &d, const gn_board *parents, const gn_board *children, int mode,
                        gn_eval *parent_out, gn_eval *child_out, size_t n, size_t total, hipStream_t s,
                        bool score_parents, bool sliced = false) {
  const gn_eval_params &P = ctx->P;
  const ExpSet &x = d.cur;
  const SlicedOut sc = {&d.net[BIG], d.part.p, x.pinfo.p, (uint64_t)(n + total), (uint64_t)n},
                  sp = {&d.net[BIG], d.part.p, x.pinfo.p, (uint64_t)(n + total), 0, x.offsets.p};
  // children from their parents as write_children unpacked them
  const bool fast = x.child_moves != nullptr;
  HIP_TRY(launch_finalize(children, total, mode, x.eb.osm.p, x.eb.obg.p, x.eb.nsm.p, x.eb.nbg.p, P, d.tables.p, child_out,
                          s, 0, nullptr, fast ? x.owner.p : nullptr, fast ? x.child_moves : nullptr,
                          fast ? x.unpacked.p : nullptr, sliced ? &sc : nullptr));
  if (parent_out) // the parents' legal-move counts are generate_children's
    HIP_TRY(launch_finalize(parents, n, mode, x.p_osm.p, x.p_obg.p, x.p_nsm.p, x.p_nbg.p, P, d.tables.p, parent_out, s,
                            score_parents ? 1 : 0, x.counts.p, nullptr, nullptr, nullptr, sliced ? &sp : nullptr));
  return GN_OK;
}

// The exclusive scan of counts[0, n] (counts[n] == 0) into offsets (the current set's temporary
// storage), and *total = offsets[n] read back: synchronous, the stream is idle on success.
static hipError_t scan_total(Dev &d, const uint64_t *counts, uint64_t *offsets, size_t n, hipStream_t s, uint64_t *total) {
  *total = 0;
  hipError_t e = exclusive_scan_u64(counts, offsets, n + 1, d.cur.scan_tmp.p, d.cur.scan_tmp.cap, s);
  if (e == hipSuccess) e = hipMemcpyAsync(total, offsets + n, sizeof(*total), hipMemcpyDeviceToHost, s);
  return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

// Legal-child count of n boards (a capacity query), synchronously.
static hipError_t count_children(Dev &d, const gn_board *parents, size_t n, hipStream_t s, size_t *total) {
  ExpSet &x = d.cur;
  hipError_t e;
  if ((e = x.counts.ensure(n + 1)) != hipSuccess || (e = x.offsets.ensure(n + 1)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(x.counts.p + n, 0, sizeof(uint64_t), s)) != hipSuccess) return e;
  if ((e = launch_count_children(parents, n, d.tables.p, x.counts.p, s)) != hipSuccess) return e;
  uint64_t t = 0;
  if ((e = scan_total(d, x.counts.p, x.offsets.p, n, s, &t)) != hipSuccess) return e;
  *total = (size_t)t;
  return hipSuccess;
}

// The marks of one timed expansion (gn_time_expand_device makes the stage times of them), each
// recorded by the function that reaches it: start by run_expansions; counted (count + scan),
// total_read (the host has the child count) and written by generate_children; classified ...
// finalized by expand_evaluate (stream_begun by a pipelined back half alone: the row stream's start
// behind its wait for the plan); scored (the score rule queued) by the timing call.
struct ExpEvents {
  hipEvent_t start, counted, total_read, written, classified, small_done, plan_done, stream_begun, stream_done, big_done,
      finalized, scored;
  hipError_t create(Events &from) {
    return from.make({&start, &counted, &total_read, &written, &classified, &small_done, &plan_done, &stream_begun,
                      &stream_done, &big_done, &finalized, &scored});
  }
};

// generate_children's optional arguments.
struct GenOpts {
  ExpEvents *ev = nullptr;            // records counted, total_read, written
  unsigned long long *rows = nullptr; // += FT rows by write_children's formula
  bool deltas = false;                // + each child's ChildDelta (the incremental evaluation's input)
  int chain_k = 1;                    // with deltas: block length of the chained walk (chain_len)
  bool plan = false;                  // with deltas: the big net runs planned (plan_path)
  // the planned big-net path reads no child board after this (finalize makes each child from its
  // unpacked parent and move), so library-internal child boards are not written
  bool skip_internal = false;
  bool trusted = false;    // the parents are the library's own boards (level 2's: level 1's children): no gate
  size_t limit = SIZE_MAX; // more children than this fail the call (GN_E_CAPACITY) before anything is written
};
// Child generation into d.cur: counts -> exclusive scan (offsets, n + 1) -> children boards
// (children_or_null, else the set's own) + moves (moves, else the set's own).  *total = children.
static int generate_children(Dev &d, const gn_board *parents, size_t n, gn_board *children_or_null, uint16_t *moves,
                             size_t *total, hipStream_t s, const GenOpts &o = {}) {
  ExpSet &x = d.cur;
  x.chain_k = o.deltas ? o.chain_k : 1;
  x.planned = o.deltas && o.plan;
  x.plan_geo = PlanGeometry{};
  if (x.planned) { // a stale error bit of an earlier expansion must not fail this one
    HIP_TRY(hipMemsetAsync(x.perr.p, 0, sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(x.pstat.p, 0, 3 * sizeof(unsigned long long), s));
  }
  if (x.chain_k > 1) HIP_TRY(d.nslot.ensure(n));
  HIP_TRY(x.counts.ensure(n + 1));
  HIP_TRY(x.offsets.ensure(n + 1));
  HIP_TRY(hipMemsetAsync(x.counts.p + n, 0, sizeof(uint64_t), s));
  if (x.planned) {
    HIP_TRY(d.ebound.ensure(n + 1));
    HIP_TRY(x.eoff.ensure(n + 1));
    HIP_TRY(hipMemsetAsync(d.ebound.p + n, 0, sizeof(uint64_t), s));
  }
  HIP_TRY(launch_count_children(parents, n, d.tables.p, x.counts.p, s, x.planned ? d.ebound.p : nullptr, o.trusted));
  HIP_TRY(exclusive_scan_u64(x.counts.p, x.offsets.p, n + 1, x.scan_tmp.p, x.scan_tmp.cap, s));
  if (x.planned) HIP_TRY(exclusive_scan_u64(d.ebound.p, x.eoff.p, n + 1, x.scan_tmp.p, x.scan_tmp.cap, s));
  if (o.ev) HIP_TRY(hipEventRecord(o.ev->counted, s));
  uint64_t t = 0;
  HIP_TRY(hipMemcpyAsync(&t, x.offsets.p + n, sizeof(t), hipMemcpyDeviceToHost, s));
  if (x.planned) HIP_TRY(hipMemcpyAsync(&x.etot, x.eoff.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *total = (size_t)t;
  if (t > o.limit) return fail(GN_E_CAPACITY, "%zu children exceed capacity %zu", (size_t)t, o.limit);
  if (o.ev) HIP_TRY(hipEventRecord(o.ev->total_read, s));
  gn_board *children = children_or_null;
  const bool skip_boards = !children_or_null && x.planned && o.skip_internal;
  if (!children && !skip_boards) {
    HIP_TRY(x.children.ensure(std::max<size_t>(t, 1)));
    children = x.children.p;
  }
  if (o.deltas) HIP_TRY(d.deltas.ensure(std::max<size_t>(t, 1)));
  HIP_TRY(x.owner.ensure(std::max<size_t>(t, 1)));
  HIP_TRY(x.unpacked.ensure(std::max<size_t>(n, 1)));
  if (!moves) {
    HIP_TRY(x.moves_tmp.ensure(std::max<size_t>(t, 1)));
    moves = x.moves_tmp.p;
  }
  x.child_moves = moves;
  if (t) {
    HIP_TRY(launch_write_children(parents, n, d.tables.p, x.offsets.p, 0, t, children, moves, x.owner.p,
                                  o.deltas ? d.deltas.p : nullptr, x.chain_k > 1 ? d.nslot.p : nullptr, x.chain_k,
                                  o.rows, s, x.unpacked.p, o.trusted));
  }
  if (o.ev) HIP_TRY(hipEventRecord(o.ev->written, s));
  return GN_OK;
}

// An expansion of n parents in mode whose children may number at most limit.
static GenOpts gen_opts(const gn_ctx *ctx, Dev &d, size_t n, int mode, size_t limit) {
  GenOpts g;
  g.deltas = ctx->incremental, g.chain_k = chain_len(ctx, d, n), g.plan = plan_path(ctx, d, mode);
  g.skip_internal = mode == GN_MODE_BIG, g.limit = limit;
  return g;
}

// expand_evaluate's optional arguments.
constexpr int EXP_FRONT = 1, EXP_BACK = 2;
struct EvalOpts {
  ExpEvents *ev = nullptr; // records classified ... finalized (EXP_FRONT: to plan_done; EXP_BACK: from stream_begun)
  unsigned long long *rows = nullptr; // += FT rows the row stream gathers
  // the parents are positions (the score rule's static part; callers run resolve_scores on them)
  // rather than child records (depth 2's level 2)
  bool score_parents = true;
  // EXP_FRONT (classify, the small net, the big net's plan) and / or EXP_BACK (the big net's row
  // stream, finalize); the expansion pipeline runs the two on different streams
  int phases = EXP_FRONT | EXP_BACK;
  hipEvent_t streamed = nullptr; // recorded after the stream launches (the pipeline's next front waits for it)
};
// Evaluate parents + children after generate_children (in d.cur).  Incremental: the
// expand_eval kernels (one workgroup per parent, children from the parent
// accumulators); otherwise every child is a full refresh (evaluate_on).
static int expand_evaluate(gn_ctx *ctx, Dev &d, const gn_board *parents, size_t n, const gn_board *children,
                           size_t total, int mode, gn_eval *parent_out, gn_eval *child_out, hipStream_t s,
                           const EvalOpts &o = {}) {
  if (mode < GN_MODE_FULL || mode > GN_MODE_SMALL) return fail(GN_E_INVALID, "bad mode %d", mode);
  if ((mode != GN_MODE_SMALL && !d.has[BIG]) || (mode != GN_MODE_BIG && !d.has[SMALL]))
    return fail(GN_E_NONET, "mode %d needs a network that is not loaded", mode);
  ExpSet &x = d.cur;
  const int phases = o.phases;
  if (!ctx->incremental) {
    if (!(phases & EXP_BACK)) return GN_OK; // (no front half: every child is a full refresh)
    EvalOnOpts as_children, as_parents;
    as_children.score = 0;
    as_parents.score = o.score_parents ? 1 : 0, as_parents.counts = x.counts.p;
    if (total) {
      int rc = evaluate_on(ctx, d, children, total, mode, child_out, s, as_children);
      if (rc) return rc;
    }
    return parent_out ? evaluate_on(ctx, d, parents, n, mode, parent_out, s, as_parents) : GN_OK;
  }
  auto mark = [&](hipEvent_t ExpEvents::*m) { return o.ev ? hipEventRecord(o.ev->*m, s) : hipSuccess; };
  const gn_eval_params &P = ctx->P;
  const uint64_t *off = x.offsets.p;
  const ChildDelta *dl = d.deltas.p;
  const bool f = mode == GN_MODE_FULL;
  const size_t K = (size_t)std::max(1, x.chain_k), nblk = (n + K - 1) / K;
  const bool ordered = ctx->king_sort && nblk > 1; // XCD-local block order
  // the planned big net: the plan's launch and the row stream's take the same arguments
  auto plan_args = [&] {
    PlanStreamArgs a;
    a.parents = parents, a.n = n, a.offsets = off, a.deltas = dl;
    a.need_parent = f ? x.p_nbg.p : nullptr, a.need_child = f ? x.eb.nbg.p : nullptr;
    a.out_parent = x.p_obg.p, a.out_child = x.eb.obg.p;
    a.next_slot = x.chain_k > 1 ? d.nslot.p : nullptr, a.chain_k = x.chain_k, a.kc = ctx->king_cache ? 1 : 0;
    a.eoff = x.eoff.p, a.ent = x.ent.p, a.tiles = x.tiles.p, a.btiles = x.btiles.p;
    a.pool = d.pool.p, a.err = x.perr.p, a.rows_out = o.rows, a.pads_out = x.pstat.p;
    a.slices = x.slices, a.npos = n + total;
    if (x.slices > 1) a.part = d.part.p, a.pinfo = x.pinfo.p;
    return a;
  };
  // ---- the front half: selections, the small net, the plan (the stream's lists and tiles)
  if (phases & EXP_FRONT) {
    const size_t nt = std::max<size_t>(total, 1);
    if (mode != GN_MODE_BIG) {
      HIP_TRY(x.eb.osm.ensure(nt));
      HIP_TRY(x.p_osm.ensure(n));
    }
    if (mode != GN_MODE_SMALL) {
      HIP_TRY(x.eb.obg.ensure(nt));
      HIP_TRY(x.p_obg.ensure(n));
    }
    if (f) {
      HIP_TRY(x.eb.nsm.ensure(nt));
      HIP_TRY(x.eb.nbg.ensure(nt));
      HIP_TRY(x.p_nsm.ensure(n));
      HIP_TRY(x.p_nbg.ensure(n));
      HIP_TRY(launch_classify(parents, n, P, x.p_nsm.p, x.p_nbg.p, s));
      HIP_TRY(launch_classify(children, total, P, x.eb.nsm.p, x.eb.nbg.p, s));
    }
    HIP_TRY(mark(&ExpEvents::classified));
    if (mode != GN_MODE_BIG) {
      HIP_TRY(launch_expand_net(d.net[SMALL], parents, n, off, children, dl, f ? x.p_nsm.p : nullptr,
                                f ? x.eb.nsm.p : nullptr, x.p_osm.p, x.eb.osm.p, ctx->swizzle & 1, s));
      if (f) {
        HIP_TRY(launch_reeval(x.p_osm.p, x.p_nsm.p, n, P, x.p_nbg.p, s));
        HIP_TRY(launch_reeval(x.eb.osm.p, x.eb.nsm.p, total, P, x.eb.nbg.p, s));
      }
    }
    HIP_TRY(mark(&ExpEvents::small_done));
    x.slices = 1;
    if (mode != GN_MODE_SMALL && x.planned) {
      HIP_TRY(x.ent.ensure(x.etot + (size_t)ENT_SPARE * (nblk + 1)));
      HIP_TRY(x.tiles.ensure((n + total) / 16 + (K + 2) * nblk + 2));
      HIP_TRY(x.btiles.ensure(nblk + 1));
      HIP_TRY(d.pool.ensure(88)); // 8 XCDs x 8 words of scratch-slot bits, then 8 block claim counters
      // the sliced stream's partial sums cost 152 B per position (include/gpu_nnue.h,
      // GN_OPT_STREAM_SLICES); when they do not fit, the whole-row stream gives the same results
      // (part_locked: a pipelined front, beside the back half of the previous expansion that reads
      // part -- it may not reallocate it; when it is too small this expansion streams whole rows)
      if (d.net[BIG].L1 == 3072 && ctx->stream_slices == 3) {
        const size_t need = (size_t)GN_PART_SLICES * GN_PART_DWORDS * (n + total);
        bool ok = d.part_locked ? d.part.cap >= need : d.part.ensure(need) == hipSuccess;
        ok = ok && x.pinfo.ensure(n + total) == hipSuccess;
        if (ok) x.slices = 3;
        else {
          (void)hipGetLastError(); // (the failed allocation's error is not the call's)
          if (!d.part_locked) d.part.release();
          x.pinfo.release();
        }
      }
      if (ordered) {
        HIP_TRY(d.bkeys.ensure(nblk));
        HIP_TRY(d.bkeys2.ensure(nblk));
        HIP_TRY(d.bidx.ensure(nblk));
        HIP_TRY(x.border.ensure(nblk));
        HIP_TRY(block_order(parents, n, (uint32_t)K, (uint32_t)nblk, d.bkeys.p, d.bidx.p, d.bkeys2.p, x.border.p,
                            x.sort_tmp.p, x.sort_tmp.cap, s));
      }
      HIP_TRY(launch_plan_stream(d.net[BIG], plan_args(), PLAN_PHASE, s));
      x.plan_geo = plan_geometry(d.net[BIG], plan_args());
      x.plan_n = n, x.plan_total = total, x.plan_ordered = ordered;
      HIP_TRY(mark(&ExpEvents::plan_done));
    }
  }
  if (!(phases & EXP_BACK)) return GN_OK;
  // ---- the back half: the big net's row stream, finalize
  // (the sliced stream's finish runs inside finalize)
  const bool sliced = mode != GN_MODE_SMALL && x.planned && x.slices > 1;
  if (mode != GN_MODE_SMALL) {
    if (x.planned) {
      HIP_TRY(hipMemsetAsync(d.pool.p, 0, 88 * sizeof(uint32_t), s)); // per stream launch (<= 3)
      if (!(phases & EXP_FRONT)) HIP_TRY(mark(&ExpEvents::stream_begun)); // (the pipeline: the stream's start)
      PlanStreamArgs a = plan_args();
      a.swz = (ctx->swizzle >> 2) & 1 ? 1 : (ctx->swizzle >> 3) & 1 ? 2 : 0;
      a.order = ordered ? x.border.p : nullptr;
      HIP_TRY(launch_plan_stream(d.net[BIG], a, STREAM_PHASE, s));
      HIP_TRY(mark(&ExpEvents::stream_done));
      if (o.streamed) HIP_TRY(hipEventRecord(o.streamed, s));
    } else { // a 128-wide net loaded as the big net
      HIP_TRY(launch_expand_net(d.net[BIG], parents, n, off, children, dl, f ? x.p_nbg.p : nullptr,
                                f ? x.eb.nbg.p : nullptr, x.p_obg.p, x.eb.obg.p, ctx->swizzle & 1, s));
    }
  }
  HIP_TRY(mark(&ExpEvents::big_done));
  int rc = finalize_all(ctx, d, parents, children, mode, parent_out, child_out, n, total, s, o.score_parents, sliced);
  if (rc) return rc;
  HIP_TRY(mark(&ExpEvents::finalized));
  return GN_OK;
}

// ---------------------------------------------------------- score rule ---
// The in-check part of the score rule (include/gpu_nnue.h, gn_eval.score): for every scored
// position of out[0, n) in check with a legal move (finalize set the rest), its legal
// replies are generated and evaluated as positions on the device, the replies in check
// are resolved one level down (depth 2 -> 1; at depth 0 a reply keeps its static value),
// and score_reduce_kernel takes the negamax over them.  sv_out (optional): the positions'
// rule values for the level above.  Synchronous (the selection's and the replies' counts
// size the next launches); a batch without such positions costs one select + scan.
// Stockfish has no static evaluation in check (Eval::evaluate asserts !checkers) and
// always prints a score from its search; fishnet requires one for every analysed
// position (/root/reference/src/stockfish.rs:366-368, src/ipc.rs:56).
// replies (optional, an expansion's parents): every position's legal replies are already
// evaluated (child records / moves at d.cur.offsets, the parents unpacked in d.cur.unpacked); they
// are reused instead of generated and evaluated again.
struct Replies {
  const gn_eval *rec;
  const uint16_t *moves;
};
static int resolve_scores(gn_ctx *ctx, Dev &d, const gn_board *boards, size_t n, int mode, gn_eval *out,
                          int32_t *sv_out, hipStream_t s, int depth = 2, const Replies *replies = nullptr) {
  if (!n || depth <= 0 || !out) return GN_OK;
  Dev::ScoreLevel &L = d.lv[2 - depth];
  HIP_TRY(L.sel.ensure(n + 1));
  HIP_TRY(L.pos.ensure(n + 1));
  HIP_TRY(launch_score_select(out, n, L.sel.p, s));
  uint64_t m = 0, t = 0; // the positions in check with a legal move, and their replies
  HIP_TRY(scan_total(d, L.sel.p, L.pos.p, n, s, &m));
  if (!m) return GN_OK;
  HIP_TRY(L.idx.ensure(m));
  HIP_TRY(L.boards.ensure(m));
  HIP_TRY(L.counts.ensure(m + 1));
  HIP_TRY(L.offsets.ensure(m + 1));
  HIP_TRY(launch_score_gather(boards, L.sel.p, L.pos.p, n, replies ? nullptr : d.tables.p, L.idx.p, L.boards.p, s));
  if (replies) {
    HIP_TRY(launch_score_replies(L.idx.p, m, d.cur.offsets.p, L.counts.p, L.offsets.p, d.cur.scan_tmp.p,
                                 d.cur.scan_tmp.cap, &t, s));
  } else {
    HIP_TRY(hipMemsetAsync(L.counts.p + m, 0, sizeof(uint64_t), s));
    HIP_TRY(launch_count_children(L.boards.p, m, d.tables.p, L.counts.p, s));
    HIP_TRY(scan_total(d, L.counts.p, L.offsets.p, m, s, &t));
  }
  const uint64_t cap = std::max<uint64_t>(t, 1);
  HIP_TRY(L.moves.ensure(cap));
  HIP_TRY(L.children.ensure(cap));
  HIP_TRY(L.ce.ensure(cap));
  HIP_TRY(L.sv.ensure(cap));
  if (replies) { // copied from the expansion's records
    HIP_TRY(launch_score_replies_fill(L.idx.p, m, d.cur.offsets.p, L.offsets.p, replies->rec, replies->moves,
                                      d.cur.unpacked.p, d.tables.p, L.ce.p, L.children.p, L.moves.p, s));
  } else { // generated and evaluated as positions
    HIP_TRY(L.owner.ensure(cap));
    HIP_TRY(launch_write_children(L.boards.p, m, d.tables.p, L.offsets.p, 0, t, L.children.p, L.moves.p, L.owner.p,
                                  nullptr, nullptr, 1, nullptr, s));
    if (int rc = evaluate_on(ctx, d, L.children.p, t, mode, L.ce.p, s)) return rc;
  }
  if (int rc = resolve_scores(ctx, d, L.children.p, t, mode, L.ce.p, L.sv.p, s, depth - 1)) return rc;
  HIP_TRY(launch_score_reduce(L.boards.p, m, L.idx.p, L.offsets.p, L.moves.p, L.ce.p, L.sv.p, ctx->P, out, sv_out, s));
  return GN_OK;
}

// --------------------------------------------------------- leaf stage ----
// The leaves of one expansion level: the children [offsets[i], offsets[i + 1]) of the n parents, their
// moves and records rec, total of them.  The parents are unpacked with 64-bit offsets, as
// write_children left them in the set, or packed with the C-ABI's 32-bit offsets.
template <class Parent, class Off>
struct Leaves {
  const Parent *parents;
  size_t n;
  const Off *offsets;
  const uint16_t *moves;
  const gn_eval *rec;
  size_t total;
};
using UnpackedLeaves = Leaves<Board, uint64_t>;
using PackedLeaves = Leaves<gn_board, uint32_t>;

// How the leaf stage reports a failed device allocation, which is the rule's.  The check extension
// fails with GN_E_HIP, as every other launch sequence does.  A quiescent call fails with GN_E_NOMEM,
// naming the two handles on its size, after it has given the stage's buffers back and cleared the
// HIP error (it is not a later call's).
struct LeafAlloc {
  Dev &d;
  LeafRule rule;
  int check(int level, size_t count, hipError_t e) const {
    if (e == hipSuccess) return GN_OK;
    if (rule.kind != LeafRule::QUIESCE)
      return fail(GN_E_HIP, "check extension: device allocation for %zu leaves failed: %s", count, hipGetErrorString(e));
    (void)hipGetLastError();
    d.leaf.release();
    return fail(GN_E_NOMEM,
                "quiescence: no device memory for level %d (%zu nodes); lower GN_OPT_CHUNK_PARENTS or depth (%d)", level,
                count, rule.depth);
  }
};
#define LEAF_ALLOC(level, count, expr) \
  do { if (int rc_ = alloc.check((level), (count), (expr))) return rc_; } while (0)

// CHECKS values the m selected leaves (d.leaf.boards -> d.leaf.sv) as positions: evaluate_on and
// resolve_scores with its sv output, as gn_evaluate_device runs them, on the stage's own records --
// resolve_scores rewrites what it is given, so it never sees the caller's.  A selected leaf without
// a legal move is no position in check with a move to the score rule: it stays GN_NOT_EXTENDED.
static int extend_checks(gn_ctx *ctx, Dev &d, size_t m, int mode, const LeafAlloc &alloc, hipStream_t s) {
  Dev::LeafStage &X = d.leaf;
  LEAF_ALLOC(0, m, X.rec.ensure(m));
  if (int rc = evaluate_on(ctx, d, X.boards.p, m, mode, X.rec.p, s)) return rc;
  return resolve_scores(ctx, d, X.boards.p, m, mode, X.rec.p, X.sv.p, s, 2);
}

// QUIESCE values them: sv[i] = Q(selected leaf i, depth), *nodes = the positions evaluated below.
// Level 0 are the m selected leaves; their statics are the caller's rec, through idx, and their
// searched-move counts the selection pass's, compacted.  Level k + 1 is made from level k's boards:
// the searched moves counted, scanned, the level's size read back, its boards written and evaluated
// as positions by evaluate_on (whose records carry the in-check and no-legal-move bits the rule
// needs).  Then one reduction per level, bottom-up.  A level of 2^31 nodes fails the call with
// GN_E_CAPACITY.  Every allocation goes through alloc, those of the scans and of evaluate_on
// included: they are reserved before the call that would make them.
// tail (the _pv calls; else NULL, and nothing below is allocated or launched): each level keeps its
// own moves instead of sharing X.moves, the reduction is quiesce_reduce_pv_kernel, which also leaves
// each node's chosen child, and quiesce_walk_kernel follows those from every selected leaf into
// tail (zeroed by the caller), between d.pev[0] and d.pev[1].
// see (the pruned rule; else NULL): the values the count and children launches prune by.
static int quiesce(gn_ctx *ctx, Dev &d, const gn_eval *rec, size_t total, size_t m, int mode, int depth,
                   const LeafAlloc &alloc, size_t *nodes, uint16_t *tail, hipStream_t s, const SeeValues *see) {
  Dev::LeafStage &X = d.leaf;
  // the levels, top-down: cnt[k] nodes at level k; top: the deepest level whose children were counted
  size_t cnt[GN_MAX_QUIESCE_DEPTH + 2] = {m};
  const gn_board *boards = X.boards.p;
  int top = depth - 1;
  for (int k = 0; k < depth; ++k) {
    Dev::LeafStage::Level &L = X.lv[k];
    LEAF_ALLOC(k, cnt[k], L.counts.ensure(cnt[k] + 1));
    LEAF_ALLOC(k, cnt[k], L.offsets.ensure(cnt[k] + 1));
    LEAF_ALLOC(k, cnt[k], reserve_scan_u64(cnt[k] + 1, d.cur.scan_tmp.p, d.cur.scan_tmp.cap));
    if (k) HIP_TRY(launch_quiesce_count(boards, cnt[k], d.tables.p, L.counts.p, s, see));
    else HIP_TRY(launch_quiesce_level0_counts(X.sel.p, X.pos.p, X.lcnt.p, total, L.counts.p, s)); // (counted by the selection)
    uint64_t t = 0;
    HIP_TRY(scan_total(d, L.counts.p, L.offsets.p, cnt[k], s, &t));
    if (t > 0x7FFFFFFFull)
      return fail(GN_E_CAPACITY,
                  "quiescence: level %d holds %llu nodes, the limit is 2^31 - 1; lower GN_OPT_CHUNK_PARENTS or depth (%d)",
                  k + 1, (unsigned long long)t, depth);
    cnt[k + 1] = (size_t)t;
    if (!t) { // no deeper level: every node of level k is valued by itself
      top = k;
      break;
    }
    Dev::LeafStage::Level &N = X.lv[k + 1];
    LEAF_ALLOC(k + 1, t, N.boards.ensure(t));
    LEAF_ALLOC(k + 1, t, N.rec.ensure(t));
    if (k + 1 < depth) LEAF_ALLOC(k + 1, t, N.val.ensure(t));
    if (tail) LEAF_ALLOC(k + 1, t, N.moves.ensure(t));
    else LEAF_ALLOC(k + 1, t, X.moves.ensure(t));
    uint16_t *const moves = tail ? N.moves.p : X.moves.p;
    LEAF_ALLOC(k + 1, t, X.owner.ensure(t));
    // (everything evaluate_on would allocate for the level: it then allocates nothing, so that no
    // allocation of the stage can fail as anything but GN_E_NOMEM)
    LEAF_ALLOC(k + 1, t, reserve_eval_outputs(d.cur.eb, t, mode));
    if (king_sorted(ctx, t)) LEAF_ALLOC(k + 1, t, reserve_king_sort_buffers(d, t, mode));
    HIP_TRY(launch_quiesce_children(boards, cnt[k], d.tables.p, L.offsets.p, t, moves, X.owner.p, N.boards.p, s, see));
    if (int rc = evaluate_on(ctx, d, N.boards.p, t, mode, N.rec.p, s)) return rc;
    *nodes += t;
    boards = N.boards.p;
  }
  // the reduction, bottom-up; level 0's records are the caller's, through idx
  for (int k = top; k >= 0; --k) {
    const size_t nc = cnt[k + 1];
    const bool last = k + 1 == depth || !nc; // the children are valued statically (or there are none)
    if (tail) {
      LEAF_ALLOC(k, cnt[k], X.lv[k].best.ensure(cnt[k]));
      HIP_TRY(launch_quiesce_reduce_pv(k ? X.lv[k].rec.p : rec, k ? nullptr : X.idx.p, cnt[k], X.lv[k].offsets.p, nc,
                                       nc ? X.lv[k + 1].rec.p : nullptr, last ? nullptr : X.lv[k + 1].val.p,
                                       nc ? X.lv[k + 1].moves.p : nullptr, k ? X.lv[k].val.p : X.sv.p, X.lv[k].best.p, s));
      continue;
    }
    HIP_TRY(launch_quiesce_reduce(k ? X.lv[k].rec.p : rec, k ? nullptr : X.idx.p, cnt[k], X.lv[k].offsets.p, nc,
                                  nc ? X.lv[k + 1].rec.p : nullptr, last ? nullptr : X.lv[k + 1].val.p,
                                  k ? X.lv[k].val.p : X.sv.p, s));
  }
  if (tail) {
    QuiescePvLevels P = {};
    P.levels = top + 1;
    for (int k = 0; k <= top; ++k) P.best[k] = X.lv[k].best.p, P.moves[k] = X.lv[k + 1].moves.p;
    for (int k = 0; k <= top + 1; ++k) P.cnt[k] = (uint32_t)cnt[k];
    HIP_TRY(hipEventRecord(d.pev[0], s));
    HIP_TRY(launch_quiesce_walk(P, X.idx.p, m, total, tail, s));
    HIP_TRY(hipEventRecord(d.pev[1], s));
  }
  return GN_OK;
}

// The leaf stage of one expansion level (include/gpu_nnue.h, gn_extend_checks_device and
// gn_quiesce_device): ext[j] = the rule's value of leaf j where the rule values it -- CHECKS:
// value(leaf j, 2) of the score rule where the leaf is in check with a legal move; QUIESCE:
// Q(leaf j, depth) where the leaf is searched, that is, has a legal move and is in check or has a
// noisy one -- and GN_NOT_EXTENDED elsewhere; *res = how many, and the positions evaluated below them.
// Level 0: the rule's kernel selects its leaves (the quiescence's makes each leaf's board and so also
// counts its searched moves) and writes GN_NOT_EXTENDED to all of ext; the selection is scanned, the
// count m read back, and the selected leaves' boards, indices and GN_NOT_EXTENDED values compacted
// (extend_boards_kernel).  The rule values them (extend_checks / quiesce); the values are scattered
// to ext and counted.  Synchronous: every buffer is sized from a read-back count before anything is
// queued on it, and the kernels clamp their offsets to those counts; the stream is idle on every
// return.  d.mu held, inside a sequence on s, no expansion in flight on d.cur.
// tail (QUIESCE alone; NULL: none): total * GN_MAX_QUIESCE_DEPTH entries, zeroed here, then the
// searched leaves' own variations (quiesce).
template <class Parent, class Off>
static int value_leaves(gn_ctx *ctx, Dev &d, const Leaves<Parent, Off> &lv, int mode, LeafRule rule, int32_t *ext,
                        uint16_t *tail, LeafCount *res, hipStream_t s) {
  *res = LeafCount{};
  if (int rc = check_leaf_rule(rule)) return rc;
  if (mode < GN_MODE_FULL || mode > GN_MODE_SMALL) return fail(GN_E_INVALID, "bad mode %d", mode);
  if ((mode != GN_MODE_SMALL && !d.has[BIG]) || (mode != GN_MODE_BIG && !d.has[SMALL]))
    return fail(GN_E_NONET, "mode %d needs a network that is not loaded", mode);
  if (!lv.total || !lv.n) return GN_OK;
  struct Idle { // a failed call too leaves the stream idle
    hipStream_t s;
    bool ok = false;
    ~Idle() { if (!ok) (void)hipStreamSynchronize(s); }
  } idle{s};
  const bool q = rule.kind == LeafRule::QUIESCE;
  const size_t total = lv.total;
  if (total > 0x7FFFFFFFull)
    return q ? fail(GN_E_CAPACITY, "quiescence: %zu leaves, a level holds < 2^31; lower GN_OPT_CHUNK_PARENTS (depth %d)",
                    total, rule.depth)
             : fail(GN_E_INVALID, "the check extension supports < 2^31 leaves per call");
  const LeafAlloc alloc{d, rule};
  const SeeValues values = see_values(ctx), *const see = q && rule.pruned ? &values : nullptr;
  Dev::LeafStage &X = d.leaf;
  if (tail) HIP_TRY(hipMemsetAsync(tail, 0, total * GN_MAX_QUIESCE_DEPTH * sizeof(uint16_t), s));
  LEAF_ALLOC(0, total, X.sel.ensure(total + 1));
  LEAF_ALLOC(0, total, X.pos.ensure(total + 1));
  if (q) {
    LEAF_ALLOC(0, total, X.lcnt.ensure(total));
    LEAF_ALLOC(0, total, reserve_scan_u64(total + 1, d.cur.scan_tmp.p, d.cur.scan_tmp.cap)); // (the scan then allocates nothing)
    HIP_TRY(hipMemsetAsync(X.sel.p, 0, (total + 1) * sizeof(uint64_t), s));
    HIP_TRY(launch_quiesce_select(lv.parents, lv.n, lv.offsets, lv.moves, total, d.tables.p, X.sel.p, X.lcnt.p, ext, s, see));
  } else {
    HIP_TRY(launch_extend_select(lv.rec, total, X.sel.p, ext, s));
  }
  uint64_t m = 0;
  HIP_TRY(scan_total(d, X.sel.p, X.pos.p, total, s, &m));
  if (m > total) return fail(GN_E_HIP, "leaf stage: %zu selected of %zu leaves", (size_t)m, total);
  size_t below = 0;
  unsigned long long valued = 0;
  if (m) {
    LEAF_ALLOC(0, m, X.idx.ensure(m));
    LEAF_ALLOC(0, m, X.boards.ensure(m));
    LEAF_ALLOC(0, m, X.sv.ensure(m));
    LEAF_ALLOC(0, m, X.count.ensure(1));
    HIP_TRY(launch_extend_boards(lv.parents, lv.n, lv.offsets, lv.moves, X.sel.p, X.pos.p, total, d.tables.p, X.idx.p,
                                 X.boards.p, X.sv.p, s));
    if (int rc = q ? quiesce(ctx, d, lv.rec, total, m, mode, rule.depth, alloc, &below, tail, s, see)
                   : extend_checks(ctx, d, m, mode, alloc, s))
      return rc;
    HIP_TRY(hipMemsetAsync(X.count.p, 0, sizeof(unsigned long long), s));
    HIP_TRY(launch_extend_scatter(X.idx.p, X.sv.p, m, ext, X.count.p, s));
    HIP_TRY(hipMemcpyAsync(&valued, X.count.p, sizeof(valued), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (tail) HIP_TRY(hipEventElapsedTime(&res->pv_ms, d.pev[0], d.pev[1]));
  }
  res->leaves = (size_t)valued, res->nodes = below;
  return idle.ok = true, GN_OK;
}
#undef LEAF_ALLOC

// ------------------------------------------------------- one level -------
// expand_level's optional arguments.
struct LevelOpts {
  gn_board *children = nullptr; // the caller's child boards (NULL: the set's own, library-internal)
  bool trusted = false;         // the parents are the library's own boards (GenOpts::trusted)
  // the parents are positions and get the score rule, from the replies this level evaluated; false:
  // they are child records (depth 2's level 2)
  bool score_parents = true;
  const char *what = "children"; // (the 32-bit offsets' message)
};
// One synchronous expansion level on stream s (gn_expand_device; both levels of expand2_on): the
// n parents' children generated (at most cap, else GN_E_CAPACITY with *total set and d_offsets
// written), d_offsets (n + 1) as 32-bit, parents and children evaluated, the parents' score rule,
// and the planned expansion's error word checked.  The stream is idle on return.
static int expand_level(gn_ctx *ctx, Dev &d, const gn_board *parents, size_t n, int mode, gn_eval *parent_out,
                        uint32_t *d_offsets, uint16_t *d_moves, gn_eval *child_out, size_t cap, size_t *total,
                        hipStream_t s, const LevelOpts &o = {}) {
  GenOpts g = gen_opts(ctx, d, n, mode, cap);
  g.trusted = o.trusted;
  size_t t = 0;
  int rc = generate_children(d, parents, n, o.children, d_moves, &t, s, g);
  *total = t;
  if (t > 0xFFFFFFFFull) return fail(GN_E_CAPACITY, "%zu %s exceed 32-bit offsets", t, o.what);
  HIP_TRY(launch_offsets_u32(d.cur.offsets.p, n + 1, d_offsets, s));
  if (rc) {
    HIP_TRY(hipStreamSynchronize(s));
    return rc;
  }
  EvalOpts e;
  e.score_parents = o.score_parents;
  if (d.cur.planned) e.rows = d.cur.pstat.p + 2; // (zeroed by generate_children)
  rc = expand_evaluate(ctx, d, parents, n, o.children ? o.children : d.cur.children.p, t, mode, parent_out, child_out, s,
                       e);
  const Replies rp{child_out, d_moves}; // the replies this level evaluated
  if (!rc && o.score_parents) rc = resolve_scores(ctx, d, parents, n, mode, parent_out, nullptr, s, 2, &rp);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return check_plan(d, s);
}

// ---------------------------------------------------------- sharding -----
// The one partitioner of the library and of bench.py / fishnet_amd/dist.py (through
// gn_partition): contiguous item ranges, cut so that shard k starts at the first item
// whose weight prefix reaches k/n_shards of the total (weights NULL: all 1, i.e. equal
// ranges).  Items are games (weight = positions) or parents (weight 1), so a game is
// never split and each device keeps a game's consecutive parents for the chained walk
// ("contiguous ranges of parents, game-aligned, per GPU"; the
// reference's analog is the worker fan-out, /root/reference/src/main.rs:151-161).
static void partition(const uint32_t *weights, size_t n, int ns, size_t *bounds) {
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) total += weights ? weights[i] : 1u;
  bounds[0] = 0;
  size_t i = 0;
  uint64_t acc = 0;
  for (int k = 1; k < ns; ++k) {
    const uint64_t target = (total * (uint64_t)k + (uint64_t)ns - 1) / (uint64_t)ns; // ceil(k * total / ns)
    while (i < n && acc < target) acc += weights ? weights[i++] : (++i, 1u);
    bounds[k] = i;
  }
  bounds[ns] = n;
}

// Runs f(k) for every device k on its own host thread (one device: inline); returns the first
// failing code with its message.
template <class F>
static int device_threads(gn_ctx *ctx, F &&f) {
  const size_t nd = ctx->devs.size();
  std::vector<int> rcs(nd, GN_OK);
  std::vector<std::string> errs(nd);
  auto work = [&](size_t k) {
    rcs[k] = f(k);
    if (rcs[k]) errs[k] = g_err;
  };
  if (nd == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (size_t k = 0; k < nd; ++k) th.emplace_back(work, k);
    for (auto &t : th) t.join();
  }
  for (size_t k = 0; k < nd; ++k)
    if (rcs[k]) {
      g_err = errs[k];
      return rcs[k];
    }
  return GN_OK;
}
// ... f(k, d) with device k's lock held.
template <class F>
static int for_each_device(gn_ctx *ctx, F &&f) {
  return device_threads(ctx, [&](size_t k) -> int {
    Dev &d = *ctx->devs[k];
    std::lock_guard<std::mutex> lk(d.mu);
    return f(k, d);
  });
}

// A FastBatch for nb positions in mode: buffers, pinned staging, the captured graph (d.mu held).
static int fast_build(gn_ctx *ctx, Dev &d, FastBatch &f, size_t nb, int mode) {
  // reply capacities: a lichess game has ~4 % of its positions in check with ~4 replies each (a
  // 128-position class: ~12 replies against 320); the evaluation is sized by the capacities, so a
  // smaller one is cheaper, and a batch beyond them reruns on the general path
  f.nb = nb, f.c1 = nb / 2 + 256, f.c2 = nb / 4 + 256, f.mode = mode, f.gen = ctx->graph_gen.load();
  const size_t na = nb + f.c1 + f.c2;
  HIP_TRY(hipEventCreateWithFlags(&f.done.h, hipEventDisableTiming));
  HIP_TRY(hipHostMalloc((void **)&f.h_in, nb * sizeof(gn_board), hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void **)&f.h_out, (nb + 1) * sizeof(gn_eval), hipHostMallocDefault));
  HIP_TRY(f.all.ensure(na));
  HIP_TRY(f.rec.ensure(na + 1));
  f.in = f.all.p, f.r1 = f.in + nb, f.r2 = f.r1 + f.c1;
  f.out = f.rec.p + 1, f.e1 = f.out + nb, f.e2 = f.e1 + f.c1;
  HIP_TRY(f.m1.ensure(f.c1));
  HIP_TRY(f.sv1.ensure(f.c1));
  HIP_TRY(f.m2.ensure(f.c2));
  HIP_TRY(f.sv2.ensure(f.c2));
  HIP_TRY(f.off0.ensure(nb + 1));
  HIP_TRY(f.off1.ensure(f.c1 + 1));
  HIP_TRY(f.eb.osm.ensure(na));
  HIP_TRY(f.eb.obg.ensure(na));
  HIP_TRY(f.eb.nsm.ensure(na));
  HIP_TRY(f.eb.nbg.ensure(na));
  const hipStream_t s = d.stream;
  uint32_t *flag = reinterpret_cast<uint32_t *>(f.rec.p);
  // (round 6: the big net on a graph branch of its own, beside the small net, measured slower --
  // p50 0.200 against 0.180 ms, the join's cross-queue wait costing more than the overlap gave)
  HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  auto seq = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(f.in, f.h_in, nb * sizeof(gn_board), hipMemcpyHostToDevice, s));
    // level 1: the replies of the in-check positions; level 2: those of the replies in check --
    // both from the boards alone (the selection is board properties), so that one evaluation
    // then covers the three levels (round 6: three evaluations, one per level, nine launches)
    HIP_TRY(launch_reply_level(f.in, nb, d.tables.p, f.off0.p, f.c1, f.r1, f.m1.p, flag, 1, s));
    HIP_TRY(launch_reply_level(f.r1, f.c1, d.tables.p, f.off1.p, f.c2, f.r2, f.m2.p, flag, 0, s));
    EvalOnOpts own; // the graph's own buffers, in the order given
    own.eb = &f.eb, own.sort = false;
    int rc = evaluate_on(ctx, d, f.all.p, na, mode, f.out, s, own);
    if (rc) return rc;
    HIP_TRY(launch_score_reduce2(f.r1, f.c1, f.off1.p, f.m2.p, f.e2, f.sv2.p, f.e1, f.sv1.p, f.in, nb, f.off0.p, f.m1.p,
                                 ctx->P, f.out, s));
    HIP_TRY(hipMemcpyAsync(f.h_out, f.rec.p, (nb + 1) * sizeof(gn_eval), hipMemcpyDeviceToHost, s));
    return GN_OK;
  };
  const int rc = seq();
  const hipError_t ec = hipStreamEndCapture(s, &f.graph.h); // (a failed sequence's graph goes with f)
  if (rc) return rc;
  HIP_TRY(ec);
  HIP_TRY(hipGraphInstantiate(&f.exec.h, f.graph, nullptr, nullptr, 0));
  return GN_OK;
}

// One small batch through its graph (one device; lk holds d.mu, released while the launch runs).
// *done = false: a reply level overflowed and nothing was written (the caller runs the general
// path).  With both instances of the class in flight, the call waits for one.
static int fast_run(gn_ctx *ctx, Dev &d, std::unique_lock<std::mutex> &lk, const gn_board *boards, size_t n, int mode,
                    gn_eval *out, bool *done) {
  *done = false;
  size_t nb = FAST_NB0;
  int k = 0;
  while (nb < n) nb <<= 1, ++k;
  auto &inst = d.fast[k][mode];
  auto busy = [&](int i) { return inst[i] && inst[i]->busy; };
  while (busy(0) && busy(1)) d.fast_cv.wait(lk);
  std::unique_ptr<FastBatch> &fp = inst[busy(0) ? 1 : 0];
  HIP_TRY(hipSetDevice(d.id));
  if (!fp || fp->gen != ctx->graph_gen.load()) {
    if (fp) HIP_TRY(hipEventSynchronize(fp->done)); // (its last launch is done: the call waited for it)
    fp.reset(new FastBatch());
    const int rc = fast_build(ctx, d, *fp, nb, mode);
    if (rc) {
      fp.reset();
      return rc;
    }
  }
  FastBatch &f = *fp;
  memcpy(f.h_in, boards, n * sizeof(gn_board));
  if (nb > n) memset(f.h_in + n, 0, (nb - n) * sizeof(gn_board));
  {
    SeqGuard sg(d, d.stream);
    HIP_TRY(sg.e);
    HIP_TRY(hipGraphLaunch(f.exec, d.stream));
    HIP_TRY(hipEventRecord(f.done, d.stream));
  }
  // wait without the device's lock: another call's launch queues behind this one meanwhile
  f.busy = true;
  lk.unlock();
  const hipError_t e = hipEventSynchronize(f.done);
  uint32_t flag = 1;
  if (e == hipSuccess) {
    memcpy(&flag, f.h_out, sizeof(flag));
    if (!flag) memcpy(out, f.h_out + 1, n * sizeof(gn_eval));
  }
  lk.lock();
  f.busy = false;
  d.fast_cv.notify_all();
  HIP_TRY(e);
  ++ctx->fast_runs;
  if (flag) {
    ++ctx->fast_fallbacks;
    return GN_OK;
  }
  *done = true;
  return GN_OK;
}

// Host boards -> device(s) -> gn_eval: contiguous shards, one host thread per device.
static int evaluate_boards_host(gn_ctx *ctx, const gn_board *boards, size_t n, int mode, gn_eval *out) {
  if (!n) return GN_OK;
  // (the graphs are built for the 128-wide small net's in-launch selection: a context with a wider net
  // in the small slot takes the general path)
  const bool small_ok = !ctx->devs.empty() && (!ctx->devs[0]->has[SMALL] || ctx->devs[0]->net[SMALL].L1 == 128);
  if (ctx->fast_batch && n <= FAST_MAX && ctx->devs.size() == 1 && small_ok && mode >= GN_MODE_FULL &&
      mode <= GN_MODE_SMALL) {
    Dev &d = *ctx->devs[0];
    std::unique_lock<std::mutex> lk(d.mu);
    bool done = false;
    const int rc = guarded([&]() -> int { return fast_run(ctx, d, lk, boards, n, mode, out, &done); });
    if (rc || done) return rc;
  }
  return guarded([&]() -> int {
    std::vector<size_t> b(ctx->devs.size() + 1);
    partition(nullptr, n, (int)ctx->devs.size(), b.data());
    return for_each_device(ctx, [&](size_t k, Dev &d) -> int {
      const size_t lo = b[k], hi = b[k + 1];
      if (lo >= hi) return GN_OK;
      HIP_TRY(hipSetDevice(d.id));
      SeqGuard sg(d, d.stream);
      HIP_TRY(sg.e);
      HIP_TRY(d.io_boards.ensure(hi - lo));
      HIP_TRY(d.io_out.ensure(hi - lo));
      HIP_TRY(hipMemcpyAsync(d.io_boards.p, boards + lo, (hi - lo) * sizeof(gn_board), hipMemcpyHostToDevice,
                             d.stream));
      int r = evaluate_on(ctx, d, d.io_boards.p, hi - lo, mode, d.io_out.p, d.stream);
      if (!r) r = resolve_scores(ctx, d, d.io_boards.p, hi - lo, mode, d.io_out.p, nullptr, d.stream);
      if (r) return r;
      HIP_TRY(hipMemcpyAsync(out + lo, d.io_out.p, (hi - lo) * sizeof(gn_eval), hipMemcpyDeviceToHost, d.stream));
      HIP_TRY(hipStreamSynchronize(d.stream));
      return GN_OK;
    });
  });
}

// Concurrent gn_evaluate_batch calls merged into one launch (group commit): a call queues
// itself; when no launch is running it leads one over every queued call of its mode (its own
// included), and the calls that queue meanwhile form the next launch.  A lone caller leads at
// once, so nothing waits on a timer.  fishnet's worker pool calls the evaluator once per chunk
// from N workers (/root/reference/src/main.rs:151-161, 263-343), so under load N small calls
// share one set of kernel launches and host round trips instead of N serialised ones.
// Results are those of separate calls (positions are independent).
static int evaluate_coalesced(gn_ctx *ctx, const gn_board *boards, size_t n, int mode, gn_eval *out) {
  if (!ctx->coalesce) return evaluate_boards_host(ctx, boards, n, mode, out);
  auto &C = ctx->co;
  BatchReq me{boards, n, mode, out};
  std::unique_lock<std::mutex> lk(C.mu);
  if (const int rc = guarded([&]() -> int { return C.q.push_back(&me), GN_OK; })) return rc;
  // every exit (an exception included) takes this call's request off the queue, so that no
  // later leader touches it after this stack frame is gone
  struct Dequeue {
    decltype(C) &c;
    BatchReq *me;
    ~Dequeue() {
      for (size_t i = 0; i < c.q.size(); ++i)
        if (c.q[i] == me) {
          c.q.erase(c.q.begin() + (ptrdiff_t)i);
          break;
        }
    }
  } dq{C, &me};
  while (!me.done) {
    if (me.taken || C.active >= MAX_LEADERS) {
      C.cv.wait(lk);
      continue;
    }
    // the queue is split before the context is marked busy: an allocation failure here leaves
    // the context free and this call off the queue (Dequeue)
    std::vector<BatchReq *> mine, rest;
    if (const int rc = guarded([&]() -> int { return mine.reserve(C.q.size()), rest.reserve(C.q.size()), GN_OK; }))
      return rc;
    for (BatchReq *r : C.q) (r->mode == mode ? mine : rest).push_back(r);
    C.q.swap(rest);
    for (BatchReq *r : mine) r->taken = true;
    ++C.active;
    lk.unlock();
    // from here to the re-lock nothing may throw outside the fence: this launch is counted in
    // C.active and only this thread takes it out
    char err[256] = "";
    const int rc = guarded([&]() -> int {
      if (mine.size() == 1) // (this call's own request: it was queued and not taken)
        return evaluate_boards_host(ctx, mine[0]->boards, mine[0]->n, mode, mine[0]->out);
      size_t tot = 0;
      for (BatchReq *r : mine) tot += r->n;
      std::vector<gn_board> all(tot);
      std::vector<gn_eval> res(tot);
      size_t at = 0;
      for (BatchReq *r : mine) std::copy(r->boards, r->boards + r->n, all.begin() + at), at += r->n;
      const int r0 = evaluate_boards_host(ctx, all.data(), tot, mode, res.data());
      at = 0;
      if (r0 == GN_OK)
        for (BatchReq *r : mine) std::copy(res.begin() + at, res.begin() + at + r->n, r->out), at += r->n;
      return r0;
    });
    if (rc) snprintf(err, sizeof err, "%s", g_err.c_str());
    lk.lock();
    for (BatchReq *r : mine) r->rc = rc, memcpy(r->err, err, sizeof err), r->done = true;
    ++C.launches, C.calls += mine.size();
    --C.active;
    C.cv.notify_all();
  }
  const int rc = me.rc;
  if (rc) {
    try {
      g_err = me.err;
    } catch (...) {
    }
  }
  return rc;
}

// ------------------------------------------------------ host pipeline ----
// The host-buffer expansion (gn_expand_and_evaluate, gn_evaluate_games with children),
// sharded over the context's devices: shard k's parents are resident on its device (uploaded
// boards, or the lichess replay's output); pass 1 counts every shard's children so that each
// shard knows where its children go in the caller's arrays; pass 2 expands a shard in chunks
// of whole games, and a drain thread downloads chunk c's records on the device's copy
// stream while chunk c + 1 computes (two slots of device output buffers).
using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t).count();
}

// The leaf stage (value_leaves) as a stage of a host-buffer call: its host time (the stage blocks)
// and its counts are added to the device's statistics of the rule's kind, whatever it returns.
template <class Parent, class Off>
static int extend_stage(gn_ctx *ctx, Dev &d, const Leaves<Parent, Off> &lv, int mode, LeafRule rule, int32_t *ext,
                        uint16_t *tail, hipStream_t s) {
  const auto t0 = Clock::now();
  LeafCount c;
  const int rc = value_leaves(ctx, d, lv, mode, rule, ext, tail, &c, s);
  Dev::LeafStage::Stats &st = d.leaf.stats[rule.kind];
  st.ms += ms_since(t0), st.leaves += c.leaves, st.nodes += c.nodes;
  d.t_pv += c.pv_ms;
  return rc;
}

// Every device lock, in slot order: a host-buffer call holds them all from here to its return.
static std::vector<std::unique_lock<std::mutex>> lock_devices(gn_ctx *ctx) {
  std::vector<std::unique_lock<std::mutex>> locks;
  for (auto &dp : ctx->devs) locks.emplace_back(dp->mu);
  return locks;
}

// One phase of a host-buffer call: f(k, d) on every device k that busy(k) names, one host thread
// per device (one device: inline), the caller holding every device lock (lock_devices).  f runs
// with its device current and inside one launch sequence on d.stream; the first failure's code
// and message.
template <class Busy, class F>
static int run_devices(gn_ctx *ctx, Busy &&busy, F &&f) {
  return device_threads(ctx, [&](size_t k) -> int {
    if (!busy(k)) return GN_OK;
    return guarded([&]() -> int {
      Dev &d = *ctx->devs[k];
      HIP_TRY(hipSetDevice(d.id));
      SeqGuard sg(d, d.stream);
      HIP_TRY(sg.e);
      return f(k, d);
    });
  });
}
// ... by item range: f(k, d, lo, hi) on every device k whose shard [b[k], b[k + 1]) is not empty.
template <class F>
static int run_shards(gn_ctx *ctx, const std::vector<size_t> &b, F &&f) {
  return run_devices(
      ctx, [&](size_t k) { return b[k] < b[k + 1]; },
      [&](size_t k, Dev &d) -> int { return f(k, d, b[k], b[k + 1]); });
}

static void reset_host_stats(gn_ctx *ctx) {
  for (auto &dp : ctx->devs) {
    dp->t_upload = dp->t_replay = dp->t_compute = dp->t_download = dp->t_tail = dp->t_rank = dp->t_rank2 = dp->t_rank3 = dp->t_keys = dp->t_pv = 0;
    for (auto &st : dp->leaf.stats) st = {};
  }
}

// Chunk bounds of a shard's m parents: cut only where `starts` allows (the first parent of each
// game, ascending; empty: anywhere), each chunk >= target parents; {0, ..., m}.
static std::vector<size_t> chunk_bounds(size_t m, const std::vector<size_t> &starts, size_t target) {
  std::vector<size_t> c{0};
  size_t j = 0;
  while (c.back() < m) {
    const size_t want = c.back() + std::max<size_t>(target, 1);
    if (want >= m) break;
    if (starts.empty()) {
      c.push_back(want);
      continue;
    }
    while (j < starts.size() && starts[j] < want) ++j;
    if (j == starts.size() || starts[j] >= m) break;
    c.push_back(starts[j]);
  }
  c.push_back(m);
  return c;
}

// The chunks of a shard's m parents for the pipeline below, cut only at `starts` (game starts;
// empty: anywhere).  opt > 0 (GN_OPT_CHUNK_PARENTS): chunks of >= opt parents.  Automatic: each
// chunk costs a fixed few ms (the row stream's and the plan's last blocks run on a part-idle
// GPU, and the chunk's launches and syncs), and only the last chunk's download is not
// overlapped, so: a shard below 3 x MIN parents is one chunk (MIN = 2,048 games of 81 parents,
// the least that keeps chain_len's full block length); otherwise a short last chunk of
// max(MIN, m / 8) parents after chunks of <= 2 M parents (round 3 cut eight equal chunks: 35 ms
// of per-chunk tails per 4 M parents).
static std::vector<size_t> chunk_plan(size_t m, const std::vector<size_t> &starts, int64_t opt) {
  if (opt > 0) return chunk_bounds(m, starts, (size_t)opt);
  constexpr size_t MIN = (size_t)2048 * 81, BIG = 2000000;
  if (m < 3 * MIN) return {0, m};
  const size_t last = std::max(MIN, m / 8), rest = m - last, k = (rest + BIG - 1) / BIG;
  std::vector<size_t> c{0};
  for (size_t i = 1; i <= k; ++i) {
    size_t x = rest * i / k; // a cut wanted here, moved to the next game start
    if (!starts.empty()) {
      auto it = std::lower_bound(starts.begin(), starts.end(), x);
      x = it == starts.end() ? m : *it;
    }
    if (x > c.back() && x < m) c.push_back(x);
  }
  c.push_back(m);
  return c;
}

// Pass 1 of a shard: its m device-resident parents' child offsets (m + 1, relative) to the host.
static int count_shard(Dev &d, const gn_board *d_par, size_t m, std::vector<uint64_t> &off) {
  size_t total = 0;
  HIP_TRY(count_children(d, d_par, m, d.stream, &total));
  off.resize(m + 1);
  HIP_TRY(hipMemcpy(off.data(), d.cur.offsets.p, (m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return GN_OK;
}

// ---- a sequence of expansions (the host-buffer calls' chunks, gn_time_expand_device's iterations)
// One expansion of the sequence, as its caller describes it.
struct ExpStep {
  const gn_board *parents = nullptr;
  size_t n = 0;
  gn_eval *parent_out = nullptr, *child_out = nullptr; // (NULL: the device's io_out / io_out2)
  uint16_t *moves = nullptr; // the children's moves (NULL: the buffer set's own)
  size_t cap = SIZE_MAX;     // more children than this fail the call (GN_E_CAPACITY)
  ExpEvents *ev = nullptr; // the expansion's marks (a timed one)
  // 2 row counters (optional): [0] += rows by write_children's formula, when no planned row stream
  // counts them (a per-wave atomic over every child would sit in a timed region), [1] += rows the
  // row stream gathered
  unsigned long long *rows = nullptr;
};
// GN_OPT_EXPAND_PIPELINE: expansion i + 1's front half (children, classify, small net, plan) runs
// on the device's second stream, in the other buffer set, while expansion i's back half runs.
static bool pipelined(const gn_ctx *ctx, const Dev &d, int mode, size_t count) {
  return ctx->pipeline && plan_path(ctx, d, mode) && ctx->incremental && count > 1;
}
// Expansions 0 .. count - 1 on d (d.mu held, inside a sequence on d.stream), serial or pipelined.
// step(i, ExpStep &) describes expansion i just before its front half is queued; done(i, total)
// runs after its score rule is queued on d.stream, d.cur being expansion i's set (it stays the
// last expansion's on return; pipelined, d.alt is then the one before's).  largest (optional):
// parents + children of the largest step, for which the sliced stream's partial sums are sized
// before any front runs (otherwise step 0's front sizes them): a later front runs beside a back
// half that reads them and may not reallocate them (part_locked).
// serial: one after another whatever GN_OPT_EXPAND_PIPELINE says (done runs a blocking stage of its
// own on the device's shared buffers: the one-ply extended games call).
template <class Step, class Done>
static int run_expansions(gn_ctx *ctx, Dev &d, int mode, size_t count, size_t largest, Step &&step, Done &&done,
                          bool serial = false) {
  if (!count) return GN_OK;
  const hipStream_t s = d.stream;
  const bool pipe = !serial && pipelined(ctx, d, mode, count);
  const hipStream_t F = pipe ? d.front : s; // the front halves' stream
  struct Guard { // on every way out: nothing of a failed call's front may still run
    Dev &d;
    bool pipe, ok = false;
    ~Guard() {
      d.part_locked = false;
      if (pipe && !ok) (void)hipStreamSynchronize(d.front);
    }
  } guard{d, pipe};
  struct Queued { // expansion i, from its front to its done, in q[i & 1]
    ExpStep st;
    size_t total = 0;
    gn_eval *po = nullptr, *co = nullptr;
  } q[2];
  auto front = [&](size_t i) -> int { // into d.cur
    Queued &x = q[i & 1];
    x = Queued();
    int rc = step(i, x.st);
    if (rc) return rc;
    const ExpStep &st = x.st;
    if (st.ev) HIP_TRY(hipEventRecord(st.ev->start, F));
    GenOpts g = gen_opts(ctx, d, st.n, mode, st.cap);
    g.ev = st.ev, g.rows = g.plan ? nullptr : st.rows;
    if ((rc = generate_children(d, st.parents, st.n, nullptr, st.moves, &x.total, F, g)) != GN_OK) return rc;
    if (!st.parent_out) HIP_TRY(d.io_out.ensure(st.n));
    if (!st.child_out) HIP_TRY(d.io_out2.ensure(std::max<size_t>(x.total, 1)));
    x.po = st.parent_out ? st.parent_out : d.io_out.p, x.co = st.child_out ? st.child_out : d.io_out2.p;
    if (!pipe) return GN_OK; // (serial: the back half evaluates both phases)
    EvalOpts e;
    e.ev = st.ev, e.rows = st.rows ? st.rows + 1 : nullptr, e.phases = EXP_FRONT;
    rc = expand_evaluate(ctx, d, st.parents, st.n, d.cur.children.p, x.total, mode, nullptr, nullptr, F, e);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(d.ev_planned, F));
    return GN_OK;
  };
  // the next front overwrites the other set: after this row stream, which reads the plan's lists
  // there (GN_OPT_EXPAND_PIPELINE 1), or beside it (2: the lists are per set), after the score
  // rule of the expansion that last used that set
  auto next_front = [&](size_t i) -> int {
    swap_sets(d);
    int rc = GN_OK;
    if (hipStreamWaitEvent(F, ctx->pipeline == 2 ? d.cur.scored : d.ev_streamed, 0) != hipSuccess)
      rc = fail(GN_E_HIP, "hipStreamWaitEvent failed");
    if (!rc) rc = front(i);
    swap_sets(d);
    return rc;
  };
  if (pipe) {
    HIP_TRY(hipEventRecord(d.ev_streamed, s)); // the front starts after what the device stream holds
    HIP_TRY(hipStreamWaitEvent(F, d.ev_streamed, 0));
    if (largest) {
      if (d.has[BIG] && d.net[BIG].L1 == 3072 && ctx->stream_slices == 3 &&
          d.part.ensure((size_t)GN_PART_SLICES * GN_PART_DWORDS * largest) != hipSuccess)
        (void)hipGetLastError(); // (then the steps that do not fit stream whole rows)
      d.part_locked = true;
    }
  }
  int rc = front(0);
  d.part_locked = pipe;
  for (size_t i = 0; i < count && rc == GN_OK; ++i) {
    const Queued &x = q[i & 1];
    const bool more = i + 1 < count;
    EvalOpts e; // d.cur's row stream and finalize
    e.ev = x.st.ev, e.rows = x.st.rows ? x.st.rows + 1 : nullptr;
    if (pipe) {
      HIP_TRY(hipStreamWaitEvent(s, d.ev_planned, 0));
      e.phases = EXP_BACK, e.streamed = d.ev_streamed;
    }
    rc = expand_evaluate(ctx, d, x.st.parents, x.st.n, d.cur.children.p, x.total, mode, x.po, x.co, s, e);
    if (rc || (pipe && more && (rc = next_front(i + 1)) != GN_OK)) return rc;
    const Replies rp{x.co, d.cur.child_moves}; // the replies this expansion evaluated
    if ((rc = resolve_scores(ctx, d, x.st.parents, x.st.n, mode, x.po, nullptr, s, 2, &rp)) != GN_OK) return rc;
    if (pipe) HIP_TRY(hipEventRecord(d.cur.scored, s));
    rc = done(i, x.total);
    if (rc || !more) break;
    if (pipe) swap_sets(d);
    else rc = front(i + 1);
  }
  guard.ok = rc == GN_OK;
  return rc;
}

// Where a shard's results go (expand_pipelined), each pointer at the shard's base: parent_out[0, m)
// (optional) and child_moves / child_out[0, off[m]); or, n_lines > 0 (gn_evaluate_games_lines), no
// child reaches the host: each chunk's children are ranked on the device and lines[0, m * n_lines)
// receives n_lines lines per parent.
constexpr RankHistory NO_HISTORY = {nullptr, 0, nullptr}; // (hist NULL: the plain ranking)
struct ExpandOut {
  gn_eval *parent_out = nullptr;
  uint16_t *child_moves = nullptr;
  gn_child *child_out = nullptr;
  int n_lines = 0;
  gn_line *lines = nullptr;
  // gn_evaluate_games_lines_history: the shard's keys (device, n_keys of them) and one gn_history per
  // parent of the shard (device; chunk c's at hist + chunks[c]); hist NULL: the plain ranking
  RankHistory history = NO_HISTORY;
  // gn_evaluate_games_lines_extended / _quiescent: each chunk's children are valued by the rule
  // before the ranking (extend_stage), and the chunks run one after another
  LeafRule leaf;
  // the _pv calls: pvs[0, m * n_lines) receives each line's gn_pv (the quiescence leaves its tails,
  // and the PVs are assembled on the device and downloaded with the chunk's lines); NULL: none
  gn_pv *pvs = nullptr;
};
// Pass 2 of a shard (see above).  off: the shard's child offsets from pass 1.
static int expand_pipelined(gn_ctx *ctx, Dev &d, const gn_board *d_par, size_t m, int mode,
                            const std::vector<uint64_t> &off, const std::vector<size_t> &chunks, const ExpandOut &o) {
  const int n_lines = o.n_lines;
  hipStream_t s = d.stream;
  size_t maxp = 1, maxc = 1;
  for (size_t c = 0; c + 1 < chunks.size(); ++c)
    maxp = std::max(maxp, chunks[c + 1] - chunks[c]),
    maxc = std::max<size_t>(maxc, off[chunks[c + 1]] - off[chunks[c]]);
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(d.po2[k].ensure(maxp));
    HIP_TRY(d.co2[k].ensure(maxc));
    if (n_lines) HIP_TRY(d.ln2[k].ensure(maxp * (size_t)n_lines));
    else HIP_TRY(d.cc2[k].ensure(maxc));
    if (o.leaf.extends()) HIP_TRY(d.leaf.ext.ensure(maxc));
    if (o.pvs) HIP_TRY(d.pv2[k].ensure(maxp * (size_t)n_lines));
    if (o.pvs) HIP_TRY(d.leaf.tail.ensure(maxc * GN_MAX_QUIESCE_DEPTH));
    HIP_TRY(d.mv2[k].ensure(maxc));
  }
  int drc[2] = {GN_OK, GN_OK};
  std::string derr[2];
  double dms[2] = {0, 0};
  std::thread drain[2];
  struct Joiner { // joins the drain threads on every way out (an exception included), before
    std::thread *t; // the state they write goes out of scope
    ~Joiner() {
      for (int i = 0; i < 2; ++i)
        if (t[i].joinable()) t[i].join();
    }
  } joiner{drain};
  auto join = [&](int k) -> int {
    if (drain[k].joinable()) drain[k].join();
    d.t_download += dms[k], dms[k] = 0;
    if (!drc[k]) return GN_OK;
    const int r = drc[k];
    drc[k] = GN_OK;
    g_err = derr[k];
    return r;
  };
  auto drain_chunk = [&](int k, size_t pa, size_t mp, size_t t, uint64_t cb) {
    drain[k] = std::thread([&, k, pa, mp, t, cb] {
      const auto t1 = Clock::now();
      hipError_t e = hipSetDevice(d.id);
      if (e == hipSuccess) e = hipStreamWaitEvent(d.copy, d.cev[k], 0);
      if (e == hipSuccess && n_lines)
        e = hipMemcpyAsync(o.lines + pa * (size_t)n_lines, d.ln2[k].p, mp * (size_t)n_lines * sizeof(gn_line),
                           hipMemcpyDeviceToHost, d.copy);
      if (e == hipSuccess && n_lines && o.pvs)
        e = hipMemcpyAsync(o.pvs + pa * (size_t)n_lines, d.pv2[k].p, mp * (size_t)n_lines * sizeof(gn_pv),
                           hipMemcpyDeviceToHost, d.copy);
      if (e == hipSuccess && t && !n_lines)
        e = hipMemcpyAsync(o.child_out + cb, d.cc2[k].p, t * sizeof(gn_child), hipMemcpyDeviceToHost, d.copy);
      if (e == hipSuccess && t && !n_lines)
        e = hipMemcpyAsync(o.child_moves + cb, d.mv2[k].p, t * sizeof(uint16_t), hipMemcpyDeviceToHost, d.copy);
      if (e == hipSuccess && o.parent_out)
        e = hipMemcpyAsync(o.parent_out + pa, d.po2[k].p, mp * sizeof(gn_eval), hipMemcpyDeviceToHost, d.copy);
      if (e == hipSuccess) e = hipStreamSynchronize(d.copy);
      if (e != hipSuccess) drc[k] = GN_E_HIP, derr[k] = std::string("result download failed: ") + hipGetErrorString(e);
      dms[k] = ms_since(t1);
    });
  };
  // chunk c computes into slot c & 1, which a drain thread then downloads on the copy stream while
  // the next chunk computes (t_compute: from one chunk's completion to the next's, less the waits
  // for a slot's download)
  auto t0 = Clock::now();
  int rc = run_expansions(
      ctx, d, mode, chunks.size() - 1, maxp + maxc,
      [&](size_t c, ExpStep &st) -> int {
        const int k = (int)(c & 1);
        const auto tj = Clock::now();
        const int r = join(k); // the slot's previous chunk is downloaded
        t0 += Clock::now() - tj;
        st.parents = d_par + chunks[c], st.n = chunks[c + 1] - chunks[c];
        st.parent_out = d.po2[k].p, st.child_out = d.co2[k].p, st.moves = d.mv2[k].p, st.cap = d.mv2[k].cap;
        return r;
      },
      [&](size_t c, size_t t) -> int {
        const int k = (int)(c & 1);
        const size_t pa = chunks[c], mp = chunks[c + 1] - pa;
        const uint64_t cb = off[pa], tc = off[chunks[c + 1]] - cb;
        if (t != tc) return fail(GN_E_HIP, "child count changed between passes (%zu != %zu)", t, (size_t)tc);
        if (n_lines) {
          // (d.cur's offsets and unpacked parents are this chunk's: the front that overwrites the
          // set is queued after the synchronisation below)
          const RankHistory h = {o.history.keys, o.history.n_keys, o.history.hist ? o.history.hist + pa : nullptr};
          // (extended: the chunks run serially, so nothing else is queued on the device while the
          // extension evaluates in the current set's and the score levels' buffers; t == 0: no entry
          // is read)
          if (o.leaf.extends())
            if (int r = extend_stage(ctx, d, UnpackedLeaves{d.cur.unpacked.p, mp, d.cur.offsets.p, d.mv2[k].p, d.co2[k].p, t},
                                     mode, o.leaf, d.leaf.ext.p, o.pvs ? d.leaf.tail.p : nullptr, s))
              return r;
          HIP_TRY(hipEventRecord(d.rev[0], s));
          HIP_TRY(launch_rank_children(d.cur.unpacked.p, mp, d.cur.offsets.p, d.mv2[k].p, d.co2[k].p, ctx->P, d.tables.p,
                                       n_lines, d.ln2[k].p, h.hist ? &h : nullptr, o.leaf.extends() ? d.leaf.ext.p : nullptr, s));
          HIP_TRY(hipEventRecord(d.rev[1], s));
          if (o.pvs) { // (t == 0: no line is searched, and the tail is not read)
            HIP_TRY(hipEventRecord(d.pev[2], s));
            HIP_TRY(launch_line_pvs(mp, d.cur.offsets.p, d.mv2[k].p, d.leaf.tail.p, d.ln2[k].p, n_lines, d.pv2[k].p, s));
            HIP_TRY(hipEventRecord(d.pev[3], s));
          }
        } else {
          HIP_TRY(launch_pack_children(d.co2[k].p, t, d.cc2[k].p, s));
        }
        int r = check_plan(d, s); // synchronises the stream: chunk c is computed
        if (r) return r;
        if (n_lines) {
          HIP_TRY(hipStreamSynchronize(s)); // (check_plan returns at once when nothing ran planned)
          float ms = 0;
          HIP_TRY(hipEventElapsedTime(&ms, d.rev[0], d.rev[1]));
          d.t_rank += ms;
          if (o.pvs) {
            HIP_TRY(hipEventElapsedTime(&ms, d.pev[2], d.pev[3]));
            d.t_pv += ms;
          }
        }
        d.t_compute += ms_since(t0), t0 = Clock::now();
        HIP_TRY(hipEventRecord(d.cev[k], s));
        drain_chunk(k, pa, mp, t, cb);
        return GN_OK;
      },
      o.leaf.extends());
  const auto tt = Clock::now();
  for (int k = 0; k < 2; ++k) {
    const int r = join(k);
    if (!rc) rc = r;
  }
  d.t_tail = ms_since(tt);
  return rc;
}

// Host parent boards -> every legal child -> parent/child gn_eval (gn_expand_and_evaluate),
// sharded over every device of the context (equal parent ranges).
static int expand_boards_host(gn_ctx *ctx, const gn_board *boards, size_t n, int mode, gn_eval *parent_out,
                              uint32_t *child_offsets, uint16_t *child_moves, gn_child *child_out, size_t cap) {
  if (!slot(ctx, 0)) return fail(GN_E_INVALID, "bad context");
  if (!n) {
    child_offsets[0] = 0;
    return GN_OK;
  }
  return guarded([&]() -> int {
    const size_t nd = ctx->devs.size();
    std::vector<size_t> b(nd + 1);
    partition(nullptr, n, (int)nd, b.data());
    const auto locks = lock_devices(ctx);
    std::vector<std::vector<uint64_t>> off(nd);
    // pass 1: upload + child counts
    int rc = run_shards(ctx, b, [&](size_t k, Dev &d, size_t lo, size_t hi) -> int {
      const auto t0 = Clock::now();
      HIP_TRY(d.par.ensure(hi - lo));
      HIP_TRY(hipMemcpyAsync(d.par.p, boards + lo, (hi - lo) * sizeof(gn_board), hipMemcpyHostToDevice, d.stream));
      HIP_TRY(hipStreamSynchronize(d.stream));
      d.t_upload += ms_since(t0);
      return count_shard(d, d.par.p, hi - lo, off[k]);
    });
    if (rc) return rc;
    std::vector<uint64_t> base(nd + 1, 0);
    for (size_t k = 0; k < nd; ++k) base[k + 1] = base[k] + (b[k] < b[k + 1] ? off[k].back() : 0);
    const uint64_t total = base[nd];
    if (total > 0xFFFFFFFFull) return fail(GN_E_CAPACITY, "children exceed 32-bit offsets");
    for (size_t k = 0; k < nd; ++k)
      for (size_t i = b[k]; i < b[k + 1]; ++i) child_offsets[i] = (uint32_t)(base[k] + off[k][i - b[k]]);
    child_offsets[n] = (uint32_t)total;
    if (total > cap) return fail(GN_E_CAPACITY, "%zu children exceed capacity %zu", (size_t)total, cap);
    if (total && (!child_moves || !child_out)) return fail(GN_E_INVALID, "NULL child buffer");
    // pass 2: chunks of 81 parents' multiples (a FEN batch has no games: blocks of 81 = chain_len)
    return run_shards(ctx, b, [&](size_t k, Dev &d, size_t lo, size_t hi) -> int {
      const size_t m = hi - lo;
      std::vector<size_t> starts;
      for (size_t i = 81; i < m; i += 81) starts.push_back(i);
      return expand_pipelined(ctx, d, d.par.p, m, mode, off[k], chunk_plan(m, starts, ctx->chunk_parents),
                              {parent_out ? parent_out + lo : nullptr, child_moves + base[k], child_out + base[k]});
    });
  });
}

// A host-buffer call over n FENs (gn_expand_and_evaluate, gn_evaluate_lines2): f(boards) on the
// packed FENs, between the host stage times.
template <class F>
static int on_packed_fens(gn_ctx *ctx, const char *const *fens, size_t n, F &&f) {
  return guarded([&]() -> int {
    const auto T0 = Clock::now();
    reset_host_stats(ctx);
    std::vector<gn_board> boards(n);
    int rc = gn_pack_fens(fens, n, boards.data(), nullptr);
    if (rc) return rc;
    ctx->t_parse = ms_since(T0);
    rc = f(boards.data());
    ctx->t_total = ms_since(T0);
    return rc;
  });
}

// ------------------------------------------------- lichess batch replay ----
// IncomingBatch::from_acquired (/root/reference/src/queue.rs:548-700) for the
// GPU path.  The root FEN is set up with Chess960 castling, ignoring an invalid
// en-passant square or castling right (queue.rs:554-560).  Every UCI move of
// AcquireResponseBody.moves (/root/reference/src/api.rs:306-321) is resolved as
// shakmaty 0.27.3's UciMove::to_move resolves it (queue.rs:576) and played
// (queue.rs:578).  That gives positions 0..=len, position i being the root after
// i moves (queue.rs:605-637); skipPositions marks the ones not analysed
// (queue.rs:617, 633).  A move that does not resolve to a legal move fails the
// game, as `uci.to_move(&pos)?` fails the whole batch in the reference.

// (shakmaty 0.27.3 UciMove::to_move: resolve_uci in chess.h, shared with the GPU replay)
static bool uci_to_move(const Board &B, const char *u, size_t len, uint16_t &out) {
  return resolve_uci(B, host_tables(), uci_code(u, (int)len), out);
}

struct Replay {
  std::vector<gn_board> boards; // positions 0..=len
  std::vector<uint16_t> moves;  // len moves, Stockfish encoding (castling = king takes rook)
  std::vector<uint8_t> skip;    // per position
  int rc = GN_OK;
  std::string err;
};

// f(token, length) for each whitespace-separated token of s (space, \t, \n, \r; NULL: none) in
// turn, until f returns false.
template <class F>
static void for_each_token(const char *s, F &&f) {
  auto space = [](char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; };
  for (s = s ? s : ""; *s;) {
    while (space(*s)) ++s;
    if (!*s) break;
    const char *e = s;
    while (*e && !space(*e)) ++e;
    if (!f(s, (size_t)(e - s))) break;
    s = e;
  }
}

// skip[p] = 1 for the positions p < npos of g's skip list (indices beyond the game are ignored),
// 0 for the rest; whether any is set.
static bool skip_mask(const gn_game &g, size_t npos, std::vector<uint8_t> &skip) {
  skip.assign(npos, 0);
  bool any = false;
  for (size_t k = 0; k < g.n_skip && g.skip_positions; ++k)
    if (g.skip_positions[k] < npos) skip[g.skip_positions[k]] = 1, any = true;
  return any;
}

static void replay_game(const gn_game &g, Replay &r) {
  Board B;
  if (!g.root_fen || !parse_fen(g.root_fen, B)) {
    r.rc = GN_E_INVALID, r.err = "bad root FEN";
    return;
  }
  gn_board pb;
  pack(B, pb);
  r.boards.push_back(pb);
  for_each_token(g.uci_moves, [&](const char *s, size_t len) {
    uint16_t m = 0;
    if (!uci_to_move(B, s, len, m)) {
      char buf[96];
      snprintf(buf, sizeof(buf), "move %zu (%.*s) is not legal", r.moves.size() + 1, (int)std::min<size_t>(len, 16), s);
      r.rc = GN_E_ILLEGAL_MOVE, r.err = buf;
      r.boards.clear(), r.moves.clear();
      return false;
    }
    B = do_move(B, m);
    pack(B, pb);
    r.boards.push_back(pb);
    r.moves.push_back(m);
    return true;
  });
  if (!r.rc) skip_mask(g, r.boards.size(), r.skip);
}

// A game prepared on the host for the GPU replay: its root (Position::set on the root FEN)
// and its move tokens as uci_code values (the wire form, whitespace-separated).
struct GamePrep {
  gn_board root;
  bool ok = false;
  std::vector<uint16_t> codes;
};

static void prep_game(const gn_game &g, GamePrep &p) {
  Board B;
  if (!g.root_fen || !parse_fen(g.root_fen, B)) return;
  pack(B, p.root);
  p.ok = true;
  for_each_token(g.uci_moves, [&](const char *s, size_t len) {
    p.codes.push_back(uci_code(s, (int)std::min<size_t>(len, 6)));
    return true;
  });
}

// the text of a game's move k (1-based), for the error message (at most 16 characters)
static std::string move_token(const gn_game &g, size_t k) {
  std::string tok;
  size_t i = 0;
  for_each_token(g.uci_moves, [&](const char *s, size_t len) {
    if (++i == k) tok.assign(s, std::min<size_t>(len, 16));
    return i < k;
  });
  return tok;
}

// ---- gn_evaluate_games, and (n_lines > 0) gn_evaluate_games_lines: the expansion with children,
// whose chunks are ranked on the device instead of downloaded (no child array, no child capacity);
// and (lines2) gn_evaluate_games_lines2: the same front, then the two-ply lines' chunk loop.

// One device's share of a games call.  In place (the common case): every game of the device
// replayed and none has a skipped position, so its evaluated positions are the replay's boards as
// they lie (rboards: game j's position p at moff[j] + j + p) and one contiguous run of
// position_out from p0: the expansion reads rboards in place and writes the caller's arrays
// directly.  Otherwise the evaluated positions are gathered (src: board index, where: output
// index) into contiguous parents (Dev::par), and their records (res, lres) scattered back.
struct GameShard {
  std::vector<size_t> games;        // the device's replayed games (global index)
  std::vector<uint64_t> moff;       // their move-code offsets (games + 1)
  std::vector<int32_t> status;      // their status (0 or the first illegal move, 1-based)
  bool in_place = false;
  size_t m = 0;                     // evaluated positions
  size_t p0 = 0;                    // in place: the first one's index in position_out
  std::vector<uint32_t> src, where; // gathered: each one's board in rboards / index in position_out
  std::vector<size_t> starts;       // first evaluated position of each game (the chunks' cuts)
  std::vector<gn_eval> res;         // gathered: the evaluated positions' records ...
  std::vector<gn_line> lres;        // ... and lines ...
  std::vector<gn_line2> l2res;      // ... or two-ply lines
  std::vector<gn_line3> l3res;      // ... or three-ply lines
  std::vector<gn_pv> pvres;         // ... and the lines' PVs (the _pv calls)
  std::vector<gn_history> hist;     // history call: each evaluated position's game so far, in rboards' indices
  std::vector<uint64_t> off;        // child offsets from pass 1 (m + 1, relative)
  uint64_t child_base = 0;          // the shard's first child in the caller's arrays
  bool has() const { return m > 0; }
  const gn_board *parents_of(const Dev &d) const { return in_place ? d.rboards.p : d.par.p; }
  gn_eval *records_of(gn_eval *position_out) { return in_place ? position_out + p0 : res.data(); }
};

// A games call's arguments: each call names what it asks for, and what it does not name stays off.
struct GamesArgs {
  gn_ctx *ctx = nullptr;
  const gn_game *games = nullptr;
  size_t n_games = 0;
  int mode = GN_MODE_FULL;
  uint32_t *position_offsets = nullptr;
  int32_t *game_status = nullptr;
  gn_eval *position_out = nullptr;
  size_t position_cap = 0, child_cap = 0;
  int with_children = 0; // gn_evaluate_games: the children too, into the three arrays below
  uint32_t *child_offsets = nullptr;
  uint16_t *child_moves = nullptr;
  gn_child *child_out = nullptr;
  int n_lines = 0;            // the lines calls: n_lines lines per position, no child reaches the host
  gn_line *lines = nullptr;   // ... one-ply (with_children 1: the children ranked on the device)
  gn_line2 *lines2 = nullptr; // ... or two-ply (with_children 0)
  gn_line3 *lines3 = nullptr; // ... or three-ply (with_children 0)
  bool history = false;       // ... with the game-history draws
  LeafRule leaf;              // ... their leaves valued by this rule (extend_stage)
  gn_pv *pvs = nullptr;       // ... and each line's whole variation (the _pv calls)
};

// A games call: its arguments, and what its phases hand on.
struct GamesCall : GamesArgs {
  explicit GamesCall(const GamesArgs &a) : GamesArgs(a) {}
  std::vector<GamePrep> prep;
  std::vector<size_t> bounds;    // the devices' game ranges
  std::vector<GameShard> shards; // one per device
  std::vector<uint32_t> npos;    // positions per game (0: failed)
  uint64_t total = 0;            // positions
  bool all_in_place = true;
  std::string last_err;          // the last failed game's message (gn_last_error after GN_OK)
};

// host: root FENs parsed, UCI moves tokenized (the wire form, AcquireResponseBody.moves); games
// sharded over the devices, never split, weighted by their positions (moves + 1)
static void games_prepare(GamesCall &c, Clock::time_point T0) {
  c.prep.resize(c.n_games);
  parallel_for(c.n_games, 64, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) prep_game(c.games[i], c.prep[i]);
  });
  c.ctx->t_parse = ms_since(T0);
  const size_t nd = c.ctx->devs.size();
  std::vector<uint32_t> w(c.n_games);
  for (size_t i = 0; i < c.n_games; ++i) w[i] = c.prep[i].ok ? (uint32_t)c.prep[i].codes.size() + 1 : 0;
  c.bounds.resize(nd + 1);
  partition(w.data(), c.n_games, (int)nd, c.bounds.data());
  c.shards.resize(nd);
}

// phase A: a device replays its games [g0, g1) (replay_games_kernel) and reports their status
static int games_replay(const GamesCall &c, GameShard &sh, Dev &d, size_t g0, size_t g1) {
  auto &gl = sh.games;
  auto &mo = sh.moff;
  mo.push_back(0);
  for (size_t g = g0; g < g1; ++g)
    if (c.prep[g].ok) gl.push_back(g), mo.push_back(mo.back() + c.prep[g].codes.size());
  const size_t ng = gl.size(), nm = mo.back();
  if (!ng) return GN_OK;
  std::vector<uint16_t> codes(std::max<size_t>(nm, 1));
  std::vector<gn_board> roots(ng);
  for (size_t j = 0; j < ng; ++j) {
    roots[j] = c.prep[gl[j]].root;
    std::copy(c.prep[gl[j]].codes.begin(), c.prep[gl[j]].codes.end(), codes.begin() + mo[j]);
  }
  const auto t0 = Clock::now();
  HIP_TRY(d.roots.ensure(ng));
  HIP_TRY(d.moff.ensure(ng + 1));
  HIP_TRY(d.codes.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(d.rboards.ensure(nm + ng));
  HIP_TRY(d.smoves.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(d.rstatus.ensure(ng));
  hipStream_t s = d.stream;
  HIP_TRY(hipMemcpyAsync(d.roots.p, roots.data(), ng * sizeof(gn_board), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d.moff.p, mo.data(), (ng + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d.codes.p, codes.data(), codes.size() * sizeof(uint16_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  d.t_upload += ms_since(t0);
  const auto t1 = Clock::now();
  HIP_TRY(launch_replay_games(d.roots.p, ng, d.moff.p, d.codes.p, d.tables.p, d.rboards.p, d.smoves.p, d.rstatus.p, s));
  if (c.history) { // the keys of every replayed board (a failed game's unwritten ones are never indexed),
                   // queued behind the replay: the status read-back below waits for both
    HIP_TRY(d.rkeys.ensure(nm + ng));
    d.n_rkeys = nm + ng;
    HIP_TRY(hipEventRecord(d.rev[0], s));
    HIP_TRY(launch_position_keys(d.rboards.p, nm + ng, false, d.tables.p, d.rkeys.p, s));
    HIP_TRY(hipEventRecord(d.rev[1], s));
  }
  sh.status.resize(ng);
  HIP_TRY(hipMemcpyAsync(sh.status.data(), d.rstatus.p, ng * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  double keys_ms = 0;
  if (c.history) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, d.rev[0], d.rev[1]));
    d.t_keys += ms, keys_ms = ms;
  }
  d.t_replay += ms_since(t1) - keys_ms;
  return GN_OK;
}

// host: every game's status and position offset into the caller's arrays, then the capacity and
// NULL checks (the offsets and status are written whatever they find)
static int games_offsets(GamesCall &c) {
  std::vector<int32_t> gst(c.n_games, GN_OK);
  c.npos.assign(c.n_games, 0);
  for (const GameShard &sh : c.shards)
    for (size_t j = 0; j < sh.games.size(); ++j) {
      const size_t g = sh.games[j];
      if (sh.status[j]) {
        gst[g] = GN_E_ILLEGAL_MOVE;
        c.last_err = "move " + std::to_string(sh.status[j]) + " (" + move_token(c.games[g], (size_t)sh.status[j]) +
                     ") is not legal";
      } else {
        c.npos[g] = (uint32_t)(sh.moff[j + 1] - sh.moff[j] + 1);
      }
    }
  for (size_t g = 0; g < c.n_games; ++g) {
    if (!c.prep[g].ok) gst[g] = GN_E_INVALID, c.last_err = "bad root FEN";
    c.game_status[g] = gst[g];
    c.position_offsets[g] = (uint32_t)c.total;
    c.total += c.npos[g];
  }
  if (c.total > 0xFFFFFFFFull) return fail(GN_E_CAPACITY, "positions exceed 32-bit offsets");
  c.position_offsets[c.n_games] = (uint32_t)c.total;
  if (c.total > c.position_cap)
    return fail(GN_E_CAPACITY, "%zu positions exceed capacity %zu", (size_t)c.total, c.position_cap);
  if (c.total && !c.position_out) return fail(GN_E_INVALID, "position_out is NULL");
  if (c.total && c.n_lines && !c.lines && !c.lines2 && !c.lines3) return fail(GN_E_INVALID, "lines is NULL");
  return GN_OK;
}

// host: a shard's evaluated positions, in place or gathered (GameShard); the skipped positions'
// records are written here
static void games_layout(const GamesCall &c, GameShard &sh) {
  std::vector<uint8_t> skip;
  sh.in_place = true;
  for (size_t j = 0; j < sh.games.size() && sh.in_place; ++j) {
    const size_t g = sh.games[j];
    sh.in_place = sh.status[j] == 0 && !(c.games[g].n_skip && skip_mask(c.games[g], c.npos[g], skip));
  }
  if (sh.in_place) {
    sh.m = sh.games.empty() ? 0 : (size_t)sh.moff.back() + sh.games.size();
    sh.p0 = sh.games.empty() ? 0 : c.position_offsets[sh.games[0]];
    for (size_t j = 0; j < sh.games.size(); ++j) sh.starts.push_back((size_t)sh.moff[j] + j);
    if (c.history) sh.hist.reserve(sh.m);
    if (c.history)
      for (size_t j = 0; j < sh.games.size(); ++j) {
        const uint32_t first = (uint32_t)(sh.moff[j] + j);
        for (uint32_t e = first; e < sh.moff[j + 1] + j + 1; ++e) sh.hist.push_back(gn_history{first, e});
      }
    return;
  }
  for (size_t j = 0; j < sh.games.size(); ++j) {
    const size_t g = sh.games[j];
    if (!c.npos[g]) continue;
    skip_mask(c.games[g], c.npos[g], skip);
    sh.starts.push_back(sh.src.size());
    for (uint32_t p = 0; p < c.npos[g]; ++p) {
      const size_t at = c.position_offsets[g] + p;
      if (skip[p]) {
        c.position_out[at] = gn_eval{0, 0, 0, 0, 0, (uint16_t)(GN_FLAG_SKIPPED | GN_FLAG_NO_SCORE), 0};
      } else {
        sh.src.push_back((uint32_t)(sh.moff[j] + j + p));
        sh.where.push_back((uint32_t)at);
        if (c.history) sh.hist.push_back(gn_history{(uint32_t)(sh.moff[j] + j), sh.src.back()});
      }
    }
  }
  sh.m = sh.src.size();
}

// phase B's front: (gathered) the evaluated positions gathered into contiguous parents; (history)
// their gn_history entries uploaded
static int games_gather(const GamesCall &c, GameShard &sh, Dev &d) {
  const size_t m = sh.m;
  hipStream_t s = d.stream;
  if (!sh.in_place) {
    const auto t0 = Clock::now();
    HIP_TRY(d.gidx.ensure(m));
    HIP_TRY(d.par.ensure(m));
    HIP_TRY(hipMemcpyAsync(d.gidx.p, sh.src.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(launch_gather_boards(d.rboards.p, d.gidx.p, m, d.par.p, s));
    HIP_TRY(hipStreamSynchronize(s));
    d.t_upload += ms_since(t0);
    sh.res.resize(m);
    if (c.lines3) sh.l3res.resize(m * (size_t)c.n_lines);
    else if (c.lines2) sh.l2res.resize(m * (size_t)c.n_lines);
    else sh.lres.resize(m * (size_t)c.n_lines);
    if (c.pvs) sh.pvres.resize(m * (size_t)c.n_lines);
  }
  if (c.history) { // one gn_history per evaluated position, uploaded once per shard
    const auto t0 = Clock::now();
    HIP_TRY(d.hist.ensure(m));
    HIP_TRY(hipMemcpyAsync(d.hist.p, sh.hist.data(), m * sizeof(gn_history), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    d.t_upload += ms_since(t0);
  }
  return GN_OK;
}

// phase B: the gather; then evaluated (no children) or counted (pass 1 of the expansion)
static int games_evaluate_or_count(const GamesCall &c, GameShard &sh, Dev &d) {
  const int rc = games_gather(c, sh, d);
  if (rc) return rc;
  const size_t m = sh.m;
  hipStream_t s = d.stream;
  if (c.with_children) return count_shard(d, sh.parents_of(d), m, sh.off);
  const auto t1 = Clock::now();
  HIP_TRY(d.io_out.ensure(m));
  int r = evaluate_on(c.ctx, d, sh.parents_of(d), m, c.mode, d.io_out.p, s);
  if (!r) r = resolve_scores(c.ctx, d, sh.parents_of(d), m, c.mode, d.io_out.p, nullptr, s);
  if (r) return r;
  HIP_TRY(hipStreamSynchronize(s));
  d.t_compute += ms_since(t1);
  const auto t2 = Clock::now();
  HIP_TRY(hipMemcpy(sh.records_of(c.position_out), d.io_out.p, m * sizeof(gn_eval), hipMemcpyDeviceToHost));
  d.t_download += ms_since(t2);
  return GN_OK;
}

// host, between the passes: every shard's child base and (gn_evaluate_games; the lines call
// returns no children: no child offsets, no child capacity) the child offsets over all
// positions, a skipped one's being the next position's; then the child capacity and NULL checks
static int games_child_offsets(GamesCall &c) {
  uint64_t ctot = 0;
  for (GameShard &sh : c.shards) sh.child_base = ctot, ctot += sh.has() ? sh.off.back() : 0;
  if (c.n_lines) return GN_OK;
  if (ctot > 0xFFFFFFFFull) return fail(GN_E_CAPACITY, "children exceed 32-bit offsets");
  uint32_t *const co = c.child_offsets;
  if (!c.all_in_place)
    for (size_t g = 0; g < c.n_games; ++g)
      for (uint32_t p = 0; p < c.npos[g]; ++p) co[c.position_offsets[g] + p] = 0xFFFFFFFFu;
  for (const GameShard &sh : c.shards) {
    if (!sh.has()) continue;
    if (sh.in_place)
      for (size_t e = 0; e < sh.m; ++e) co[sh.p0 + e] = (uint32_t)(sh.child_base + sh.off[e]);
    else
      for (size_t e = 0; e < sh.where.size(); ++e) co[sh.where[e]] = (uint32_t)(sh.child_base + sh.off[e]);
  }
  if (!c.all_in_place) {
    uint32_t next = (uint32_t)ctot;
    for (size_t at = c.total; at-- > 0;) {
      if (co[at] == 0xFFFFFFFFu) co[at] = next;
      else next = co[at];
    }
  }
  co[c.total] = (uint32_t)ctot;
  if (ctot > c.child_cap) return fail(GN_E_CAPACITY, "%zu children exceed capacity %zu", (size_t)ctot, c.child_cap);
  if (ctot && (!c.child_moves || !c.child_out)) return fail(GN_E_INVALID, "NULL child buffer");
  return GN_OK;
}

// phase C: the expansion pipeline, chunks cut at game starts
static int games_expand(const GamesCall &c, GameShard &sh, Dev &d) {
  gn_eval *const rec = sh.records_of(c.position_out);
  gn_line *const ln = sh.in_place ? c.lines + sh.p0 * (size_t)c.n_lines : sh.lres.data();
  ExpandOut o = c.n_lines ? ExpandOut{rec, nullptr, nullptr, c.n_lines, ln}
                          : ExpandOut{rec, c.child_moves + sh.child_base, c.child_out + sh.child_base};
  if (c.history) o.history = RankHistory{d.rkeys.p, d.n_rkeys, d.hist.p};
  o.leaf = c.leaf;
  if (c.pvs) o.pvs = sh.in_place ? c.pvs + sh.p0 * (size_t)c.n_lines : sh.pvres.data();
  return expand_pipelined(c.ctx, d, sh.parents_of(d), sh.m, c.mode, sh.off,
                          chunk_plan(sh.m, sh.starts, c.ctx->chunk_parents), o);
}

// host: the gathered shards' lines (the shard's vector `res`) to their places in the caller's
// array; the skipped positions' lines are `empty`
template <class Line>
static void games_scatter_lines(const GamesCall &c, Line *lines, std::vector<Line> GameShard::*res, const Line &empty) {
  const size_t K = (size_t)c.n_lines;
  if (!c.all_in_place)
    for (size_t g = 0; g < c.n_games; ++g)
      for (size_t at = c.position_offsets[g]; at < c.position_offsets[g + 1]; ++at)
        if (c.position_out[at].flags & GN_FLAG_SKIPPED)
          for (size_t j = 0; j < K; ++j) lines[at * K + j] = empty;
  for (const GameShard &sh : c.shards)
    for (size_t e = 0; e < sh.where.size(); ++e)
      std::copy((sh.*res).begin() + e * K, (sh.*res).begin() + (e + 1) * K, lines + (size_t)sh.where[e] * K);
}

// host: the gathered shards' records and lines to their places in the caller's arrays
static void games_scatter(const GamesCall &c) {
  for (const GameShard &sh : c.shards)
    for (size_t e = 0; e < sh.where.size(); ++e) c.position_out[sh.where[e]] = sh.res[e];
  if (!c.n_lines) return;
  if (c.lines3) games_scatter_lines(c, c.lines3, &GameShard::l3res, gn_line3{0, 0, 0, 0, 0, (uint16_t)GN_FLAG_NO_SCORE, 0, 0});
  else if (c.lines2) games_scatter_lines(c, c.lines2, &GameShard::l2res, gn_line2{0, 0, 0, 0, (uint16_t)GN_FLAG_NO_SCORE, 0});
  else games_scatter_lines(c, c.lines, &GameShard::lres, gn_line{0, 0, 0, (uint16_t)GN_FLAG_NO_SCORE});
  if (c.pvs) games_scatter_lines(c, c.pvs, &GameShard::pvres, gn_pv{});
}

// phase B of gn_evaluate_games_lines2: the gather, then the two-ply lines' chunk loop (below, with
// gn_evaluate_lines2)
static int games_lines2(const GamesCall &c, GameShard &sh, Dev &d);
// ... and of gn_evaluate_games_lines3: the gather, then the three-ply lines' chunk loop
static int games_lines3(const GamesCall &c, GameShard &sh, Dev &d);

static int evaluate_games(const GamesArgs &a) {
  if (!slot(a.ctx, 0)) return fail(GN_E_INVALID, "bad context");
  if (a.n_games && (!a.games || !a.position_offsets || !a.game_status)) return fail(GN_E_INVALID, "NULL argument");
  if (a.with_children && !a.n_lines && !a.child_offsets) return fail(GN_E_INVALID, "child_offsets is NULL");
  if (a.mode < GN_MODE_FULL || a.mode > GN_MODE_SMALL) return fail(GN_E_INVALID, "bad mode %d", a.mode);
  GamesCall c(a);
  return guarded([&]() -> int {
    const auto T0 = Clock::now();
    gn_ctx *const ctx = c.ctx;
    reset_host_stats(ctx);
    games_prepare(c, T0);
    const auto locks = lock_devices(ctx);
    int rc = run_shards(ctx, c.bounds, [&](size_t k, Dev &d, size_t g0, size_t g1) -> int {
      return games_replay(c, c.shards[k], d, g0, g1);
    });
    if (rc || (rc = games_offsets(c)) != GN_OK) return rc;
    for (GameShard &sh : c.shards) games_layout(c, sh), c.all_in_place = c.all_in_place && sh.in_place;
    auto has = [&](size_t k) { return c.shards[k].has(); };
    rc = run_devices(ctx, has, [&](size_t k, Dev &d) -> int {
      return c.lines3   ? games_lines3(c, c.shards[k], d)
             : c.lines2 ? games_lines2(c, c.shards[k], d)
                        : games_evaluate_or_count(c, c.shards[k], d);
    });
    if (rc) return rc;
    if (c.with_children) {
      if ((rc = games_child_offsets(c)) != GN_OK) return rc;
      rc = run_devices(ctx, has, [&](size_t k, Dev &d) -> int { return games_expand(c, c.shards[k], d); });
      if (rc) return rc;
    }
    games_scatter(c);
    ctx->t_total = ms_since(T0);
    if (!c.last_err.empty()) g_err = c.last_err;
    return GN_OK;
  });
}

// The games calls with lines: one-ply (gn_line: the children ranked on the device) or two-ply
template <class Line>
static int evaluate_games_lines(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines, bool history,
                                LeafRule leaf, uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                                size_t position_cap, Line *lines, gn_pv *pvs = nullptr) {
  if (int rc = check_leaf_rule(leaf)) return rc;
  if (int rc = check_n_lines(n_lines)) return rc;
  GamesArgs a;
  a.pvs = pvs;
  a.ctx = ctx, a.games = games, a.n_games = n_games, a.mode = mode, a.position_offsets = position_offsets;
  a.game_status = game_status, a.position_out = position_out, a.position_cap = position_cap;
  a.n_lines = n_lines, a.history = history, a.leaf = leaf;
  if constexpr (std::is_same<Line, gn_line>::value) a.with_children = 1, a.lines = lines;
  else if constexpr (std::is_same<Line, gn_line3>::value) a.lines3 = lines;
  else a.lines2 = lines;
  return evaluate_games(a);
}

// ============================================================ C-ABI ========
extern "C" {

int gn_replay_game(const gn_game *game, gn_board *positions, uint8_t *skipped, uint16_t *moves, size_t cap,
                   size_t *n_positions) {
  if (!game || !n_positions) return fail(GN_E_INVALID, "NULL argument");
  return guarded([&]() -> int {
    Replay r;
    replay_game(*game, r);
    *n_positions = r.boards.size();
    if (r.rc) return fail(r.rc, "%s", r.err.c_str());
    if (r.boards.size() > cap) return fail(GN_E_CAPACITY, "%zu positions exceed capacity %zu", r.boards.size(), cap);
    if (positions) memcpy(positions, r.boards.data(), r.boards.size() * sizeof(gn_board));
    if (skipped) memcpy(skipped, r.skip.data(), r.skip.size());
    if (moves && !r.moves.empty()) memcpy(moves, r.moves.data(), r.moves.size() * sizeof(uint16_t));
    return GN_OK;
  });
}

int gn_evaluate_games(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int with_children,
                      uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out, size_t position_cap,
                      uint32_t *child_offsets, uint16_t *child_moves, gn_child *child_out, size_t child_cap) {
  GamesArgs a;
  a.ctx = ctx, a.games = games, a.n_games = n_games, a.mode = mode, a.position_offsets = position_offsets;
  a.game_status = game_status, a.position_out = position_out, a.position_cap = position_cap;
  a.with_children = with_children, a.child_offsets = child_offsets, a.child_moves = child_moves;
  a.child_out = child_out, a.child_cap = child_cap;
  return evaluate_games(a);
}

int gn_evaluate_games_lines(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                            uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                            size_t position_cap, gn_line *lines) {
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, false, LeafRule{}, position_offsets, game_status,
                              position_out, position_cap, lines);
}

int gn_evaluate_games_lines_history(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                    uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                                    size_t position_cap, gn_line *lines) {
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, true, LeafRule{}, position_offsets, game_status,
                              position_out, position_cap, lines);
}

int gn_evaluate_games_lines_extended(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                     int history, uint32_t *position_offsets, int32_t *game_status,
                                     gn_eval *position_out, size_t position_cap, gn_line *lines) {
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, history != 0, LeafRule::checks(), position_offsets,
                              game_status, position_out, position_cap, lines);
}

int gn_evaluate_games_lines_quiescent(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                      int history, int depth, uint32_t *position_offsets, int32_t *game_status,
                                      gn_eval *position_out, size_t position_cap, gn_line *lines) {
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, history != 0, LeafRule::quiesce(ctx, depth), position_offsets,
                              game_status, position_out, position_cap, lines);
}

int gn_evaluate_games_lines_quiescent_pv(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                         int history, int depth, uint32_t *position_offsets, int32_t *game_status,
                                         gn_eval *position_out, size_t position_cap, gn_line *lines, gn_pv *pvs) {
  if (n_games && !pvs) return fail(GN_E_INVALID, "pvs is NULL");
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, history != 0, LeafRule::quiesce(ctx, depth), position_offsets,
                              game_status, position_out, position_cap, lines, pvs);
}

int gn_evaluate_games_lines2(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                             uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                             size_t position_cap, gn_line2 *lines) {
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, false, LeafRule{}, position_offsets, game_status,
                              position_out, position_cap, lines);
}

int gn_evaluate_games_lines2_history(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                     uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                                     size_t position_cap, gn_line2 *lines) {
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, true, LeafRule{}, position_offsets, game_status,
                              position_out, position_cap, lines);
}

int gn_evaluate_games_lines2_extended(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                      int history, uint32_t *position_offsets, int32_t *game_status,
                                      gn_eval *position_out, size_t position_cap, gn_line2 *lines) {
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, history != 0, LeafRule::checks(), position_offsets,
                              game_status, position_out, position_cap, lines);
}

int gn_evaluate_games_lines2_quiescent(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                       int history, int depth, uint32_t *position_offsets, int32_t *game_status,
                                       gn_eval *position_out, size_t position_cap, gn_line2 *lines) {
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, history != 0, LeafRule::quiesce(ctx, depth), position_offsets,
                              game_status, position_out, position_cap, lines);
}

int gn_evaluate_games_lines2_quiescent_pv(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                          int history, int depth, uint32_t *position_offsets, int32_t *game_status,
                                          gn_eval *position_out, size_t position_cap, gn_line2 *lines, gn_pv *pvs) {
  if (n_games && !pvs) return fail(GN_E_INVALID, "pvs is NULL");
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, history != 0, LeafRule::quiesce(ctx, depth), position_offsets,
                              game_status, position_out, position_cap, lines, pvs);
}

int gn_partition(const uint32_t *weights, size_t n_items, int n_shards, size_t *bounds) {
  if (n_shards <= 0 || !bounds) return fail(GN_E_INVALID, "bad shard count / NULL bounds");
  return guarded([&]() -> int { return partition(weights, n_items, n_shards, bounds), GN_OK; });
}

int gn_abi_version(void) { return GN_ABI_VERSION; }

const char *gn_last_error(void) { return g_err.c_str(); }

// Stockfish names nets "nn-" + the first 12 hex digits of the file's SHA-256 + ".nnue"
// (checked after download by Stockfish's `make net`, which fishnet's build runs,
// /root/reference/build.rs:318-333).  A file named that way must hash to its name.
static int check_net_name(const char *path, const std::vector<uint8_t> &data) {
  const char *base = strrchr(path, '/');
  base = base ? base + 1 : path;
  if (strlen(base) != 20 || strncmp(base, "nn-", 3) != 0 || strcmp(base + 15, ".nnue") != 0) return GN_OK;
  for (int i = 3; i < 15; ++i)
    if (!((base[i] >= '0' && base[i] <= '9') || (base[i] >= 'a' && base[i] <= 'f'))) return GN_OK;
  Sha256 h;
  h.update(data.data(), data.size());
  char hex[65];
  h.hex(hex);
  if (strncmp(hex, base + 3, 12) != 0)
    return fail(GN_E_FORMAT, "%s: content hashes to nn-%.12s.nnue (corrupt or renamed net)", path, hex);
  return GN_OK;
}

int gn_net_sha256(const uint8_t *data, size_t len, char *hex65) {
  if ((!data && len) || !hex65) return fail(GN_E_INVALID, "NULL argument");
  Sha256 h;
  h.update(data, len);
  h.hex(hex65);
  return GN_OK;
}

int gn_load_net(const char *big_path, const char *small_path, const int *devices, int n_devices, gn_ctx **out) {
  return guarded([&]() -> int {
    std::vector<uint8_t> b, s;
    if (big_path && !read_file(big_path, b)) return fail(GN_E_IO, "cannot read %s", big_path);
    if (small_path && !read_file(small_path, s)) return fail(GN_E_IO, "cannot read %s", small_path);
    int rc;
    if (big_path && (rc = check_net_name(big_path, b)) != GN_OK) return rc;
    if (small_path && (rc = check_net_name(small_path, s)) != GN_OK) return rc;
    return create(big_path ? b.data() : nullptr, b.size(), small_path ? s.data() : nullptr, s.size(), devices,
                  n_devices, out);
  });
}

// L1 width of a .nnue image from its header hashes (0: not a supported net)
static int net_l1(const uint8_t *d, size_t n) {
  auto u32 = [&](size_t o) { return (uint32_t)d[o] | (uint32_t)d[o + 1] << 8 | (uint32_t)d[o + 2] << 16 | (uint32_t)d[o + 3] << 24; };
  if (n < 12 || u32(0) != NNUE_VERSION) return 0;
  const size_t dl = u32(8);
  if (12 + dl + 4 > n) return 0;
  const uint32_t hash = u32(4), fth = u32(12 + dl);
  for (int c : {3072, 1024, 128})
    if (ft_hash(c) == fth && (ft_hash(c) ^ arch_hash(c)) == hash) return c;
  return 0;
}

// The members of an assets archive (zstd + ar, archive.h); GN_OK or a failure.
static int read_archive(const char *path, std::vector<uint8_t> &img, std::vector<archive::Member> &mem) {
  std::vector<uint8_t> file;
  if (!path || !read_file(path, file)) return fail(GN_E_IO, "cannot read %s", path ? path : "(null)");
  std::string err;
  if (!archive::load_image(file, img, err) || !archive::ar_members(img.data(), img.size(), mem, err))
    return fail(GN_E_FORMAT, "%s: %s", path, err.c_str());
  return GN_OK;
}

int gn_archive_read(const char *path, const char *member, uint8_t *buf, size_t cap, size_t *size) {
  return guarded([&]() -> int {
    if (!member || !size) return fail(GN_E_INVALID, "bad argument");
    std::vector<uint8_t> img;
    std::vector<archive::Member> mem;
    int rc = read_archive(path, img, mem);
    if (rc) return rc;
    for (const auto &m : mem)
      if (m.name == member) {
        *size = m.size;
        if (m.size > cap || (!buf && m.size)) return fail(GN_E_CAPACITY, "%s is %zu bytes", member, m.size);
        if (m.size) memcpy(buf, img.data() + m.off, m.size);
        return GN_OK;
      }
    return fail(GN_E_IO, "%s has no member %s", path, member);
  });
}

int gn_load_net_archive(const char *path, const char *big_member, const char *small_member, const int *devices,
                        int n_devices, gn_ctx **out) {
  return guarded([&]() -> int {
    std::vector<uint8_t> img;
    std::vector<archive::Member> mem;
    int rc = read_archive(path, img, mem);
    if (rc) return rc;
    const archive::Member *pick[2] = {nullptr, nullptr};
    const char *want[2] = {big_member, small_member};
    for (int w = 0; w < 2; ++w)
      for (const auto &m : mem) {
        const uint8_t *d = img.data() + m.off;
        const int l1 = net_l1(d, m.size);
        const bool ends = m.name.size() > 5 && m.name.compare(m.name.size() - 5, 5, ".nnue") == 0;
        // by name, or the first .nnue of the right kind (big: L1 3072 / 1024, small: 128)
        if (want[w] ? m.name == want[w] : (ends && l1 && ((w == 0) == (l1 != 128)))) {
          pick[w] = &m;
          break;
        }
      }
    if (!pick[0] && !pick[1]) return fail(GN_E_IO, "%s holds no usable .nnue member", path);
    if ((big_member && !pick[0]) || (small_member && !pick[1]))
      return fail(GN_E_IO, "%s has no member %s", path, !pick[0] && big_member ? big_member : small_member);
    for (int w = 0; w < 2; ++w)
      if (pick[w]) { // Stockfish's name check: nn-<first 12 hex of SHA-256>.nnue
        std::vector<uint8_t> data(img.begin() + pick[w]->off, img.begin() + pick[w]->off + pick[w]->size);
        if ((rc = check_net_name(pick[w]->name.c_str(), data)) != GN_OK) return rc;
      }
    return create(pick[0] ? img.data() + pick[0]->off : nullptr, pick[0] ? pick[0]->size : 0,
                  pick[1] ? img.data() + pick[1]->off : nullptr, pick[1] ? pick[1]->size : 0, devices, n_devices,
                  out);
  });
}

int gn_load_net_memory(const uint8_t *big, size_t big_len, const uint8_t *small, size_t small_len, const int *devices,
                       int n_devices, gn_ctx **out) {
  return guarded([&]() -> int { return create(big, big_len, small, small_len, devices, n_devices, out); });
}

void gn_free(gn_ctx *ctx) { destroy(ctx); }

int gn_get_eval_params(const gn_ctx *ctx, gn_eval_params *out) {
  if (!out) return fail(GN_E_INVALID, "out is NULL");
  *out = ctx ? ctx->P : default_params();
  return GN_OK;
}

int gn_set_eval_params(gn_ctx *ctx, const gn_eval_params *p) {
  if (!ctx || !p) return fail(GN_E_INVALID, "NULL argument");
  if (p->material_base == 0 || p->rule50_div == 0 || p->complexity_div_small == 0 || p->complexity_div_big == 0 ||
      p->wdl_material_anchor == 0)
    return fail(GN_E_INVALID, "zero divisor in eval params");
  if (p->wdl_material_min > p->wdl_material_max) return fail(GN_E_INVALID, "wdl material range is empty");
  if ((int64_t)p->wdl_material_max - p->wdl_material_min > 4096) return fail(GN_E_INVALID, "wdl material range too wide");
  if (p->value_clamp < 0 || p->value_clamp >= VALUE_MATE_IN_MAX_PLY)
    return fail(GN_E_INVALID, "value_clamp must be in [0, %d) (static values stay below mate scores)",
                (int)VALUE_MATE_IN_MAX_PLY);
  // to_cp's a(material) >= 1 wherever it is evaluated (every clamped material value), so that
  // |final_cp| <= 100 * value_clamp < 2^23 fits gn_child's 24-bit field (defaults: a ~ 370-400)
  for (int64_t mc = p->wdl_material_min; mc <= (int64_t)p->wdl_material_max; ++mc) { // (int64: max may be INT_MAX)
#pragma clang fp contract(off)
    const double m = (double)mc / (double)p->wdl_material_anchor;
    const double a = ((p->wdl_a[0] * m + p->wdl_a[1]) * m + p->wdl_a[2]) * m + p->wdl_a[3];
    if (!(a >= 1.0)) return fail(GN_E_INVALID, "win-rate model a(material %lld) = %g < 1", (long long)mc, a);
  }
  ctx->P = *p;
  ++ctx->graph_gen; // (the small-batch graphs hold the parameters they were captured with)
  return GN_OK;
}

int gn_net_info(const gn_ctx *ctx, int *big_l1, uint32_t *big_hash, int *small_l1, uint32_t *small_hash) {
  if (!ctx) return fail(GN_E_INVALID, "ctx is NULL");
  if (big_l1) *big_l1 = ctx->l1[BIG];
  if (big_hash) *big_hash = ctx->hash[BIG];
  if (small_l1) *small_l1 = ctx->l1[SMALL];
  if (small_hash) *small_hash = ctx->hash[SMALL];
  return GN_OK;
}

int gn_pack_fens(const char *const *fens, size_t n, gn_board *out, uint8_t *ok) {
  if (n && (!fens || !out)) return fail(GN_E_INVALID, "NULL argument");
  try {
    parallel_for(n, 4096, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        Board B;
        bool good = parse_fen(fens[i], B);
        if (good) pack(B, out[i]);
        else memset(&out[i], 0, sizeof(gn_board));
        if (ok) ok[i] = good;
      }
    });
  } catch (...) {
    return fail(GN_E_NOMEM, "thread start failed");
  }
  return GN_OK;
}

int gn_board_to_fen(const gn_board *board, char *buf, size_t buflen) {
  if (!board || !buf) return fail(GN_E_INVALID, "NULL argument");
  Board B;
  if (!unpack(*board, B, host_tables())) return fail(GN_E_INVALID, "invalid board");
  if (board_to_fen(B, buf, buflen) < 0) return fail(GN_E_CAPACITY, "buffer too small");
  return GN_OK;
}

int gn_boards_to_fens(const gn_board *boards, size_t n, char *buf, size_t stride) {
  if (n && (!boards || !buf)) return fail(GN_E_INVALID, "NULL argument");
  if (stride < 100) return fail(GN_E_INVALID, "stride < 100");
  try {
    parallel_for(n, 4096, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        Board B;
        char *o = buf + i * stride;
        if (!unpack(boards[i], B, host_tables()) || board_to_fen(B, o, stride) < 0) o[0] = '\0';
      }
    });
  } catch (...) {
    return fail(GN_E_NOMEM, "thread start failed");
  }
  return GN_OK;
}

int gn_position_keys(const gn_board *boards, size_t n, uint64_t *keys) {
  if (n && (!boards || !keys)) return fail(GN_E_INVALID, "NULL argument");
  try {
    parallel_for(n, 4096, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        Board B;
        keys[i] = unpack(boards[i], B, host_tables()) ? position_key(B) : 0;
      }
    });
  } catch (...) {
    return fail(GN_E_NOMEM, "thread start failed");
  }
  return GN_OK;
}

int gn_random_positions(uint64_t seed, size_t first_index, size_t n, int max_plies, gn_board *out) {
  if (n && !out) return fail(GN_E_INVALID, "NULL argument");
  if (max_plies < 0) return fail(GN_E_INVALID, "max_plies < 0");
  try {
    parallel_for(n, 256, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) pack(random_playout(seed + first_index + i, max_plies), out[i]);
    });
  } catch (...) {
    return fail(GN_E_NOMEM, "thread start failed");
  }
  return GN_OK;
}

int gn_evaluate_device(gn_ctx *ctx, int device_slot, const gn_board *d_boards, size_t n, int mode, gn_eval *d_out,
                       void *stream) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad context or device slot");
  if (n && (!d_boards || !d_out)) return fail(GN_E_INVALID, "NULL buffer");
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  const hipStream_t s = call.s;
  int rc = evaluate_on(ctx, *d, d_boards, n, mode, d_out, s);
  if (!rc) rc = resolve_scores(ctx, *d, d_boards, n, mode, d_out, nullptr, s);
  if (rc) return rc;
  HIP_TRY(call.sg->finish()); // blocking (gpu_nnue.h): d_out is written when the call returns
  return GN_OK;
}

int gn_time_evaluate_device(gn_ctx *ctx, int device_slot, const gn_board *d_boards, size_t n, int mode,
                            gn_eval *d_out, int iters, float *ms_total, float *per_kernel_ms, uint64_t *ft_rows) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad context or device slot");
  if (iters <= 0 || !ms_total) return fail(GN_E_INVALID, "bad iters / ms_total");
  DevCall call(*d);
  if (call.rc) return call.rc;
  const hipStream_t s = call.s;
  Events events;
  hipEvent_t begin, end;
  HIP_TRY(events.make({&begin, &end}));
  std::vector<EvalEvents> marks(per_kernel_ms ? (size_t)iters : 0);
  for (EvalEvents &e : marks) HIP_TRY(e.create(events));
  if (ft_rows) {
    HIP_TRY(d->sum.ensure(2));
    HIP_TRY(hipMemsetAsync(d->sum.p, 0, sizeof(unsigned long long), s));
  }
  HIP_TRY(hipEventRecord(begin, s));
  for (int it = 0; it < iters; ++it) {
    EvalOnOpts o;
    o.ev = per_kernel_ms ? &marks[it] : nullptr, o.rows = ft_rows && it == 0 ? d->sum.p : nullptr;
    int rc = evaluate_on(ctx, *d, d_boards, n, mode, d_out, s, o);
    if (rc == GN_OK) rc = resolve_scores(ctx, *d, d_boards, n, mode, d_out, nullptr, s);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(end, s));
  HIP_TRY(hipEventSynchronize(end));
  HIP_TRY(hipEventElapsedTime(ms_total, begin, end));
  if (per_kernel_ms) {
    float acc[4] = {0, 0, 0, 0};
    for (const EvalEvents &e : marks) {
      const hipEvent_t in_order[5] = {e.begun, e.sorted, e.small_done, e.big_done, e.finalized};
      for (int k = 0; k < 4; ++k) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, in_order[k], in_order[k + 1]));
        acc[k] += ms;
      }
    }
    for (int k = 0; k < 4; ++k) per_kernel_ms[k] = acc[k] / (float)iters;
  }
  if (ft_rows) {
    unsigned long long r = 0;
    HIP_TRY(hipMemcpy(&r, d->sum.p, sizeof(r), hipMemcpyDeviceToHost));
    *ft_rows = r;
  }
  return GN_OK;
}

int gn_random_games_uci(uint64_t seed, size_t first_game, size_t n_games, int plies, char *buf, size_t stride) {
  if (n_games && !buf) return fail(GN_E_INVALID, "NULL argument");
  if (plies < 0 || plies > 1000) return fail(GN_E_INVALID, "plies out of range");
  if (stride < 6 * (size_t)plies + 1) return fail(GN_E_INVALID, "stride < 6 * plies + 1");
  try {
    parallel_for(n_games, 64, [&](size_t lo, size_t hi) {
      for (size_t g = lo; g < hi; ++g) {
        char *o = buf + g * stride;
        size_t len = 0;
        random_game(seed + first_game + g, plies, host_tables(), [&](int k, const Board &, uint16_t m) {
          if (!k || !m) return;
          if (len) o[len++] = ' ';
          len += (size_t)move_uci(m, o + len);
        });
        o[len] = '\0';
      }
    });
  } catch (...) {
    return fail(GN_E_NOMEM, "thread start failed");
  }
  return GN_OK;
}

int gn_random_positions_device(gn_ctx *ctx, int device_slot, uint64_t seed, size_t first_index, size_t n,
                               int max_plies, gn_board *d_out, void *stream) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad context or device slot");
  if (n && !d_out) return fail(GN_E_INVALID, "NULL buffer");
  if (max_plies < 0) return fail(GN_E_INVALID, "max_plies < 0");
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  HIP_TRY(launch_random_positions(seed, first_index, n, max_plies, d->tables.p, d_out, call.s));
  return GN_OK;
}

int gn_device_alloc(gn_ctx *ctx, int device_slot, size_t bytes, void **ptr) {
  Dev *d = slot(ctx, device_slot);
  if (!d || !ptr) return fail(GN_E_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(d->id));
  if (hipMalloc(ptr, std::max<size_t>(bytes, 1)) != hipSuccess) return fail(GN_E_NOMEM, "hipMalloc(%zu) failed", bytes);
  return GN_OK;
}

int gn_device_free(gn_ctx *ctx, int device_slot, void *ptr) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(d->id));
  if (ptr) HIP_TRY(hipFree(ptr));
  return GN_OK;
}

int gn_memcpy_h2d(gn_ctx *ctx, int device_slot, void *dst, const void *src, size_t bytes) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad argument");
  DevCall call(*d);
  if (call.rc) return call.rc;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return GN_OK;
}

int gn_memcpy_d2h(gn_ctx *ctx, int device_slot, void *dst, const void *src, size_t bytes) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad argument");
  DevCall call(*d);
  if (call.rc) return call.rc;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return GN_OK;
}

int gn_synchronize(gn_ctx *ctx, int device_slot) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(d->mu);
  HIP_TRY(hipSetDevice(d->id));
  if (d->done_on) HIP_TRY(hipEventSynchronize(d->done)); // the last launch sequence, on whatever stream
  HIP_TRY(hipStreamSynchronize(d->stream));
  return GN_OK;
}

int gn_evaluate_batch_mode(gn_ctx *ctx, const char *const *fens, size_t n, int mode, gn_eval *out) {
  if (!ctx) return fail(GN_E_INVALID, "ctx is NULL");
  if (n && (!fens || !out)) return fail(GN_E_INVALID, "NULL argument");
  if (!n) return GN_OK;
  return guarded([&]() -> int {
    std::vector<gn_board> boards(n);
    int rc = gn_pack_fens(fens, n, boards.data(), nullptr);
    if (rc) return rc;
    return evaluate_coalesced(ctx, boards.data(), n, mode, out);
  });
}

int gn_evaluate_batch(gn_ctx *ctx, const char *const *fens, size_t n, gn_eval *out) {
  return gn_evaluate_batch_mode(ctx, fens, n, GN_MODE_FULL, out);
}

int gn_expand_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, int mode,
                     gn_eval *d_parent_out, uint32_t *d_offsets, gn_board *d_children, uint16_t *d_moves,
                     gn_eval *d_child_out, size_t cap, size_t *total, void *stream) {
  Dev *d = slot(ctx, device_slot);
  if (!d || !total) return fail(GN_E_INVALID, "bad argument");
  if (n && (!d_parents || !d_offsets)) return fail(GN_E_INVALID, "NULL buffer");
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  const hipStream_t s = call.s;
  *total = 0;
  if (!n) return GN_OK;
  if (!d_children || !d_moves || !d_child_out) return fail(GN_E_INVALID, "NULL child buffer");
  LevelOpts o;
  o.children = d_children;
  return expand_level(ctx, *d, d_parents, n, mode, d_parent_out, d_offsets, d_moves, d_child_out, cap, total, s, o);
}

// What the gn_rank_*_device calls check before they take the device, in this order: the slot,
// n_lines, the buffers every parent needs (the child and grandchild buffers may be NULL when no
// parent has a child: they are then never read) and, for the history forms (h), the entries and
// the keys.  d: the slot's device.
static int rank_call_args(gn_ctx *ctx, int device_slot, size_t n, const gn_board *d_parents, const uint32_t *d_offsets,
                          int n_lines, const void *d_lines, const RankHistory *h, Dev *&d) {
  d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad context or device slot");
  if (int rc = check_n_lines(n_lines)) return rc;
  if (n && (!d_parents || !d_offsets || !d_lines || (h && !h->hist))) return fail(GN_E_INVALID, "NULL buffer");
  if (h && h->n_keys && !h->keys) return fail(GN_E_INVALID, "d_keys is NULL");
  return GN_OK;
}

// gn_rank_children_device and its forms: with a history, the game-history draws (the extended forms'
// d_hist NULL: no history at all); with d_ext, the leaves' values from the leaf stage.
static int rank_children_call(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, const uint32_t *d_offsets,
                              const uint16_t *d_moves, const gn_eval *d_child_out, const std::optional<RankHistory> &history,
                              const int32_t *d_ext, int n_lines, gn_line *d_lines, void *stream) {
  const RankHistory *h = history ? &*history : nullptr;
  Dev *d;
  if (int rc = rank_call_args(ctx, device_slot, n, d_parents, d_offsets, n_lines, d_lines, h, d)) return rc;
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  HIP_TRY(launch_rank_children(d_parents, n, d_offsets, d_moves, d_child_out, ctx->P, d->tables.p, n_lines, d_lines, h,
                               d_ext, call.s));
  return GN_OK;
}

int gn_rank_children_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                            const uint32_t *d_offsets, const uint16_t *d_moves, const gn_eval *d_child_out, int n_lines,
                            gn_line *d_lines, void *stream) {
  return rank_children_call(ctx, device_slot, d_parents, n, d_offsets, d_moves, d_child_out, std::nullopt, nullptr,
                            n_lines, d_lines, stream);
}

int gn_position_keys_device(gn_ctx *ctx, int device_slot, const gn_board *d_boards, size_t n, uint64_t *d_keys,
                            void *stream) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad context or device slot");
  if (n && (!d_boards || !d_keys)) return fail(GN_E_INVALID, "NULL buffer");
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  HIP_TRY(launch_position_keys(d_boards, n, true, d->tables.p, d_keys, call.s));
  return GN_OK;
}

int gn_rank_children_history_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                    const uint32_t *d_offsets, const uint16_t *d_moves, const gn_eval *d_child_out,
                                    const uint64_t *d_keys, size_t n_keys, const gn_history *d_hist, int n_lines,
                                    gn_line *d_lines, void *stream) {
  return rank_children_call(ctx, device_slot, d_parents, n, d_offsets, d_moves, d_child_out,
                            RankHistory{d_keys, n_keys, d_hist}, nullptr, n_lines, d_lines, stream);
}

int gn_rank_children_extended_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                     const uint32_t *d_offsets, const uint16_t *d_moves, const gn_eval *d_child_out,
                                     const uint64_t *d_keys, size_t n_keys, const gn_history *d_hist,
                                     const int32_t *d_ext, int n_lines, gn_line *d_lines, void *stream) {
  return rank_children_call(ctx, device_slot, d_parents, n, d_offsets, d_moves, d_child_out,
                            d_hist ? std::optional<RankHistory>({d_keys, n_keys, d_hist}) : std::nullopt, d_ext, n_lines,
                            d_lines, stream);
}

// gn_extend_checks_device / gn_quiesce_device: the leaf stage on a caller's buffers.  *leaves = the
// leaves valued, *nodes (QUIESCE alone; else NULL) = the positions evaluated below them.
static int value_leaves_call(gn_ctx *ctx, int device_slot, const PackedLeaves &lv, int mode, LeafRule rule, int32_t *d_ext,
                             size_t *leaves, size_t *nodes, void *stream, uint16_t *d_tail = nullptr) {
  Dev *d = slot(ctx, device_slot);
  if (!d || !leaves || (rule.kind == LeafRule::QUIESCE && !nodes)) return fail(GN_E_INVALID, "bad argument");
  *leaves = 0;
  if (nodes) *nodes = 0;
  if (lv.total && (!lv.n || !lv.parents || !lv.offsets || !lv.moves || !lv.rec || !d_ext))
    return fail(GN_E_INVALID, "NULL buffer");
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  LeafCount c;
  if (int rc = value_leaves(ctx, *d, lv, mode, rule, d_ext, d_tail, &c, call.s)) return rc;
  *leaves = c.leaves;
  if (nodes) *nodes = c.nodes;
  HIP_TRY(call.sg->finish()); // blocking (gpu_nnue.h): d_ext is written when the call returns
  return GN_OK;
}

int gn_extend_checks_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, const uint32_t *d_offsets,
                            const uint16_t *d_moves, const gn_eval *d_rec, size_t total, int mode, int32_t *d_ext,
                            size_t *extended, void *stream) {
  return value_leaves_call(ctx, device_slot, PackedLeaves{d_parents, n, d_offsets, d_moves, d_rec, total}, mode,
                           LeafRule::checks(), d_ext, extended, nullptr, stream);
}

int gn_quiesce_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, const uint32_t *d_offsets,
                      const uint16_t *d_moves, const gn_eval *d_rec, size_t total, int mode, int depth, int32_t *d_ext,
                      size_t *searched, size_t *nodes, void *stream) {
  return value_leaves_call(ctx, device_slot, PackedLeaves{d_parents, n, d_offsets, d_moves, d_rec, total}, mode,
                           LeafRule::quiesce(ctx, depth), d_ext, searched, nodes, stream);
}

int gn_quiesce_pv_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, const uint32_t *d_offsets,
                         const uint16_t *d_moves, const gn_eval *d_rec, size_t total, int mode, int depth, int32_t *d_ext,
                         uint16_t *d_tail, size_t *searched, size_t *nodes, void *stream) {
  if (total && !d_tail) return fail(GN_E_INVALID, "d_tail is NULL");
  return value_leaves_call(ctx, device_slot, PackedLeaves{d_parents, n, d_offsets, d_moves, d_rec, total}, mode,
                           LeafRule::quiesce(ctx, depth), d_ext, searched, nodes, stream, d_tail);
}

// The exchange evaluation by itself (include/gpu_nnue.h at gn_line, "exchange evaluation"): the
// host form runs chess.h's see() on the host tables, the device form see_moves_kernel.
int gn_see_moves(const gn_board *boards, size_t n, const uint16_t *moves, const int32_t *piece_value, int32_t *out) {
  if (n && (!boards || !moves || !out)) return fail(GN_E_INVALID, "NULL buffer");
  SeeValues V;
  const gn_eval_params defaults = default_params();
  for (int i = 0; i < 5; ++i) V.v[i] = piece_value ? piece_value[i] : defaults.piece_value[i];
  const Tables &T = host_tables();
  for (size_t i = 0; i < n; ++i) {
    out[i] = GN_NOT_EXTENDED;
    Board B;
    if (!unpack(boards[i], B, T)) continue;
    const uint16_t m = moves[i];
    bool legal = false;
    gen_legal(B, T, [&](uint16_t x) { return legal = x == m; });
    if (legal) out[i] = see(B, T, m, V);
  }
  return GN_OK;
}

int gn_see_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, const uint32_t *d_offsets,
                  const uint16_t *d_moves, size_t total, int32_t *d_see, void *stream) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad context or device slot");
  if (total && (!d_parents || !d_offsets || !d_moves || !d_see)) return fail(GN_E_INVALID, "NULL buffer");
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  HIP_TRY(launch_see_moves(d_parents, n, d_offsets, d_moves, total, d->tables.p, see_values(ctx), d_see, call.s));
  return GN_OK;
}

// gn_line_pvs_device / gn_line2_pvs_device: checked as the ranking calls are (rank_call_args, without
// parents), then one launch.
static int line_pvs_args(gn_ctx *ctx, int device_slot, size_t n, const uint32_t *d_offsets, int n_lines,
                         const void *d_lines, const void *d_pvs, Dev *&d) {
  d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad context or device slot");
  if (int rc = check_n_lines(n_lines)) return rc;
  if (n && (!d_offsets || !d_lines || !d_pvs)) return fail(GN_E_INVALID, "NULL buffer");
  return GN_OK;
}

int gn_line_pvs_device(gn_ctx *ctx, int device_slot, size_t n, const uint32_t *d_offsets, const uint16_t *d_moves,
                       const uint16_t *d_tail, const gn_line *d_lines, int n_lines, gn_pv *d_pvs, void *stream) {
  Dev *d;
  if (int rc = line_pvs_args(ctx, device_slot, n, d_offsets, n_lines, d_lines, d_pvs, d)) return rc;
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  HIP_TRY(launch_line_pvs(n, d_offsets, d_moves, d_moves ? d_tail : nullptr, d_lines, n_lines, d_pvs, call.s));
  return GN_OK;
}

int gn_line2_pvs_device(gn_ctx *ctx, int device_slot, size_t n, const uint32_t *d_offsets, const uint16_t *d_moves,
                        const uint32_t *d_goffsets, const uint16_t *d_gmoves, const uint16_t *d_gtail,
                        const gn_line2 *d_lines, int n_lines, gn_pv *d_pvs, void *stream) {
  Dev *d;
  if (int rc = line_pvs_args(ctx, device_slot, n, d_offsets, n_lines, d_lines, d_pvs, d)) return rc;
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  const bool tails = d_moves && d_goffsets && d_gmoves; // (a NULL level: nothing to find a leaf in)
  HIP_TRY(launch_line2_pvs(n, d_offsets, d_moves, d_goffsets, d_gmoves, tails ? d_gtail : nullptr, d_lines, n_lines, d_pvs,
                           call.s));
  return GN_OK;
}

// Depth 2: the children of gn_expand_device's children.  Level 2 is
// the same machinery with the children as parents: they arrive in sibling order, so a
// block of consecutive siblings refreshes each from its predecessor's king-cache row
// (plan_kernel: cache row + the placement difference, a few rows instead of ~30) and
// every grandchild is incremental from its parent's accumulator.  The children are
// evaluated again at level 2 (as parents); those results must equal level 1's and are
// compared on the device (GN_E_HIP if not: an internal consistency check).
//
// gn_expand2_device's work on stream s (d.mu held, the launch sequence begun).  size_grand
// (optional, gn_evaluate_lines2): called with the grandchild count once level 1 is done, it
// provides the level-2 buffers (d_goffsets: total + 1, d_gmoves / d_grand_out / gcap: the count)
// instead of the caller's.
struct Expand2Grand {
  uint32_t *d_goffsets;
  uint16_t *d_gmoves;
  gn_eval *d_grand_out;
  size_t gcap;
};
static int expand2_on(gn_ctx *ctx, Dev *d, const gn_board *d_parents, size_t n, int mode, gn_eval *d_parent_out,
                      uint32_t *d_offsets, gn_board *d_children, uint16_t *d_moves, gn_eval *d_child_out, size_t cap,
                      Expand2Grand gr, size_t *total, size_t *gtotal, hipStream_t s,
                      const std::function<int(size_t, size_t, Expand2Grand &)> *size_grand = nullptr) {
  *total = *gtotal = 0;
  if (!n) return GN_OK;
  // a size query (NULL child buffers or too small): the counts, GN_E_CAPACITY
  if (!d_children || !d_moves || !d_child_out || !cap) {
    HIP_TRY(count_children(*d, d_parents, n, s, total));
    return *total ? fail(GN_E_CAPACITY, "%zu children exceed capacity %zu", *total, cap) : GN_OK;
  }
  LevelOpts l1;
  l1.children = d_children;
  int rc = expand_level(ctx, *d, d_parents, n, mode, d_parent_out, d_offsets, d_moves, d_child_out, cap, total, s, l1);
  if (rc) return rc;
  const size_t t = *total;
  size_t g = 0;
  if (size_grand) { // (the library's own level-2 buffers, grown to the exact count)
    if (t) HIP_TRY(count_children(*d, d_children, t, s, &g));
    if ((rc = (*size_grand)(t, g, gr)) != GN_OK) return rc;
  }
  if (!t) {
    HIP_TRY(hipMemsetAsync(gr.d_goffsets, 0, sizeof(uint32_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    return GN_OK;
  }
  // level 2: the children as parents (their grandchildren boards stay library-internal)
  if (!gr.d_goffsets || !gr.d_gmoves || !gr.d_grand_out || !gr.gcap) {
    HIP_TRY(count_children(*d, d_children, t, s, gtotal));
    return *gtotal ? fail(GN_E_CAPACITY, "%zu grandchildren exceed capacity %zu", *gtotal, gr.gcap) : GN_OK;
  }
  // (level 1's children, written above: trusted; as parents they are child records here too,
  // compared with level 1's below)
  LevelOpts l2;
  l2.trusted = true, l2.score_parents = false, l2.what = "grandchildren";
  HIP_TRY(d->io_out.ensure(t));
  rc = expand_level(ctx, *d, d_children, t, mode, d->io_out.p, gr.d_goffsets, gr.d_gmoves, gr.d_grand_out, gr.gcap, gtotal,
                    s, l2);
  if (rc) return rc;
  // the children evaluated twice (level 1 as children, level 2 as parents) must agree
  HIP_TRY(d->sum.ensure(2));
  HIP_TRY(hipMemsetAsync(d->sum.p, 0, 2 * sizeof(unsigned long long), s));
  HIP_TRY(launch_checksum(d_child_out, t * sizeof(gn_eval), d->sum.p, s));
  HIP_TRY(launch_checksum(d->io_out.p, t * sizeof(gn_eval), d->sum.p + 1, s));
  unsigned long long cs[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(cs, d->sum.p, sizeof(cs), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (cs[0] != cs[1]) return fail(GN_E_HIP, "depth 2: the children's level-1 and level-2 evaluations differ");
  return GN_OK;
}

int gn_expand2_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, int mode,
                      gn_eval *d_parent_out, uint32_t *d_offsets, gn_board *d_children, uint16_t *d_moves,
                      gn_eval *d_child_out, size_t cap, uint32_t *d_goffsets, uint16_t *d_gmoves,
                      gn_eval *d_grand_out, size_t gcap, size_t *total, size_t *gtotal, void *stream) {
  Dev *d = slot(ctx, device_slot);
  if (!d || !total || !gtotal) return fail(GN_E_INVALID, "bad argument");
  if (n && (!d_parents || !d_offsets)) return fail(GN_E_INVALID, "NULL buffer");
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  return expand2_on(ctx, d, d_parents, n, mode, d_parent_out, d_offsets, d_children, d_moves, d_child_out, cap,
                    Expand2Grand{d_goffsets, d_gmoves, d_grand_out, gcap}, total, gtotal, call.s);
}

// gn_rank_lines2_device and its forms, as rank_children_call.
static int rank_lines2_call(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, const uint32_t *d_offsets,
                            const gn_board *d_children, const gn_eval *d_child_out, const uint16_t *d_moves,
                            const uint32_t *d_goffsets, const uint16_t *d_gmoves, const gn_eval *d_grand_out,
                            const std::optional<RankHistory> &history, const int32_t *d_gext, int n_lines,
                            gn_line2 *d_lines, void *stream) {
  const RankHistory *h = history ? &*history : nullptr;
  Dev *d;
  if (int rc = rank_call_args(ctx, device_slot, n, d_parents, d_offsets, n_lines, d_lines, h, d)) return rc;
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  HIP_TRY(launch_rank_lines2(d_parents, n, d_offsets, d_children, d_child_out, d_moves, d_goffsets, d_gmoves, d_grand_out,
                             ctx->P, d->tables.p, n_lines, d_lines, h, d_gext, call.s));
  return GN_OK;
}

int gn_rank_lines2_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, const uint32_t *d_offsets,
                          const gn_board *d_children, const gn_eval *d_child_out, const uint16_t *d_moves,
                          const uint32_t *d_goffsets, const uint16_t *d_gmoves, const gn_eval *d_grand_out, int n_lines,
                          gn_line2 *d_lines, void *stream) {
  return rank_lines2_call(ctx, device_slot, d_parents, n, d_offsets, d_children, d_child_out, d_moves, d_goffsets,
                          d_gmoves, d_grand_out, std::nullopt, nullptr, n_lines, d_lines, stream);
}

int gn_rank_lines2_history_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                  const uint32_t *d_offsets, const gn_board *d_children, const gn_eval *d_child_out,
                                  const uint16_t *d_moves, const uint32_t *d_goffsets, const uint16_t *d_gmoves,
                                  const gn_eval *d_grand_out, const uint64_t *d_keys, size_t n_keys,
                                  const gn_history *d_hist, int n_lines, gn_line2 *d_lines, void *stream) {
  return rank_lines2_call(ctx, device_slot, d_parents, n, d_offsets, d_children, d_child_out, d_moves, d_goffsets,
                          d_gmoves, d_grand_out, RankHistory{d_keys, n_keys, d_hist}, nullptr, n_lines, d_lines, stream);
}

int gn_rank_lines2_extended_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                   const uint32_t *d_offsets, const gn_board *d_children, const gn_eval *d_child_out,
                                   const uint16_t *d_moves, const uint32_t *d_goffsets, const uint16_t *d_gmoves,
                                   const gn_eval *d_grand_out, const uint64_t *d_keys, size_t n_keys,
                                   const gn_history *d_hist, const int32_t *d_gext, int n_lines, gn_line2 *d_lines,
                                   void *stream) {
  return rank_lines2_call(ctx, device_slot, d_parents, n, d_offsets, d_children, d_child_out, d_moves, d_goffsets,
                          d_gmoves, d_grand_out, d_hist ? std::optional<RankHistory>({d_keys, n_keys, d_hist}) : std::nullopt,
                          d_gext, n_lines, d_lines, stream);
}

int gn_rank_lines2_ahead_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                const uint32_t *d_offsets, const gn_board *d_children, const gn_eval *d_child_out,
                                const uint16_t *d_moves, const uint32_t *d_goffsets, const uint16_t *d_gmoves,
                                const gn_eval *d_grand_out, const uint64_t *d_keys, size_t n_keys,
                                const gn_history *d_hist, const int32_t *d_gext, int ahead, int n_lines,
                                gn_line2 *d_lines, void *stream) {
  if (ahead < 0 || ahead > 1) return fail(GN_E_INVALID, "ahead %d outside 0..1", ahead);
  return rank_lines2_call(ctx, device_slot, d_parents, n, d_offsets, d_children, d_child_out, d_moves, d_goffsets,
                          d_gmoves, d_grand_out,
                          d_hist ? std::optional<RankHistory>({d_keys, n_keys, d_hist, (uint32_t)ahead}) : std::nullopt,
                          d_gext, n_lines, d_lines, stream);
}

// gn_rank_lines3_device and its history form (h NULL: the plain kernel, d_children unread)
static int rank_lines3_call(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, const uint32_t *d_offsets,
                            const uint16_t *d_moves, const gn_eval *d_child_out, size_t total,
                            const gn_line2 *d_child_lines, const gn_pv *d_child_pvs, const gn_board *d_children,
                            const RankHistory *h, int n_lines, gn_line3 *d_lines, gn_pv *d_pvs, void *stream) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad context or device slot");
  if (int rc = check_n_lines(n_lines)) return rc;
  if (d_pvs && !d_child_pvs) return fail(GN_E_INVALID, "d_pvs without d_child_pvs");
  if (n && !d_lines) return fail(GN_E_INVALID, "NULL buffer");
  if (n && total && (!d_parents || !d_offsets || !d_moves || !d_child_out || !d_child_lines || (h && !d_children)))
    return fail(GN_E_INVALID, "NULL buffer");
  if (n && total && h && h->n_keys && !h->keys) return fail(GN_E_INVALID, "d_keys is NULL");
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  HIP_TRY(launch_rank_lines3(d_parents, n, d_offsets, d_moves, d_child_out, total, d_child_lines, d_child_pvs, ctx->P,
                             d->tables.p, n_lines, d_lines, d_pvs, call.s, d_children, h));
  return GN_OK;
}

int gn_rank_lines3_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, const uint32_t *d_offsets,
                          const uint16_t *d_moves, const gn_eval *d_child_out, size_t total, const gn_line2 *d_child_lines,
                          const gn_pv *d_child_pvs, int n_lines, gn_line3 *d_lines, gn_pv *d_pvs, void *stream) {
  return rank_lines3_call(ctx, device_slot, d_parents, n, d_offsets, d_moves, d_child_out, total, d_child_lines,
                          d_child_pvs, nullptr, nullptr, n_lines, d_lines, d_pvs, stream);
}

int gn_rank_lines3_history_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                  const uint32_t *d_offsets, const uint16_t *d_moves, const gn_eval *d_child_out,
                                  size_t total, const gn_line2 *d_child_lines, const gn_pv *d_child_pvs,
                                  const gn_board *d_children, const uint64_t *d_keys, size_t n_keys,
                                  const gn_history *d_hist, int n_lines, gn_line3 *d_lines, gn_pv *d_pvs, void *stream) {
  const RankHistory h = {d_keys, n_keys, d_hist};
  return rank_lines3_call(ctx, device_slot, d_parents, n, d_offsets, d_moves, d_child_out, total, d_child_lines,
                          d_child_pvs, d_children, d_hist ? &h : nullptr, n_lines, d_lines, d_pvs, stream);
}

int gn_time_expand_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, int mode, int iters,
                          float *ms_total, size_t *total, float *stage_ms, uint64_t *ft_rows, gn_eval *d_parent_out,
                          uint32_t *d_offsets, uint16_t *d_moves, gn_eval *d_child_out, size_t cap) {
  Dev *d = slot(ctx, device_slot);
  if (!d || !ms_total || !total || iters <= 0) return fail(GN_E_INVALID, "bad argument");
  DevCall call(*d);
  if (call.rc) return call.rc;
  const hipStream_t s = call.s;
  Events events;
  hipEvent_t begin, end;
  HIP_TRY(events.make({&begin, &end}));
  std::vector<ExpEvents> marks((size_t)iters);
  for (ExpEvents &e : marks) HIP_TRY(e.create(events));
  HIP_TRY(d->sum.ensure(2)); // [0] rows by write_children's formula, [1] rows the row stream gathered
  HIP_TRY(hipMemsetAsync(d->sum.p, 0, 2 * sizeof(unsigned long long), s));
  HIP_TRY(hipEventRecord(begin, s));
  const bool pipe = pipelined(ctx, *d, mode, (size_t)iters);
  size_t t = 0;
  int rc = run_expansions(
      ctx, *d, mode, (size_t)iters, 0,
      [&](size_t it, ExpStep &st) -> int {
        st.parents = d_parents, st.n = n, st.parent_out = d_parent_out, st.child_out = d_child_out;
        // (pipelined, the moves go into the set's own buffer: the caller's is written once, after
        // the last expansion)
        st.moves = pipe ? nullptr : d_moves;
        if (d_moves || d_child_out) st.cap = cap;
        st.ev = &marks[it];
        st.rows = it == 0 ? d->sum.p : nullptr;
        return GN_OK;
      },
      [&](size_t it, size_t children) -> int {
        t = children;
        HIP_TRY(hipEventRecord(marks[it].scored, s));
        return GN_OK;
      });
  *total = t;
  if (rc) return rc;
  if (pipe && d_moves && t)
    HIP_TRY(hipMemcpyAsync(d_moves, d->cur.child_moves, t * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
  if (d_offsets) HIP_TRY(launch_offsets_u32(d->cur.offsets.p, n + 1, d_offsets, s));
  HIP_TRY(hipEventRecord(end, s));
  HIP_TRY(hipEventSynchronize(end));
  HIP_TRY(hipEventElapsedTime(ms_total, begin, end));
  // The eight public stages (include/gpu_nnue.h) and the planned big net's three parts, each a span
  // between two marks of an iteration, averaged over the iterations.  Pipelined, the front's stages
  // are on the second stream, and two spans differ: the big net is its plan plus its row stream
  // from the stream's own start (behind its wait for the plan), and the stream's part starts there.
  using E = ExpEvents;
  struct Span {
    hipEvent_t E::*from, E::*to;
  };
  constexpr Span STAGE_SPANS[8] = {{&E::start, &E::counted},         {&E::counted, &E::total_read},
                                   {&E::total_read, &E::written},    {&E::written, &E::classified},
                                   {&E::classified, &E::small_done}, {&E::small_done, &E::big_done},
                                   {&E::big_done, &E::finalized},    {&E::finalized, &E::scored}};
  constexpr int BIG_NET = 5;
  constexpr Span PLAN = {&E::small_done, &E::plan_done}, STREAM = {&E::plan_done, &E::stream_done},
                 FINISH = {&E::stream_done, &E::big_done}, // (the sliced stream's finish)
      PIPE_BIG_NET_STREAM = {&E::stream_begun, &E::big_done}, PIPE_STREAM = {&E::stream_begun, &E::stream_done};
  float stage[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pl = 0, st = 0, fi = 0;
  for (const ExpEvents &e : marks) {
    auto add_ms = [&](float &acc, const Span &sp) -> hipError_t {
      float ms = 0;
      const hipError_t r = hipEventElapsedTime(&ms, e.*sp.from, e.*sp.to);
      acc += ms / (float)iters;
      return r;
    };
    for (int k = 0; k < 8 && stage_ms; ++k)
      if (pipe && k == BIG_NET) {
        HIP_TRY(add_ms(stage[k], PLAN));
        HIP_TRY(add_ms(stage[k], PIPE_BIG_NET_STREAM));
      } else {
        HIP_TRY(add_ms(stage[k], STAGE_SPANS[k]));
      }
    if (!d->cur.planned) continue; // the big net's two kernels apart
    HIP_TRY(add_ms(pl, PLAN));
    HIP_TRY(add_ms(st, pipe ? PIPE_STREAM : STREAM));
    HIP_TRY(add_ms(fi, FINISH));
  }
  if (stage_ms) std::copy(stage, stage + 8, stage_ms);
  if (d->cur.planned) d->plan_ms = pl, d->stream_ms = st, d->finish_ms = fi;
  if ((rc = check_plan(*d, s)) != GN_OK) return rc;
  if (pipe) { // (the other set's expansion too)
    swap_sets(*d);
    rc = check_plan(*d, s);
    swap_sets(*d);
    if (rc) return rc;
  }
  if (ft_rows) {
    unsigned long long r[2] = {0, 0};
    HIP_TRY(hipMemcpy(r, d->sum.p, sizeof(r), hipMemcpyDeviceToHost));
    *ft_rows = ctx->incremental ? (r[1] ? r[1] : r[0]) : 0; // the row stream's own count when it ran
  }
  return GN_OK;
}

int gn_checksum_device(gn_ctx *ctx, int device_slot, const void *d_ptr, size_t bytes, uint64_t *sum) {
  Dev *d = slot(ctx, device_slot);
  if (!d || !sum || (bytes && !d_ptr)) return fail(GN_E_INVALID, "bad argument");
  if ((uintptr_t)d_ptr & 7) return fail(GN_E_INVALID, "d_ptr is not 8-byte aligned"); // the kernel loads 8-byte words
  DevCall call(*d);
  if (call.rc) return call.rc;
  HIP_TRY(d->sum.ensure(2));
  HIP_TRY(hipMemsetAsync(d->sum.p, 0, sizeof(unsigned long long), d->stream));
  HIP_TRY(launch_checksum(d_ptr, bytes, d->sum.p, d->stream));
  unsigned long long r = 0;
  HIP_TRY(hipMemcpyAsync(&r, d->sum.p, sizeof(r), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  *sum = r;
  return GN_OK;
}

int gn_random_games_device(gn_ctx *ctx, int device_slot, uint64_t seed, size_t first_game, size_t n_games, int plies,
                           gn_board *d_out, void *stream) {
  Dev *d = slot(ctx, device_slot);
  if (!d) return fail(GN_E_INVALID, "bad context or device slot");
  if (n_games && !d_out) return fail(GN_E_INVALID, "NULL buffer");
  if (plies < 0 || plies > 1000) return fail(GN_E_INVALID, "plies out of range");
  DevCall call(*d, stream);
  if (call.rc) return call.rc;
  HIP_TRY(launch_random_games(seed, first_game, n_games, plies, d->tables.p, d_out, call.s));
  return GN_OK;
}

int gn_set_option(gn_ctx *ctx, int option, int64_t value) {
  if (!ctx) return fail(GN_E_INVALID, "ctx is NULL");
  if (option == GN_OPT_QUIESCE_SEE) { // stored before the generation moves; a bad value changes nothing
    if (value != 0 && value != 1) return fail(GN_E_INVALID, "GN_OPT_QUIESCE_SEE %lld not 0 or 1", (long long)value);
    ctx->quiesce_see = value != 0;
    ++ctx->graph_gen;
    return GN_OK;
  }
  ++ctx->graph_gen; // (the small-batch graphs hold the options they were captured with)
  switch (option) {
  case GN_OPT_INCREMENTAL_CHILDREN:
    ctx->incremental = value != 0;
    return GN_OK;
  case GN_OPT_XCD_SWIZZLE:
    ctx->swizzle = (int)(value & 15);
    return GN_OK;
  case GN_OPT_KING_SORT:
    if (value < 0 || value > 2) return fail(GN_E_INVALID, "king sort must be 0, 1 or 2");
    ctx->king_sort = (int)value;
    return GN_OK;
  case GN_OPT_KING_CACHE:
    ctx->king_cache = value != 0;
    return GN_OK;
  case GN_OPT_CHAIN:
    if (value < -(1 << 20) || value > (1 << 20)) return fail(GN_E_INVALID, "chain length out of range");
    ctx->chain = (int)value;
    return GN_OK;
  case GN_OPT_STREAM_SLICES:
    if (value != 1 && value != 3) return fail(GN_E_INVALID, "stream slices must be 1 or 3");
    ctx->stream_slices = (int)value;
    return GN_OK;
  case GN_OPT_CHUNK_PARENTS:
    if (value < 0) return fail(GN_E_INVALID, "chunk size < 0");
    ctx->chunk_parents = value;
    return GN_OK;
  case GN_OPT_COALESCE:
    ctx->coalesce = value != 0;
    return GN_OK;
  case GN_OPT_FAST_BATCH:
    ctx->fast_batch = value != 0;
    return GN_OK;
  case GN_OPT_EXPAND_PIPELINE:
    if (value < 0 || value > 2) return fail(GN_E_INVALID, "GN_OPT_EXPAND_PIPELINE %lld not in 0..2", (long long)value);
    ctx->pipeline = (int)value;
    return GN_OK;
  default:
    return fail(GN_E_INVALID, "unknown option %d", option);
  }
}

int gn_get_option(const gn_ctx *ctx, int option, int64_t *value) {
  if (!ctx || !value) return fail(GN_E_INVALID, "NULL argument");
  switch (option) {
  case GN_OPT_INCREMENTAL_CHILDREN:
    *value = ctx->incremental;
    return GN_OK;
  case GN_OPT_XCD_SWIZZLE:
    *value = ctx->swizzle;
    return GN_OK;
  case GN_OPT_KING_SORT:
    *value = ctx->king_sort;
    return GN_OK;
  case GN_OPT_KING_CACHE:
    *value = ctx->king_cache;
    return GN_OK;
  case GN_OPT_CHAIN:
    *value = ctx->chain;
    return GN_OK;
  case GN_OPT_STREAM_SLICES:
    *value = ctx->stream_slices;
    return GN_OK;
  case GN_OPT_CHUNK_PARENTS:
    *value = ctx->chunk_parents;
    return GN_OK;
  case GN_OPT_COALESCE:
    *value = ctx->coalesce;
    return GN_OK;
  case GN_OPT_FAST_BATCH:
    *value = ctx->fast_batch;
    return GN_OK;
  case GN_OPT_EXPAND_PIPELINE:
    *value = ctx->pipeline;
    return GN_OK;
  case GN_OPT_QUIESCE_SEE:
    *value = ctx->quiesce_see;
    return GN_OK;
  case GN_STAT_FAST_BATCHES:
    *value = (int64_t)ctx->fast_runs.load();
    return GN_OK;
  case GN_STAT_FAST_FALLBACKS:
    *value = (int64_t)ctx->fast_fallbacks.load();
    return GN_OK;
  case GN_STAT_BATCH_LAUNCHES:
  case GN_STAT_BATCH_CALLS: { // cumulative since load (the coalescer's counters)
    auto &C = const_cast<gn_ctx *>(ctx)->co;
    std::lock_guard<std::mutex> lk(C.mu);
    *value = (int64_t)(option == GN_STAT_BATCH_LAUNCHES ? C.launches : C.calls);
    return GN_OK;
  }
  case GN_STAT_PLAN_NS:
  case GN_STAT_STREAM_NS:
  case GN_STAT_FINISH_NS: { // read-only: the last gn_time_expand_device's planned kernels (max over devices)
    float m = 0;
    for (auto &dp : ctx->devs)
      m = std::max(m, option == GN_STAT_PLAN_NS     ? dp->plan_ms
                      : option == GN_STAT_STREAM_NS ? dp->stream_ms
                                                    : dp->finish_ms);
    *value = (int64_t)((double)m * 1e6);
    return GN_OK;
  }
  case GN_STAT_HOST_PARSE_NS:
  case GN_STAT_HOST_TOTAL_NS:
    *value = (int64_t)((option == GN_STAT_HOST_PARSE_NS ? ctx->t_parse : ctx->t_total) * 1e6);
    return GN_OK;
  case GN_STAT_HOST_UPLOAD_NS:
  case GN_STAT_HOST_REPLAY_NS:
  case GN_STAT_HOST_COMPUTE_NS:
  case GN_STAT_HOST_DOWNLOAD_NS:
  case GN_STAT_RANK_NS:
  case GN_STAT_RANK2_NS:
  case GN_STAT_RANK3_NS:
  case GN_STAT_KEYS_NS:
  case GN_STAT_PV_NS:
  case GN_STAT_HOST_TAIL_NS: { // the last host-buffer call, max over devices
    double m = 0;
    for (auto &dp : ctx->devs) {
      const Dev &d = *dp;
      m = std::max(m, option == GN_STAT_HOST_UPLOAD_NS    ? d.t_upload
                      : option == GN_STAT_HOST_REPLAY_NS  ? d.t_replay
                      : option == GN_STAT_HOST_COMPUTE_NS ? d.t_compute
                      : option == GN_STAT_HOST_DOWNLOAD_NS ? d.t_download
                      : option == GN_STAT_RANK_NS          ? d.t_rank
                      : option == GN_STAT_RANK2_NS         ? d.t_rank2
                      : option == GN_STAT_RANK3_NS         ? d.t_rank3
                      : option == GN_STAT_KEYS_NS          ? d.t_keys
                      : option == GN_STAT_PV_NS            ? d.t_pv
                                                           : d.t_tail);
    }
    *value = (int64_t)(m * 1e6);
    return GN_OK;
  }
  case GN_STAT_EXTEND_NS: // the last host-buffer call's leaf stage, by the rule it ran: its time, the
  case GN_STAT_QUIESCE_NS: // slowest device; the leaves it valued and the nodes it evaluated below
  case GN_STAT_EXTENDED_LEAVES: // them, summed over the devices
  case GN_STAT_QUIESCE_LEAVES:
  case GN_STAT_QUIESCE_NODES: {
    const bool checks = option == GN_STAT_EXTEND_NS || option == GN_STAT_EXTENDED_LEAVES;
    double ms = 0;
    uint64_t leaves = 0, nodes = 0;
    for (auto &dp : ctx->devs) {
      const Dev::LeafStage::Stats &st = dp->leaf.stats[checks ? LeafRule::CHECKS : LeafRule::QUIESCE];
      ms = std::max(ms, st.ms), leaves += st.leaves, nodes += st.nodes;
    }
    const bool time = option == GN_STAT_EXTEND_NS || option == GN_STAT_QUIESCE_NS;
    *value = time ? (int64_t)(ms * 1e6) : (int64_t)(option == GN_STAT_QUIESCE_NODES ? nodes : leaves);
    return GN_OK;
  }
  case GN_STAT_ZERO_ROW_ENTRIES: // ... and its entries on the zero row summed
  case GN_STAT_SCRATCH_PADS: { // read-only: the last planned expansion's GN_SCR_GAP no-op entries, summed
    int64_t sum = 0;
    for (auto &dp : ctx->devs) {
      Dev &d = *dp;
      std::lock_guard<std::mutex> lk(d.mu);
      if (!d.cur.pstat.p) continue;
      HIP_TRY(hipSetDevice(d.id));
      if (d.done_on) HIP_TRY(hipEventSynchronize(d.done));
      unsigned long long v[2] = {0, 0};
      HIP_TRY(hipMemcpy(v, d.cur.pstat.p, sizeof(v), hipMemcpyDeviceToHost));
      sum += (int64_t)(option == GN_STAT_SCRATCH_PADS ? v[0] : v[1]);
    }
    *value = sum;
    return GN_OK;
  }
  default:
    return fail(GN_E_INVALID, "unknown option %d", option);
  }
}

int gn_expand_and_evaluate(gn_ctx *ctx, const char *const *parent_fens, size_t n, int mode, gn_eval *parent_out,
                           uint32_t *child_offsets, uint16_t *child_moves, gn_child *child_out, size_t cap) {
  if (!slot(ctx, 0)) return fail(GN_E_INVALID, "bad context");
  if (n && (!parent_fens || !child_offsets)) return fail(GN_E_INVALID, "NULL argument");
  if (!n) {
    if (child_offsets) child_offsets[0] = 0;
    return GN_OK;
  }
  return on_packed_fens(ctx, parent_fens, n, [&](const gn_board *boards) -> int {
    return expand_boards_host(ctx, boards, n, mode, parent_out, child_offsets, child_moves, child_out, cap);
  });
}

// One chunk of the two-ply lines (gn_evaluate_lines2, gn_evaluate_games_lines2; the three-ply calls,
// with a root chunk's children as the parents): the mp device-resident parents' depth-2 expansion into
// the device's Lines2 buffers (expand2_on), the leaf stage where the rule extends (extend_stage; the
// children as parents, the library's own boards), rank_lines2_kernel -- its history variant when h
// names the keys and these parents' gn_history entries (h.hist NULL: the plain one) -- and, with d_pvs,
// the PVs' assembly (the quiescent rule's leaf stage leaves the grandchildren's tails).  The parents'
// records go to x.po, the lines to d_lines and the PVs to d_pvs (NULL: none), all on the device; the
// stream is idle on return, and the chunk's times are added to the device's stage times.
static int lines2_compute(gn_ctx *ctx, Dev &d, const gn_board *par, size_t mp, int mode, int K, const RankHistory &h,
                          LeafRule leaf, gn_line2 *d_lines, gn_pv *d_pvs) {
  hipStream_t s = d.stream;
  Dev::Lines2 &x = d.l2;
  const std::function<int(size_t, size_t, Expand2Grand &)> size_grand = [&](size_t t, size_t g, Expand2Grand &gr) -> int {
    HIP_TRY(x.goff.ensure(t + 1));
    HIP_TRY(x.gmv.ensure(std::max<size_t>(g, 1)));
    HIP_TRY(x.gco.ensure(std::max<size_t>(g, 1)));
    gr = Expand2Grand{x.goff.p, x.gmv.p, x.gco.p, std::max<size_t>(g, 1)};
    return GN_OK;
  };
  const bool tails = d_pvs && leaf.kind == LeafRule::QUIESCE; // (the check extension's replies are not reported)
  const auto t0 = Clock::now();
  size_t t = 0, g = 0;
  HIP_TRY(count_children(d, par, mp, s, &t));
  const size_t cap = std::max<size_t>(t, 1);
  HIP_TRY(x.po.ensure(mp));
  HIP_TRY(x.off.ensure(mp + 1));
  HIP_TRY(x.ch.ensure(cap));
  HIP_TRY(x.mv.ensure(cap));
  HIP_TRY(x.co.ensure(cap));
  int rc = expand2_on(ctx, &d, par, mp, mode, x.po.p, x.off.p, x.ch.p, x.mv.p, x.co.p, cap, Expand2Grand{}, &t, &g, s,
                      &size_grand);
  if (rc) return rc;
  if (leaf.extends()) { // (t == 0 or g == 0: nothing is read)
    HIP_TRY(x.gext.ensure(std::max<size_t>(g, 1)));
    if (tails) HIP_TRY(x.gtail.ensure(std::max<size_t>(g, 1) * GN_MAX_QUIESCE_DEPTH));
    rc = extend_stage(ctx, d, PackedLeaves{x.ch.p, t, x.goff.p, x.gmv.p, x.gco.p, g}, mode, leaf, x.gext.p,
                      tails ? x.gtail.p : nullptr, s);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(d.rev[0], s));
  HIP_TRY(launch_rank_lines2(par, mp, x.off.p, x.ch.p, x.co.p, x.mv.p, x.goff.p, x.gmv.p, x.gco.p, ctx->P, d.tables.p, K,
                             d_lines, h.hist ? &h : nullptr, leaf.extends() ? x.gext.p : nullptr, s));
  HIP_TRY(hipEventRecord(d.rev[1], s));
  if (d_pvs) { // (g == 0: no line is searched, and the tails are not read)
    HIP_TRY(hipEventRecord(d.pev[2], s));
    HIP_TRY(launch_line2_pvs(mp, x.off.p, x.mv.p, x.goff.p, x.gmv.p, tails ? x.gtail.p : nullptr, d_lines, K, d_pvs, s));
    HIP_TRY(hipEventRecord(d.pev[3], s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, d.rev[0], d.rev[1]));
  d.t_rank2 += ms;
  if (d_pvs) {
    HIP_TRY(hipEventElapsedTime(&ms, d.pev[2], d.pev[3]));
    d.t_pv += ms;
  }
  d.t_compute += ms_since(t0);
  return GN_OK;
}

// the ranked-lines calls' parents per chunk (GN_OPT_CHUNK_PARENTS; 0: 1,024 parents, ~1 M
// grandchildren: a few hundred MB of records, boards and partial sums)
static size_t lines_chunk(const gn_ctx *ctx) { return ctx->chunk_parents > 0 ? (size_t)ctx->chunk_parents : 1024; }

// A shard's two-ply lines (gn_evaluate_lines2, gn_evaluate_games_lines2): its m device-resident
// parents in chunks of chunk parents; per chunk lines2_compute into the device's Lines2 buffers and
// one download of the chunk's parent records and lines (and, with pvs, the _pv calls, its PVs) into
// out / lines / pvs (the shard's first parent's).  history: the shard's keys and its parents'
// gn_history entries (hist NULL: none); the chunks need no cut at game starts: the keys are the whole
// shard's.
static int lines2_chunks(gn_ctx *ctx, Dev &d, const gn_board *parents, size_t m, int mode, int K, gn_eval *out,
                         gn_line2 *lines, const RankHistory &history, LeafRule leaf, gn_pv *pvs = nullptr) {
  hipStream_t s = d.stream;
  Dev::Lines2 &x = d.l2;
  const size_t chunk = lines_chunk(ctx);
  for (size_t a = 0; a < m; a += chunk) {
    const size_t mp = std::min(chunk, m - a);
    HIP_TRY(x.ln.ensure(mp * (size_t)K));
    if (pvs) HIP_TRY(x.pv.ensure(mp * (size_t)K));
    const RankHistory h = {history.keys, history.n_keys, history.hist ? history.hist + a : nullptr};
    if (int rc = lines2_compute(ctx, d, parents + a, mp, mode, K, h, leaf, x.ln.p, pvs ? x.pv.p : nullptr)) return rc;
    const auto t0 = Clock::now();
    HIP_TRY(hipMemcpyAsync(out + a, x.po.p, mp * sizeof(gn_eval), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(lines + a * (size_t)K, x.ln.p, mp * (size_t)K * sizeof(gn_line2), hipMemcpyDeviceToHost, s));
    if (pvs) HIP_TRY(hipMemcpyAsync(pvs + a * (size_t)K, x.pv.p, mp * (size_t)K * sizeof(gn_pv), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    d.t_download += ms_since(t0);
  }
  return GN_OK;
}

// A shard's three-ply lines (gn_evaluate_lines3, gn_evaluate_games_lines3; the rule at gn_line3): its
// m device-resident roots in chunks of chunk roots.  Per chunk: the depth-1 expansion into the
// device's Lines3 buffers (expand_level: the root records, the child boards, moves and records); the
// children as parents through lines2_compute with K = 1, the call's leaf rule and, without a history,
// none, in chunks of the same number of children, cut wherever they fall, each child's line 1 (and,
// with pvs, its PV) written beside its record and never downloaded; rank_lines3_kernel; one download
// of the chunk's root records, lines and (with pvs) PVs.
// history (gn_evaluate_games_lines3_history; hist NULL: none): the shard's keys and its roots'
// gn_history entries.  A chunk's entries are spread to its children (launch_spread_history; its
// device time is in no stage statistic, only in the host total), whose chunks index them as they
// index the child boards and run the two-ply history ranking one ply ahead of the game
// (RankHistory::ahead = 1); the root step is the history variant.  A drawn child's two-ply line is
// computed all the same and dropped by the root step.
static int lines3_chunks(gn_ctx *ctx, Dev &d, const gn_board *roots, size_t m, int mode, int K, gn_eval *out,
                         gn_line3 *lines, const RankHistory &history, LeafRule leaf, gn_pv *pvs) {
  hipStream_t s = d.stream;
  Dev::Lines3 &x = d.l3;
  const size_t chunk = lines_chunk(ctx);
  for (size_t a = 0; a < m; a += chunk) {
    const size_t mp = std::min(chunk, m - a);
    const gn_board *par = roots + a;
    auto t0 = Clock::now();
    size_t t = 0;
    HIP_TRY(count_children(d, par, mp, s, &t));
    const size_t cap = std::max<size_t>(t, 1);
    HIP_TRY(x.po.ensure(mp));
    HIP_TRY(x.off.ensure(mp + 1));
    HIP_TRY(x.ch.ensure(cap));
    HIP_TRY(x.mv.ensure(cap));
    HIP_TRY(x.co.ensure(cap));
    HIP_TRY(x.cln.ensure(cap));
    if (pvs) HIP_TRY(x.cpv.ensure(cap));
    HIP_TRY(x.ln.ensure(mp * (size_t)K));
    if (pvs) HIP_TRY(x.pv.ensure(mp * (size_t)K));
    LevelOpts root;
    root.children = x.ch.p;
    if (int rc = expand_level(ctx, d, par, mp, mode, x.po.p, x.off.p, x.mv.p, x.co.p, cap, &t, s, root)) return rc;
    const RankHistory h = {history.keys, history.n_keys, history.hist ? history.hist + a : nullptr};
    if (h.hist) {
      HIP_TRY(x.chist.ensure(cap));
      HIP_TRY(launch_spread_history(h.hist, mp, x.off.p, t, x.chist.p, s));
    }
    d.t_compute += ms_since(t0);
    for (size_t b = 0; b < t; b += chunk) { // (lines2_compute adds its own time)
      const RankHistory hc = {h.keys, h.n_keys, h.hist ? x.chist.p + b : nullptr, 1};
      if (int rc = lines2_compute(ctx, d, x.ch.p + b, std::min(chunk, t - b), mode, 1, hc, leaf, x.cln.p + b,
                                  pvs ? x.cpv.p + b : nullptr))
        return rc;
    }
    t0 = Clock::now();
    HIP_TRY(hipEventRecord(d.r3ev[0], s));
    HIP_TRY(launch_rank_lines3(par, mp, x.off.p, x.mv.p, x.co.p, t, x.cln.p, pvs ? x.cpv.p : nullptr, ctx->P, d.tables.p, K,
                               x.ln.p, pvs ? x.pv.p : nullptr, s, x.ch.p, h.hist ? &h : nullptr));
    HIP_TRY(hipEventRecord(d.r3ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, d.r3ev[0], d.r3ev[1]));
    d.t_rank3 += ms;
    d.t_compute += ms_since(t0), t0 = Clock::now();
    HIP_TRY(hipMemcpyAsync(out + a, x.po.p, mp * sizeof(gn_eval), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(lines + a * (size_t)K, x.ln.p, mp * (size_t)K * sizeof(gn_line3), hipMemcpyDeviceToHost, s));
    if (pvs) HIP_TRY(hipMemcpyAsync(pvs + a * (size_t)K, x.pv.p, mp * (size_t)K * sizeof(gn_pv), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    d.t_download += ms_since(t0);
  }
  return GN_OK;
}

// gn_evaluate_lines2: the boards sharded equally over the devices, each shard uploaded and run
// through lines2_chunks
static int lines2_boards_host(gn_ctx *ctx, const gn_board *boards, size_t n, int mode, int K, gn_eval *out,
                              gn_line2 *lines, LeafRule leaf, gn_pv *pvs) {
  const size_t nd = ctx->devs.size();
  std::vector<size_t> b(nd + 1);
  partition(nullptr, n, (int)nd, b.data());
  const auto locks = lock_devices(ctx);
  return run_shards(ctx, b, [&](size_t, Dev &d, size_t lo, size_t hi) -> int {
    const auto t0 = Clock::now();
    HIP_TRY(d.par.ensure(hi - lo));
    HIP_TRY(hipMemcpyAsync(d.par.p, boards + lo, (hi - lo) * sizeof(gn_board), hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    d.t_upload += ms_since(t0);
    return lines2_chunks(ctx, d, d.par.p, hi - lo, mode, K, out + lo, lines + lo * (size_t)K, NO_HISTORY, leaf,
                         pvs ? pvs + lo * (size_t)K : nullptr);
  });
}

// (declared with the games phases above) the shard's lines go into the caller's arrays when it is
// in place, or into its vectors to be scattered
static int games_lines2(const GamesCall &c, GameShard &sh, Dev &d) {
  const int rc = games_gather(c, sh, d);
  if (rc) return rc;
  gn_line2 *const ln = sh.in_place ? c.lines2 + sh.p0 * (size_t)c.n_lines : sh.l2res.data();
  return lines2_chunks(c.ctx, d, sh.parents_of(d), sh.m, c.mode, c.n_lines, sh.records_of(c.position_out), ln,
                       c.history ? RankHistory{d.rkeys.p, d.n_rkeys, d.hist.p} : NO_HISTORY, c.leaf,
                       !c.pvs ? nullptr : sh.in_place ? c.pvs + sh.p0 * (size_t)c.n_lines : sh.pvres.data());
}

// ... and the same two for the three-ply lines
static int lines3_boards_host(gn_ctx *ctx, const gn_board *boards, size_t n, int mode, int K, gn_eval *out,
                              gn_line3 *lines, LeafRule leaf, gn_pv *pvs) {
  const size_t nd = ctx->devs.size();
  std::vector<size_t> b(nd + 1);
  partition(nullptr, n, (int)nd, b.data());
  const auto locks = lock_devices(ctx);
  return run_shards(ctx, b, [&](size_t, Dev &d, size_t lo, size_t hi) -> int {
    const auto t0 = Clock::now();
    HIP_TRY(d.par.ensure(hi - lo));
    HIP_TRY(hipMemcpyAsync(d.par.p, boards + lo, (hi - lo) * sizeof(gn_board), hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    d.t_upload += ms_since(t0);
    return lines3_chunks(ctx, d, d.par.p, hi - lo, mode, K, out + lo, lines + lo * (size_t)K, NO_HISTORY, leaf,
                         pvs ? pvs + lo * (size_t)K : nullptr);
  });
}
static int games_lines3(const GamesCall &c, GameShard &sh, Dev &d) {
  const int rc = games_gather(c, sh, d);
  if (rc) return rc;
  gn_line3 *const ln = sh.in_place ? c.lines3 + sh.p0 * (size_t)c.n_lines : sh.l3res.data();
  return lines3_chunks(c.ctx, d, sh.parents_of(d), sh.m, c.mode, c.n_lines, sh.records_of(c.position_out), ln,
                       c.history ? RankHistory{d.rkeys.p, d.n_rkeys, d.hist.p} : NO_HISTORY, c.leaf,
                       !c.pvs ? nullptr : sh.in_place ? c.pvs + sh.p0 * (size_t)c.n_lines : sh.pvres.data());
}

// The three-ply calls' leaf and depth (include/gpu_nnue.h at gn_line3) as a LeafRule; the quiescent
// rule's depth is 1..GN_MAX_QUIESCE_DEPTH3 here: three moves and the tail fit a gn_pv
static int leaf_rule3(const gn_ctx *ctx, int leaf, int depth, LeafRule &rule) {
  if (leaf < GN_LEAF_STATIC || leaf > GN_LEAF_QUIESCE) return fail(GN_E_INVALID, "leaf rule %d outside 0..2", leaf);
  if (leaf == GN_LEAF_QUIESCE && (depth < 1 || depth > GN_MAX_QUIESCE_DEPTH3))
    return fail(GN_E_INVALID, "quiescence depth %d outside 1..%d", depth, GN_MAX_QUIESCE_DEPTH3);
  if (leaf != GN_LEAF_QUIESCE && depth != 0) return fail(GN_E_INVALID, "depth %d with a leaf rule that takes none", depth);
  rule = leaf == GN_LEAF_QUIESCE ? LeafRule::quiesce(ctx, depth) : leaf == GN_LEAF_CHECKS ? LeafRule::checks() : LeafRule{};
  return GN_OK;
}

// The FEN lines2 calls
static int evaluate_lines2(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines, LeafRule leaf,
                           gn_eval *out, gn_line2 *lines, gn_pv *pvs = nullptr) {
  if (int rc = check_leaf_rule(leaf)) return rc;
  if (!slot(ctx, 0)) return fail(GN_E_INVALID, "bad context");
  if (int rc = check_n_lines(n_lines)) return rc;
  if (n && (!fens || !out || !lines)) return fail(GN_E_INVALID, "NULL argument");
  if (!n) return GN_OK;
  return on_packed_fens(ctx, fens, n, [&](const gn_board *boards) -> int {
    return lines2_boards_host(ctx, boards, n, mode, n_lines, out, lines, leaf, pvs);
  });
}

int gn_evaluate_lines2(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines, gn_eval *out,
                       gn_line2 *lines) {
  return evaluate_lines2(ctx, fens, n, mode, n_lines, LeafRule{}, out, lines);
}

int gn_evaluate_lines2_extended(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines, gn_eval *out,
                                gn_line2 *lines) {
  return evaluate_lines2(ctx, fens, n, mode, n_lines, LeafRule::checks(), out, lines);
}

int gn_evaluate_lines2_quiescent(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines, int depth,
                                 gn_eval *out, gn_line2 *lines) {
  return evaluate_lines2(ctx, fens, n, mode, n_lines, LeafRule::quiesce(ctx, depth), out, lines);
}

int gn_evaluate_lines2_quiescent_pv(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines, int depth,
                                    gn_eval *out, gn_line2 *lines, gn_pv *pvs) {
  if (n && !pvs) return fail(GN_E_INVALID, "pvs is NULL");
  return evaluate_lines2(ctx, fens, n, mode, n_lines, LeafRule::quiesce(ctx, depth), out, lines, pvs);
}

int gn_evaluate_lines3(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines, int leaf, int depth,
                       gn_eval *out, gn_line3 *lines, gn_pv *pvs) {
  if (!slot(ctx, 0)) return fail(GN_E_INVALID, "bad context");
  if (int rc = check_n_lines(n_lines)) return rc;
  LeafRule rule;
  if (int rc = leaf_rule3(ctx, leaf, depth, rule)) return rc;
  if (n && (!fens || !out || !lines)) return fail(GN_E_INVALID, "NULL argument");
  if (!n) return GN_OK;
  return on_packed_fens(ctx, fens, n, [&](const gn_board *boards) -> int {
    return lines3_boards_host(ctx, boards, n, mode, n_lines, out, lines, rule, pvs);
  });
}

static int evaluate_games_lines3(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines, int leaf,
                                 int depth, bool history, uint32_t *position_offsets, int32_t *game_status,
                                 gn_eval *position_out, size_t position_cap, gn_line3 *lines, gn_pv *pvs) {
  if (!slot(ctx, 0)) return fail(GN_E_INVALID, "bad context");
  if (int rc = check_n_lines(n_lines)) return rc;
  LeafRule rule;
  if (int rc = leaf_rule3(ctx, leaf, depth, rule)) return rc;
  if (n_games && !lines) return fail(GN_E_INVALID, "lines is NULL");
  return evaluate_games_lines(ctx, games, n_games, mode, n_lines, history, rule, position_offsets, game_status,
                              position_out, position_cap, lines, pvs);
}

int gn_evaluate_games_lines3(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines, int leaf,
                             int depth, uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                             size_t position_cap, gn_line3 *lines, gn_pv *pvs) {
  return evaluate_games_lines3(ctx, games, n_games, mode, n_lines, leaf, depth, false, position_offsets, game_status,
                               position_out, position_cap, lines, pvs);
}

int gn_evaluate_games_lines3_history(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines, int leaf,
                                     int depth, uint32_t *position_offsets, int32_t *game_status,
                                     gn_eval *position_out, size_t position_cap, gn_line3 *lines, gn_pv *pvs) {
  return evaluate_games_lines3(ctx, games, n_games, mode, n_lines, leaf, depth, true, position_offsets, game_status,
                               position_out, position_cap, lines, pvs);
}

int gn_perft(gn_ctx *ctx, const char *fen, int depth, uint64_t *nodes) {
  Dev *d = slot(ctx, 0);
  if (!d || !fen || !nodes) return fail(GN_E_INVALID, "bad argument");
  Board B;
  if (!parse_fen(fen, B)) return fail(GN_E_INVALID, "bad FEN");
  if (depth <= 0) {
    *nodes = 1;
    return GN_OK;
  }
  DevCall call(*d);
  if (call.rc) return call.rc;
  const hipStream_t s = call.s;
  gn_board root;
  pack(B, root);
  HIP_TRY(d->frontier.ensure(1));
  HIP_TRY(hipMemcpyAsync(d->frontier.p, &root, sizeof(root), hipMemcpyHostToDevice, s));
  size_t n = 1;
  for (int level = 1; level < depth; ++level) {
    size_t total = 0;
    int rc = generate_children(*d, d->frontier.p, n, nullptr, nullptr, &total, s);
    if (rc) return rc;
    std::swap(d->frontier, d->cur.children);
    n = total;
    if (!n) break;
  }
  unsigned long long sum = 0;
  if (n) {
    HIP_TRY(d->sum.ensure(1));
    HIP_TRY(hipMemsetAsync(d->sum.p, 0, sizeof(unsigned long long), s));
    HIP_TRY(launch_count_sum(d->frontier.p, n, d->tables.p, d->sum.p, s));
    HIP_TRY(hipMemcpyAsync(&sum, d->sum.p, sizeof(sum), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  *nodes = sum;
  return GN_OK;
}

// plan_snapshot.h (internal, for the tests): the current set's plan copied to host memory.
int gn_debug_plan_snapshot(gn_ctx *ctx, int device_slot, gn_plan_snapshot_header *header,
                           const gn_plan_snapshot_bufs *bufs) {
  Dev *d = slot(ctx, device_slot);
  if (!d || !header) return fail(GN_E_INVALID, "bad argument");
  DevCall call(*d);
  if (call.rc) return call.rc;
  HIP_TRY(hipStreamSynchronize(call.s));
  const ExpSet &x = d->cur;
  const PlanGeometry &g = x.plan_geo;
  if (!x.planned || !g.nblk || !x.plan_n)
    return fail(GN_E_INVALID, "the device slot's last expansion was not planned: no plan to copy");
  const size_t n = x.plan_n, K = g.K, nblk = g.nblk;
  std::vector<uint64_t> off(n + 1);
  std::vector<uint32_t> bt(nblk);
  HIP_TRY(hipMemcpy(off.data(), x.offsets.p, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(bt.data(), x.btiles.p, nblk * sizeof(uint32_t), hipMemcpyDeviceToHost));
  unsigned long long st[3] = {0, 0, 0};
  HIP_TRY(hipMemcpy(st, x.pstat.p, sizeof(st), hipMemcpyDeviceToHost));
  const size_t last = (nblk - 1) * K; // the last block's first parent
  gn_plan_snapshot_header h = {};
  h.header_bytes = (uint32_t)sizeof(h), h.tile_bytes = (uint32_t)sizeof(TileDesc);
  h.l1 = (uint32_t)d->net[BIG].L1, h.row_stride = ft_row_stride(h.l1);
  h.ft_rows = FT_ROWS, h.ft_bias_row = FT_BIAS_ROW, h.zero_row = ZERO_ROW, h.scr_rows = SCR_ROWS;
  h.ent_spare = ENT_SPARE, h.scr_gap = GN_SCR_GAP, h.ring = GN_RING, h.slice_ring = GN_SLICE_RING;
  h.np = (uint32_t)n, h.k = g.K, h.nblk = g.nblk, h.slices = g.sliced ? 3 : 1, h.xu = g.xu, h.hu = g.hu;
  h.kc = (uint32_t)g.kc, h.ordered = x.plan_ordered ? 1 : 0;
  h.npos = n + x.plan_total;
  h.n_ent = x.etot + (uint64_t)ENT_SPARE * nblk;
  // (the descriptors stay inside the allocation even where a broken plan's btiles does not)
  h.n_tiles = std::min<uint64_t>((last + off[last]) / 16 + (K + 2) * (nblk - 1) + bt[nblk - 1], x.tiles.cap);
  h.n_pinfo = g.sliced ? h.npos : 0;
  h.pads = st[0], h.zero_row_entries = st[1], h.rows = st[2];
  if (off[n] != x.plan_total) return fail(GN_E_INVALID, "the set's offsets are not the planned expansion's");
  *header = h;
  if (!bufs) return GN_OK;
  const struct {
    const char *name;
    void *dst;
    size_t cap, need, size;
    const void *src;
  } copies[] = {
      {"eoff", bufs->eoff, bufs->eoff_cap, n + 1, sizeof(uint64_t), x.eoff.p},
      {"ent", bufs->ent, bufs->ent_cap, (size_t)h.n_ent, sizeof(uint64_t), x.ent.p},
      {"tiles", bufs->tiles, bufs->tiles_cap, (size_t)h.n_tiles, sizeof(TileDesc), x.tiles.p},
      {"btiles", bufs->btiles, bufs->btiles_cap, nblk, sizeof(uint32_t), x.btiles.p},
      {"order", bufs->order, bufs->order_cap, nblk, sizeof(uint32_t), x.plan_ordered ? x.border.p : nullptr},
      {"pinfo", bufs->pinfo, bufs->pinfo_cap, (size_t)h.n_pinfo, 2 * sizeof(int32_t), x.pinfo.p},
      {"offsets", bufs->offsets, bufs->offsets_cap, n + 1, sizeof(uint64_t), x.offsets.p},
  };
  for (const auto &c : copies) {
    if (!c.need) continue;
    if (!c.dst || c.cap < c.need)
      return fail(GN_E_INVALID, "plan snapshot: buffer %s holds %zu elements, %zu needed", c.name, c.dst ? c.cap : 0, c.need);
    if (c.src) HIP_TRY(hipMemcpy(c.dst, c.src, c.need * c.size, hipMemcpyDeviceToHost));
    else
      for (size_t i = 0; i < c.need; ++i) static_cast<uint32_t *>(c.dst)[i] = (uint32_t)i; // (order: as they come)
  }
  return GN_OK;
}

// plan_snapshot.h (internal, for the tests): the big net's packed-partial-sum tables as the device holds them.
int gn_debug_part_offsets(gn_ctx *ctx, int device_slot, int32_t *part_off, int32_t *b0p) {
  Dev *d = slot(ctx, device_slot);
  if (!d || !part_off || !b0p) return fail(GN_E_INVALID, "bad argument");
  DevCall call(*d);
  if (call.rc) return call.rc;
  const NetDevice &n = d->net[BIG];
  if (!d->has[BIG] || !n.part_off || !n.b0p) return fail(GN_E_INVALID, "no 3072-wide big net is loaded");
  HIP_TRY(hipStreamSynchronize(call.s));
  HIP_TRY(hipMemcpy(part_off, n.part_off, (size_t)LAYER_STACKS * 3 * 16 * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(b0p, n.b0p, (size_t)LAYER_STACKS * 16 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return GN_OK;
}

} // extern "C"
