// device_util.h — device helpers shared by the kernels of libgpu_nnue (kernels.hip,
// stream.hip): wrapping integer ops, FT row loads, wave-parallel feature extraction
// (lane = square), the transform, and the one-wave layer stack.
#pragma once
#include <hip/hip_runtime.h>

#include "nnue.h"

namespace gn {

typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));
typedef int int4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int32_t wmul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
__device__ __forceinline__ int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// feature row index as gathered: clamped into the table so that no stale or
// corrupt index can ever address outside the weights (indices built by this
// library are always < FT_INPUTS; the clamp is a single v_min per row)
__device__ __forceinline__ uint32_t ft_row(uint32_t idx) { return idx < FT_INPUTS ? idx : FT_INPUTS - 1; }

__device__ __forceinline__ void load_tables(Tables &dst, const Tables *src) {
  const uint4 *s = reinterpret_cast<const uint4 *>(src);
  uint4 *d = reinterpret_cast<uint4 *>(&dst);
  for (int i = threadIdx.x; i < (int)(sizeof(Tables) / 16); i += blockDim.x) d[i] = s[i];
  __syncthreads();
}

// Wave-uniform value as an SGPR (readfirstlane) when U: descriptors and row
// indices of a slot perspective are the same for every lane of a wave whenever a
// perspective group is a whole number of waves (PAR == 1, L1 / 16 % 64 == 0), so
// control flow on them is scalar and the row offsets fold into the load's SGPR base.
template <bool U>
__device__ __forceinline__ int uni(int x) {
  if constexpr (U) return __builtin_amdgcn_readfirstlane(x);
  else return x;
}

// FT row loads as SGPR base + 32-bit VGPR offset (the table is < 4 GiB): one VGPR
// per address instead of a 64-bit pointer, and the +L1 half folds into the
// instruction's immediate offset
__device__ __forceinline__ ushort8 ldft(const uint8_t *__restrict__ ft, uint32_t off) {
  return *reinterpret_cast<const ushort8 *>(ft + off);
}
__device__ __forceinline__ uint32_t ldpd(const uint8_t *__restrict__ ft, uint32_t off) {
  return *reinterpret_cast<const uint32_t *>(ft + off);
}
__device__ __forceinline__ int4v ldps(const uint8_t *__restrict__ ft, uint32_t off) {
  return *reinterpret_cast<const int4v *>(ft + off);
}

// --------------------------------------------------- feature extraction --
// One wave turns a packed board into its HalfKAv2_hm rows, lane = square:
// the lane's rank among occupied squares is a popcount, king squares and
// validity come from ballots.  Writes rows_w[k] / rows_b[k] (k = square
// order) for the non-null outputs; returns the piece count, or 0 (nothing
// written) for an invalid board.  Must be called by all 64 lanes of a wave.
__device__ __forceinline__ int wave_features(const gn_board &p, uint16_t *rows_w, uint16_t *rows_b, int lane) {
  const uint64_t occ = p.occ;
  const int c = popcnt(occ);
  const bool has = (occ >> lane) & 1;
  const int k = popcnt(occ & ((1ull << lane) - 1));
  uint64_t wlo, whi;
  piece_words(p, wlo, whi);
  const int pc = has && k < 32 ? piece_nibble(wlo, whi, k) : 0;
  const int pt = pc & 7;
  const uint64_t bad = __ballot(has && (pt < PAWN || pt > KING));
  const uint64_t wkb = __ballot(has && pc == make_piece(WHITE, KING));
  const uint64_t bkb = __ballot(has && pc == make_piece(BLACK, KING));
  if (c < 2 || c > 32 || bad || popcnt(wkb) != 1 || popcnt(bkb) != 1) return 0;
  if (has) {
    if (rows_w) rows_w[k] = (uint16_t)feature_index(WHITE, lane, pc, __builtin_ctzll(wkb));
    if (rows_b) rows_b[k] = (uint16_t)feature_index(BLACK, lane, pc, __builtin_ctzll(bkb));
  }
  return c;
}

// piece nibble on this lane's square (0: empty); lane = square.
__device__ __forceinline__ int lane_piece(const gn_board &p, int lane) {
  const uint64_t occ = p.occ;
  const bool has = (occ >> lane) & 1;
  const int k = popcnt(occ & ((1ull << lane) - 1));
  uint64_t wlo, whi;
  piece_words(p, wlo, whi);
  return has && k < 32 ? piece_nibble(wlo, whi, k) : 0;
}

// wave_features without the squares of excl (the tile's common rows, eval_net):
// rows in square order among occ & ~excl; returns the full piece count (bucket) or 0.
__device__ __forceinline__ int wave_features_excl(const gn_board &p, uint16_t *rows_w, uint16_t *rows_b, int lane,
                                                  uint64_t excl) {
  const uint64_t occ = p.occ;
  const int c = popcnt(occ);
  const bool has = (occ >> lane) & 1;
  const int pc = lane_piece(p, lane);
  const int pt = pc & 7;
  const uint64_t bad = __ballot(has && (pt < PAWN || pt > KING));
  const uint64_t wkb = __ballot(has && pc == make_piece(WHITE, KING));
  const uint64_t bkb = __ballot(has && pc == make_piece(BLACK, KING));
  if (c < 2 || c > 32 || bad || popcnt(wkb) != 1 || popcnt(bkb) != 1) return 0;
  if (has && !((excl >> lane) & 1)) {
    const int k = popcnt(occ & ~excl & ((1ull << lane) - 1));
    rows_w[k] = (uint16_t)feature_index(WHITE, lane, pc, __builtin_ctzll(wkb));
    rows_b[k] = (uint16_t)feature_index(BLACK, lane, pc, __builtin_ctzll(bkb));
  }
  return c;
}

// Rows of perspective h of a child in which h's own king moved, straight from
// the parent board (lane = square): the king goes kfrom -> kto (capturing
// whatever stood there) and, for castling, the rook rfrom -> rto (64 = none).
// The parent must be valid (its rows were extracted).  All 64 lanes.
__device__ __forceinline__ void wave_features_king_move(const gn_board &p, int h, int kfrom, int kto, int rfrom,
                                                        int rto, uint16_t *rows, int lane) {
  const uint64_t occ = p.occ;
  const bool has = (occ >> lane) & 1;
  const int k = popcnt(occ & ((1ull << lane) - 1));
  uint64_t wlo, whi;
  piece_words(p, wlo, whi);
  int pc = has && k < 32 ? piece_nibble(wlo, whi, k) : 0;
  if (lane == kfrom || lane == rfrom) pc = 0;
  if (lane == rto) pc = make_piece(h, ROOK);
  if (lane == kto) pc = make_piece(h, KING);
  const uint64_t cocc = __ballot(pc != 0);
  if (pc) rows[popcnt(cocc & ((1ull << lane) - 1))] = (uint16_t)feature_index(h, lane, pc, kto);
}

// FeatureTransformer::transform for 8 columns pairs of one perspective, packed
// 16-bit math: clamp both halves to [0, 254] (the doubled domain), multiply
// (<= 64516, fits u16), >> 9, then v_perm the low bytes into 8 u8 outputs.
typedef short short2v __attribute__((ext_vector_type(2)));
typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 transform8(ushort8 lo, ushort8 hi) {
  uint32_t o[4];
  const short2v z = {0, 0}, m = {254, 254};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    short2v a = {(short)lo[2 * i], (short)lo[2 * i + 1]}, b = {(short)hi[2 * i], (short)hi[2 * i + 1]};
    a = __builtin_elementwise_min(__builtin_elementwise_max(a, z), m);
    b = __builtin_elementwise_min(__builtin_elementwise_max(b, z), m);
    ushort2v pr = __builtin_bit_cast(ushort2v, a) * __builtin_bit_cast(ushort2v, b);
    pr = pr >> (ushort2v){9, 9};
    o[i] = __builtin_bit_cast(uint32_t, pr);
  }
  return make_uint2(__builtin_amdgcn_perm(o[1], o[0], 0x06040200u), __builtin_amdgcn_perm(o[3], o[2], 0x06040200u));
}

// Layer stack of one bucket by ONE wave (eval_net's small net): fc_0 accumulates all L1/64
// k-steps in registers (no partial sums through LDS, no workgroup barrier), so a tile's
// buckets run on separate waves at once and the workgroup's other waves are done.  The fc_0
// result is in the lane layout of the MFMA accumulator, which is exactly what the
// epilogue of layer_stack_tile reads back from LDS, so the math below is the same.
// in1: this wave's 16 x 32 B, fwd: its 16 ints (LDS, private to the wave).
template <int L1, class Valid, class Emit>
__device__ __forceinline__ void layer_stack_wave(const NetDevice &net, const uint8_t *xt, uint8_t (*in1)[32],
                                                 int32_t *fwd, const int32_t (*psq)[2], int b, int lane,
                                                 Valid &&valid, Emit &&emit) {
  constexpr int XS = L1 + 16, KS = L1 / 64, BATCH = KS % 6 == 0 ? 6 : KS % 4 == 0 ? 4 : KS;
  static_assert(KS % BATCH == 0, "k-steps per batch");
  const int row = lane & 15, kg = lane >> 4;
  // fc_1 / fc_2 parameters first: their latency hides behind fc_0.  Loaded by every lane, with
  // no branch around them (a branch made the compiler wait for them before fc_0's loads): the
  // lanes kg >= 2 hold a copy whose products meet fc_1's zero A operand (a1 below)
  const int4v zero = {0, 0, 0, 0};
  const int4v wl = *reinterpret_cast<const int4v *>(net.w1 + ((size_t)b * 32 + row) * 32 + (kg & 1) * 16);
  const int4v wh = *reinterpret_cast<const int4v *>(net.w1 + ((size_t)b * 32 + 16 + row) * 32 + (kg & 1) * 16);
  const int32_t bias0 = net.b0[b * 16 + row];
  const int32_t b1l = net.b1[b * 32 + row], b1h = net.b1[b * 32 + 16 + row];
  const int32_t w2l = net.w2[b * 32 + row], w2h = net.w2[b * 32 + 16 + row];
  const int32_t b2v = net.b2[b];
  constexpr bool FRAG = L1 > 128; // as layer_stack_tile: w0f for the big nets, row-major w0 for 128
  const int8_t *wb = FRAG ? net.w0f + ((size_t)b * KS * 64 + lane) * 16 : net.w0 + ((size_t)b * 16 + row) * L1 + kg * 16;
  const uint8_t *xa = xt + row * XS + kg * 16;
  int4v acc = zero;
#pragma unroll 1
  for (int k0 = 0; k0 < KS; k0 += BATCH) {
    int4v w[BATCH], a[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) w[j] = *reinterpret_cast<const int4v *>(wb + (FRAG ? 1024 : 64) * (k0 + j));
#pragma unroll
    for (int j = 0; j < BATCH; ++j) a[j] = *reinterpret_cast<const int4v *>(xa + 64 * (k0 + j));
#pragma unroll
    for (int j = 0; j < BATCH; ++j) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[j], w[j], acc, 0, 0, 0);
  }
  // SqrClippedReLU / ClippedReLU of fc_0 outputs 0..14, skip term from output 15
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pos = 4 * kg + i;
    const int32_t v = wadd(acc[i], bias0);
    if (row < 15) {
      const long long s2 = ((long long)v * v) >> 19;
      in1[pos][row] = (uint8_t)(s2 < 127 ? s2 : 127);
      in1[pos][15 + row] = (uint8_t)clampi(v >> 6, 0, 127);
    } else {
      fwd[pos] = wmul(v, 600 * 16) / (127 * 64);
      in1[pos][30] = 0;
      in1[pos][31] = 0;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int4v a1 = kg < 2 ? *reinterpret_cast<const int4v *>(&in1[row][kg * 16]) : zero;
  const int4v cl = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, wl, zero, 0, 0, 0);
  const int4v ch = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, wh, zero, 0, 0, 0);
  int32_t part[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int32_t l = clampi(wadd(cl[i], b1l) >> 6, 0, 127), hh = clampi(wadd(ch[i], b1h) >> 6, 0, 127);
    part[i] = w2l * l + w2h * hh;
  }
#pragma unroll
  for (int off = 8; off; off >>= 1)
#pragma unroll
    for (int i = 0; i < 4; ++i) part[i] = wadd(part[i], __shfl_xor(part[i], off, 16));
  if (row == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pos = 4 * kg + i;
      if (valid(pos, b)) {
        const int32_t positional = wadd(wadd(b2v, part[i]), fwd[pos]);
        const int32_t psqt = (int32_t)((uint32_t)psq[pos][0] - (uint32_t)psq[pos][1]) / 2;
        emit(pos, make_int2(psqt / 16, positional / 16));
      }
    }
  }
}

// rows of perspective h of a child whose h-king moved kf -> kt (castling: rook rf -> rt,
// 64 = none), from the parent board, lane = square: the row of this lane's piece in
// the child (or -1) and its rank among the child's pieces.  All 64 lanes.
__device__ __forceinline__ int king_move_row(const gn_board &pb, int h, int kf, int kt, int rf, int rt, int lane,
                                             int &pos, int *piece = nullptr) {
  const uint64_t occ = pb.occ;
  const bool has = (occ >> lane) & 1;
  const int k = popcnt(occ & ((1ull << lane) - 1));
  uint64_t wlo, whi;
  piece_words(pb, wlo, whi);
  int pc = has && k < 32 ? piece_nibble(wlo, whi, k) : 0;
  if (lane == kf || lane == rf) pc = 0;
  if (lane == rt) pc = make_piece(h, ROOK);
  if (lane == kt) pc = make_piece(h, KING);
  const uint64_t cocc = __ballot(pc != 0);
  pos = popcnt(cocc & ((1ull << lane) - 1));
  if (piece) *piece = pc;
  return pc ? feature_index(h, lane, pc, kt) : -1;
}

// king_move_row from the parent's piece on this lane's square (lane_piece, computed once per
// parent by the caller) instead of the packed board.
__device__ __forceinline__ int king_move_row_pc(int pc, int h, int kf, int kt, int rf, int rt, int lane, int &pos,
                                                int &piece) {
  if (lane == kf || lane == rf) pc = 0;
  if (lane == rt) pc = make_piece(h, ROOK);
  if (lane == kt) pc = make_piece(h, KING);
  const uint64_t cocc = __ballot(pc != 0);
  pos = popcnt(cocc & ((1ull << lane) - 1));
  piece = pc;
  return pc ? feature_index(h, lane, pc, kt) : -1;
}

__device__ __forceinline__ int32_t wave_sum(int32_t v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v = wadd(v, __shfl_xor(v, off));
  return v;
}

// Inclusive scans over the 64 lanes on DPP: six VALU steps with no LDS round trip (a
// __shfl_up / __shfl_xor step is a ds_bpermute, ~100 cycles of latency each in a chain).
// row_shr:1/2/4/8 scan each row of 16 (lanes shifted in from outside the row read 0), then
// row_bcast:15 adds row 0's total to row 1 and row 2's to row 3, and row_bcast:31 adds
// lane 31's (rows 0-1) to rows 2 and 3.
template <class Op>
__device__ __forceinline__ uint32_t dpp_scan(uint32_t x, Op op) {
  x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true)); // row_shr:1
  x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true)); // row_shr:2
  x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true)); // row_shr:4
  x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true)); // row_shr:8
  x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false)); // row_bcast:15
  x = op(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false)); // row_bcast:31
  return x;
}
__device__ __forceinline__ uint32_t scan_add(uint32_t x) {
  return dpp_scan(x, [](uint32_t a, uint32_t b) { return a + b; });
}
__device__ __forceinline__ uint32_t scan_or(uint32_t x) {
  return dpp_scan(x, [](uint32_t a, uint32_t b) { return a | b; });
}
// OR over each group of 8 lanes (quad_perm [1,0,3,2], [2,3,0,1], then row_half_mirror)
__device__ __forceinline__ uint32_t or8(uint32_t x) {
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xb1, 0xf, 0xf, false);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4e, 0xf, 0xf, false);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xf, 0xf, false);
  return x;
}
// the wave's (wrapping) sum, uniform
__device__ __forceinline__ int32_t wave_sum_dpp(int32_t v) {
  return __builtin_amdgcn_readlane((int)scan_add((uint32_t)v), 63);
}

// ---- the column-sliced stream's finishing step for one position (finalize_kernel, which
// takes the big net's outputs from the partial sums itself): the NPART
// slices' fc_0 sums (part[t * npos + q], one record of GN_PART_DWORDS dwords) + bias, the activations, fc_1, fc_2 -- the
// whole-row kernel's finishing step in scalar integer arithmetic (exact: every sum is an
// integer sum, the wrapping adds as there).  info = pinfo[q] (PSQT value, bucket >= 0).
// w1s: the 8 buckets' fc_1 weights (32 outputs x 32 int8, 8 dwords per output) staged in LDS
// by stage_fc1 (8 KiB).
__device__ __forceinline__ void stage_fc1(int4v *w1s, const NetDevice &net) {
  for (int i = threadIdx.x; i < 8 * 32 * 2; i += blockDim.x) w1s[i] = reinterpret_cast<const int4v *>(net.w1)[i];
}
// Four unsigned 24-bit values in three dwords (the packed partial sums' record, kernels.h), and back
typedef uint32_t uint3v __attribute__((ext_vector_type(3)));
__device__ __forceinline__ uint3v pack24x4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return uint3v{a | b << 24, b >> 8 | c << 16, c >> 16 | d << 8};
}
__device__ __forceinline__ int4v unpack24x4(uint32_t x, uint32_t y, uint32_t z) {
  return int4v{(int)(x & 0xFFFFFFu), (int)(x >> 24 | (y & 0xFFFFu) << 8), (int)(y >> 16 | (z & 0xFFu) << 16),
               (int)(z >> 8)};
}
// a position's fc_0 sums over the NPART slices (sums[k]: outputs 4k .. 4k + 3, bias not added),
// read by its own lane.  Packed records (DW = GN_PART_DWORDS = 12): three 16-B loads per slice, the
// values biased by the slice's part_off, which slice_finish_from's b0p takes off again; int32
// records (DW 16, the in-place array): wrapping int32 adds, as the LDS atomics
template <int NPART, int DW>
__device__ __forceinline__ void slice_sums(const int32_t *__restrict__ part, uint64_t npos, uint64_t q, int4v (&sums)[4]) {
  static_assert(DW == 12 || DW == 16, "record width");
  if constexpr (DW == 12) {
  int4v rec[NPART][3];
#pragma unroll
  for (int t = 0; t < NPART; ++t)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      rec[t][r] = *reinterpret_cast<const int4v *>(part + ((uint64_t)t * npos + q) * 12 + 4 * r);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sums[r] = int4v{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < NPART; ++t) {
      auto dw = [&](int i) { return (uint32_t)rec[t][i >> 2][i & 3]; }; // (constant indices once unrolled)
      const int4v c = unpack24x4(dw(3 * r), dw(3 * r + 1), dw(3 * r + 2));
#pragma unroll
      for (int k = 0; k < 4; ++k) sums[r][k] = wadd(sums[r][k], c[k]);
    }
  }
  } else {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sums[r] = *reinterpret_cast<const int4v *>(part + q * 16 + 4 * r);
#pragma unroll
    for (int t = 1; t < NPART; ++t) { // (one array: the last slice's sums are the totals)
      const int4v c = *reinterpret_cast<const int4v *>(part + ((uint64_t)t * npos + q) * 16 + 4 * r);
#pragma unroll
      for (int k = 0; k < 4; ++k) sums[r][k] = wadd(sums[r][k], c[k]);
    }
  }
  }
}
// ... and the finishing step from them (bias0: net.b0p for packed records, whose values carry the
// slices' offsets; net.b0 for int32 records)
__device__ __forceinline__ int2 slice_finish_from(const NetDevice &net, const int32_t *__restrict__ bias0,
                                                  const int4v *w1s, const int4v (&sums)[4], int2 info) {
  const int b = info.y & 7;
  int32_t v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = wadd(sums[r >> 2][r & 3], bias0[b * 16 + r]);
  // fc_1's 32 inputs as int8 packed 4 per dword: 15 squared, 15 clipped, 2 zero
  uint32_t x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 15; ++r) {
    // min(v^2 >> 19, 127) in 32 bits: |v| >= 8160 gives 127 (8160^2 >> 19 = 127, 8159^2 >> 19 =
    // 126), so |v| clamped to 8160 squares below 2^26 -- one 24-bit multiply, no 64-bit product
    const uint32_t u = v[r] < 0 ? 0u - (uint32_t)v[r] : (uint32_t)v[r], m = u < 8160u ? u : 8160u;
    const uint32_t a = (m * m) >> 19, c = (uint32_t)clampi(v[r] >> 6, 0, 127);
    x[r >> 2] |= a << (8 * (r & 3));
    x[(15 + r) >> 2] |= c << (8 * ((15 + r) & 3));
  }
  const int32_t fwd = wmul(v[15], 600 * 16) / (127 * 64);
  int32_t sum = 0;
#pragma unroll 4
  for (int o = 0; o < 32; ++o) {
    const int4v wa = w1s[(b * 32 + o) * 2], wb = w1s[(b * 32 + o) * 2 + 1];
    int32_t acc = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) acc = __builtin_amdgcn_sdot4((int)x[d], wa[d], acc, false);
#pragma unroll
    for (int d = 0; d < 4; ++d) acc = __builtin_amdgcn_sdot4((int)x[4 + d], wb[d], acc, false);
    const int32_t l = clampi(wadd(acc, net.b1[b * 32 + o]) >> 6, 0, 127);
    sum = wadd(sum, (int32_t)net.w2[b * 32 + o] * l);
  }
  const int32_t positional = wadd(wadd(net.b2[b], sum), fwd);
  return make_int2(info.x / 16, positional / 16);
}

} // namespace gn
