// plan_snapshot.h — a copy of the last planned expansion's plan for the tests (internal).
//
// plan_kernel's output (stream.hip: the two entry lists of every block and a TileDesc per tile) is
// plain data in device memory.  gn_debug_plan_snapshot copies it, with the build and launch
// constants a reader needs, to host memory, so that tests/plan_replay.py can execute the lists on
// the CPU and check the ordering rules the row stream relies on (DESIGN.md §4.7 "What checks the
// plan").  Host code only: a copy of library-owned buffers, no kernel.
//
// Not part of the public ABI: the symbol is exported from the library but is absent from
// include/gpu_nnue.h, GN_ABI_VERSION does not count it, and its layout may change with the plan's.
//
// Which expansion: the device slot's current buffer set (ExpSet, gpu_nnue.hip Dev::cur), i.e. the
// last expansion whose front half ran in it.  After a blocking gn_expand_device that is the call's
// expansion, complete.  After a pipelined call (GN_OPT_EXPAND_PIPELINE 1 or 2: gn_time_expand_device,
// the host-buffer game calls) the sets have been swapped once per expansion; Dev::cur is then the
// set of the last expansion whose back half ran, which is the call's last expansion, but `rows`
// below is 0 (the pipeline counts rows for its caller, not here).  The tests call it with
// GN_OPT_EXPAND_PIPELINE 0 after gn_expand_device only.
//
// Use: call once with bufs == NULL to get the header (the sizes), allocate, call again with the
// buffers.  GN_E_INVALID with a message when the slot's last expansion was not planned (the small
// net alone, GN_OPT_INCREMENTAL_CHILDREN 0, a 128-wide big net, no expansion yet, or no parents) or
// a buffer is too small.  The call waits for the device's stream.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct gn_ctx;

// Build constants (nnue.h, kernels.h), the launch's arguments (plan_kernel) and its counters.
typedef struct gn_plan_snapshot_header {
  uint32_t header_bytes; // sizeof(gn_plan_snapshot_header)
  uint32_t tile_bytes;   // sizeof(TileDesc): e_end[2] u32, p_first u32, first u32, meta[16] u8,
                         // psq[16][2] i32, adj[16] i16 (kernels.h)
  uint32_t l1;           // the big net's accumulator width
  uint32_t row_stride;   // ft_row_stride(l1): bytes from one row to the next
  uint32_t ft_rows;      // FT_ROWS: the feature rows and the bias row
  uint32_t ft_bias_row;  // FT_BIAS_ROW
  uint32_t zero_row;     // ZERO_ROW
  uint32_t scr_rows;     // SCR_ROWS: rows of a workgroup's scratch slot (king-cache row 2 + 64 h + ksq)
  uint32_t ent_spare;    // ENT_SPARE
  uint32_t scr_gap;      // GN_SCR_GAP
  uint32_t ring;         // GN_RING
  uint32_t slice_ring;   // GN_SLICE_RING
  uint32_t np;           // parents
  uint32_t k;            // block length (consecutive parents per block)
  uint32_t nblk;         // blocks
  uint32_t slices;       // 3: the column-sliced stream (pinfo is written), 1: whole rows
  uint32_t xu, hu;       // units of the LAST entry's tile field hi[31:22] = slot * xu + side * hu
  uint32_t kc;           // the king cache was on
  uint32_t ordered;      // the stream took the blocks in `order` (else: 0, 1, ...; order[] is that)
  uint64_t npos;         // np + the children: positions by output index (parent p: p, child c: np + c)
  uint64_t n_ent;        // entries: eoff[np] + ent_spare * nblk
  uint64_t n_tiles;      // tile descriptors up to the last block's last
  uint64_t n_pinfo;      // npos when slices == 3, else 0
  uint64_t pads;         // GN_STAT_SCRATCH_PADS: no-op entries (multiplier 0)
  uint64_t zero_row_entries; // GN_STAT_ZERO_ROW_ENTRIES
  uint64_t rows;         // the plan's FT-row count (gn_expand_device counts it; else 0)
} gn_plan_snapshot_header;

// Host buffers and their capacities in elements (a capacity below the header's count fails).
typedef struct gn_plan_snapshot_bufs {
  uint64_t *eoff;     // [np + 1] entry offsets of the parents (exclusive scan of the entry bounds)
  size_t eoff_cap;
  uint64_t *ent;      // [n_ent] entries (lo | hi << 32); block b's region is
  size_t ent_cap;     //   [eoff[b k] + ent_spare b, eoff[min(b k + k, np)] + ent_spare (b + 1))
  void *tiles;        // [n_tiles] TileDesc; block b's start at (b k + offsets[b k]) / 16 + (k + 2) b
  size_t tiles_cap;
  uint32_t *btiles;   // [nblk] tiles of each block
  size_t btiles_cap;
  uint32_t *order;    // [nblk] the stream's block order
  size_t order_cap;
  int32_t *pinfo;     // [n_pinfo][2] (PSQT term, bucket / PINFO_ALIAS) by output index
  size_t pinfo_cap;
  uint64_t *offsets;  // [np + 1] child offsets of the parents
  size_t offsets_cap;
} gn_plan_snapshot_bufs;

__attribute__((visibility("default"))) int gn_debug_plan_snapshot(struct gn_ctx *ctx, int device_slot,
                                                                  gn_plan_snapshot_header *header,
                                                                  const gn_plan_snapshot_bufs *bufs);

// The loaded big net's tables for the column slices' packed partial sums (nnue.h NetDevice, kernels.h
// GN_PART_DWORDS), copied from the device: part_off [8 buckets][3 slices][16 outputs] and b0p [8][16]
// int32.  GN_E_INVALID when the context has no 3072-wide big net.  Internal, as above.
__attribute__((visibility("default"))) int gn_debug_part_offsets(struct gn_ctx *ctx, int device_slot,
                                                                 int32_t *part_off, int32_t *b0p);

#ifdef __cplusplus
}
#endif
