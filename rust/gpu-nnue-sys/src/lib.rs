//! gpu-nnue-sys — raw FFI of libgpu_nnue.so, 1:1 with `include/gpu_nnue.h` (ABI v4).
//!
//! fishnet's `src/main.rs:1` forbids unsafe code in the binary crate, so the FFI lives in
//! this separate crate; the safe wrapper is `fishnet-gpu/src/gpu_nnue.rs`.  Every item here
//! mirrors a declaration of the header; `tests/test_host.py::test_rust_sys_crate_matches_header`
//! checks names, argument counts, struct fields and constants against it (cargo is not
//! in the build image, so that test is what keeps this file honest).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

pub const GN_ABI_VERSION: c_int = 4;

// return codes
pub const GN_OK: c_int = 0;
pub const GN_E_INVALID: c_int = -1;
pub const GN_E_IO: c_int = -2;
pub const GN_E_FORMAT: c_int = -3;
pub const GN_E_HIP: c_int = -4;
pub const GN_E_NOMEM: c_int = -5;
pub const GN_E_CAPACITY: c_int = -6;
pub const GN_E_NODEVICE: c_int = -7;
pub const GN_E_NONET: c_int = -8;
pub const GN_E_ILLEGAL_MOVE: c_int = -9;

// evaluation modes
pub const GN_MODE_FULL: c_int = 0;
pub const GN_MODE_BIG: c_int = 1;
pub const GN_MODE_SMALL: c_int = 2;

// options (gn_set_option / gn_get_option); results never depend on them, GN_OPT_QUIESCE_SEE excepted
pub const GN_OPT_INCREMENTAL_CHILDREN: c_int = 1;
pub const GN_OPT_XCD_SWIZZLE: c_int = 2;
pub const GN_OPT_KING_SORT: c_int = 3;
pub const GN_OPT_CHAIN: c_int = 4;
pub const GN_OPT_KING_CACHE: c_int = 5;
pub const GN_OPT_CHUNK_PARENTS: c_int = 6;
pub const GN_OPT_COALESCE: c_int = 7;
pub const GN_OPT_STREAM_SLICES: c_int = 8;
pub const GN_OPT_FAST_BATCH: c_int = 9;
pub const GN_OPT_EXPAND_PIPELINE: c_int = 10;
pub const GN_OPT_QUIESCE_SEE: c_int = 11;
// read-only statistics (gn_get_option)
pub const GN_STAT_PLAN_NS: c_int = 101;
pub const GN_STAT_STREAM_NS: c_int = 102;
pub const GN_STAT_SCRATCH_PADS: c_int = 103;
pub const GN_STAT_FINISH_NS: c_int = 104;
pub const GN_STAT_ZERO_ROW_ENTRIES: c_int = 105;
pub const GN_STAT_HOST_PARSE_NS: c_int = 110;
pub const GN_STAT_HOST_UPLOAD_NS: c_int = 111;
pub const GN_STAT_HOST_REPLAY_NS: c_int = 112;
pub const GN_STAT_HOST_COMPUTE_NS: c_int = 113;
pub const GN_STAT_HOST_DOWNLOAD_NS: c_int = 114;
pub const GN_STAT_HOST_TAIL_NS: c_int = 115;
pub const GN_STAT_HOST_TOTAL_NS: c_int = 116;
pub const GN_STAT_BATCH_LAUNCHES: c_int = 117;
pub const GN_STAT_BATCH_CALLS: c_int = 118;
pub const GN_STAT_FAST_BATCHES: c_int = 119;
pub const GN_STAT_FAST_FALLBACKS: c_int = 120;
pub const GN_STAT_RANK_NS: c_int = 121;
pub const GN_STAT_RANK2_NS: c_int = 122;
pub const GN_STAT_KEYS_NS: c_int = 123;
pub const GN_STAT_EXTEND_NS: c_int = 124;
pub const GN_STAT_EXTENDED_LEAVES: c_int = 125;
/// A d_ext entry of a leaf the check extension does not value (gn_extend_checks_device).
pub const GN_NOT_EXTENDED: i32 = i32::MIN;
pub const GN_STAT_QUIESCE_NS: c_int = 126;
pub const GN_STAT_QUIESCE_LEAVES: c_int = 127;
pub const GN_STAT_QUIESCE_NODES: c_int = 128;
pub const GN_STAT_PV_NS: c_int = 129;
pub const GN_STAT_RANK3_NS: c_int = 130;

// per-position flags
pub const GN_FLAG_IN_CHECK: u16 = 1;
pub const GN_FLAG_SMALLNET: u16 = 2;
pub const GN_FLAG_BAD_FEN: u16 = 4;
pub const GN_FLAG_REEVAL: u16 = 8;
pub const GN_FLAG_SKIPPED: u16 = 16;
pub const GN_FLAG_MATE: u16 = 32;
pub const GN_FLAG_NO_SCORE: u16 = 64;
pub const GN_FLAG_SEARCHED: u16 = 128;
pub const GN_FLAG_NO_MOVES: u16 = 256;
pub const GN_FLAG_DRAW: u16 = 512;

/// One result: NetworkOutput (psqt, positional) of the net that produced final_v,
/// Eval::evaluate (internal units), UCIEngine::to_cp, and the score fishnet posts for the
/// position (`score cp` / `score mate` with GN_FLAG_MATE; the in-check rule's reply in
/// best_move with GN_FLAG_SEARCHED; see the header at gn_eval).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct gn_eval {
    pub psqt: i32,
    pub positional: i32,
    pub final_v: i32,
    pub final_cp: i32,
    pub score: i32,
    pub flags: u16,
    pub best_move: u16,
}

/// One legal child from the host-buffer expansion calls (ABI v4, 12 bytes): psqt, positional and
/// cp_flags = final_cp (signed 24 bits) | the low 8 flag bits << 24 (see the header at gn_child).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct gn_child {
    pub psqt: i32,
    pub positional: i32,
    pub cp_flags: i32,
}

impl gn_child {
    /// GN_CHILD_FINAL_CP
    pub fn final_cp(&self) -> i32 {
        ((self.cp_flags as u32) << 8) as i32 >> 8
    }
    /// GN_CHILD_FLAGS
    pub fn flags(&self) -> u16 {
        ((self.cp_flags as u32) >> 24) as u16
    }
}

/// The header's GN_MAX_LINES: the most lines per position the ranking calls return.
pub const MAX_LINES: usize = 8;
/// The header's GN_MAX_QUIESCE_DEPTH: the quiescent calls' depth is 1..=MAX_QUIESCE_DEPTH.
pub const MAX_QUIESCE_DEPTH: c_int = 4;
/// The header's GN_MAX_PV: a line's two moves and the quiescence's own.
pub const MAX_PV: usize = 6;

/// The whole variation of one ranked line (16 bytes): the line's move (and reply), followed by the
/// quiescence's own moves below its leaf when the line carries GN_FLAG_SEARCHED; unused entries
/// and reserved are 0; an empty line has len 0.  See the header at gn_pv.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct gn_pv {
    pub len: u16,
    pub moves: [u16; MAX_PV],
    pub reserved: u16,
}

/// One ranked line of a position (MultiPV, 12 bytes): the rule value of a legal move, its score
/// (`cp`, or the mate distance with GN_FLAG_MATE), the move and its flags (GN_FLAG_IN_CHECK: the
/// move gives check; GN_FLAG_NO_MOVES: it ends the game; GN_FLAG_NO_SCORE: an empty line); see
/// the header at gn_line.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct gn_line {
    pub value: i32,
    pub score: i32,
    pub r#move: u16,
    pub flags: u16,
}

/// A parent's game so far in a key array (gn_position_keys): keys[first..=self] are the keys of
/// the game's positions up to and including the parent; first > self means "no history".  See
/// the header at gn_history for the draw rule the history calls apply (GN_FLAG_DRAW lines).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct gn_history {
    pub first: u32,
    pub r#self: u32,
}

/// One ranked two-ply line of a position (16 bytes): a two-move principal variation (`move`, then
/// the opponent's best `reply`; reply 0 and plies 1 when the move ends the game) with its minimax
/// value and score; flags as gn_line's; an empty line is (0, 0, 0, 0, GN_FLAG_NO_SCORE, 0); see the
/// header at gn_line2.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct gn_line2 {
    pub value: i32,
    pub score: i32,
    pub r#move: u16,
    pub reply: u16,
    pub flags: u16,
    pub plies: u16,
}

/// The three-ply calls' leaf rule (the header's GN_LEAF_*): static leaves, the check extension, or the
/// capture quiescence to `depth` plies, 1..=MAX_QUIESCE_DEPTH3 (GN_MAX_QUIESCE_DEPTH3).
pub const LEAF_STATIC: c_int = 0;
pub const LEAF_CHECKS: c_int = 1;
pub const LEAF_QUIESCE: c_int = 2;
pub const MAX_QUIESCE_DEPTH3: c_int = 3;

/// One ranked three-ply line of a position (20 bytes): `move`, the opponent's best `reply` and the
/// side's best answer `reply2` with the minimax value after three plies and its score; plies is 3, or
/// 2 / 1 when the game ends earlier (reply2 / reply 0, GN_FLAG_NO_MOVES); an empty line is
/// (0, 0, 0, 0, 0, GN_FLAG_NO_SCORE, 0, 0); see the header at gn_line3.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct gn_line3 {
    pub value: i32,
    pub score: i32,
    pub r#move: u16,
    pub reply: u16,
    pub reply2: u16,
    pub flags: u16,
    pub plies: u16,
    pub reserved: u16,
}

/// Packed position (32 bytes), the device input format.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct gn_board {
    pub occ: u64,
    pub pc: [u8; 16],
    pub stm_ep: u8,
    pub reserved: u8,
    pub castle: u16,
    pub rule50: u16,
    pub fullmove: u16,
}

/// Eval::evaluate constants and the to_cp win-rate model (defaults: Stockfish 17.1).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq)]
pub struct gn_eval_params {
    pub small_net_threshold: i32,
    pub psqt_weight: i32,
    pub positional_weight: i32,
    pub reeval_threshold: i32,
    pub complexity_div_small: i32,
    pub complexity_div_big: i32,
    pub material_pawn_small: i32,
    pub material_pawn_big: i32,
    pub material_base: i32,
    pub rule50_div: i32,
    pub value_clamp: i32,
    pub piece_value: [i32; 5],
    pub wdl_a: [f64; 4],
    pub wdl_material_min: i32,
    pub wdl_material_max: i32,
    pub wdl_material_anchor: i32,
    pub wdl_piece_weight: [i32; 5],
}

/// One acquired lichess batch (AcquireResponseBody, src/api.rs:306-321).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct gn_game {
    pub root_fen: *const c_char,
    pub uci_moves: *const c_char,
    pub skip_positions: *const u32,
    pub n_skip: usize,
}

#[repr(C)]
pub struct gn_ctx {
    _private: [u8; 0],
}

#[link(name = "gpu_nnue")]
extern "C" {
    pub fn gn_load_net(big_path: *const c_char, small_path: *const c_char, devices: *const c_int, n_devices: c_int,
                       out: *mut *mut gn_ctx) -> c_int;
    pub fn gn_load_net_memory(big: *const u8, big_len: usize, small: *const u8, small_len: usize,
                              devices: *const c_int, n_devices: c_int, out: *mut *mut gn_ctx) -> c_int;
    pub fn gn_load_net_archive(archive_path: *const c_char, big_member: *const c_char, small_member: *const c_char,
                               devices: *const c_int, n_devices: c_int, out: *mut *mut gn_ctx) -> c_int;
    pub fn gn_archive_read(archive_path: *const c_char, member: *const c_char, buf: *mut u8, cap: usize,
                           size: *mut usize) -> c_int;
    pub fn gn_free(ctx: *mut gn_ctx);
    pub fn gn_last_error() -> *const c_char;
    pub fn gn_abi_version() -> c_int;
    pub fn gn_get_eval_params(ctx: *const gn_ctx, out: *mut gn_eval_params) -> c_int;
    pub fn gn_set_eval_params(ctx: *mut gn_ctx, params: *const gn_eval_params) -> c_int;
    pub fn gn_set_option(ctx: *mut gn_ctx, option: c_int, value: i64) -> c_int;
    pub fn gn_get_option(ctx: *const gn_ctx, option: c_int, value: *mut i64) -> c_int;
    pub fn gn_net_sha256(data: *const u8, len: usize, hex65: *mut c_char) -> c_int;
    pub fn gn_net_info(ctx: *const gn_ctx, big_l1: *mut c_int, big_hash: *mut u32, small_l1: *mut c_int,
                       small_hash: *mut u32) -> c_int;
    pub fn gn_evaluate_batch(ctx: *mut gn_ctx, fens: *const *const c_char, n: usize, out: *mut gn_eval) -> c_int;
    pub fn gn_evaluate_batch_mode(ctx: *mut gn_ctx, fens: *const *const c_char, n: usize, mode: c_int,
                                  out: *mut gn_eval) -> c_int;
    pub fn gn_expand_and_evaluate(ctx: *mut gn_ctx, parent_fens: *const *const c_char, n: usize, mode: c_int,
                                  parent_out: *mut gn_eval, child_offsets: *mut u32, child_moves: *mut u16,
                                  child_out: *mut gn_child, cap: usize) -> c_int;
    pub fn gn_replay_game(game: *const gn_game, positions: *mut gn_board, skipped: *mut u8, moves: *mut u16,
                          cap: usize, n_positions: *mut usize) -> c_int;
    pub fn gn_evaluate_games(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                             with_children: c_int, position_offsets: *mut u32, game_status: *mut i32,
                             position_out: *mut gn_eval, position_cap: usize, child_offsets: *mut u32,
                             child_moves: *mut u16, child_out: *mut gn_child, child_cap: usize) -> c_int;
    pub fn gn_evaluate_games_lines(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                   n_lines: c_int, position_offsets: *mut u32, game_status: *mut i32,
                                   position_out: *mut gn_eval, position_cap: usize, lines: *mut gn_line) -> c_int;
    pub fn gn_evaluate_games_lines_history(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                           n_lines: c_int, position_offsets: *mut u32, game_status: *mut i32,
                                           position_out: *mut gn_eval, position_cap: usize, lines: *mut gn_line)
                                           -> c_int;
    pub fn gn_evaluate_games_lines2(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                    n_lines: c_int, position_offsets: *mut u32, game_status: *mut i32,
                                    position_out: *mut gn_eval, position_cap: usize, lines: *mut gn_line2) -> c_int;
    pub fn gn_evaluate_games_lines2_history(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                            n_lines: c_int, position_offsets: *mut u32, game_status: *mut i32,
                                            position_out: *mut gn_eval, position_cap: usize, lines: *mut gn_line2)
                                            -> c_int;
    pub fn gn_evaluate_lines2(ctx: *mut gn_ctx, fens: *const *const c_char, n: usize, mode: c_int, n_lines: c_int,
                              out: *mut gn_eval, lines: *mut gn_line2) -> c_int;
    pub fn gn_evaluate_lines2_extended(ctx: *mut gn_ctx, fens: *const *const c_char, n: usize, mode: c_int,
                                       n_lines: c_int, out: *mut gn_eval, lines: *mut gn_line2) -> c_int;
    pub fn gn_evaluate_games_lines2_extended(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                             n_lines: c_int, history: c_int, position_offsets: *mut u32,
                                             game_status: *mut i32, position_out: *mut gn_eval, position_cap: usize,
                                             lines: *mut gn_line2) -> c_int;
    pub fn gn_evaluate_games_lines_extended(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                            n_lines: c_int, history: c_int, position_offsets: *mut u32,
                                            game_status: *mut i32, position_out: *mut gn_eval, position_cap: usize,
                                            lines: *mut gn_line) -> c_int;
    pub fn gn_evaluate_lines2_quiescent(ctx: *mut gn_ctx, fens: *const *const c_char, n: usize, mode: c_int,
                                        n_lines: c_int, depth: c_int, out: *mut gn_eval, lines: *mut gn_line2)
                                        -> c_int;
    pub fn gn_evaluate_games_lines2_quiescent(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                              n_lines: c_int, history: c_int, depth: c_int,
                                              position_offsets: *mut u32, game_status: *mut i32,
                                              position_out: *mut gn_eval, position_cap: usize, lines: *mut gn_line2)
                                              -> c_int;
    pub fn gn_evaluate_games_lines_quiescent(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                             n_lines: c_int, history: c_int, depth: c_int, position_offsets: *mut u32,
                                             game_status: *mut i32, position_out: *mut gn_eval, position_cap: usize,
                                             lines: *mut gn_line) -> c_int;
    pub fn gn_evaluate_lines2_quiescent_pv(ctx: *mut gn_ctx, fens: *const *const c_char, n: usize, mode: c_int,
                                           n_lines: c_int, depth: c_int, out: *mut gn_eval, lines: *mut gn_line2,
                                           pvs: *mut gn_pv) -> c_int;
    pub fn gn_evaluate_games_lines2_quiescent_pv(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                                 n_lines: c_int, history: c_int, depth: c_int,
                                                 position_offsets: *mut u32, game_status: *mut i32,
                                                 position_out: *mut gn_eval, position_cap: usize,
                                                 lines: *mut gn_line2, pvs: *mut gn_pv) -> c_int;
    pub fn gn_evaluate_games_lines_quiescent_pv(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                                n_lines: c_int, history: c_int, depth: c_int,
                                                position_offsets: *mut u32, game_status: *mut i32,
                                                position_out: *mut gn_eval, position_cap: usize, lines: *mut gn_line,
                                                pvs: *mut gn_pv) -> c_int;
    pub fn gn_evaluate_lines3(ctx: *mut gn_ctx, fens: *const *const c_char, n: usize, mode: c_int, n_lines: c_int,
                              leaf: c_int, depth: c_int, out: *mut gn_eval, lines: *mut gn_line3, pvs: *mut gn_pv)
                              -> c_int;
    pub fn gn_evaluate_games_lines3(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                    n_lines: c_int, leaf: c_int, depth: c_int, position_offsets: *mut u32,
                                    game_status: *mut i32, position_out: *mut gn_eval, position_cap: usize,
                                    lines: *mut gn_line3, pvs: *mut gn_pv) -> c_int;
    pub fn gn_evaluate_games_lines3_history(ctx: *mut gn_ctx, games: *const gn_game, n_games: usize, mode: c_int,
                                            n_lines: c_int, leaf: c_int, depth: c_int, position_offsets: *mut u32,
                                            game_status: *mut i32, position_out: *mut gn_eval, position_cap: usize,
                                            lines: *mut gn_line3, pvs: *mut gn_pv) -> c_int;
    pub fn gn_partition(weights: *const u32, n_items: usize, n_shards: c_int, bounds: *mut usize) -> c_int;
    pub fn gn_perft(ctx: *mut gn_ctx, fen: *const c_char, depth: c_int, nodes: *mut u64) -> c_int;
    pub fn gn_pack_fens(fens: *const *const c_char, n: usize, out: *mut gn_board, ok: *mut u8) -> c_int;
    pub fn gn_board_to_fen(board: *const gn_board, buf: *mut c_char, buflen: usize) -> c_int;
    pub fn gn_boards_to_fens(boards: *const gn_board, n: usize, buf: *mut c_char, stride: usize) -> c_int;
    pub fn gn_position_keys(boards: *const gn_board, n: usize, keys: *mut u64) -> c_int;
    pub fn gn_random_positions(seed: u64, first_index: usize, n: usize, max_plies: c_int, out: *mut gn_board)
                               -> c_int;
    // device-resident entry points (pointers are device memory of device_slot; stream: a
    // hipStream_t or NULL for the library's own)
    pub fn gn_random_positions_device(ctx: *mut gn_ctx, device_slot: c_int, seed: u64, first_index: usize, n: usize,
                                      max_plies: c_int, d_out: *mut gn_board, stream: *mut c_void) -> c_int;
    pub fn gn_evaluate_device(ctx: *mut gn_ctx, device_slot: c_int, d_boards: *const gn_board, n: usize, mode: c_int,
                              d_out: *mut gn_eval, stream: *mut c_void) -> c_int;
    pub fn gn_expand_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize, mode: c_int,
                            d_parent_out: *mut gn_eval, d_offsets: *mut u32, d_children: *mut gn_board,
                            d_moves: *mut u16, d_child_out: *mut gn_eval, cap: usize, total: *mut usize,
                            stream: *mut c_void) -> c_int;
    pub fn gn_rank_children_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                   d_offsets: *const u32, d_moves: *const u16, d_child_out: *const gn_eval,
                                   n_lines: c_int, d_lines: *mut gn_line, stream: *mut c_void) -> c_int;
    pub fn gn_position_keys_device(ctx: *mut gn_ctx, device_slot: c_int, d_boards: *const gn_board, n: usize,
                                   d_keys: *mut u64, stream: *mut c_void) -> c_int;
    pub fn gn_rank_children_history_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                           d_offsets: *const u32, d_moves: *const u16, d_child_out: *const gn_eval,
                                           d_keys: *const u64, n_keys: usize, d_hist: *const gn_history,
                                           n_lines: c_int, d_lines: *mut gn_line, stream: *mut c_void) -> c_int;
    pub fn gn_rank_lines2_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                 d_offsets: *const u32, d_children: *const gn_board, d_child_out: *const gn_eval,
                                 d_moves: *const u16, d_goffsets: *const u32, d_gmoves: *const u16,
                                 d_grand_out: *const gn_eval, n_lines: c_int, d_lines: *mut gn_line2,
                                 stream: *mut c_void) -> c_int;
    pub fn gn_rank_lines2_history_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                         d_offsets: *const u32, d_children: *const gn_board,
                                         d_child_out: *const gn_eval, d_moves: *const u16, d_goffsets: *const u32,
                                         d_gmoves: *const u16, d_grand_out: *const gn_eval, d_keys: *const u64,
                                         n_keys: usize, d_hist: *const gn_history, n_lines: c_int,
                                         d_lines: *mut gn_line2, stream: *mut c_void) -> c_int;
    pub fn gn_extend_checks_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                   d_offsets: *const u32, d_moves: *const u16, d_rec: *const gn_eval, total: usize,
                                   mode: c_int, d_ext: *mut i32, extended: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gn_quiesce_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                             d_offsets: *const u32, d_moves: *const u16, d_rec: *const gn_eval, total: usize,
                             mode: c_int, depth: c_int, d_ext: *mut i32, searched: *mut usize, nodes: *mut usize,
                             stream: *mut c_void) -> c_int;
    pub fn gn_quiesce_pv_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                d_offsets: *const u32, d_moves: *const u16, d_rec: *const gn_eval, total: usize,
                                mode: c_int, depth: c_int, d_ext: *mut i32, d_tail: *mut u16, searched: *mut usize,
                                nodes: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gn_see_moves(boards: *const gn_board, n: usize, moves: *const u16, piece_value: *const i32,
                        out: *mut i32) -> c_int;
    pub fn gn_see_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                         d_offsets: *const u32, d_moves: *const u16, total: usize, d_see: *mut i32,
                         stream: *mut c_void) -> c_int;
    pub fn gn_line_pvs_device(ctx: *mut gn_ctx, device_slot: c_int, n: usize, d_offsets: *const u32,
                              d_moves: *const u16, d_tail: *const u16, d_lines: *const gn_line, n_lines: c_int,
                              d_pvs: *mut gn_pv, stream: *mut c_void) -> c_int;
    pub fn gn_line2_pvs_device(ctx: *mut gn_ctx, device_slot: c_int, n: usize, d_offsets: *const u32,
                               d_moves: *const u16, d_goffsets: *const u32, d_gmoves: *const u16,
                               d_gtail: *const u16, d_lines: *const gn_line2, n_lines: c_int, d_pvs: *mut gn_pv,
                               stream: *mut c_void) -> c_int;
    pub fn gn_rank_lines3_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                 d_offsets: *const u32, d_moves: *const u16, d_child_out: *const gn_eval, total: usize,
                                 d_child_lines: *const gn_line2, d_child_pvs: *const gn_pv, n_lines: c_int,
                                 d_lines: *mut gn_line3, d_pvs: *mut gn_pv, stream: *mut c_void) -> c_int;
    pub fn gn_rank_lines3_history_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                         d_offsets: *const u32, d_moves: *const u16, d_child_out: *const gn_eval,
                                         total: usize, d_child_lines: *const gn_line2, d_child_pvs: *const gn_pv,
                                         d_children: *const gn_board, d_keys: *const u64, n_keys: usize,
                                         d_hist: *const gn_history, n_lines: c_int, d_lines: *mut gn_line3,
                                         d_pvs: *mut gn_pv, stream: *mut c_void) -> c_int;
    pub fn gn_rank_lines2_ahead_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                       d_offsets: *const u32, d_children: *const gn_board,
                                       d_child_out: *const gn_eval, d_moves: *const u16, d_goffsets: *const u32,
                                       d_gmoves: *const u16, d_grand_out: *const gn_eval, d_keys: *const u64,
                                       n_keys: usize, d_hist: *const gn_history, d_gext: *const i32, ahead: c_int,
                                       n_lines: c_int, d_lines: *mut gn_line2, stream: *mut c_void) -> c_int;
    pub fn gn_rank_children_extended_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                            d_offsets: *const u32, d_moves: *const u16, d_child_out: *const gn_eval,
                                            d_keys: *const u64, n_keys: usize, d_hist: *const gn_history,
                                            d_ext: *const i32, n_lines: c_int, d_lines: *mut gn_line,
                                            stream: *mut c_void) -> c_int;
    pub fn gn_rank_lines2_extended_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                          d_offsets: *const u32, d_children: *const gn_board,
                                          d_child_out: *const gn_eval, d_moves: *const u16, d_goffsets: *const u32,
                                          d_gmoves: *const u16, d_grand_out: *const gn_eval, d_keys: *const u64,
                                          n_keys: usize, d_hist: *const gn_history, d_gext: *const i32, n_lines: c_int,
                                          d_lines: *mut gn_line2, stream: *mut c_void) -> c_int;
    pub fn gn_expand2_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize, mode: c_int,
                             d_parent_out: *mut gn_eval, d_offsets: *mut u32, d_children: *mut gn_board,
                             d_moves: *mut u16, d_child_out: *mut gn_eval, cap: usize, d_goffsets: *mut u32,
                             d_gmoves: *mut u16, d_grand_out: *mut gn_eval, gcap: usize, total: *mut usize,
                             gtotal: *mut usize, stream: *mut c_void) -> c_int;
    pub fn gn_time_expand_device(ctx: *mut gn_ctx, device_slot: c_int, d_parents: *const gn_board, n: usize,
                                 mode: c_int, iters: c_int, ms_total: *mut f32, total: *mut usize,
                                 stage_ms: *mut f32, ft_rows: *mut u64, d_parent_out: *mut gn_eval,
                                 d_offsets: *mut u32, d_moves: *mut u16, d_child_out: *mut gn_eval, cap: usize)
                                 -> c_int;
    pub fn gn_checksum_device(ctx: *mut gn_ctx, device_slot: c_int, d_ptr: *const c_void, bytes: usize,
                              sum: *mut u64) -> c_int;
    pub fn gn_random_games_device(ctx: *mut gn_ctx, device_slot: c_int, seed: u64, first_game: usize,
                                  n_games: usize, plies: c_int, d_out: *mut gn_board, stream: *mut c_void) -> c_int;
    pub fn gn_random_games_uci(seed: u64, first_game: usize, n_games: usize, plies: c_int, buf: *mut c_char,
                               stride: usize) -> c_int;
    pub fn gn_device_alloc(ctx: *mut gn_ctx, device_slot: c_int, bytes: usize, ptr: *mut *mut c_void) -> c_int;
    pub fn gn_device_free(ctx: *mut gn_ctx, device_slot: c_int, ptr: *mut c_void) -> c_int;
    pub fn gn_memcpy_h2d(ctx: *mut gn_ctx, device_slot: c_int, dst: *mut c_void, src: *const c_void, bytes: usize)
                         -> c_int;
    pub fn gn_memcpy_d2h(ctx: *mut gn_ctx, device_slot: c_int, dst: *mut c_void, src: *const c_void, bytes: usize)
                         -> c_int;
    pub fn gn_synchronize(ctx: *mut gn_ctx, device_slot: c_int) -> c_int;
    pub fn gn_time_evaluate_device(ctx: *mut gn_ctx, device_slot: c_int, d_boards: *const gn_board, n: usize,
                                   mode: c_int, d_out: *mut gn_eval, iters: c_int, ms_total: *mut f32,
                                   per_kernel_ms: *mut f32, ft_rows: *mut u64) -> c_int;
}

#[cfg(test)]
mod tests {
    use super::*;
    #[test]
    fn layouts() {
        assert_eq!(std::mem::size_of::<gn_eval>(), 24);
        assert_eq!(std::mem::size_of::<gn_child>(), 12);
        assert_eq!(std::mem::size_of::<gn_line>(), 12);
        assert_eq!(std::mem::size_of::<gn_line2>(), 16);
        let c = gn_child { psqt: 0, positional: 0, cp_flags: (0x00FF_FFFEu32 | 65u32 << 24) as i32 };
        assert_eq!((c.final_cp(), c.flags()), (-2, 65));
        assert_eq!(std::mem::size_of::<gn_board>(), 32);
        assert_eq!(std::mem::size_of::<gn_eval_params>(), 128);
    }
}
