//! src/gpu_nnue.rs of the fishnet crate: the safe wrapper over `gpu-nnue-sys`.
//!
//! Drop this file into fishnet's `src/` (`mod gpu_nnue;` in main.rs) and add
//! `gpu-nnue-sys = { path = "..." }` to its Cargo.toml.  The unsafe
//! blocks stay here: fishnet's own `#![forbid(unsafe_code)]` (src/main.rs:1) covers the
//! binary's modules, so this module carries an `#[allow(unsafe_code)]` at its `mod` line
//! in main.rs, or lives in a small library crate beside the -sys crate.
//!
//! Boundary (include/gpu_nnue.h): a `GpuNnue` owns one `gn_ctx`; the library serialises
//! calls on a context, so `&self` methods are safe to share across threads; call them
//! from `tokio::task::spawn_blocking` (the worker runtime is current_thread,
//! /root/reference/src/main.rs:44).
use std::{
    ffi::{CStr, CString},
    path::Path,
    ptr,
};

use gpu_nnue_sys as sys;
use shakmaty::{fen::Fen, uci::UciMove, Role, Square};

pub use sys::gn_child as GpuChild;
pub use sys::gn_eval as GpuEval;
pub use sys::gn_line as GpuLine;
pub use sys::gn_line2 as GpuLine2;
pub use sys::gn_pv as GpuPv;
pub use sys::gn_line3 as GpuLine3;

pub struct GpuNnue(*mut sys::gn_ctx);

// SAFETY: the library serialises every call on one context internally (gpu_nnue.h).
unsafe impl Send for GpuNnue {}
unsafe impl Sync for GpuNnue {}

#[derive(Debug, Clone)]
pub struct GpuError {
    pub code: i32,
    pub message: String,
}

impl std::fmt::Display for GpuError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "gpu_nnue error {}: {}", self.code, self.message)
    }
}

impl std::error::Error for GpuError {}

fn last_error(code: i32) -> GpuError {
    // SAFETY: gn_last_error returns a thread-local, NUL-terminated string.
    let message = unsafe { CStr::from_ptr(sys::gn_last_error()) }.to_string_lossy().into_owned();
    GpuError { code, message }
}

fn check(code: i32) -> Result<(), GpuError> {
    if code == sys::GN_OK {
        Ok(())
    } else {
        Err(last_error(code))
    }
}

fn cpath(p: &Path) -> CString {
    CString::new(p.as_os_str().as_encoded_bytes()).expect("path without NUL")
}

/// Every position plus every legal child (gn_evaluate_games with_children = 1).
pub struct GamesResult {
    pub position_offsets: Vec<u32>, // per game, into `positions`
    pub game_status: Vec<i32>,      // GN_OK or GN_E_ILLEGAL_MOVE per game
    pub positions: Vec<GpuEval>,
    pub child_offsets: Vec<u32>, // per position, into `children`
    pub child_moves: Vec<u16>,   // Stockfish move encoding
    pub children: Vec<GpuChild>, // (psqt, positional, final_cp + flags), ABI v4
}

impl GpuNnue {
    /// The two nets as files: nn-1c0000000000.nnue (big) and nn-37f18f62d772.nnue
    /// (small) (/root/reference/build.rs:8-9).
    pub fn load_net(big: &Path, small: &Path, devices: &[i32]) -> Result<GpuNnue, GpuError> {
        let (b, s) = (cpath(big), cpath(small));
        let mut ctx = ptr::null_mut();
        // SAFETY: valid C strings and an out pointer; devices may be empty (device 0).
        check(unsafe {
            sys::gn_load_net(b.as_ptr(), s.as_ptr(), devices.as_ptr(), devices.len() as i32, &mut ctx)
        })?;
        Ok(GpuNnue(ctx))
    }

    /// Both nets straight out of fishnet's embedded assets.ar.zst (the archive
    /// Assets::prepare reads, /root/reference/src/assets.rs:186-226), written once to a
    /// file; the first big and the first small .nnue member are taken.
    pub fn load_net_archive(archive: &Path, devices: &[i32]) -> Result<GpuNnue, GpuError> {
        let a = cpath(archive);
        let mut ctx = ptr::null_mut();
        // SAFETY: as above; NULL member names select by kind.
        check(unsafe {
            sys::gn_load_net_archive(a.as_ptr(), ptr::null(), ptr::null(), devices.as_ptr(), devices.len() as i32,
                                     &mut ctx)
        })?;
        Ok(GpuNnue(ctx))
    }

    /// evaluate_batch(&[Fen]) -> (psqt, positional, final_v, final_cp) per position,
    /// side-to-move POV, plus the score fishnet posts (score / GN_FLAG_MATE / best_move:
    /// checkmate, stalemate and checks included, include/gpu_nnue.h at gn_eval).
    pub fn evaluate_batch(&self, fens: &[Fen]) -> Result<Vec<GpuEval>, GpuError> {
        let owned: Vec<CString> = fens.iter().map(|f| CString::new(f.to_string()).unwrap()).collect();
        let ptrs: Vec<*const std::os::raw::c_char> = owned.iter().map(|c| c.as_ptr()).collect();
        let mut out = vec![GpuEval::default(); fens.len()];
        // SAFETY: ptrs / out have fens.len() elements and outlive the call.
        check(unsafe { sys::gn_evaluate_batch(self.0, ptrs.as_ptr(), ptrs.len(), out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// evaluate_batch plus the best `n_lines` moves of every position (MultiPV, 1..=8): the
    /// records as evaluate_batch returns them and `n_lines` ranked lines per position
    /// (lines[i * n_lines + k] = line k + 1 of position i; empty lines carry GN_FLAG_NO_SCORE;
    /// include/gpu_nnue.h at gn_line).  Each FEN goes to gn_evaluate_games_lines as a game without
    /// moves, so the children are ranked on the GPU and only the lines come back.  A FEN the
    /// library refuses fails the call, as it would fail the chunk.
    pub fn evaluate_lines(&self, fens: &[Fen], n_lines: usize) -> Result<(Vec<GpuEval>, Vec<GpuLine>), GpuError> {
        let owned: Vec<CString> = fens.iter().map(|f| CString::new(f.to_string()).unwrap()).collect();
        let gs: Vec<sys::gn_game> = owned
            .iter()
            .map(|root| sys::gn_game { root_fen: root.as_ptr(), uci_moves: ptr::null(), skip_positions: ptr::null(), n_skip: 0 })
            .collect();
        let mut offsets = vec![0u32; fens.len() + 1];
        let mut status = vec![0i32; fens.len()];
        let mut evals = vec![GpuEval::default(); fens.len()];
        let mut lines = vec![GpuLine::default(); fens.len() * n_lines];
        // SAFETY: a game without moves is one position, so fens.len() positions is the capacity
        // needed; every buffer has the length the call is told.
        check(unsafe {
            sys::gn_evaluate_games_lines(self.0, gs.as_ptr(), gs.len(), sys::GN_MODE_FULL, n_lines as i32,
                                         offsets.as_mut_ptr(), status.as_mut_ptr(), evals.as_mut_ptr(), fens.len(),
                                         lines.as_mut_ptr())
        })?;
        if let Some(&code) = status.iter().find(|&&s| s != sys::GN_OK) {
            return Err(last_error(code));
        }
        Ok((evals, lines))
    }

    /// The games-taking sibling of evaluate_lines: whole acquired batches (root FEN, UCI moves,
    /// skipPositions) with `n_lines` ranked lines per position, and the game's history taken into
    /// account as Stockfish takes `position fen ... moves ...`: a move that repeats a position for
    /// the third time or reaches the hundredth reversible half-move is valued 0 and carries
    /// GN_FLAG_DRAW (gn_evaluate_games_lines_history; include/gpu_nnue.h at gn_history).  Returns
    /// (position_offsets per game, game_status per game, records, lines[position * n_lines + k]);
    /// a game that fails has no positions, the others are still evaluated.
    #[allow(clippy::type_complexity)]
    pub fn evaluate_games_lines(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize)
                                -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine>), GpuError> {
        let gs: Vec<sys::gn_game> = games
            .iter()
            .map(|(root, moves, skip)| sys::gn_game {
                root_fen: root.as_ptr(),
                uci_moves: moves.as_ptr(),
                skip_positions: if skip.is_empty() { ptr::null() } else { skip.as_ptr() },
                n_skip: skip.len(),
            })
            .collect();
        let mut offsets = vec![0u32; games.len() + 1];
        let mut status = vec![0i32; games.len()];
        // a game has at most one position per move token and one for the root
        let cap: usize = games.iter().map(|(_, m, _)| m.as_bytes().split(|&b| b == b' ').filter(|t| !t.is_empty()).count() + 1).sum();
        let mut evals = vec![GpuEval::default(); cap];
        let mut lines = vec![GpuLine::default(); cap * n_lines];
        // SAFETY: offsets / status have games.len() (+ 1) elements, evals `cap` and lines
        // cap * n_lines; the call checks n_lines and the capacity before it writes.
        check(unsafe {
            sys::gn_evaluate_games_lines_history(self.0, gs.as_ptr(), gs.len(), sys::GN_MODE_FULL, n_lines as i32,
                                                 offsets.as_mut_ptr(), status.as_mut_ptr(), evals.as_mut_ptr(), cap,
                                                 lines.as_mut_ptr())
        })?;
        let total = offsets[games.len()] as usize;
        evals.truncate(total);
        lines.truncate(total * n_lines);
        Ok((offsets, status, evals, lines))
    }

    /// evaluate_games_lines with two-ply lines: per position `n_lines` lines of a move, the
    /// opponent's best reply and the minimax value after both, with the game's history taken into
    /// account at the child and at the reply (gn_evaluate_games_lines2_history; include/gpu_nnue.h
    /// at gn_line2).  A line that ends in a position drawn by rule is valued 0 and carries
    /// GN_FLAG_DRAW; `plies` is 1 when the move itself reaches the draw, 2 when the best reply does.
    /// Returns (position_offsets per game, game_status per game, records,
    /// lines[position * n_lines + k]); a game that fails has no positions.
    #[allow(clippy::type_complexity)]
    pub fn evaluate_games_lines2(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize)
                                 -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine2>), GpuError> {
        let gs: Vec<sys::gn_game> = games
            .iter()
            .map(|(root, moves, skip)| sys::gn_game {
                root_fen: root.as_ptr(),
                uci_moves: moves.as_ptr(),
                skip_positions: if skip.is_empty() { ptr::null() } else { skip.as_ptr() },
                n_skip: skip.len(),
            })
            .collect();
        let mut offsets = vec![0u32; games.len() + 1];
        let mut status = vec![0i32; games.len()];
        // a game has at most one position per move token and one for the root
        let cap: usize = games.iter().map(|(_, m, _)| m.as_bytes().split(|&b| b == b' ').filter(|t| !t.is_empty()).count() + 1).sum();
        let mut evals = vec![GpuEval::default(); cap];
        let mut lines = vec![GpuLine2::default(); cap * n_lines];
        // SAFETY: offsets / status have games.len() (+ 1) elements, evals `cap` and lines
        // cap * n_lines; the call checks n_lines and the capacity before it writes.
        check(unsafe {
            sys::gn_evaluate_games_lines2_history(self.0, gs.as_ptr(), gs.len(), sys::GN_MODE_FULL, n_lines as i32,
                                                  offsets.as_mut_ptr(), status.as_mut_ptr(), evals.as_mut_ptr(), cap,
                                                  lines.as_mut_ptr())
        })?;
        let total = offsets[games.len()] as usize;
        evals.truncate(total);
        lines.truncate(total * n_lines);
        Ok((offsets, status, evals, lines))
    }

    /// The best `n_lines` two-ply lines of every position (1..=8): the records as evaluate_batch
    /// returns them and, per position, `n_lines` lines of a move, the opponent's best reply and the
    /// minimax value after both (lines[i * n_lines + k] = line k + 1 of position i; `plies` is the
    /// PV's length, 1 when the move ends the game; empty lines carry GN_FLAG_NO_SCORE;
    /// include/gpu_nnue.h at gn_line2).  gn_evaluate_lines2 expands two plies and ranks on the GPU:
    /// only the records and the lines come back.  A FEN the library refuses has the
    /// GN_FLAG_BAD_FEN record and empty lines.
    pub fn evaluate_lines2(&self, fens: &[Fen], n_lines: usize) -> Result<(Vec<GpuEval>, Vec<GpuLine2>), GpuError> {
        let owned: Vec<CString> = fens.iter().map(|f| CString::new(f.to_string()).unwrap()).collect();
        let ptrs: Vec<*const std::os::raw::c_char> = owned.iter().map(|c| c.as_ptr()).collect();
        let mut evals = vec![GpuEval::default(); fens.len()];
        let mut lines = vec![GpuLine2::default(); fens.len() * n_lines];
        // SAFETY: ptrs / evals have fens.len() elements, lines fens.len() * n_lines; the call
        // checks n_lines before it writes.
        check(unsafe {
            sys::gn_evaluate_lines2(self.0, ptrs.as_ptr(), ptrs.len(), sys::GN_MODE_FULL, n_lines as i32,
                                    evals.as_mut_ptr(), lines.as_mut_ptr())
        })?;
        Ok((evals, lines))
    }

    /// evaluate_lines2 with check-extended leaves (gn_evaluate_lines2_extended; include/gpu_nnue.h at
    /// gn_line, "check-extended"): a grandchild in check with a legal move is valued as
    /// evaluate_batch would score it, by the in-check rule over its replies, instead of by a static
    /// number Stockfish never computes.  A line whose chosen reply reaches such a grandchild carries
    /// GN_FLAG_SEARCHED and may be a mate score.  The records equal evaluate_lines2's.
    pub fn evaluate_lines2_extended(&self, fens: &[Fen], n_lines: usize)
                                    -> Result<(Vec<GpuEval>, Vec<GpuLine2>), GpuError> {
        let owned: Vec<CString> = fens.iter().map(|f| CString::new(f.to_string()).unwrap()).collect();
        let ptrs: Vec<*const std::os::raw::c_char> = owned.iter().map(|c| c.as_ptr()).collect();
        let mut evals = vec![GpuEval::default(); fens.len()];
        let mut lines = vec![GpuLine2::default(); fens.len() * n_lines];
        // SAFETY: ptrs / evals have fens.len() elements, lines fens.len() * n_lines; the call
        // checks n_lines before it writes.
        check(unsafe {
            sys::gn_evaluate_lines2_extended(self.0, ptrs.as_ptr(), ptrs.len(), sys::GN_MODE_FULL, n_lines as i32,
                                             evals.as_mut_ptr(), lines.as_mut_ptr())
        })?;
        Ok((evals, lines))
    }

    /// evaluate_games_lines with check-extended leaves (gn_evaluate_games_lines_extended with the
    /// game's history): a move that gives check is valued by the in-check rule over the replies
    /// (GN_FLAG_SEARCHED), unless its child is drawn by rule (GN_FLAG_DRAW comes first).
    #[allow(clippy::type_complexity)]
    pub fn evaluate_games_lines_extended(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize)
                                         -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine>), GpuError> {
        let (gs, cap) = games_and_capacity(games);
        let mut offsets = vec![0u32; games.len() + 1];
        let mut status = vec![0i32; games.len()];
        let mut evals = vec![GpuEval::default(); cap];
        let mut lines = vec![GpuLine::default(); cap * n_lines];
        // SAFETY: offsets / status have games.len() (+ 1) elements, evals `cap` and lines
        // cap * n_lines; the call checks n_lines and the capacity before it writes.
        check(unsafe {
            sys::gn_evaluate_games_lines_extended(self.0, gs.as_ptr(), gs.len(), sys::GN_MODE_FULL, n_lines as i32, 1,
                                                  offsets.as_mut_ptr(), status.as_mut_ptr(), evals.as_mut_ptr(), cap,
                                                  lines.as_mut_ptr())
        })?;
        let total = offsets[games.len()] as usize;
        evals.truncate(total);
        lines.truncate(total * n_lines);
        Ok((offsets, status, evals, lines))
    }

    /// evaluate_games_lines2 with check-extended leaves (gn_evaluate_games_lines2_extended with the
    /// game's history): the grandchildren in check are valued by the in-check rule.
    #[allow(clippy::type_complexity)]
    pub fn evaluate_games_lines2_extended(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize)
                                          -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine2>), GpuError> {
        let (gs, cap) = games_and_capacity(games);
        let mut offsets = vec![0u32; games.len() + 1];
        let mut status = vec![0i32; games.len()];
        let mut evals = vec![GpuEval::default(); cap];
        let mut lines = vec![GpuLine2::default(); cap * n_lines];
        // SAFETY: as evaluate_games_lines_extended.
        check(unsafe {
            sys::gn_evaluate_games_lines2_extended(self.0, gs.as_ptr(), gs.len(), sys::GN_MODE_FULL, n_lines as i32, 1,
                                                   offsets.as_mut_ptr(), status.as_mut_ptr(), evals.as_mut_ptr(), cap,
                                                   lines.as_mut_ptr())
        })?;
        let total = offsets[games.len()] as usize;
        evals.truncate(total);
        lines.truncate(total * n_lines);
        Ok((offsets, status, evals, lines))
    }

    /// evaluate_lines2 with quiescent leaves (gn_evaluate_lines2_quiescent; include/gpu_nnue.h at
    /// gn_line, "quiescent"): a grandchild in check, or with a capture, an en-passant capture or a
    /// queen promotion to play, is valued by the capture search Q(x, depth) on the device instead of
    /// by its static evaluation; depth is 1..=sys::MAX_QUIESCE_DEPTH.  A line whose chosen reply
    /// reaches such a grandchild carries GN_FLAG_SEARCHED.  The records equal evaluate_lines2's.
    pub fn evaluate_lines2_quiescent(&self, fens: &[Fen], n_lines: usize, depth: i32, mode: i32)
                                     -> Result<(Vec<GpuEval>, Vec<GpuLine2>), GpuError> {
        let owned: Vec<CString> = fens.iter().map(|f| CString::new(f.to_string()).unwrap()).collect();
        let ptrs: Vec<*const std::os::raw::c_char> = owned.iter().map(|c| c.as_ptr()).collect();
        let mut evals = vec![GpuEval::default(); fens.len()];
        let mut lines = vec![GpuLine2::default(); fens.len() * n_lines];
        // SAFETY: ptrs / evals have fens.len() elements, lines fens.len() * n_lines; the call
        // checks n_lines and depth before it writes.
        check(unsafe {
            sys::gn_evaluate_lines2_quiescent(self.0, ptrs.as_ptr(), ptrs.len(), mode, n_lines as i32, depth,
                                              evals.as_mut_ptr(), lines.as_mut_ptr())
        })?;
        Ok((evals, lines))
    }

    /// evaluate_games_lines with quiescent leaves (gn_evaluate_games_lines_quiescent): a move whose
    /// child is searched is valued by Q(child, depth) (GN_FLAG_SEARCHED).  history: with the game's
    /// history, where a child drawn by rule comes first (GN_FLAG_DRAW, not searched); mode: GN_MODE_*.
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn evaluate_games_lines_quiescent(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize, depth: i32,
                                          history: bool, mode: i32)
                                          -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine>), GpuError> {
        let (gs, cap) = games_and_capacity(games);
        let mut offsets = vec![0u32; games.len() + 1];
        let mut status = vec![0i32; games.len()];
        let mut evals = vec![GpuEval::default(); cap];
        let mut lines = vec![GpuLine::default(); cap * n_lines];
        // SAFETY: as evaluate_games_lines_extended; depth is checked before anything is written.
        check(unsafe {
            sys::gn_evaluate_games_lines_quiescent(self.0, gs.as_ptr(), gs.len(), mode, n_lines as i32, history as i32,
                                                   depth, offsets.as_mut_ptr(), status.as_mut_ptr(), evals.as_mut_ptr(),
                                                   cap, lines.as_mut_ptr())
        })?;
        let total = offsets[games.len()] as usize;
        evals.truncate(total);
        lines.truncate(total * n_lines);
        Ok((offsets, status, evals, lines))
    }

    /// evaluate_games_lines2 with quiescent leaves (gn_evaluate_games_lines2_quiescent): the searched
    /// grandchildren are valued by Q(grandchild, depth); history and mode as above.
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn evaluate_games_lines2_quiescent(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize, depth: i32,
                                           history: bool, mode: i32)
                                           -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine2>), GpuError> {
        let (gs, cap) = games_and_capacity(games);
        let mut offsets = vec![0u32; games.len() + 1];
        let mut status = vec![0i32; games.len()];
        let mut evals = vec![GpuEval::default(); cap];
        let mut lines = vec![GpuLine2::default(); cap * n_lines];
        // SAFETY: as evaluate_games_lines_quiescent.
        check(unsafe {
            sys::gn_evaluate_games_lines2_quiescent(self.0, gs.as_ptr(), gs.len(), mode, n_lines as i32, history as i32,
                                                    depth, offsets.as_mut_ptr(), status.as_mut_ptr(), evals.as_mut_ptr(),
                                                    cap, lines.as_mut_ptr())
        })?;
        let total = offsets[games.len()] as usize;
        evals.truncate(total);
        lines.truncate(total * n_lines);
        Ok((offsets, status, evals, lines))
    }

    /// evaluate_lines2_quiescent with each line's whole variation (gn_evaluate_lines2_quiescent_pv;
    /// the header at gn_pv): pvs[i * n_lines + k] is line k's move and reply followed by the
    /// quiescence's own moves below the grandchild, what `pvs[multipv][depth]` takes.
    #[allow(clippy::type_complexity)]
    pub fn evaluate_lines2_quiescent_pv(&self, fens: &[Fen], n_lines: usize, depth: i32, mode: i32)
                                        -> Result<(Vec<GpuEval>, Vec<GpuLine2>, Vec<GpuPv>), GpuError> {
        let owned: Vec<CString> = fens.iter().map(|f| CString::new(f.to_string()).unwrap()).collect();
        let ptrs: Vec<*const std::os::raw::c_char> = owned.iter().map(|c| c.as_ptr()).collect();
        let mut evals = vec![GpuEval::default(); fens.len()];
        let mut lines = vec![GpuLine2::default(); fens.len() * n_lines];
        let mut pvs = vec![GpuPv::default(); fens.len() * n_lines];
        // SAFETY: as evaluate_lines2_quiescent; pvs has as many elements as lines.
        check(unsafe {
            sys::gn_evaluate_lines2_quiescent_pv(self.0, ptrs.as_ptr(), ptrs.len(), mode, n_lines as i32, depth,
                                                 evals.as_mut_ptr(), lines.as_mut_ptr(), pvs.as_mut_ptr())
        })?;
        Ok((evals, lines, pvs))
    }

    /// evaluate_games_lines_quiescent with each line's whole variation
    /// (gn_evaluate_games_lines_quiescent_pv): the move, then the quiescence's own moves.
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn evaluate_games_lines_quiescent_pv(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize, depth: i32,
                                             history: bool, mode: i32)
                                             -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine>, Vec<GpuPv>), GpuError> {
        let (gs, cap) = games_and_capacity(games);
        let mut offsets = vec![0u32; games.len() + 1];
        let mut status = vec![0i32; games.len()];
        let mut evals = vec![GpuEval::default(); cap];
        let mut lines = vec![GpuLine::default(); cap * n_lines];
        let mut pvs = vec![GpuPv::default(); cap * n_lines];
        // SAFETY: as evaluate_games_lines_quiescent; pvs has as many elements as lines.
        check(unsafe {
            sys::gn_evaluate_games_lines_quiescent_pv(self.0, gs.as_ptr(), gs.len(), mode, n_lines as i32,
                                                      history as i32, depth, offsets.as_mut_ptr(), status.as_mut_ptr(),
                                                      evals.as_mut_ptr(), cap, lines.as_mut_ptr(), pvs.as_mut_ptr())
        })?;
        let total = offsets[games.len()] as usize;
        evals.truncate(total);
        lines.truncate(total * n_lines);
        pvs.truncate(total * n_lines);
        Ok((offsets, status, evals, lines, pvs))
    }

    /// evaluate_games_lines2_quiescent with each line's whole variation
    /// (gn_evaluate_games_lines2_quiescent_pv): move, reply, then the quiescence's own moves.
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn evaluate_games_lines2_quiescent_pv(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize, depth: i32,
                                              history: bool, mode: i32)
                                              -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine2>, Vec<GpuPv>), GpuError> {
        let (gs, cap) = games_and_capacity(games);
        let mut offsets = vec![0u32; games.len() + 1];
        let mut status = vec![0i32; games.len()];
        let mut evals = vec![GpuEval::default(); cap];
        let mut lines = vec![GpuLine2::default(); cap * n_lines];
        let mut pvs = vec![GpuPv::default(); cap * n_lines];
        // SAFETY: as evaluate_games_lines_quiescent_pv.
        check(unsafe {
            sys::gn_evaluate_games_lines2_quiescent_pv(self.0, gs.as_ptr(), gs.len(), mode, n_lines as i32,
                                                       history as i32, depth, offsets.as_mut_ptr(), status.as_mut_ptr(),
                                                       evals.as_mut_ptr(), cap, lines.as_mut_ptr(), pvs.as_mut_ptr())
        })?;
        let total = offsets[games.len()] as usize;
        evals.truncate(total);
        lines.truncate(total * n_lines);
        pvs.truncate(total * n_lines);
        Ok((offsets, status, evals, lines, pvs))
    }

    /// Three-ply ranked lines (gn_evaluate_lines3; the header at gn_line3): per FEN the best n_lines
    /// lines of move, reply and the answer to it, valued after three plies under the leaf rule
    /// (sys::LEAF_*; depth 1..=sys::MAX_QUIESCE_DEPTH3 with LEAF_QUIESCE, else 0), and each line's
    /// whole variation: what `scores[multipv][depth]` / `pvs[multipv][depth]` take at depth 3.
    #[allow(clippy::type_complexity)]
    pub fn evaluate_lines3(&self, fens: &[Fen], n_lines: usize, leaf: i32, depth: i32, mode: i32)
                           -> Result<(Vec<GpuEval>, Vec<GpuLine3>, Vec<GpuPv>), GpuError> {
        let owned: Vec<CString> = fens.iter().map(|f| CString::new(f.to_string()).unwrap()).collect();
        let ptrs: Vec<*const std::os::raw::c_char> = owned.iter().map(|c| c.as_ptr()).collect();
        let mut evals = vec![GpuEval::default(); fens.len()];
        let mut lines = vec![GpuLine3::default(); fens.len() * n_lines];
        let mut pvs = vec![GpuPv::default(); fens.len() * n_lines];
        // SAFETY: as evaluate_lines2_quiescent_pv; lines and pvs have fens.len() * n_lines elements.
        check(unsafe {
            sys::gn_evaluate_lines3(self.0, ptrs.as_ptr(), ptrs.len(), mode, n_lines as i32, leaf, depth,
                                    evals.as_mut_ptr(), lines.as_mut_ptr(), pvs.as_mut_ptr())
        })?;
        Ok((evals, lines, pvs))
    }

    /// evaluate_lines3 from whole games (gn_evaluate_games_lines3): the front of
    /// evaluate_games_lines2, three-ply lines and their PVs per position, no game history.
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn evaluate_games_lines3(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize, leaf: i32, depth: i32,
                                 mode: i32)
                                 -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine3>, Vec<GpuPv>), GpuError> {
        self.games_lines3(games, n_lines, leaf, depth, mode, false)
    }

    /// evaluate_games_lines3 with each game's history (gn_evaluate_games_lines3_history; the header at
    /// gn_line3, "game history"): a child, reply or answer that is a third occurrence or reaches the
    /// fifty-move rule is the draw Stockfish sees there (GN_FLAG_DRAW, value 0; `plies` says at which
    /// of the three it lies).  What `position fen ... moves ...` analysis takes at depth 3.
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn evaluate_games_lines3_history(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize, leaf: i32,
                                         depth: i32, mode: i32)
                                         -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine3>, Vec<GpuPv>), GpuError> {
        self.games_lines3(games, n_lines, leaf, depth, mode, true)
    }

    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    fn games_lines3(&self, games: &[(CString, CString, Vec<u32>)], n_lines: usize, leaf: i32, depth: i32, mode: i32,
                    history: bool)
                    -> Result<(Vec<u32>, Vec<i32>, Vec<GpuEval>, Vec<GpuLine3>, Vec<GpuPv>), GpuError> {
        let (gs, cap) = games_and_capacity(games);
        let mut offsets = vec![0u32; games.len() + 1];
        let mut status = vec![0i32; games.len()];
        let mut evals = vec![GpuEval::default(); cap];
        let mut lines = vec![GpuLine3::default(); cap * n_lines];
        let mut pvs = vec![GpuPv::default(); cap * n_lines];
        // SAFETY: as evaluate_games_lines2_quiescent_pv.
        let call = if history { sys::gn_evaluate_games_lines3_history } else { sys::gn_evaluate_games_lines3 };
        check(unsafe {
            call(self.0, gs.as_ptr(), gs.len(), mode, n_lines as i32, leaf, depth, offsets.as_mut_ptr(),
                 status.as_mut_ptr(), evals.as_mut_ptr(), cap, lines.as_mut_ptr(), pvs.as_mut_ptr())
        })?;
        let total = offsets[games.len()] as usize;
        evals.truncate(total);
        lines.truncate(total * n_lines);
        pvs.truncate(total * n_lines);
        Ok((offsets, status, evals, lines, pvs))
    }

    /// GN_OPT_QUIESCE_SEE: with `true` the quiescent calls above prune the noisy moves whose exchange
    /// loses (see < 0; include/gpu_nnue.h at gn_line, "exchange evaluation").  The one option that
    /// changes results; off by default.
    pub fn set_quiesce_see(&self, on: bool) -> Result<(), GpuError> {
        // SAFETY: the context is live; the call only stores the value.
        check(unsafe { sys::gn_set_option(self.0, sys::GN_OPT_QUIESCE_SEE, i64::from(on)) })
    }

    /// Whole acquired batches: replay root FEN + UCI moves (skipPositions honoured) and
    /// evaluate every position and every legal child; buffers grow on GN_E_CAPACITY.
    pub fn evaluate_games(&self, games: &[(CString, CString, Vec<u32>)], mode: i32) -> Result<GamesResult, GpuError> {
        let gs: Vec<sys::gn_game> = games
            .iter()
            .map(|(root, moves, skip)| sys::gn_game {
                root_fen: root.as_ptr(),
                uci_moves: moves.as_ptr(),
                skip_positions: skip.as_ptr(),
                n_skip: skip.len(),
            })
            .collect();
        let (mut pcap, mut ccap) = (games.len() * 128, games.len() * 128 * 40);
        loop {
            let mut r = GamesResult {
                position_offsets: vec![0; games.len() + 1],
                game_status: vec![0; games.len()],
                positions: vec![GpuEval::default(); pcap],
                child_offsets: vec![0; pcap + 1],
                child_moves: vec![0; ccap],
                children: vec![GpuChild::default(); ccap],
            };
            // SAFETY: every buffer has the length the call is told.
            let rc = unsafe {
                sys::gn_evaluate_games(self.0, gs.as_ptr(), gs.len(), mode, 1, r.position_offsets.as_mut_ptr(),
                                       r.game_status.as_mut_ptr(), r.positions.as_mut_ptr(), pcap,
                                       r.child_offsets.as_mut_ptr(), r.child_moves.as_mut_ptr(),
                                       r.children.as_mut_ptr(), ccap)
            };
            if rc == sys::GN_E_CAPACITY {
                // the offsets hold the sizes needed
                pcap = pcap.max(*r.position_offsets.last().unwrap() as usize);
                let np = (*r.position_offsets.last().unwrap() as usize).min(r.child_offsets.len() - 1);
                ccap = ccap.max(r.child_offsets[np] as usize).max(ccap * 2);
                continue;
            }
            check(rc)?;
            let np = *r.position_offsets.last().unwrap() as usize;
            let nc = r.child_offsets[np] as usize;
            r.positions.truncate(np);
            r.child_offsets.truncate(np + 1);
            r.child_moves.truncate(nc);
            r.children.truncate(nc);
            return Ok(r);
        }
    }
}

/// The games as the C-ABI takes them (borrowing the strings and skip lists) and the position
/// capacity they need: a game has at most one position per move token and one for the root.
fn games_and_capacity(games: &[(CString, CString, Vec<u32>)]) -> (Vec<sys::gn_game>, usize) {
    let gs = games
        .iter()
        .map(|(root, moves, skip)| sys::gn_game {
            root_fen: root.as_ptr(),
            uci_moves: moves.as_ptr(),
            skip_positions: if skip.is_empty() { ptr::null() } else { skip.as_ptr() },
            n_skip: skip.len(),
        })
        .collect();
    let cap = games.iter().map(|(_, m, _)| m.as_bytes().split(|&b| b == b' ').filter(|t| !t.is_empty()).count() + 1).sum();
    (gs, cap)
}

/// The exchange evaluation of moves[i] on boards[i] (gn_see_moves; host only): what a CPU search
/// orders its captures by.  piece_value: P N B R Q, None: the defaults.  An entry of i32::MIN
/// (GN_NOT_EXTENDED) marks a rejected board or a move that is not legal there.
pub fn see_moves(boards: &[sys::gn_board], moves: &[u16], piece_value: Option<&[i32; 5]>) -> Result<Vec<i32>, GpuError> {
    assert_eq!(boards.len(), moves.len());
    let mut out = vec![0i32; boards.len()];
    // SAFETY: boards, moves and out have the same length; piece_value is 5 values or NULL.
    check(unsafe {
        sys::gn_see_moves(boards.as_ptr(), boards.len(), moves.as_ptr(),
                          piece_value.map_or(ptr::null(), |p| p.as_ptr()), out.as_mut_ptr())
    })?;
    Ok(out)
}

/// A move in Stockfish's 16-bit encoding (gn_eval.best_move, child_moves) as the Chess960 UCI
/// fishnet runs its engines with (castling = king takes rook, stockfish.rs:200).
pub fn move_to_uci(m: u16) -> UciMove {
    const PROMO: [Role; 4] = [Role::Knight, Role::Bishop, Role::Rook, Role::Queen];
    UciMove::Normal {
        from: Square::new(u32::from((m >> 6) & 63)),
        to: Square::new(u32::from(m & 63)),
        promotion: (m >> 14 == 1).then(|| PROMO[usize::from((m >> 12) & 3)]),
    }
}

impl Drop for GpuNnue {
    fn drop(&mut self) {
        // SAFETY: the context was created by gn_load_net* and is freed once.
        unsafe { sys::gn_free(self.0) }
    }
}
