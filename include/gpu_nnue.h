/*
 * gpu_nnue.h — C-ABI of libgpu_nnue.so, the MI355X (gfx950) batched Stockfish
 * NNUE evaluator for fishnet.
 *
 * Boundary being replaced / extended (reference = ounben/fishnet @ 2025-05-09):
 *   - StockfishStub::go_multiple(Chunk) -> Result<Vec<PositionResponse>, ChunkFailed>
 *     /root/reference/src/stockfish.rs:36-47 — the engine plugin API.  A GPU
 *     backend sits beside it; the Rust `gpu_nnue` module calls
 *     the functions below from tokio::task::spawn_blocking.
 *   - The static evaluation those engine processes run at every search leaf
 *     (Stockfish `Eval::evaluate`, inside the empty Stockfish submodule,
 *     /root/reference/.gitmodules:1-3) is what gn_evaluate_batch computes.
 *   - Nets: the reference ships nn-1c0000000000.nnue (big) and
 *     nn-37f18f62d772.nnue (small) next to the engine (/root/reference/build.rs:8-9,
 *     src/assets.rs:186-226); gn_load_net takes those files.
 *
 * Conventions: plain pointers and sizes; the caller owns every input and output
 * buffer, the library owns device memory.  Every function returns GN_OK (0) or a
 * negative GN_E_* code and never aborts or throws across the ABI; the message of
 * the last failure on the calling thread is gn_last_error().  A gn_ctx may be
 * shared between threads: calls on one context are serialised internally.
 */
#ifndef GPU_NNUE_H
#define GPU_NNUE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* v2: gn_eval carries final_cp (UCIEngine::to_cp) and 16-bit flags; gn_eval_params
 * carries the win-rate model; expansion shards over every device of the context.
 * v3: gn_eval is 24 bytes: final_cp is int32 and every evaluated position carries the
 * score fishnet posts (score, GN_FLAG_MATE / GN_FLAG_SEARCHED / GN_FLAG_NO_MOVES,
 * best_move): checkmate, stalemate and in-check positions included. */
/* v4: the host-buffer expansion calls (gn_expand_and_evaluate, gn_evaluate_games with
 * children) return every legal child as a 12-byte gn_child (psqt, positional, final_cp + flags:
 * the north star's (i32 psqt, i32 positional, i32 final_cp)) instead of a 24-byte gn_eval;
 * GN_OPT_CHUNK_PARENTS; GN_STAT_CHAIN_FALLBACKS removed (the planned expansion has no
 * fallback); the device-resident calls are documented as blocking (they were since v3). */
#define GN_ABI_VERSION 4

#if defined(__GNUC__)
#define GN_API __attribute__((visibility("default")))
#else
#define GN_API
#endif

/* return codes */
#define GN_OK 0
#define GN_E_INVALID (-1)  /* bad argument                                    */
#define GN_E_IO (-2)       /* cannot read a net file                          */
#define GN_E_FORMAT (-3)   /* not a supported .nnue (version/hash/size)       */
#define GN_E_HIP (-4)      /* HIP runtime error (message has the detail)      */
#define GN_E_NOMEM (-5)    /* host or device allocation failed                */
#define GN_E_CAPACITY (-6) /* caller's output buffer too small                */
#define GN_E_NODEVICE (-7) /* no usable gfx950 device                         */
#define GN_E_NONET (-8)    /* the requested mode needs a net that is not loaded */
#define GN_E_ILLEGAL_MOVE (-9) /* a game's UCI move does not resolve to a legal move */

/* evaluation modes */
#define GN_MODE_FULL 0  /* Eval::evaluate: small net when |simple_eval| > 962,
                           big-net re-evaluation when |nnue| < 236            */
#define GN_MODE_BIG 1   /* big net for every position (epilogue: smallNet=false) */
#define GN_MODE_SMALL 2 /* small net for every position (epilogue: smallNet=true) */

/* options (gn_set_option / gn_get_option) */
#define GN_OPT_CHUNK_PARENTS 6        /* host-buffer expansion pipeline (gn_expand_and_evaluate,
                                         gn_evaluate_games with children): parents per chunk,
                                         cut at game starts; 0 (default): automatic (whole
                                         games, >= 165,888 parents per chunk, a short last
                                         chunk).  gn_evaluate_lines2 (depth 2, ~1,000
                                         grandchildren per parent): exactly this many parents
                                         per chunk; 0 (default): 1,024.  Results are
                                         identical for every value.                         */
#define GN_OPT_COALESCE 7             /* 1 (default): concurrent gn_evaluate_batch calls on one
                                         context are merged into one launch (each call
                                         queues; one call leads a launch over every queued
                                         call of its mode; a lone call runs at once, no
                                         timer); 0: calls run one after another.  Results
                                         are identical either way.                        */
#define GN_OPT_FAST_BATCH 9           /* 1 (default): a gn_evaluate_batch of <= 4,096 positions on
                                         a one-device context runs as one captured HIP graph
                                         (upload, evaluation, both levels of the score rule's
                                         in-check replies, download: one host synchronisation
                                         per call); 0: the general path (a launch sequence with
                                         a host round trip per reply level).  Results are
                                         identical either way.                              */
#define GN_OPT_EXPAND_PIPELINE 10     /* 1: consecutive planned expansions of one call
                                         (gn_time_expand_device's iterations, the host-buffer
                                         pipeline's chunks) overlap: expansion k + 1's child
                                         generation and plan run on a second stream while
                                         expansion k's finalize and score rule run (two
                                         buffer sets); 2 (default): the next child
                                         generation and plan start while expansion k's row
                                         stream still runs (151.3 against 153.9 ms per bench
                                         step unpipelined); 0: one after another.  Results
                                         are identical for every value.                     */
#define GN_OPT_QUIESCE_SEE 11         /* 0 (default): the quiescent calls search every noisy
                                         move (Q / PVQ at gn_line).  1: gn_quiesce_device,
                                         gn_quiesce_pv_device and the six _quiescent /
                                         _quiescent_pv host-buffer calls follow Qs / PVQs: a
                                         node that is not in check searches only its noisy
                                         moves with see >= 0 (gn_line, "exchange
                                         evaluation").  Read once when a call starts; no
                                         other call reads it.  Any other value:
                                         GN_E_INVALID, the option unchanged.  This is the one
                                         option whose values give DIFFERENT results.        */
#define GN_OPT_INCREMENTAL_CHILDREN 1 /* 1 (default): children from the parent accumulators
                                         by add/sub deltas; 0: full refresh per child    */
#define GN_OPT_XCD_SWIZZLE 2          /* bit mask, default 9: each XCD takes a contiguous
                                         range of parents (bit 0, small-net expansion) / of
                                         16-position tiles (bit 1, batch evaluation) / of
                                         blocks (bit 2, big-net expansion); 0: dispatch order
                                         (big-net expansion: blocks claimed in order by an
                                         atomic counter); bit 3 (big-net expansion, without
                                         bit 2; default): each XCD claims blocks of its own
                                         eighth of the order, then of the others' (stream
                                         205.1 -> 203.6 ms against one counter)          */
#define GN_OPT_KING_SORT 3            /* 1 (default): evaluate a batch of >= 1,024 positions
                                         (2: of any size) in (white king, black
                                         king) square order for L2 / Infinity-Cache
                                         locality, then (big net) by layer-stack bucket and
                                         30 home-square bits (ranks 1, 2, 7, 8 without
                                         e1/e8: the start position's piece still stands
                                         there) so that 16-position tiles share rows
                                         gathered once per tile and one layer stack; small
                                         net: by bucket, then kings; results in input
                                         order; 0: input order                            */
#define GN_OPT_KING_CACHE 5           /* 1 (default): with the chained walk, a king-move
                                         child's refresh starts from the accumulator the
                                         workgroup last computed for that (perspective,
                                         king square) in the same block, plus the placement
                                         difference, when that is shorter (Stockfish's
                                         AccumulatorCaches analog); 0: full refresh.
                                         Results are identical either way.               */
#define GN_OPT_CHAIN 4                /* expansion (big net): a workgroup walks blocks of up to
                                         this many consecutive parents (default 81: one
                                         80-ply game); a parent that is a child of the
                                         previous one (same placement) starts from that
                                         child's accumulators instead of a refresh.
                                         Shortened when the blocks would not fill the GPU;
                                         -k: exactly k.  0, 1 or -1: every parent
                                         refreshes.  Results are identical either way.    */
#define GN_OPT_STREAM_SLICES 8        /* expansion with a 3072-wide big net: 3 (default): the
                                         accumulator columns in three slices of 1,024, one
                                         stream launch each over every entry, so that an
                                         XCD's L2 holds the slice's rows of the king buckets
                                         in flight; 1: one launch over whole rows.  Results
                                         are identical either way.  The slices' fc_0 partial
                                         sums take 152 B of device memory per evaluated
                                         position (parents + children of a call or chunk);
                                         when that allocation fails the call runs the
                                         whole-row stream instead.                        */

/* read-only statistics (gn_get_option) */
#define GN_STAT_PLAN_NS 101           /* the last gn_time_expand_device's planned big net
                                         (max over devices, per iteration, nanoseconds):
                                         plan_kernel (lists, tiles, PSQT) ...            */
#define GN_STAT_STREAM_NS 102         /* ... and stream_eval_kernel (row stream + layer
                                         stack; all its launches: three column slices by
                                         default), the expansion's dominant kernel ...   */
#define GN_STAT_FINISH_NS 104         /* ... and the column-sliced stream's layer-stack
                                         finish as a step of its own (~0: finalize computes
                                         each output itself, as with one launch)           */
#define GN_STAT_ZERO_ROW_ENTRIES 105  /* list entries the last planned expansion put on the
                                         all-zero row (per device, summed): entries that
                                         move no feature row and add nothing.  0: a chained
                                         parent takes the result of the child that is its
                                         position, and a king-cache store rides on its
                                         slot's last row entry (both were such entries)  */
#define GN_STAT_SCRATCH_PADS 103      /* no-op entries the last planned expansion inserted
                                         (per device, summed) so that every king-cache load
                                         sits >= ring depth (4) list entries after the
                                         list's last king-cache store (the load then issues
                                         after the store, from the same lanes)            */
/* stage times of the last gn_evaluate_games / gn_expand_and_evaluate (nanoseconds; per-device
 * stages: the slowest device).  The expansion runs in chunks of whole games; a drain thread
 * downloads chunk c's records on a copy stream while chunk c + 1 computes.  The two-ply lines
 * calls (gn_evaluate_lines2, gn_evaluate_games_lines2 and its history form) fill them too:
 * their chunks run one after the other, compute then download, and leave no tail.         */
#define GN_STAT_HOST_PARSE_NS 110     /* host: root FENs / FENs parsed, UCI moves tokenized */
#define GN_STAT_HOST_UPLOAD_NS 111    /* host -> device copies of the inputs               */
#define GN_STAT_HOST_REPLAY_NS 112    /* the GPU replay of the games' moves (games only)   */
#define GN_STAT_HOST_COMPUTE_NS 113   /* children, evaluation and score rule, all chunks   */
#define GN_STAT_HOST_DOWNLOAD_NS 114  /* device -> host result copies, all chunks (they
                                         overlap the next chunk's compute)               */
#define GN_STAT_HOST_TAIL_NS 115      /* the downloads still running after the last chunk
                                         computed (not overlapped)                        */
#define GN_STAT_HOST_TOTAL_NS 116     /* the whole call                                    */
#define GN_STAT_RANK_NS 121           /* rank_children_kernel in the last
                                         gn_evaluate_games_lines, or its history variant in
                                         the last gn_evaluate_games_lines_history, summed
                                         over its chunks (0 after any other host-buffer
                                         call)                                             */
#define GN_STAT_KEYS_NS 123           /* position_keys_kernel in the last
                                         gn_evaluate_games_lines_history,
                                         gn_evaluate_games_lines2_history or
                                         gn_evaluate_games_lines3_history (the slowest
                                         device; 0 after any other host-buffer call)       */
#define GN_STAT_RANK2_NS 122          /* rank_lines2_kernel in the last gn_evaluate_lines2 or
                                         gn_evaluate_games_lines2, or its history variant in
                                         the last gn_evaluate_games_lines2_history, summed
                                         over its chunks (the slowest device; 0 after any
                                         other host-buffer call)                           */
#define GN_STAT_EXTEND_NS 124         /* the check extension (gn_line "check-extended") in the
                                         last gn_evaluate_lines2_extended or
                                         gn_evaluate_games_lines[2]_extended, summed over its
                                         chunks (the slowest device; 0 after any other
                                         host-buffer call) ...                             */
#define GN_STAT_EXTENDED_LEAVES 125   /* ... and the leaves it extended, summed over the
                                         devices (0 after any other host-buffer call)      */
#define GN_STAT_QUIESCE_NS 126        /* the capture quiescence (gn_line "quiescent") in the last
                                         gn_evaluate_lines2_quiescent or
                                         gn_evaluate_games_lines[2]_quiescent, summed over its
                                         chunks (the slowest device; 0 after any other
                                         host-buffer call) ...                             */
#define GN_STAT_QUIESCE_LEAVES 127    /* ... the leaves it searched, summed over the devices */
#define GN_STAT_QUIESCE_NODES 128     /* ... and the positions it evaluated below them (both
                                         0 after any other host-buffer call)               */
#define GN_STAT_PV_NS 129             /* the PV kernels (the walk down the quiescence's levels and
                                         the assembly of the gn_pv entries) in the last
                                         gn_evaluate_lines2_quiescent_pv or
                                         gn_evaluate_games_lines[2]_quiescent_pv, summed over its
                                         chunks (the slowest device; 0 after any other
                                         host-buffer call)                                 */
#define GN_STAT_RANK3_NS 130          /* rank_lines3_kernel in the last gn_evaluate_lines3 or
                                         gn_evaluate_games_lines3, or its history variant in the
                                         last gn_evaluate_games_lines3_history, summed over its
                                         chunks (the slowest device); 0 after any other
                                         host-buffer call.
                                         The two-ply stages below the root feed GN_STAT_RANK2_NS,
                                         GN_STAT_EXTEND_*, GN_STAT_QUIESCE_*, GN_STAT_PV_NS and
                                         GN_STAT_HOST_* as they do for the two-ply calls       */
#define GN_STAT_BATCH_LAUNCHES 117    /* merged gn_evaluate_batch launches since load ...   */
#define GN_STAT_BATCH_CALLS 118       /* ... and the calls they served (GN_OPT_COALESCE)    */
#define GN_STAT_FAST_BATCHES 119      /* evaluations run by the captured small-batch graphs
                                         (GN_OPT_FAST_BATCH) since load ...                 */
#define GN_STAT_FAST_FALLBACKS 120    /* ... and those rerun on the general path because a
                                         reply level exceeded the graph's capacity          */

/* per-position flags */
#define GN_FLAG_IN_CHECK 1u /* side to move in check: Stockfish has no static eval
                               (Eval::evaluate asserts !checkers); values are still
                               computed but are not a Stockfish result            */
#define GN_FLAG_SMALLNET 2u /* final_v came from the small net                    */
#define GN_FLAG_BAD_FEN 4u  /* unparsable / unsupported position; values are 0     */
#define GN_FLAG_REEVAL 8u   /* small net was run, then the big net re-evaluated   */
#define GN_FLAG_SKIPPED 16u /* listed in skipPositions: not evaluated, values 0    */
#define GN_FLAG_MATE 32u    /* score is a mate distance (UCI `score mate <score>`)  */
#define GN_FLAG_NO_SCORE 64u /* no score: skipped / bad position, or a child record */
#define GN_FLAG_SEARCHED 128u /* score from the in-check rule over the legal replies
                                 (best_move set), not from the static evaluation; on
                                 gn_line.flags / gn_line2.flags of the check-extended
                                 calls only: the line's leaf is valued by that rule;
                                 of the quiescent calls: by the quiescence Q(x, depth) */
#define GN_FLAG_NO_MOVES 256u /* no legal move: checkmate (with IN_CHECK) or stalemate */
#define GN_FLAG_DRAW 512u /* gn_line.flags, gn_line2.flags and gn_line3.flags of the history
                             calls only: the line ends in a position drawn by rule (threefold
                             repetition or fifty-move rule; gn_history, gn_line2 and gn_line3
                             below)                                                     */

/* One result.  psqt/positional are Network::evaluate's NetworkOutput (already
 * divided by OutputScale = 16) of the net that produced final_v; final_v is
 * Eval::evaluate(pos, optimism = 0) in internal Value units; final_cp is
 * final_v in centipawns as Stockfish prints it (UCIEngine::to_cp: the win-rate
 * model's a(material), round(100 * v / a)); all side-to-move POV.
 *
 * score is what fishnet posts for the position: the `score cp X` / `score mate N` a
 * Stockfish `go` prints and stockfish.rs:419-431 parses; fishnet requires one for
 * every analysed position (stockfish.rs:366-368, ipc.rs:56 `expect("got score")`).
 * The rule, for every position a call is given (batch, game and parent positions):
 *   - no legal move: checkmate -> `mate 0` (GN_FLAG_MATE, score 0), stalemate -> `cp 0`
 *     (what Stockfish prints at depth 0); GN_FLAG_NO_MOVES;
 *   - not in check: score = final_cp (the static evaluation);
 *   - in check with legal moves (Stockfish has no static eval there): a check extension,
 *     value(p, d) = max over legal replies c of -value(c, d - 1) from d = 2, where a reply
 *     with no legal move is mated (-VALUE_MATE = -32000) or stalemated (0), a reply not in
 *     check -- or any reply at d = 0 -- takes its static final_v, and mate values move one
 *     ply toward zero per level (VALUE_MATE - ply); ties go to the smaller move encoding.
 *     score = `mate (ply + 1) / 2` / `mate -ply / 2` for |value| >= 31754
 *     (VALUE_MATE_IN_MAX_PLY), else to_cp(value) with this position's material;
 *     GN_FLAG_SEARCHED, best_move = the reply (Stockfish encoding).
 * Child and grandchild records of the expansion calls carry GN_FLAG_NO_SCORE (score 0):
 * they are search data, not positions fishnet posts. */
typedef struct gn_eval {
  int32_t psqt;
  int32_t positional;
  int32_t final_v;
  int32_t final_cp;
  int32_t score;
  uint16_t flags;
  uint16_t best_move;
} gn_eval;

/* One legal child as the host-buffer expansion calls return it (ABI v4, 12 bytes): the child's
 * static evaluation, north star `(i32 psqt, i32 positional, i32 final_cp)`, with the flags
 * packed beside final_cp.  psqt / positional / final_cp are those of the child's gn_eval record
 * (side-to-move POV); cp_flags = (final_cp & 0xFFFFFF) | (flags & 0xFF) << 24: final_cp as a
 * signed 24-bit integer (|final_cp| < 2^23 always: gn_set_eval_params keeps the win-rate
 * model's a(material) >= 1, and |final_v| <= value_clamp), flags the record's low 8 flag bits
 * (GN_FLAG_IN_CHECK, GN_FLAG_SMALLNET, GN_FLAG_REEVAL; GN_FLAG_NO_SCORE is always set: a child
 * carries no score).  Decode with GN_CHILD_FINAL_CP / GN_CHILD_FLAGS. */
typedef struct gn_child {
  int32_t psqt;
  int32_t positional;
  int32_t cp_flags;
} gn_child;
#define GN_CHILD_FINAL_CP(c) ((int32_t)((uint32_t)(c).cp_flags << 8) >> 8)
#define GN_CHILD_FLAGS(c) ((uint32_t)(c).cp_flags >> 24)

/* One ranked line of a position (MultiPV): what fishnet's `multipv` asks the engine for
 * (Work::Analysis in the reference's src/api.rs; src/stockfish.rs sends `setoption name MultiPV`
 * and fills scores[multipv][depth] / pvs[multipv][depth] of a PositionResponse from the `info`
 * lines).  gn_rank_children_device and gn_evaluate_games_lines return n_lines of them per
 * position, 1 <= n_lines <= GN_MAX_LINES.
 * The rule, for a position p a call evaluates (not skipped, not bad) with at least one legal
 * move, over every legal move m with child c:
 *   value(m) = negate_ply(V(c)): negated, mate values one ply further from the mate, where
 *   V(c) = -VALUE_MATE (-32000) when c has no legal move and is in check (m mates),
 *   V(c) = 0 when c has no legal move and is not in check (m stalemates),
 *   V(c) = c's static final_v in the call's mode otherwise -- also when c is in check (the
 *   values gn_eval documents as "still computed").
 * This is the score rule above at depth 1, without its recursion into replies that give check.
 * Lines are ordered by value descending, ties to the smaller 16-bit move encoding (the score
 * rule's tie rule).  A position with fewer legal moves than n_lines has empty lines after its
 * last move (value 0, score 0, move 0, flags GN_FLAG_NO_SCORE); a skipped, bad, checkmated or
 * stalemated position has only empty lines.
 * Line 1 and gn_eval.score: for a position in check, line 1's score / move / GN_FLAG_MATE equal
 * that position's gn_eval.score / best_move / GN_FLAG_MATE whenever none of its replies is
 * itself in check with a legal move; otherwise they may differ, the score rule going one level
 * deeper at such a reply.
 *
 * Check-extended lines (gn_extend_checks_device, gn_rank_children_extended_device,
 * gn_rank_lines2_extended_device, gn_evaluate_lines2_extended, gn_evaluate_games_lines_extended,
 * gn_evaluate_games_lines2_extended).  The calls above value a leaf in check by a static number
 * Stockfish never computes.  The extended calls value every leaf exactly as the library would
 * score that position if it were handed to gn_evaluate_batch_mode: leaf value E(x), in this order
 * of precedence:
 *   1. x has no legal move: -VALUE_MATE when in check, else 0, GN_FLAG_NO_MOVES (unchanged);
 *   2. the history forms only: x is drawn by rule (gn_history below): 0 with GN_FLAG_DRAW; the
 *      extension is not consulted (Stockfish tests the draw at node entry);
 *   3. x is in check with a legal move: E(x) = value(x, 2) of the gn_eval.score rule in the call's
 *      mode -- the maximum over the legal replies of negate_ply, a reply in check with a legal move
 *      going one level down, any reply at depth 0 taking its static final_v, ties to the smaller
 *      move -- and the line carries GN_FLAG_SEARCHED.  The extension knows no history, as
 *      gn_eval.score knows none;
 *   4. otherwise x's static final_v.
 * A gn_line uses V(c) := E(c).  A gn_line2 uses V1(g) := E(g); the child c stays an interior node,
 * searched through all its replies, its own value never used, and GN_FLAG_SEARCHED is set exactly
 * when the chosen reply's grandchild was extended (as GN_FLAG_DRAW is).  move, reply, plies (1 or 2:
 * the extension's own replies are not reported), negate_ply, rule_score, the order, the ties and
 * the empty lines are unchanged.  Consequences: for an extended leaf x, rule_score(E(x), x's
 * material) and the mate flag are what gn_evaluate_batch_mode returns for x in the same mode; a
 * position none of whose leaves is in check with a legal move has byte-equal lines from the plain
 * and the extended call; for a child with a reply, (R(c), reply) is line 1 of the extended one-ply
 * ranking over the children as parents; and mate values can appear on lines through a check
 * (`mate -1` for a check that allows a mating reply, `mate 2`, ...).
 *
 * Quiescent lines (gn_quiesce_device, gn_evaluate_lines2_quiescent,
 * gn_evaluate_games_lines_quiescent, gn_evaluate_games_lines2_quiescent).  The calls above value a
 * leaf that is not in check by its static final_v even when the side to move can take a queen or
 * the leaf sits in the middle of an exchange.  The quiescent calls value a non-quiet leaf by a
 * capture search to a fixed depth, on the device.
 * Noisy moves.  A legal move is noisy when it is a capture (the destination holds an enemy piece
 * and the move is not castling: castling is encoded king-takes-own-rook and is never noisy, Chess960
 * included), an en-passant capture, or a promotion to a queen, capturing or not.  An underpromotion
 * is noisy only when it captures.
 * Q(x, d), self-contained (it does not call the score rule):
 *   1. x has no legal move: -VALUE_MATE when in check, else 0;
 *   2. d == 0: x's static final_v in the call's mode (in check too, as the score rule at depth 0);
 *   3. x is in check: the maximum over ALL legal moves of negate_ply(Q(child, d - 1)); no stand pat;
 *   4. otherwise max(final_v(x), the maximum over the noisy legal moves of negate_ply(Q(child, d - 1))).
 * The leaf value, depth in 1..GN_MAX_QUIESCE_DEPTH: a leaf x of a line is searched when it has a
 * legal move and is in check, or has a legal move and at least one noisy legal move.  A searched
 * leaf's value is Q(x, depth) and its line carries GN_FLAG_SEARCHED; every other leaf keeps
 * GN_NOT_EXTENDED and the ranking values it as the plain calls do: mate, stalemate or static.  The
 * precedence in the ranking is the extended calls': no legal move, then (history forms) drawn by
 * rule, then the d_ext override, then static.  The quiescence knows no history and no fifty-move
 * rule inside its tree, as the extension knows none, and its own moves are not reported in the line
 * (plies stays 1 or 2; the _pv calls below return them beside it).  The quiescent calls do not also run the check extension: rule 3 is how they treat a leaf
 * in check.  Consequences: for a leaf in check, Q(x, 1) equals the score rule's value(x, 1); for a
 * searched leaf not in check, Q(x, d) >= final_v(x); a position none of whose leaves is searched has
 * byte-equal lines from the plain and the quiescent call; and mate values can appear on a line
 * through a capture.
 *
 * The quiescence's own moves (gn_pv below; gn_quiesce_pv_device, gn_line_pvs_device,
 * gn_line2_pvs_device, gn_evaluate_lines2_quiescent_pv, gn_evaluate_games_lines_quiescent_pv,
 * gn_evaluate_games_lines2_quiescent_pv).  PVQ(x, d) is the quiescence's variation below a leaf x,
 * with the same Q, noisy moves, negate_ply and searched set:
 *   1. x has no legal move, or d == 0: PVQ is empty;
 *   2. x is in check: m* = the legal move that maximises negate_ply(Q(child(m), d - 1)), ties to
 *      the smaller 16-bit move encoding; PVQ = [m*] + PVQ(child(m*), d - 1);
 *   3. otherwise m* = the same argmax over the noisy legal moves, if there is one; if
 *      negate_ply(Q(child(m*), d - 1)) > final_v(x), PVQ = [m*] + PVQ(child(m*), d - 1), else PVQ
 *      is empty: stand pat wins a tie with a move, so the shorter PV wins.
 * Consequences: len(PVQ(x, d)) <= d; every move of it is legal where it is played, and noisy
 * unless the mover is in check; and with x_end the position after PVQ and v = -VALUE_MATE (in
 * check) or 0 when x_end has no legal move, else x_end's static final_v in the call's mode,
 * negate_ply applied len times to v equals Q(x, d).
 * A line's PV (gn_pv): an empty line (GN_FLAG_NO_SCORE) has len 0; a gn_line has [move], followed
 * by PVQ(child, depth) exactly when the line carries GN_FLAG_SEARCHED; a gn_line2 has [move] when
 * plies == 1, else [move, reply], followed by PVQ(grandchild, depth) exactly when plies == 2 and
 * the line carries GN_FLAG_SEARCHED.  A leaf the ranking values as mate, as stalemate or, in the
 * history forms, as drawn by rule has no tail, even where the quiescence searched it: such a line
 * never carries GN_FLAG_SEARCHED.  The check extension's replies are not reported.
 *
 * Exchange evaluation (gn_see_moves, gn_see_device, GN_OPT_QUIESCE_SEE).  see(x, m) is an int32_t,
 * defined for a position x that passes the gate (gn_board) and a legal move m of x: the classical swap
 * list on m's destination.  v(P N B R Q) = gn_eval_params.piece_value[0..4] (the host call takes them
 * as an argument; NULL: the defaults 208 781 825 1276 2538); v(K) = 0.
 *   - m is castling, an en-passant capture or a promotion (capturing or not): see = 0 (Stockfish's
 *     convention for non-normal moves).
 *   - Otherwise, with `to` m's destination, P0 the type of the moving piece, occ0 the occupancy of x
 *     without m's origin square and c = v(type of the piece on `to`), 0 when `to` is empty:
 *     see = c - R(P0, occ0, the side that did not move).
 *   - R(P, occ, s).  A = the pieces of x, as they stand in x, that are in occ and attack `to` with
 *     occupancy occ: a pawn by its colour's capture direction, knights and kings by their steps, a
 *     bishop, rook or queen along its lines with occ as the blockers (so a slider behind a piece that
 *     has left occ counts).  The piece that moved is not in occ, and `to` is never in A.
 *       If A holds no piece of side s: R = 0.  Otherwise a = s's piece in A of the lowest type in the
 *       order P, N, B, R, Q, K (by type, never by the configured values), among those the one on the
 *       lowest square index.
 *       a is a king and A holds a piece of the other side: R = 0 (a king does not capture onto an
 *       attacked square; the same A, not a recomputed one).
 *       a is a king and A holds no piece of the other side: R = max(0, v(P)), and the exchange ends.
 *       Otherwise R = max(0, v(P) - R(type(a), occ without a's square, the other side)).
 * Pins are ignored, and a pawn that recaptures on a back rank stays a pawn.  Arithmetic is int32; the
 * result is defined while 32 * max|piece_value| < 2^31.  see is NOT invariant under the board
 * symmetries: between two attackers of one type the lower square captures first.
 * Pruned quiescence.  Qs(x, d) is Q(x, d) with rule 4 replaced by
 *   4s. otherwise max(final_v(x), the maximum over the noisy legal moves m with see(x, m) >= 0 of
 *       negate_ply(Qs(child, d - 1))).
 * Rules 1 to 3 stand: a node in check searches every legal move.  A kept move is a noisy legal move
 * with see >= 0; a leaf is searched when it has a legal move and is in check, or has a kept move.  A
 * leaf whose noisy moves all lose keeps GN_NOT_EXTENDED: its line carries no GN_FLAG_SEARCHED and
 * takes the static value.  PVQs is PVQ over the kept moves.  The ranking's precedence, the history
 * forms, negate_ply, the score rule, the ties and the empty lines are unchanged, and the searched /
 * nodes counts and GN_STAT_QUIESCE_* count the pruned tree.  Consequences: Qs(x, 1) <= Q(x, 1) for a
 * leaf not in check (no inequality holds from depth 2 on: pruning the opponent's moves raises a
 * value); the nodes under pruning are at most those without it; and a position below none of whose
 * searched leaves a noisy legal move loses has byte-equal results with and without pruning. */
#define GN_NOT_EXTENDED INT32_MIN /* a d_ext entry of a leaf the extension / quiescence does not value */
#define GN_MAX_QUIESCE_DEPTH 4    /* the quiescent calls' depth is 1..GN_MAX_QUIESCE_DEPTH */
#define GN_MAX_PV (2 + GN_MAX_QUIESCE_DEPTH) /* a line's two moves and the quiescence's own */
#define GN_MAX_LINES 8 /* lichess sends multipv <= 5 */
typedef struct gn_line {
  int32_t value;  /* the rule value, p's side-to-move POV, Stockfish units              */
  int32_t score;  /* rule_score(value, p's win-rate material): cp, or the mate distance
                     with GN_FLAG_MATE (as gn_eval.score)                                */
  uint16_t move;  /* Stockfish encoding, castling = king takes rook                      */
  uint16_t flags; /* GN_FLAG_MATE; GN_FLAG_IN_CHECK: the move gives check;
                     GN_FLAG_NO_MOVES: the move ends the game (mate or stalemate);
                     GN_FLAG_NO_SCORE: an empty line; GN_FLAG_DRAW: the history calls
                     only (gn_history below); GN_FLAG_SEARCHED: the check-extended
                     and the quiescent calls only (above)                                */
} gn_line;

/* The whole variation of one ranked line (the rule at gn_line, "the quiescence's own moves"):
 * what fishnet's pvs[multipv][depth], a Vec<UciMove>, takes.  Unused entries and reserved are 0. */
typedef struct gn_pv { /* 16 bytes */
  uint16_t len;              /* moves in the PV, 0..GN_MAX_PV */
  uint16_t moves[GN_MAX_PV]; /* Stockfish encoding, castling = king takes rook */
  uint16_t reserved;
} gn_pv;

/* Game-history draws in ranked lines (gn_rank_children_history_device,
 * gn_evaluate_games_lines_history): what Stockfish, given `position fen ... moves ...`, scores
 * as a draw at ply 1 of a search (Position::is_draw).
 * Identity.  A position's identity is its piece placement, its side to move, the canonical
 * castling rook squares and the canonical en-passant square: the first four fields of the FEN
 * gn_board_to_fen writes for the canonical board.  rule50, fullmove and reserved are not part
 * of it.
 * Key.  gn_position_keys gives a 64-bit key that is a function of exactly the identity, never 0
 * for a position that passes the gate (0: a rejected board).  With the board's bitboards
 * (bit s = square s) w0..w5 = pawns, knights, bishops, rooks, queens, kings of both colours,
 * w6 = white's pieces, w7 = stm | ep << 8 | rook[0] << 16 | rook[1] << 24 | rook[2] << 32 |
 * rook[3] << 40 (stm 1 = black; ep and the castling rook squares [white O-O, white O-O-O, black
 * O-O, black O-O-O] as squares, 64 = none):
 *   h = 0x9E3779B97F4A7C15; for w0..w7: h = (h ^ w) * 0xBF58476D1CE4E5B9, h ^= h >> 29;
 *   h = (h ^ h >> 27) * 0x94D049BB133111EB; h ^= h >> 31; key = h ? h : 1   (mod 2^64).
 * Equality of keys stands for equality of identity: 64 bits, as Stockfish's own repetition
 * test compares 64-bit keys.  The same value on the host and on the device.
 * Rule.  For position k of a game (positions 0..=moves, skipped ones included; history starts
 * at the root FEN, nothing before it is known) and a legal move m with child c: c is drawn by
 * rule when c is not checkmated and either c.rule50 >= 100 (Stockfish: rule50 > 99 && (!checkers
 * || a legal move exists)), or c's identity equals the identity of at least two of the game's
 * positions 0..=k -- the third occurrence; a second occurrence is not a draw.
 * Value, in this order of precedence: a checkmated child -VALUE_MATE and a child with no legal
 * move and not in check 0 with GN_FLAG_NO_MOVES (both as gn_line above, without GN_FLAG_DRAW);
 * a child drawn by rule V(c) = 0 with GN_FLAG_DRAW (and GN_FLAG_IN_CHECK if m gives check);
 * otherwise the static final_v.  value = negate_ply(V), score = rule_score(value, ...), order by
 * value descending, ties to the smaller move: all as gn_line.  A drawn line has value 0 and
 * score 0 and ties with a static 0 by the move encoding.
 * (The kernel tests only positions k + 1 - d for d = 4, 6, ... <= min(c.rule50, k + 1): a pawn
 * move or a capture lies between c and anything older.  The result is that of the rule above.)
 * A gn_history entry names a parent's game so far in a key array: keys[first..=self] are the
 * keys of the game's positions up to and including the parent (self).  first > self, or self
 * at or beyond the key count given with the array, means "no history": only the fifty-move part
 * applies.
 * Two plies deep (gn_rank_lines2_history_device, gn_evaluate_games_lines2_history) the same test,
 * against the same positions 0..=k, applies to the child and to each grandchild: the rule at
 * gn_line2 below.  For a grandchild g the kernel tests positions k + 2 - d for d = 4, 6, ... <=
 * min(g.rule50, k + 2). */
typedef struct gn_history {
  uint32_t first, self;
} gn_history;

/* One ranked two-ply line of a position: a two-move principal variation (fishnet's
 * pvs[multipv][depth] is a Vec<UciMove>, not a single move) with its minimax value.
 * gn_rank_lines2_device and gn_evaluate_lines2 return n_lines of them per position,
 * 1 <= n_lines <= GN_MAX_LINES.  A gn_line values a move by its child's static evaluation, also
 * where the child is in check, and cannot see that the move hangs a mate in one; a gn_line2
 * values it by the opponent's best reply.
 * The rule, for a position p a call evaluates (not bad) with at least one legal move, over every
 * legal move m with child c:
 *   V1(g) for a grandchild g is gn_line's V: -VALUE_MATE (-32000) when g has no legal move and is
 *   in check, 0 when g has no legal move and is not in check, g's static final_v in the call's
 *   mode otherwise;
 *   c has a legal move: R(c) = max over c's legal replies r (grandchild g) of negate_ply(V1(g)),
 *   ties to the smaller 16-bit move encoding; reply = that r, plies = 2.  This holds when c is in
 *   check too: c's own static value is never used;
 *   c has no legal move: R(c) = -VALUE_MATE when c is in check (m mates), 0 when it is not (m
 *   stalemates); reply = 0, plies = 1, GN_FLAG_NO_MOVES;
 *   value(m) = negate_ply(R(c)), score = rule_score(value, p's win-rate material): the same
 *   negate_ply and rule_score as everywhere else (gn_eval.score above).
 * Lines are ordered by value descending, ties to the smaller `move`.  Missing lines are empty,
 * (0, 0, 0, 0, GN_FLAG_NO_SCORE, 0); a bad, checkmated or stalemated position has only empty
 * lines.
 * Relation to gn_line: take the children as parents with their grandchildren's records; for a
 * child c with a legal move, (R(c), reply) is exactly line 1's (value, move) from
 * gn_rank_children_device.
 * Relation to gn_eval.score: none is claimed.  The score rule searches only positions that are in
 * check (and then only replies that give check); these lines search two plies everywhere.
 * With the game-history draws (gn_rank_lines2_history_device, gn_evaluate_games_lines2_history;
 * GN_FLAG_DRAW is valid on gn_line2.flags for these calls only).  Position k of a game has the
 * history of gn_history above: positions 0..=k, skipped ones included.  For a legal move m with
 * child c, in this order of precedence:
 *   1. c has no legal move: nothing changes.  R(c) = -VALUE_MATE when c is in check, else 0;
 *      reply = 0, plies = 1, GN_FLAG_NO_MOVES, no GN_FLAG_DRAW.
 *   2. c has a legal move and is drawn by rule -- c.rule50 >= 100, or c's identity equals that of
 *      at least two of positions 0..=k (the gn_history rule): R(c) = 0, reply = 0, plies = 1,
 *      GN_FLAG_DRAW, no GN_FLAG_NO_MOVES, GN_FLAG_IN_CHECK if m gives check.  c's grandchildren are
 *      not consulted: Stockfish returns the draw at that node without searching it.
 *   3. otherwise, for each reply r with grandchild g: g has no legal move: V1(g) = -VALUE_MATE when
 *      g is in check, else 0, as above; else g drawn by rule -- g.rule50 >= 100, or g's identity
 *      equals that of at least two of positions 0..=k (c has the other side to move and can never
 *      equal g): V1(g) = 0; else V1(g) = g's static final_v.  R(c) = max negate_ply(V1(g)), ties to
 *      the smaller reply encoding, plies = 2, and GN_FLAG_DRAW exactly when the chosen reply's
 *      grandchild is drawn by rule.  A drawn reply ties with a static 0 by the reply encoding alone.
 * value = negate_ply(R(c)), score, the order, the tie rule and the empty lines are unchanged.  A
 * drawn line has value 0 and score 0; plies tells the two kinds apart (1: the move's child is the
 * draw; 2: the best reply reaches it).
 * Why "third occurrence" is the whole rule at ply 2 as well: Stockfish's is_draw(ply) also draws a
 * single repetition that lies strictly after the root.  Two positions with the same side to move
 * and equal identity are at least 4 plies apart, so at ply 1 or 2 the earlier occurrence always
 * lies at or before the root, and the threefold test is all there is. */
typedef struct gn_line2 { /* 16 bytes */
  int32_t value;  /* minimax value after two plies, p's side-to-move POV, Stockfish units  */
  int32_t score;  /* rule_score(value, p's win-rate material): cp, or the mate distance with
                     GN_FLAG_MATE                                                          */
  uint16_t move;  /* p's move (Stockfish encoding, castling = king takes rook)             */
  uint16_t reply; /* the opponent's best reply to it; 0 when the move ends the game        */
  uint16_t flags; /* GN_FLAG_MATE; GN_FLAG_IN_CHECK: the move gives check; GN_FLAG_NO_MOVES:
                     the move ends the game; GN_FLAG_NO_SCORE: an empty line; GN_FLAG_DRAW:
                     the history calls only; GN_FLAG_SEARCHED: the check-extended calls only
                     (at gn_line): the chosen reply's grandchild was extended              */
  uint16_t plies; /* moves in the PV: 2, or 1 when the move ends the game (or, in the history
                     calls, reaches a position drawn by rule), 0 for an empty line         */
} gn_line2;

/* One ranked three-ply line of a position: p's move, the opponent's best reply and p's side's best
 * answer to it, with the minimax value after three plies (fishnet's scores[multipv][depth] and
 * pvs[multipv][depth] at depth 3).  gn_evaluate_lines3, gn_evaluate_games_lines3 and
 * gn_rank_lines3_device return n_lines of them per position, 1 <= n_lines <= GN_MAX_LINES.  A gn_line2
 * ends with the opponent to move and nothing of p's side behind it: it cannot see a mate in two, nor
 * a quiet move that wins material a move later.  A three-ply line of p is a two-ply line of each child
 * of p, negated.
 * The leaf rule (the calls' `leaf` and `depth`) says how the positions after the third ply are valued:
 *   GN_LEAF_STATIC   as gn_rank_lines2_device values its leaves (the rule at gn_line2);  depth 0
 *   GN_LEAF_CHECKS   the check-extended rule (at gn_line, "check-extended");             depth 0
 *   GN_LEAF_QUIESCE  the quiescent rule at `depth` (at gn_line, "quiescent lines"), Qs instead of Q
 *                    when GN_OPT_QUIESCE_SEE is 1, read once when the call starts;       depth 1..
 *                    GN_MAX_QUIESCE_DEPTH3: 3 + depth <= GN_MAX_PV, the PV and its tail fit a gn_pv
 * The rule, for a position p a call evaluates (not bad, not skipped) with at least one legal move,
 * over every legal move m with child c, under the call's leaf rule:
 *   c has no legal move: R3(c) = -VALUE_MATE when c is in check (m mates), else 0 (m stalemates);
 *   reply = reply2 = 0, plies = 1, GN_FLAG_NO_MOVES;
 *   otherwise let L be line 1 of the two-ply ranking with c as the parent, under the same leaf rule
 *   and with no history: R3(c) = L.value, reply = L.move, reply2 = L.reply, plies = 1 + L.plies;
 *   GN_FLAG_NO_MOVES exactly when L carries it (the reply ends the game: plies == 2, reply2 == 0);
 *   GN_FLAG_SEARCHED exactly when L carries it;
 *   value(m) = negate_ply(R3(c)), score = rule_score(value, p's win-rate material), which sets
 *   GN_FLAG_MATE: the same negate_ply and rule_score as everywhere else.  GN_FLAG_IN_CHECK is set
 *   exactly when c is in check (m gives check).
 * Lines are ordered by value descending, ties to the smaller `move`; reply and reply2 inherit the
 * two-ply rule's ties.  Missing lines are empty, (0, 0, 0, 0, 0, GN_FLAG_NO_SCORE, 0, 0); a bad,
 * skipped, checkmated or stalemated position has only empty lines.  GN_FLAG_DRAW never appears in
 * these three calls: they know no game history ("game history" below is the form that does).
 * A line's PV (gn_pv): an empty line has len 0; otherwise [move, reply, reply2][:plies], followed by
 * PVQ(great-grandchild, depth) (PVQs under GN_OPT_QUIESCE_SEE) exactly when the leaf rule is
 * GN_LEAF_QUIESCE, plies == 3 and the line carries GN_FLAG_SEARCHED.  Equivalently: [move] + the gn_pv
 * of L.  The check extension's replies are not reported.
 * Consequences:
 *   - for a child c with a legal move, (R3(c), reply, reply2) is exactly line 1's (value, move, reply)
 *     of gn_evaluate_lines2 (or its _extended / _quiescent form, by the leaf rule) for c's FEN at
 *     n_lines = 1;
 *   - `mate 2` appears on a mate in two, and `mate -2` on its defender's side, at plies == 3;
 *   - a line that gets mated by the reply has plies == 2 and GN_FLAG_NO_MOVES (`mate -1`);
 *   - played out from p, the PV ends in a position whose own value -- -VALUE_MATE (mated), 0
 *     (stalemated) or its static final_v in the call's mode -- carried back by negate_ply once per
 *     move of the PV, is the line's value.
 * Game history (gn_evaluate_games_lines3_history, gn_rank_lines3_history_device; GN_FLAG_DRAW is valid
 * on gn_line3.flags for these calls only).  Position k of a game has the history of gn_history above:
 * positions 0..=k, skipped ones included; nothing before the root FEN is known.  A position x that is
 * the child, grandchild or great-grandchild of position k is drawn by rule when it has a legal move
 * and x.rule50 >= 100 or x's identity equals that of at least two of positions 0..=k.  For a legal
 * move m of position k with child c, in this order of precedence:
 *   1. c has no legal move: nothing changes (plies = 1, GN_FLAG_NO_MOVES, no GN_FLAG_DRAW).
 *   2. c is drawn by rule: R3(c) = 0, reply = reply2 = 0, plies = 1, GN_FLAG_DRAW, GN_FLAG_IN_CHECK if
 *      m gives check, no GN_FLAG_NO_MOVES and no GN_FLAG_SEARCHED.  c's two-ply line is not consulted
 *      (it is computed all the same, and dropped by the root step).
 *   3. otherwise let L be line 1 of the two-ply history ranking (the rule at gn_line2, "with the
 *      game-history draws") with c as the parent, under the call's leaf rule, where c's game so far is
 *      positions 0..=k followed by c: R3(c) = L.value, reply = L.move, reply2 = L.reply,
 *      plies = 1 + L.plies, and GN_FLAG_NO_MOVES, GN_FLAG_SEARCHED and GN_FLAG_DRAW exactly when L
 *      carries them.
 * A drawn line has value 0 and score 0; plies tells the three kinds apart (1: the child is the draw;
 * 2: the reply reaches it; 3: the answer reaches it).  Value, score, order, ties and empty lines are
 * unchanged, and so is the precedence inside the leaf (no legal move, then drawn by rule, then the leaf
 * rule's search, then static), which is the two-ply history rule's; the check extension and the
 * quiescence know no history inside their own trees.  PV: [move, reply, reply2][:plies]; the
 * quiescence's tail follows only when plies == 3 and the line carries GN_FLAG_SEARCHED, which a drawn
 * leaf never does.
 * Why "third occurrence against 0..=k" is the whole rule at ply 3 as well (extending the paragraph at
 * gn_line2): two positions of equal identity have the same side to move, and no pair of moves, one by
 * each side, restores a position, so equal positions are at least 4 plies apart; at ply <= 3 the
 * earlier occurrence therefore always lies at or before the root, Stockfish's "single repetition after
 * the root" cannot trigger, and neither c nor the grandchild g can be one of the occurrences that
 * count for a position below them.  For a grandchild the kernel tests positions k + 2 - d and for a
 * great-grandchild k + 3 - d, d = 4, 6, ... up to min(rule50, k + 2) and min(rule50, k + 3).
 * Consequences:
 *   (a) for a child c that has a legal move and is not drawn, (R3(c), reply, reply2) and L's flags are
 *       line 1 at position k + 1 of gn_evaluate_games_lines2_history (its _extended / _quiescent form
 *       with history = 1 when the leaf rule is not static) for the same game with m appended;
 *   (b) where nothing is drawn at any of the three levels, the lines are byte-equal to
 *       gn_evaluate_games_lines3's;
 *   (c) position_offsets, game_status and position_out are byte-equal to gn_evaluate_games_lines3's
 *       always. */
#define GN_LEAF_STATIC 0  /* leaves by their static records (gn_line2's plain rule)          */
#define GN_LEAF_CHECKS 1  /* leaves in check by the check extension (gn_line "check-extended") */
#define GN_LEAF_QUIESCE 2 /* searched leaves by Q(x, depth), or Qs under GN_OPT_QUIESCE_SEE   */
#define GN_MAX_QUIESCE_DEPTH3 (GN_MAX_PV - 3) /* 3: a three-ply PV plus its tail fits a gn_pv */
typedef struct gn_line3 { /* 20 bytes */
  int32_t value;     /* minimax value after three plies, p's side-to-move POV, Stockfish units  */
  int32_t score;     /* rule_score(value, p's win-rate material): cp, or the mate distance with
                        GN_FLAG_MATE                                                            */
  uint16_t move;     /* p's move (Stockfish encoding, castling = king takes rook)               */
  uint16_t reply;    /* the opponent's best reply; 0 when plies == 1                            */
  uint16_t reply2;   /* p's side's best answer to it; 0 when plies <= 2                         */
  uint16_t flags;    /* GN_FLAG_MATE; GN_FLAG_IN_CHECK: the move gives check; GN_FLAG_NO_MOVES: the
                        move or the reply ends the game; GN_FLAG_SEARCHED: the leaf was valued by
                        the leaf rule's search; GN_FLAG_NO_SCORE: an empty line; GN_FLAG_DRAW: the
                        history calls only                                                      */
  uint16_t plies;    /* 3; 2 or 1 when the game ends earlier (or, in the history calls, reaches a
                        position drawn by rule); 0 for an empty line                            */
  uint16_t reserved; /* 0 */
} gn_line3;

/* Packed position, 32 bytes, the device input format.
 *   occ      occupied squares (bit s = square s, a1 = 0 .. h8 = 63)
 *   pc       piece codes (Stockfish encoding: 1..6 white P N B R Q K, 9..14 black)
 *            of the occupied squares in ascending square order, two per byte,
 *            low nibble first
 *   stm_ep   bit 7 = side to move (1 = black); bits 0..6 = en-passant square
 *            or 64 when none
 *   castle   4 nibbles [white O-O, white O-O-O, black O-O, black O-O-O]:
 *            bit 3 = right present, bits 0..2 = file of the castling rook
 *   rule50   half-move clock; fullmove = full-move number
 *
 * A board a caller makes itself (gn_evaluate_device, gn_expand_device,
 * gn_expand2_device, gn_rank_children_device, gn_time_*, gn_board_to_fen) behaves
 * exactly like the FEN text that spells its fields without validating them --
 * castling rights as Shredder file letters, the en-passant field as its square
 * name, rule50 and fullmove as numbers -- handed to gn_evaluate_batch /
 * gn_expand_and_evaluate.  One gate decides this on the host and on the device
 * (position_ok, fishnet_amd/csrc/chess.h).
 * Rejected: the record is exactly (0, 0, 0, 0, 0, GN_FLAG_BAD_FEN |
 * GN_FLAG_NO_SCORE, 0), the position has no children, only empty lines and no
 * grandchildren, gn_board_to_fen fails with GN_E_INVALID and gn_boards_to_fens
 * writes "":
 *   - popcount(occ) < 2 or > 32;
 *   - a piece nibble of an occupied square whose type is 0 or 7 (0, 7, 8, 15);
 *   - not exactly one king per colour;
 *   - a pawn on rank 1 or rank 8;
 *   - stm_ep & 0x7F above 64;
 *   - the side not to move is in check.
 * Normalised, then valid (every result is that of the canonical board):
 *   - `reserved` and the nibbles beyond popcount(occ) are ignored;
 *   - the low bits of a castle nibble are ignored when bit 3 is clear;
 *   - a castling right is dropped unless an own rook stands on that square of the
 *     own back rank, the own king stands on that rank, and the rook is on the
 *     king's right for slots 0 / 2, on its left for slots 1 / 3 (a text spells a
 *     right by its file alone; a right in the other side's slot has no spelling);
 *   - the en-passant square is none unless it is on rank 6 (white to move) or
 *     rank 3 (black to move), a pawn of the side to move attacks it, an enemy
 *     pawn stands behind it, and it and the square before it are empty;
 *   - rule50 and fullmove are taken as they are, any 16-bit value: rule50 enters
 *     the evaluation, fullmove 0 is valid (a FEN text's 0 reads as 1).
 * Boards the library writes (children, gn_pack_fens, gn_random_*) are canonical:
 * reserved = 0, unused nibbles 0, no right or en-passant square the gate drops. */
typedef struct gn_board {
  uint64_t occ;
  uint8_t pc[16];
  uint8_t stm_ep;
  uint8_t reserved;
  uint16_t castle;
  uint16_t rule50;
  uint16_t fullmove;
} gn_board;

/* Eval::evaluate constants (defaults = Stockfish 17.1). */
typedef struct gn_eval_params {
  int32_t small_net_threshold; /* 962   |simple_eval| above which the small net is used */
  int32_t psqt_weight;         /* 125   nnue = (psqt_w*psqt + pos_w*positional) / 128  */
  int32_t positional_weight;   /* 131                                                */
  int32_t reeval_threshold;    /* 236   small-net |nnue| below which big re-evaluates */
  int32_t complexity_div_small;/* 18000 nnue -= nnue * |psqt - positional| / div      */
  int32_t complexity_div_big;  /* 18000                                              */
  int32_t material_pawn_small; /* 535   material = k * pawns + non_pawn_material     */
  int32_t material_pawn_big;   /* 535                                                */
  int32_t material_base;       /* 77777 v = nnue * (base + material) / base          */
  int32_t rule50_div;          /* 212   v -= v * rule50 / div                        */
  int32_t value_clamp;         /* 31506 |v| <= VALUE_TB_WIN_IN_MAX_PLY - 1           */
  int32_t piece_value[5];      /* 208 781 825 1276 2538 (P N B R Q)                  */
  /* UCIEngine::to_cp / win_rate_params (Stockfish 17-era uci.cpp; recalled, parity
   * unpinned like the constants above):
   *   material = sum wdl_piece_weight[pt] * count(pt) over both colours (P N B R Q)
   *   m = clamp(material, wdl_material_min, wdl_material_max) / (double)wdl_material_anchor
   *   a = ((wdl_a[0] * m + wdl_a[1]) * m + wdl_a[2]) * m + wdl_a[3]   (no FMA contraction)
   *   final_cp = round(100 * final_v / a)                             (half away from zero) */
  double wdl_a[4];             /* -37.45051876 121.19101539 -132.78783573 420.70576692 */
  int32_t wdl_material_min;    /* 17 */
  int32_t wdl_material_max;    /* 78 */
  int32_t wdl_material_anchor; /* 58 */
  int32_t wdl_piece_weight[5]; /* 1 3 3 5 9 */
} gn_eval_params;

typedef struct gn_ctx gn_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
/* Load nets and upload them to each listed device (devices = NULL: device 0).
 * small_path may be NULL (then only GN_MODE_BIG works); big_path may be NULL
 * (then only GN_MODE_SMALL works).  A net wider than 128 in the small slot is
 * evaluated (gn_evaluate_*; mode FULL's selection then runs as launches of its
 * own and the small-batch graphs are not used); the expansion calls support it
 * in GN_MODE_BIG only. */
GN_API int gn_load_net(const char *big_path, const char *small_path, const int *devices, int n_devices,
                gn_ctx **out);
/* A file named like Stockfish's nets, "nn-" + 12 lowercase hex digits + ".nnue"
 * (build.rs:8-9), must hash to its name: the first 12 hex digits of its SHA-256
 * (the check Stockfish's `make net` does after download, build.rs:318-333);
 * otherwise gn_load_net fails with GN_E_FORMAT.  Other file names are not checked. */
/* Same from in-memory .nnue images (e.g. after an RCCL broadcast). */
GN_API int gn_load_net_memory(const uint8_t *big, size_t big_len, const uint8_t *small, size_t small_len,
                       const int *devices, int n_devices, gn_ctx **out);
/* Nets from fishnet's asset archive (assets.ar.zst: a zstd-compressed `ar` archive, as
 * /root/reference/build.rs:398-420 writes it and src/assets.rs:186-226 reads it; a plain
 * `ar` works too).  big_member / small_member: member names (e.g. "nn-1c0000000000.nnue"),
 * or NULL for the first .nnue member of that kind (big: L1 3072 / 1024; small: 128).
 * Members named nn-<hex>.nnue are checked against their SHA-256 prefix.  zstd is
 * decoded by the system's libzstd.so.1, opened at run time. */
GN_API int gn_load_net_archive(const char *archive_path, const char *big_member, const char *small_member,
                               const int *devices, int n_devices, gn_ctx **out);
/* One member's bytes (CPU only): GN_E_CAPACITY with *size set when cap is too small. */
GN_API int gn_archive_read(const char *archive_path, const char *member, uint8_t *buf, size_t cap, size_t *size);
GN_API void gn_free(gn_ctx *ctx);
GN_API const char *gn_last_error(void); /* thread-local; valid until the next call */
GN_API int gn_abi_version(void);
GN_API int gn_get_eval_params(const gn_ctx *ctx, gn_eval_params *out);
GN_API int gn_set_eval_params(gn_ctx *ctx, const gn_eval_params *params);
GN_API int gn_set_option(gn_ctx *ctx, int option, int64_t value);
GN_API int gn_get_option(const gn_ctx *ctx, int option, int64_t *value);
/* SHA-256 of a buffer as 64 lowercase hex digits + NUL (net provenance; host only). */
GN_API int gn_net_sha256(const uint8_t *data, size_t len, char *hex65);
/* network hashes / widths actually loaded (0 when absent) */
GN_API int gn_net_info(const gn_ctx *ctx, int *big_l1, uint32_t *big_hash, int *small_l1, uint32_t *small_hash);

/* ---- host-buffer API (what the Rust gpu_nnue module calls) -------------- */
/* Evaluate n FENs (Chess960 castling accepted: KQkq, Shredder and X-FEN).
 * gn_evaluate_batch == gn_evaluate_batch_mode(..., GN_MODE_FULL, ...).
 * Bad FENs do not fail the batch: their entry carries GN_FLAG_BAD_FEN. */
GN_API int gn_evaluate_batch(gn_ctx *ctx, const char *const *fens, size_t n, gn_eval *out);
GN_API int gn_evaluate_batch_mode(gn_ctx *ctx, const char *const *fens, size_t n, int mode, gn_eval *out);

/* Every parent plus every legal child of it, sharded over every device of the
 * context (gn_partition, one host thread per device).  child_offsets[n+1] receives the
 * prefix sums (children of parent i are [child_offsets[i], child_offsets[i+1])),
 * child_moves / child_out receive one entry per child in the order the device
 * generator emits them (moves in Stockfish 16-bit encoding; castling = king
 * takes own rook; records as gn_child).  GN_E_CAPACITY when the children exceed cap
 * (child_offsets is still filled so the caller can retry with the right size). */
GN_API int gn_expand_and_evaluate(gn_ctx *ctx, const char *const *parent_fens, size_t n, int mode,
                           gn_eval *parent_out, uint32_t *child_offsets, uint16_t *child_moves,
                           gn_child *child_out, size_t cap);

/* ---- lichess analysis batches ------------------------------------------ */
/* One acquired batch as the server sends it (AcquireResponseBody,
 * /root/reference/src/api.rs:306-321): the root FEN, the game's UCI moves as
 * one whitespace-separated string (the wire form; NULL or "" = no moves) and
 * skipPositions (indices into positions 0..=moves). */
typedef struct gn_game {
  const char *root_fen;
  const char *uci_moves;
  const uint32_t *skip_positions;
  size_t n_skip;
} gn_game;

/* Replaces IncomingBatch::from_acquired (/root/reference/src/queue.rs:548-700)
 * for the evaluator: position i = root after i moves, i = 0..=moves.  Moves are
 * resolved as shakmaty 0.27.3's UciMove::to_move does (queue.rs:576): king onto
 * a castling rook = castling (Chess960 form), e1g1/e1c1-style king moves =
 * castling with the h/a rook (standard form), promotion letter n/b/r/q.  moves[]
 * receives them in Stockfish encoding (castling = king takes rook, i.e. the
 * Chess960 UCI the reference forwards, queue.rs:577).  A bad root FEN fails with
 * GN_E_INVALID, a move that is not legal with GN_E_ILLEGAL_MOVE (the reference
 * fails the whole batch, `uci.to_move(&pos)?`).  *n_positions = moves + 1 is set
 * on GN_E_CAPACITY too.  Host only, no context and no GPU needed. */
GN_API int gn_replay_game(const gn_game *game, gn_board *positions, uint8_t *skipped, uint16_t *moves, size_t cap,
                          size_t *n_positions);

/* Replay + evaluate n_games batches at once.  position_offsets[n_games + 1]:
 * positions of game g are [position_offsets[g], position_offsets[g + 1]);
 * game_status[g] = GN_OK or that game's GN_E_* (a failed game has no positions;
 * the other games are still evaluated and the call returns GN_OK).  Games are
 * sharded over the devices of the context, never split (gn_partition weighted by
 * evaluated positions), so a game's consecutive positions share a device.  Skipped
 * positions get GN_FLAG_SKIPPED and no children.  with_children != 0: also every
 * legal child of every evaluated position, child_offsets[total positions + 1]
 * indexed by position (as gn_expand_and_evaluate).  GN_E_CAPACITY when the
 * positions exceed position_cap or the children child_cap, so that the caller can
 * retry with the right sizes: position_offsets and game_status are filled in both
 * cases.  The positions are checked first, before anything is evaluated or counted:
 * when they exceed position_cap, child_offsets is not written at all (nor is any
 * other output array), so a caller sizes the positions first
 * (position_offsets[n_games]) and then, with position_cap large enough, the children:
 * when only the children exceed child_cap, child_offsets is completely filled
 * (child_offsets[total positions] = the children needed).  What the record, move
 * and child arrays hold after GN_E_CAPACITY is unspecified; nothing is ever written
 * beyond the capacities given. */
GN_API int gn_evaluate_games(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int with_children,
                             uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                             size_t position_cap, uint32_t *child_offsets, uint16_t *child_moves,
                             gn_child *child_out, size_t child_cap);

/* gn_evaluate_games with children, except for what it downloads: instead of every legal child,
 * lines[position * n_lines + k] = line k + 1 of each position (gn_line; position_cap * n_lines
 * entries), ranked on the device as each chunk of the expansion finishes (rank_children_kernel
 * where the children would be packed for the host; the drain thread copies positions x n_lines
 * lines).  Same chunking (GN_OPT_CHUNK_PARENTS), two-slot overlap and sharding; position_offsets,
 * game_status, position_out and GN_E_CAPACITY for the positions exactly as gn_evaluate_games.
 * n_lines outside 1..GN_MAX_LINES: GN_E_INVALID.  GN_STAT_RANK_NS: the ranking's time. */
GN_API int gn_evaluate_games_lines(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                   uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                                   size_t position_cap, gn_line *lines);

/* gn_evaluate_games_lines with the game-history draws (gn_history above): each game's positions
 * 0..=k, skipped ones included, are position k's history.  Arguments, GN_E_CAPACITY behaviour,
 * chunking, two-slot overlap and sharding as gn_evaluate_games_lines; position_offsets,
 * game_status and position_out are byte-equal to its; the lines follow the rule at gn_history,
 * and equal gn_evaluate_games_lines' wherever no legal move of the position is drawn by rule.
 * The keys of every replayed position are made on the device once per shard
 * (GN_STAT_KEYS_NS); GN_STAT_RANK_NS: the ranking's time. */
GN_API int gn_evaluate_games_lines_history(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                           uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                                           size_t position_cap, gn_line *lines);

/* gn_evaluate_games_lines with two-ply lines (gn_line2) instead: the same front (the games
 * prepared, replayed on the device, sharded by game; position_offsets, game_status, position_out
 * and GN_E_CAPACITY for the positions exactly as gn_evaluate_games), then each shard's evaluated
 * positions through gn_evaluate_lines2's chunk loop: chunks of exactly GN_OPT_CHUNK_PARENTS
 * parents (0: 1,024), one download per chunk.  lines[position * n_lines + k] = line k + 1 of each
 * position, equal to gn_evaluate_lines2's for the position's FEN; a skipped position has only
 * empty lines, a failed game no positions.  n_lines outside 1..GN_MAX_LINES: GN_E_INVALID.
 * GN_STAT_HOST_* and GN_STAT_RANK2_NS: the call's stage times. */
GN_API int gn_evaluate_games_lines2(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                    uint32_t *position_offsets, int32_t *game_status, gn_eval *position_out,
                                    size_t position_cap, gn_line2 *lines);

/* gn_evaluate_games_lines2 with the game-history draws at both levels (the rule at gn_line2): each
 * game's positions 0..=k, skipped ones included, are position k's history.  position_offsets,
 * game_status and position_out are byte-equal to gn_evaluate_games_lines2's, and so are the lines
 * wherever the rule draws nothing at either level.  The keys of every replayed position are made
 * on the device once per shard (GN_STAT_KEYS_NS), so the chunks need no cut at game starts;
 * GN_STAT_RANK2_NS: the ranking's time. */
GN_API int gn_evaluate_games_lines2_history(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                            uint32_t *position_offsets, int32_t *game_status,
                                            gn_eval *position_out, size_t position_cap, gn_line2 *lines);

/* Two-ply ranked lines from FENs: out[i] = position i's record (byte-equal to
 * gn_expand_and_evaluate's parent_out for the same FENs and mode), lines[i * n_lines + k] = line
 * k + 1 of position i (gn_line2).  The FENs are sharded equally over the context's devices; each
 * shard runs in chunks of GN_OPT_CHUNK_PARENTS parents (0: 1,024): the depth-2 expansion into
 * library-owned buffers, rank_lines2_kernel, one download of the chunk's records and lines
 * (24 + 16 * n_lines bytes per position; no child or grandchild reaches the host).  A bad FEN
 * gets the GN_FLAG_BAD_FEN record and empty lines; the call still returns GN_OK.  Results are
 * identical for every chunk size and device count.  n_lines outside 1..GN_MAX_LINES:
 * GN_E_INVALID.  GN_STAT_HOST_* and GN_STAT_RANK2_NS: the call's stage times. */
GN_API int gn_evaluate_lines2(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines,
                              gn_eval *out, gn_line2 *lines); /* lines[n * n_lines] */

/* gn_evaluate_lines2 with check-extended leaves (the rule at gn_line, "check-extended"): after each
 * chunk's depth-2 expansion the grandchildren in check are extended on the device, then ranked.
 * out is byte-equal to gn_evaluate_lines2's, and so are the lines of every position none of whose
 * grandchildren is in check with a legal move.  Results are identical for every chunk size and
 * device count.  GN_STAT_EXTEND_NS / GN_STAT_EXTENDED_LEAVES: the extension's time and count. */
GN_API int gn_evaluate_lines2_extended(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines,
                                       gn_eval *out, gn_line2 *lines); /* lines[n * n_lines] */
/* gn_evaluate_games_lines2 (history == 0) or gn_evaluate_games_lines2_history (history != 0) with
 * check-extended leaves.  position_offsets, game_status, position_out and the GN_E_CAPACITY
 * behaviour are byte-equal to those calls'. */
GN_API int gn_evaluate_games_lines2_extended(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                             int history, uint32_t *position_offsets, int32_t *game_status,
                                             gn_eval *position_out, size_t position_cap, gn_line2 *lines);
/* gn_evaluate_games_lines (history == 0) or gn_evaluate_games_lines_history (history != 0) with
 * check-extended leaves: each chunk's children in check are extended before the ranking.  This
 * call runs its chunks one after another, as GN_OPT_EXPAND_PIPELINE 0 does (the extension is a
 * blocking multi-launch stage on per-device buffers); the drain thread, the slots and the chunking
 * are gn_evaluate_games_lines'.  position_offsets, game_status, position_out and the
 * GN_E_CAPACITY behaviour are byte-equal to those calls'; results are identical for every
 * GN_OPT_CHUNK_PARENTS, GN_OPT_EXPAND_PIPELINE and device count. */
GN_API int gn_evaluate_games_lines_extended(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                            int history, uint32_t *position_offsets, int32_t *game_status,
                                            gn_eval *position_out, size_t position_cap, gn_line *lines);

/* The three calls above with quiescent leaves (the rule at gn_line, "quiescent") instead of
 * check-extended ones: the same drivers, the leaves valued by the capture quiescence to `depth`
 * (1..GN_MAX_QUIESCE_DEPTH, else GN_E_INVALID) after each chunk's expansion; the check extension
 * does not run.  out / position_offsets, game_status, position_out and the GN_E_CAPACITY behaviour
 * are byte-equal to the plain calls', and so are the lines of every position none of whose leaves is
 * searched.  The one-ply games call runs its chunks one after another, as
 * gn_evaluate_games_lines_extended does.  Results are identical for every GN_OPT_CHUNK_PARENTS,
 * GN_OPT_EXPAND_PIPELINE and device count.  The quiescence's levels live in device memory sized
 * from their counts: a level of 2^31 nodes or more fails the call with GN_E_CAPACITY, a failed
 * device allocation of the stage (its levels, its scans and its evaluations alike) with GN_E_NOMEM
 * after the stage's buffers are given back; the message names GN_OPT_CHUNK_PARENTS and depth, the
 * two handles on the size, and the context stays usable.  GN_STAT_QUIESCE_NS / GN_STAT_QUIESCE_LEAVES /
 * GN_STAT_QUIESCE_NODES: the quiescence's time, searched leaves and evaluated nodes. */
GN_API int gn_evaluate_lines2_quiescent(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines,
                                        int depth, gn_eval *out, gn_line2 *lines); /* lines[n * n_lines] */
GN_API int gn_evaluate_games_lines2_quiescent(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                              int history, int depth, uint32_t *position_offsets, int32_t *game_status,
                                              gn_eval *position_out, size_t position_cap, gn_line2 *lines);
GN_API int gn_evaluate_games_lines_quiescent(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                             int history, int depth, uint32_t *position_offsets, int32_t *game_status,
                                             gn_eval *position_out, size_t position_cap, gn_line *lines);

/* The three quiescent calls above with the lines' whole variations (gn_pv): the same arguments, plus
 * pvs[positions * n_lines] as the last; pvs[position * n_lines + k] belongs to
 * lines[position * n_lines + k].  Every other output is byte-equal to the quiescent call's; skipped,
 * bad and failed positions have len 0.  pvs == NULL: GN_E_INVALID.  The PVs are identical for every
 * GN_OPT_CHUNK_PARENTS, GN_OPT_EXPAND_PIPELINE and device count.  With PVs each level of the
 * quiescence keeps its moves and its chosen children (6 bytes per node more), and 16 * n_lines bytes
 * more per position are downloaded.  GN_STAT_PV_NS: the PV kernels' time. */
GN_API int gn_evaluate_lines2_quiescent_pv(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines,
                                           int depth, gn_eval *out, gn_line2 *lines, gn_pv *pvs);
GN_API int gn_evaluate_games_lines2_quiescent_pv(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode,
                                                 int n_lines, int history, int depth, uint32_t *position_offsets,
                                                 int32_t *game_status, gn_eval *position_out, size_t position_cap,
                                                 gn_line2 *lines, gn_pv *pvs);
GN_API int gn_evaluate_games_lines_quiescent_pv(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode,
                                                int n_lines, int history, int depth, uint32_t *position_offsets,
                                                int32_t *game_status, gn_eval *position_out, size_t position_cap,
                                                gn_line *lines, gn_pv *pvs);

/* Three-ply ranked lines (the rule at gn_line3): lines[i * n_lines + k] = line k + 1 of position i,
 * pvs[i * n_lines + k] its gn_pv (pvs NULL: no PVs are made or downloaded); out as
 * gn_evaluate_lines2's, byte for byte.  leaf is GN_LEAF_STATIC, GN_LEAF_CHECKS or GN_LEAF_QUIESCE;
 * depth is 1..GN_MAX_QUIESCE_DEPTH3 with GN_LEAF_QUIESCE and 0 otherwise.  The FENs are sharded
 * equally over the devices; each device runs its roots in chunks of exactly GN_OPT_CHUNK_PARENTS (0:
 * 1,024): the chunk's depth-1 expansion into library-owned buffers, then its children as parents
 * through gn_evaluate_lines2's chunk computation at n_lines = 1 under the leaf rule -- in chunks of
 * the same number of children, cut wherever they fall, also inside one root's children -- their line
 * 1 (and its gn_pv) staying on the device, then rank_lines3_kernel, then one download of the chunk's
 * records, 20 * n_lines bytes of lines and, with pvs, 16 * n_lines bytes of PVs per position.  Results
 * are identical for every chunk size, GN_OPT_EXPAND_PIPELINE and device count.  GN_E_INVALID: n_lines
 * outside 1..GN_MAX_LINES, leaf outside 0..2, a depth the leaf rule does not take, NULL lines with
 * n > 0.  GN_E_NOMEM / GN_E_CAPACITY from the quiescence as for gn_evaluate_lines2_quiescent: the
 * context stays usable.  GN_STAT_RANK3_NS: the root kernel's time; the stages below it feed the
 * two-ply calls' statistics. */
GN_API int gn_evaluate_lines3(gn_ctx *ctx, const char *const *fens, size_t n, int mode, int n_lines, int leaf,
                              int depth, gn_eval *out, gn_line3 *lines, gn_pv *pvs);
/* The same from games: the front (replay, position_offsets, game_status, position_out,
 * GN_E_CAPACITY) exactly as gn_evaluate_games_lines2, byte for byte; n_lines lines per position, equal
 * to gn_evaluate_lines3's for the position's FEN.  The call knows no game history.  A skipped position
 * has only empty lines (and PVs of len 0), a failed game no positions. */
GN_API int gn_evaluate_games_lines3(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                    int leaf, int depth, uint32_t *position_offsets, int32_t *game_status,
                                    gn_eval *position_out, size_t position_cap, gn_line3 *lines, gn_pv *pvs);
/* gn_evaluate_games_lines3 with the game-history draws at the child, the reply and the answer (the
 * rule at gn_line3, "game history"): the same arguments, errors and front, byte for byte.  The keys of
 * the replayed positions are computed on the device once per shard (GN_STAT_KEYS_NS), as for
 * gn_evaluate_games_lines2_history; per chunk the roots' gn_history entries are spread to their
 * children, which run through the two-ply history ranking one ply ahead of the game, and the root step
 * is rank_lines3_kernel's history variant (GN_STAT_RANK3_NS); the spreading kernel's time is counted
 * in no stage statistic, only in GN_STAT_HOST_TOTAL_NS.  A drawn child's two-ply line is computed and
 * then dropped.  Results are identical for every chunk size, GN_OPT_EXPAND_PIPELINE and
 * device count. */
GN_API int gn_evaluate_games_lines3_history(gn_ctx *ctx, const gn_game *games, size_t n_games, int mode, int n_lines,
                                            int leaf, int depth, uint32_t *position_offsets, int32_t *game_status,
                                            gn_eval *position_out, size_t position_cap, gn_line3 *lines,
                                            gn_pv *pvs);

/* The partitioner the library uses to shard work over the devices of a context and
 * that multi-process callers use to shard over ranks: contiguous ranges of n_items
 * items, bounds[k] = first item of shard k, bounds[n_shards] = n_items; shard k
 * starts at the first item whose weight prefix reaches ceil(k * total / n_shards)
 * (weights NULL: every item weighs 1).  gn_evaluate_games shards games weighted
 * by evaluated positions; gn_expand_and_evaluate / gn_evaluate_batch shard parents /
 * positions equally.  Host only. */
GN_API int gn_partition(const uint32_t *weights, size_t n_items, int n_shards, size_t *bounds);

/* Legal-move-tree node count from fen to depth (GPU movegen, breadth-first). */
GN_API int gn_perft(gn_ctx *ctx, const char *fen, int depth, uint64_t *nodes);

/* ---- packed / device-resident API (benchmarks, multi-GPU shards) -------- */
/* Host FEN -> packed board; ok[i] = 0 marks a bad FEN (its board is zeroed).
 * Needs no context and no GPU. */
GN_API int gn_pack_fens(const char *const *fens, size_t n, gn_board *out, uint8_t *ok);
/* Packed board -> FEN text (Chess960-aware X-FEN castling); buf >= 100 bytes. */
GN_API int gn_board_to_fen(const gn_board *board, char *buf, size_t buflen);
/* n boards -> n NUL-terminated FENs at buf + i * stride (stride >= 100); an invalid
 * board gives "".  Host only, multithreaded. */
GN_API int gn_boards_to_fens(const gn_board *boards, size_t n, char *buf, size_t stride);
/* keys[i] = the position key of boards[i] (gn_history above); each board goes through the gate
 * of a caller's board, a rejected board's key is 0.  Host only, needs no context. */
GN_API int gn_position_keys(const gn_board *boards, size_t n, uint64_t *keys);
/* Deterministic random-playout positions (xoshiro256**, seed + index): plays
 * k ~ U{0..max_plies} uniformly random legal plies from the start position
 * (stopping at mate/stalemate), resampling positions in check. Host only. */
GN_API int gn_random_positions(uint64_t seed, size_t first_index, size_t n, int max_plies, gn_board *out);

/* Same generator on the GPU (identical boards for identical seeds): writes n
 * boards to device memory d_out; asynchronous on `stream` (NULL = context stream). */
GN_API int gn_random_positions_device(gn_ctx *ctx, int device_slot, uint64_t seed, size_t first_index, size_t n,
                                      int max_plies, gn_board *d_out, void *stream);

/* Evaluate boards already resident on device `device_slot` (index into the
 * devices given at load).  d_boards / d_out are device pointers; stream is a
 * hipStream_t (NULL = the context's own stream).  Blocking: the score rule reads the
 * number of in-check positions back to size its launches (so the call synchronises
 * `stream` while it runs and cannot be captured into a HIP graph), and the call returns
 * with `stream` idle and d_out written.  The other gn_*_device calls that evaluate
 * (gn_expand_device, gn_expand2_device, gn_time_*) block the same way;
 * gn_random_positions_device / gn_random_games_device are asynchronous. */
GN_API int gn_evaluate_device(gn_ctx *ctx, int device_slot, const gn_board *d_boards, size_t n, int mode,
                       gn_eval *d_out, void *stream);
/* Device-resident expansion: counts children (d_counts[n]), writes d_offsets
 * (n+1 prefix sums), the child boards, moves and evaluations.  Synchronous;
 * returns the total child count in *total. */
GN_API int gn_expand_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, int mode,
                     gn_eval *d_parent_out, uint32_t *d_offsets, gn_board *d_children,
                     uint16_t *d_moves, gn_eval *d_child_out, size_t cap, size_t *total, void *stream);
/* Ranks the outputs of a preceding gn_expand_device of the same parents (d_offsets, d_moves,
 * d_child_out as it wrote them): d_lines[i * n_lines + k] = line k + 1 of parent i (gn_line).
 * Asynchronous on `stream` (NULL = the context's own), no read-back.  n_lines outside
 * 1..GN_MAX_LINES: GN_E_INVALID. */
GN_API int gn_rank_children_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                   const uint32_t *d_offsets, const uint16_t *d_moves, const gn_eval *d_child_out,
                                   int n_lines, gn_line *d_lines, void *stream);
/* The same values as gn_position_keys for n device-resident boards, into d_keys[n]; one lane per
 * board.  Asynchronous on `stream` (NULL = the context's own). */
GN_API int gn_position_keys_device(gn_ctx *ctx, int device_slot, const gn_board *d_boards, size_t n,
                                   uint64_t *d_keys, void *stream);
/* gn_rank_children_device with the game-history draws (the rule at gn_history): d_hist[i] names
 * parent i's game so far in d_keys[0, n_keys).  An entry with first > self or self >= n_keys is
 * "no history" (the fifty-move part still applies); d_keys is never read at or beyond n_keys, and
 * may be NULL when n_keys is 0.  Asynchronous, no read-back.  n_lines outside 1..GN_MAX_LINES:
 * GN_E_INVALID. */
GN_API int gn_rank_children_history_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                           const uint32_t *d_offsets, const uint16_t *d_moves,
                                           const gn_eval *d_child_out, const uint64_t *d_keys, size_t n_keys,
                                           const gn_history *d_hist, int n_lines, gn_line *d_lines, void *stream);
/* Depth 2 (grandchildren): gn_expand_device, then every child's legal children
 * evaluated incrementally from the child's accumulator (a sibling block refreshes each
 * child from its predecessor through the king cache).  d_goffsets: total + 1 offsets of
 * each child's grandchildren in d_gmoves / d_grand_out (gcap entries); grandchild boards
 * are not returned.  GN_E_CAPACITY: *total / *gtotal hold the counts needed. */
GN_API int gn_expand2_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, int mode,
                             gn_eval *d_parent_out, uint32_t *d_offsets, gn_board *d_children, uint16_t *d_moves,
                             gn_eval *d_child_out, size_t cap, uint32_t *d_goffsets, uint16_t *d_gmoves,
                             gn_eval *d_grand_out, size_t gcap, size_t *total, size_t *gtotal, void *stream);
/* Ranks the outputs of a preceding gn_expand2_device of the same parents (d_offsets, d_children,
 * d_child_out, d_moves, d_goffsets, d_gmoves, d_grand_out as it wrote them): d_lines[i * n_lines + k]
 * = line k + 1 of parent i (gn_line2).  One launch (rank_lines2_kernel): nothing but 16 * n_lines
 * bytes per parent needs to leave the device.  Asynchronous on `stream` (NULL = the context's
 * own), no read-back.  n_lines outside 1..GN_MAX_LINES: GN_E_INVALID.  The child and grandchild
 * buffers may be NULL when no parent has a child. */
GN_API int gn_rank_lines2_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                 const uint32_t *d_offsets, const gn_board *d_children, const gn_eval *d_child_out,
                                 const uint16_t *d_moves, const uint32_t *d_goffsets, const uint16_t *d_gmoves,
                                 const gn_eval *d_grand_out, int n_lines, gn_line2 *d_lines, void *stream);
/* gn_rank_lines2_device with the game-history draws at both levels (the rule at gn_line2):
 * d_hist[i] names parent i's game so far in d_keys[0, n_keys), as for
 * gn_rank_children_history_device.  An entry with first > self or self >= n_keys is "no history"
 * (the fifty-move part still applies, at both levels); d_keys is never read at or beyond n_keys,
 * and may be NULL when n_keys is 0.  Asynchronous, no read-back.  n_lines outside
 * 1..GN_MAX_LINES: GN_E_INVALID. */
GN_API int gn_rank_lines2_history_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                         const uint32_t *d_offsets, const gn_board *d_children,
                                         const gn_eval *d_child_out, const uint16_t *d_moves,
                                         const uint32_t *d_goffsets, const uint16_t *d_gmoves,
                                         const gn_eval *d_grand_out, const uint64_t *d_keys, size_t n_keys,
                                         const gn_history *d_hist, int n_lines, gn_line2 *d_lines, void *stream);
/* The check extension of one expansion level (the rule at gn_line, "check-extended"): the leaves
 * are those a preceding gn_expand_device left on the device (d_parents, n, d_offsets, d_moves,
 * d_rec = d_child_out, total), or level 2 of gn_expand2_device with the children as parents
 * (d_children, total, d_goffsets, d_gmoves, d_grand_out, gtotal).  d_ext[j] (total entries) = E of
 * leaf j where it is in check with a legal move, GN_NOT_EXTENDED everywhere else (a mated leaf
 * included: the ranking values it); *extended = the number of extended leaves.  The leaves'
 * boards are made on the device and evaluated as positions by the path gn_evaluate_device runs, in
 * records the library owns: d_rec is only read.  Blocking, like gn_evaluate_device (its counts size
 * the next launches).  total == 0: GN_OK, nothing is read and the buffers may be NULL.
 * GN_E_NONET as elsewhere. */
GN_API int gn_extend_checks_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                   const uint32_t *d_offsets, const uint16_t *d_moves, const gn_eval *d_rec,
                                   size_t total, int mode, int32_t *d_ext, size_t *extended, void *stream);
/* The capture quiescence of one expansion level (the rule at gn_line, "quiescent"): inputs and
 * contract as gn_extend_checks_device -- one level of gn_expand_device, or level 2 of
 * gn_expand2_device with the children as parents.  d_ext[j] (total entries) = Q(leaf j, depth) where
 * leaf j is searched, GN_NOT_EXTENDED everywhere else (entries no parent's offsets cover included);
 * *searched = the number of searched leaves,
 * *nodes = the positions evaluated below them (the searched moves' children, level by level down
 * to depth).  There is no ranking call of its own: gn_rank_children_extended_device and
 * gn_rank_lines2_extended_device take this d_ext as they take the extension's.  d_rec is only read
 * (the leaves' statics).  Blocking.  total == 0: GN_OK, nothing is read and the buffers may be NULL.
 * depth outside 1..GN_MAX_QUIESCE_DEPTH: GN_E_INVALID.  GN_E_CAPACITY / GN_E_NOMEM as for the
 * host-buffer quiescent calls: the stream is idle on return and the context usable afterwards.
 * GN_E_NONET as elsewhere. */
GN_API int gn_quiesce_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                             const uint32_t *d_offsets, const uint16_t *d_moves, const gn_eval *d_rec, size_t total,
                             int mode, int depth, int32_t *d_ext, size_t *searched, size_t *nodes, void *stream);
/* gn_quiesce_device plus the searched leaves' own variations: d_tail[j * GN_MAX_QUIESCE_DEPTH + k]
 * (total * GN_MAX_QUIESCE_DEPTH entries) = move k of PVQ(leaf j, depth) (the rule at gn_line),
 * 0-terminated when shorter than GN_MAX_QUIESCE_DEPTH: move 0 is never legal.  All entries of an
 * unsearched leaf are 0, entries no parent's offsets cover included.  d_ext, *searched and *nodes are
 * byte-equal to gn_quiesce_device's.  Blocking; errors as gn_quiesce_device; d_tail == NULL with
 * total > 0: GN_E_INVALID. */
GN_API int gn_quiesce_pv_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                const uint32_t *d_offsets, const uint16_t *d_moves, const gn_eval *d_rec, size_t total,
                                int mode, int depth, int32_t *d_ext, uint16_t *d_tail, size_t *searched, size_t *nodes,
                                void *stream);
/* The exchange evaluation of a list of moves (the rule at gn_line, "exchange evaluation"), on the
 * host and without a context: out[i] = see(boards[i], moves[i]) with the values piece_value[0..4]
 * (P N B R Q; NULL: the defaults).  Each board goes through the gate; a rejected board, or a move
 * that is not legal there, gives GN_NOT_EXTENDED in out[i], and the call still returns GN_OK.
 * n == 0: GN_OK, the buffers may be NULL; a NULL buffer otherwise: GN_E_INVALID. */
GN_API int gn_see_moves(const gn_board *boards, size_t n, const uint16_t *moves, const int32_t *piece_value,
                        int32_t *out);
/* ... and of one expansion level on the device: inputs as gn_quiesce_device takes them (a preceding
 * gn_expand_device, or level 2 of gn_expand2_device with the children as parents).  d_see[j] (total
 * entries) = see(parent of j, d_moves[j]) with the context's piece values (gn_set_eval_params) for
 * every j a parent's offsets cover, GN_NOT_EXTENDED for every other j < total and for the moves of a
 * parent the gate rejects.  Offsets are clamped to total; the moves are taken as legal.  Asynchronous
 * on `stream` (NULL = the context's own), no read-back.  total == 0: GN_OK, the buffers may be NULL;
 * a NULL buffer with total > 0: GN_E_INVALID. */
GN_API int gn_see_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                         const uint32_t *d_offsets, const uint16_t *d_moves, size_t total, int32_t *d_see,
                         void *stream);
/* d_pvs[i * n_lines + k] = the gn_pv of d_lines[i * n_lines + k], the lines a ranking call wrote for
 * the same expansion (d_offsets, d_moves as gn_expand_device wrote them) and d_tail as
 * gn_quiesce_pv_device wrote it for the level the ranking took d_ext from; d_tail == NULL: no tails
 * (the lines' own moves only).  A line's leaf is found by its move; every range is clamped to
 * d_offsets[n], and a move that is not found gives the PV without a tail.  Asynchronous on `stream`
 * (NULL = the context's own), no read-back.  n_lines outside 1..GN_MAX_LINES: GN_E_INVALID. */
GN_API int gn_line_pvs_device(gn_ctx *ctx, int device_slot, size_t n, const uint32_t *d_offsets,
                              const uint16_t *d_moves, const uint16_t *d_tail, const gn_line *d_lines, int n_lines,
                              gn_pv *d_pvs, void *stream);
/* The same for two-ply lines: the expansion as gn_expand2_device wrote it, d_gtail as
 * gn_quiesce_pv_device wrote it for the grandchild level (NULL: no tails). */
GN_API int gn_line2_pvs_device(gn_ctx *ctx, int device_slot, size_t n, const uint32_t *d_offsets,
                               const uint16_t *d_moves, const uint32_t *d_goffsets, const uint16_t *d_gmoves,
                               const uint16_t *d_gtail, const gn_line2 *d_lines, int n_lines, gn_pv *d_pvs,
                               void *stream);
/* gn_rank_children_history_device with check-extended (or quiescent) leaves: d_ext as
 * gn_extend_checks_device (or gn_quiesce_device)
 * wrote it for the same expansion (NULL: nothing is extended).  d_hist == NULL selects no history
 * at all (not even the fifty-move part; d_keys / n_keys are then ignored): the plain rule plus the
 * extension.  Asynchronous, no read-back. */
GN_API int gn_rank_children_extended_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                            const uint32_t *d_offsets, const uint16_t *d_moves,
                                            const gn_eval *d_child_out, const uint64_t *d_keys, size_t n_keys,
                                            const gn_history *d_hist, const int32_t *d_ext, int n_lines,
                                            gn_line *d_lines, void *stream);
/* gn_rank_lines2_history_device with check-extended leaves: d_gext as gn_extend_checks_device wrote
 * it for the grandchild level (NULL: nothing is extended); d_hist == NULL: no history at all.
 * Asynchronous, no read-back. */
GN_API int gn_rank_lines2_extended_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                          const uint32_t *d_offsets, const gn_board *d_children,
                                          const gn_eval *d_child_out, const uint16_t *d_moves,
                                          const uint32_t *d_goffsets, const uint16_t *d_gmoves,
                                          const gn_eval *d_grand_out, const uint64_t *d_keys, size_t n_keys,
                                          const gn_history *d_hist, const int32_t *d_gext, int n_lines,
                                          gn_line2 *d_lines, void *stream);
/* gn_rank_lines2_extended_device with the history window `ahead` plies ahead of the game: parent i is
 * not the position at d_keys[d_hist[i].self] but lies `ahead` plies after it (ahead = 1: a child of
 * it, the three-ply chain's parents; the parent itself has no key in the array).  A child is then
 * tested against the len + ahead positions first..=self, being 1 + ahead plies after the newest, and a
 * grandchild likewise 2 + ahead plies after it; "no history" entries stay so.  No key at or beyond
 * n_keys or below first is read.  ahead = 0: byte-equal to gn_rank_lines2_extended_device; ahead
 * outside 0..1: GN_E_INVALID. */
GN_API int gn_rank_lines2_ahead_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                       const uint32_t *d_offsets, const gn_board *d_children,
                                       const gn_eval *d_child_out, const uint16_t *d_moves,
                                       const uint32_t *d_goffsets, const uint16_t *d_gmoves,
                                       const gn_eval *d_grand_out, const uint64_t *d_keys, size_t n_keys,
                                       const gn_history *d_hist, const int32_t *d_gext, int ahead, int n_lines,
                                       gn_line2 *d_lines, void *stream);
/* The root step of the three-ply lines alone (the rule at gn_line3): d_lines[i * n_lines + k] = line
 * k + 1 of parent i, from the root expansion as gn_expand_device wrote it (d_offsets, d_moves,
 * d_child_out: only the records' GN_FLAG_IN_CHECK is read) and d_child_lines[j] = line 1 of the
 * two-ply ranking with child j as the parent (gn_rank_lines2_device or a form of it at n_lines = 1
 * over the `total` children); an empty child line (GN_FLAG_NO_SCORE) is what "child j has no legal
 * move" means, and no move is generated here.  d_pvs (NULL: none) needs d_child_pvs, the gn_pv of
 * each child line (gn_line2_pvs_device): d_pvs[i * n_lines + k] = [move] + the child's PV.  Every
 * child range is clamped to total, and nothing at or beyond total is read; a range longer than 256
 * children (no position has more than 218 legal moves) is cut to its first 256.  One launch
 * (rank_lines3_kernel), asynchronous on `stream` (NULL = the context's own), no read-back.
 * n == 0: GN_OK, nothing is read or written; total == 0: GN_OK, no input buffer is read (they may
 * be NULL) and every line is empty.  GN_E_INVALID: n_lines outside 1..GN_MAX_LINES, a NULL buffer
 * that would be read or written, d_pvs without d_child_pvs. */
GN_API int gn_rank_lines3_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                 const uint32_t *d_offsets, const uint16_t *d_moves, const gn_eval *d_child_out,
                                 size_t total, const gn_line2 *d_child_lines, const gn_pv *d_child_pvs, int n_lines,
                                 gn_line3 *d_lines, gn_pv *d_pvs, void *stream);
/* gn_rank_lines3_device with the game-history draws at the child (the rule at gn_line3, "game
 * history"): d_children are the root expansion's child boards as gn_expand_device wrote them, and
 * d_hist[i] names parent i's game so far in d_keys[0, n_keys), as for gn_rank_lines2_history_device:
 * an entry with first > self or self >= n_keys is "no history" (the fifty-move part still applies),
 * d_keys is never read at or beyond n_keys and may be NULL when n_keys is 0.  A child whose line is
 * not empty and that is drawn by rule overrides its line (rule 2); a child line's GN_FLAG_DRAW passes
 * into the root's line, so d_child_lines are to come from gn_rank_lines2_ahead_device at ahead = 1
 * with each child's entry its parent's.  d_hist == NULL: no history at all, byte-equal to
 * gn_rank_lines3_device (d_children and d_keys are not read).  Otherwise as gn_rank_lines3_device;
 * d_children is one of the buffers that may be NULL only when total is 0. */
GN_API int gn_rank_lines3_history_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n,
                                         const uint32_t *d_offsets, const uint16_t *d_moves,
                                         const gn_eval *d_child_out, size_t total, const gn_line2 *d_child_lines,
                                         const gn_pv *d_child_pvs, const gn_board *d_children,
                                         const uint64_t *d_keys, size_t n_keys, const gn_history *d_hist,
                                         int n_lines, gn_line3 *d_lines, gn_pv *d_pvs, void *stream);
/* Time `iters` complete expansions of device-resident parents (child count +
 * scan + child generation with deltas + evaluation of parents and children in
 * `mode` + the parents' score rule).  Outputs go to the caller's device buffers when given (d_parent_out[n],
 * d_offsets[n + 1], d_moves[cap], d_child_out[cap]; GN_E_CAPACITY when the
 * children exceed cap), else to library-owned buffers; every iteration writes the
 * same values, so after the call they hold the timed expansion's results.
 * *total = children per expansion;
 * stage_ms (optional, length 8) = average ms of [count+scan, total read-back,
 * write children, classify, small net, big net, finalize, score rule]; ft_rows (optional)
 * = feature-transformer rows one incremental expansion gathers: for the big
 * nets the row stream's own count (bias, carry and king-cache rows included:
 * GN_OPT_CHAIN, GN_OPT_KING_CACHE), else parent refreshes + child deltas /
 * king-move refreshes; 0 when not incremental. */
GN_API int gn_time_expand_device(gn_ctx *ctx, int device_slot, const gn_board *d_parents, size_t n, int mode,
                                 int iters, float *ms_total, size_t *total, float *stage_ms, uint64_t *ft_rows,
                                 gn_eval *d_parent_out, uint32_t *d_offsets, uint16_t *d_moves,
                                 gn_eval *d_child_out, size_t cap);
/* *sum = position-sensitive 64-bit checksum of `bytes` bytes at device pointer d_ptr
 * (sum over 8-byte words w_i of splitmix64(w_i ^ i * 0x9E3779B97F4A7C15), wrapping):
 * compares large device-resident results without a download.  The words are
 * little-endian, word i at byte 8 * i; a tail of bytes % 8 bytes is zero-padded into a
 * last word; 0 bytes give 0.  splitmix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31.  d_ptr must be 8-byte aligned
 * (the kernel loads whole words): GN_E_INVALID otherwise, checked on the host before
 * anything is launched. */
GN_API int gn_checksum_device(gn_ctx *ctx, int device_slot, const void *d_ptr, size_t bytes, uint64_t *sum);
/* n_games random games of `plies` plies (xoshiro256**, seed + game index) on
 * the GPU: d_out[g * (plies + 1) + k] = position after k plies of game g (a
 * game that ends early repeats its final position).  Asynchronous. */
GN_API int gn_random_games_device(gn_ctx *ctx, int device_slot, uint64_t seed, size_t first_game, size_t n_games,
                                  int plies, gn_board *d_out, void *stream);
/* The UCI moves of the same games gn_random_games_device plays, as the lichess API sends a
 * game (AcquireResponseBody.moves: space-separated, standard castling notation e1g1): game g's
 * NUL-terminated string at buf + g * stride (stride >= 6 * plies + 1); a game that ended
 * (mate, stalemate, rule50) stops there.  Host only, multithreaded. */
GN_API int gn_random_games_uci(uint64_t seed, size_t first_game, size_t n_games, int plies, char *buf, size_t stride);
/* Device memory helpers (so callers need no HIP headers). */
GN_API int gn_device_alloc(gn_ctx *ctx, int device_slot, size_t bytes, void **ptr);
GN_API int gn_device_free(gn_ctx *ctx, int device_slot, void *ptr);
GN_API int gn_memcpy_h2d(gn_ctx *ctx, int device_slot, void *dst, const void *src, size_t bytes);
GN_API int gn_memcpy_d2h(gn_ctx *ctx, int device_slot, void *dst, const void *src, size_t bytes);
GN_API int gn_synchronize(gn_ctx *ctx, int device_slot);
/* Time `iters` back-to-back gn_evaluate_device calls with HIP events recorded
 * on the launch stream; *ms_total = elapsed time.  per_kernel_ms (optional,
 * length 4) receives the average per-call time of the [classify(+reeval),
 * small net, big net, finalize] stages, from events recorded between the
 * launches of that same timed pass (one host sync at the end).  ft_rows
 * (optional) = feature-transformer rows one call's gather reads (the big net's,
 * or the small net's in GN_MODE_SMALL), counted by the kernel. */
GN_API int gn_time_evaluate_device(gn_ctx *ctx, int device_slot, const gn_board *d_boards, size_t n, int mode,
                            gn_eval *d_out, int iters, float *ms_total, float *per_kernel_ms, uint64_t *ft_rows);

#ifdef __cplusplus
}
#endif
#endif
