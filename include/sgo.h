/*
 * sgo.h -- C ABI of libsgo_hip.so, the MI355X (gfx950) self-play hot path of sejonggo.
 *
 * The reference (drsagitn/sejonggo) is pure Python and has no FFI; its boundary for this path is a
 * set of Python module symbols.  This header is the C ABI placed underneath those
 * symbols: plain pointers and sizes, no torch types, `int` return 0 = ok / negative = error (text via
 * sgo_last_error()).  Each entry point cites the reference interface it replaces (file:line relative
 * to the reference repo).  INTEGRATION.md shows the ctypes binding a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   board17   int32 [n][S][S][17]  the reference's board tensor (play.py:295-299), NHWC, plane 2k =
 *             to-play side's stones k plies ago, 2k+1 = opponent's, plane 16 = to-play colour (+1/-1).
 *   action    a = y*S + x, pass = S*S                                   (play.py:31-37)
 *   packed    uint32 [n][sgo_packed_words(S)]  16 bit-planes of ceil(S*S/32) words, ABSOLUTE colours: bit a of plane
 *             2k = black stone at a, k plies ago; plane 2k+1 = white (board17's planes are relative to the side to
 *             move: relative plane c = absolute plane c ^ [white to play]).  The to-play flag is the top bit of the
 *             last word of plane 0 (1 = white to play).  19x19: 192 words = 768 B.
 *   legal     uint32 [n][sgo_plane_words(S)]   bit a = 1 <=> action a is LEGAL (pass bit always 1).
 *   *_dev     arguments are DEVICE pointers; `stream` is a hipStream_t passed as void*.
 *   host entry points (no _dev suffix) copy caller HOST buffers to the GPU, run the same kernels and
 *   copy back; they exist for drop-in use and parity tests, not for throughput.
 *   Supported board sizes: 5, 7, 9, 13, 19.
 *
 * There is no CPU fallback anywhere in this library: without a HIP device every call fails.
 */
#ifndef SGO_H
#define SGO_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGO_OK 0
#define SGO_ERR_ARG (-1)          /* bad size / null pointer / unsupported board size */
#define SGO_ERR_HIP (-2)          /* HIP runtime error, see sgo_last_error() */
#define SGO_ERR_UNSUPPORTED (-3)  /* no hand-written kernel for this shape; the caller takes another route */
#define SGO_ERR_OCCUPIED (-101)   /* play.py:233-234 assert: stone on an occupied point */
#define SGO_ERR_RANGE (-102)      /* coordinates outside the board (IndexError in the reference) */
#define SGO_ERR_CAPACITY (-201)   /* a game's tree-block pool is exhausted */
#define SGO_ERR_DRAWS (-202)      /* ran out of injected random draws */
#define SGO_ERR_STATE (-203)      /* call sequence violated */

/* Bumped whenever a signature or a struct layout below changes; PURE ADDITIONS (new entry points, new error codes) do not bump
 * it -- a binding finds out that a library is older than its header when a symbol is missing (sejonggo_amd/_lib.py load()).  A binding compares it with sgo_version() of the
 * library it loaded and refuses a mismatch (sejonggo_amd/_lib.py load(); INTEGRATION.md §B does the same).
 *   1: round 1.   2: sgo_start_games(+stream), sgo_game_result.first_model (40 bytes), sgo_config.two_model,
 *   sgo_conv_backend removed.   3: the "half-populations" and "packed stem" sections.   4: sgo_heads_* and sgo_net_* (the heads
 *   as one kernel, the whole-net forward).   Added since without a bump: the "interactive games" section (sgo_session_*),
 *   the "policy rollouts" section (sgo_rollout_*), the "game records" section (sgo_records_*), the "position keys" section
 *   (sgo_keys*, sgo_session_keys), the "chains and ladders" section (sgo_tactics*, sgo_session_tactics), the "unconditional life" section
 *   (sgo_life*, sgo_session_life), the "shape search" section (sgo_shape_compile, sgo_shapes*, sgo_session_shapes), the "move
 *   outcomes" section (sgo_moves*, sgo_session_moves), the "influence" section (sgo_influence*, sgo_session_influence), the "securing moves"
 *   section (sgo_secure*, sgo_session_secure), the "life and death" section (sgo_solve*, sgo_session_solve), the "capturing races"
 *   section (sgo_race*, sgo_session_race), the "connections" section (sgo_connect*, sgo_session_connect), the "superko" section
 *   (sgo_superko*; no session form), the "light playouts" section (sgo_playout*, sgo_session_playout),
 *   the "playout tree search" section (sgo_uct*, sgo_session_uct). */
#define SGO_ABI_VERSION 4

const char *sgo_last_error(void);
int sgo_version(void);            /* SGO_ABI_VERSION the library was built with */
int sgo_device_count(void);
int sgo_set_device(int device_id);

/* ---- geometry ---------------------------------------------------------------------------------- */
int sgo_plane_words(int S);   /* ceil(S*S/32); also the number of words of a legal bitset */
int sgo_packed_words(int S);  /* words per packed position record */
int sgo_apad(int S);          /* child slots per tree block (= 32 * plane_words) */

/* ---- stateless rules on HOST buffers (drop-in for play.py) -------------------------------------- */
/* play.py:295-299 game_init */
int sgo_game_init(int S, int n, int32_t *board17);
/* play.py:226-242 make_play (+ :182-217 take_stones, :159-180 capture_group, :219-224 swap_player).
 * colors[i] = 0 means "color=None".  movers[i] receives the player who moved; status[i] is SGO_OK or
 * SGO_ERR_OCCUPIED / SGO_ERR_RANGE (board i is then left untouched).  Returns SGO_OK if the batch ran. */
int sgo_make_play(int S, int n, int32_t *board17, const int32_t *xs, const int32_t *ys, const int32_t *colors,
                  int32_t *movers, int32_t *status);
/* play.py:71-104 legal_moves: mask[n][S*S+1], 1 = ILLEGAL (the reference's convention), pass = 0 */
int sgo_legal_moves(int S, int n, const int32_t *board17, uint8_t *mask);
/* play.py:274-292 get_winner/_get_points: winner +1/0/-1, black points, white points (incl. komi) */
int sgo_get_winner(int S, int n, const int32_t *board17, double komi, int32_t *winner, int32_t *black, double *white);
/* play.py:182-217 take_stones on board tensors in place (planes 0/1 only): removes the opponent groups next to (x, y)
 * that have no liberty, then the own groups among (x, y) and its four neighbours that have none (suicide executed). */
int sgo_take_stones(int S, int n, int32_t *board17, const int32_t *xs, const int32_t *ys);
/* Group / territory queries on plain boards (play.py:159-180 capture_group, :55-69 get_liberties, :244-271 color_board).
 * cells int8 [n][S][S]: +1 black, -1 white, 0 empty, any other value = wall (neither stone nor liberty).
 * mode 0: member[i] = the seed (xs[i], ys[i]) plus the stones of colour colors[i] connected to it; liberty[i] = empty
 *         points next to a member.  mode 1: member[i] = empty points connected through empty points to a stone of
 *         colour colors[i] (color_board's fill); liberty is zeroed.  member / liberty: uint8 [n][S][S]. */
int sgo_board_query(int S, int n, int mode, const int8_t *cells, const int32_t *xs, const int32_t *ys, const int32_t *colors,
                    uint8_t *member, uint8_t *liberty);
/* symmetry.py:45-114 board transforms; k: 0 id, 1 left_diagonal, 2 vertical_axis, 3 horizontal_axis,
 * 4 rotation_90, 5 rotation_180, 6 rotation_270 (order of symmetry.SYMMETRIES, :117-125), 7 right_diagonal */
int sgo_sym_apply(int S, int k, int n, const int32_t *in17, int32_t *out17);
/* symmetry.py reverse_*: out[i][a] = in[i][SWAP_k[a]] */
int sgo_sym_invert_policy(int S, int k, int n, const float *in, float *out);
/* symmetry.py:12-42 the SWAP table itself (A entries) */
int sgo_sym_lut(int S, int k, int32_t *lut);

/* ---- device-resident batch kernels (the data-parallel hot path) --------------------------------- */
int sgo_pack_dev(int S, int n, const int32_t *d_board17, uint32_t *d_packed, void *stream);
int sgo_unpack_dev(int S, int n, const uint32_t *d_packed, int32_t *d_board17, void *stream);
/* board_advance: for i<n  out[out_idx?out_idx[i]:i] = make_play(in[in_idx?in_idx[i]:i], moves[i]) and
 * legal[...] = legal bits of the new position.  moves[i] = action index; colors may be NULL (None);
 * status may be NULL.  in and out may alias record-for-record (in place). */
int sgo_advance_legal_dev(int S, int n, const uint32_t *d_in, const int32_t *d_in_idx, const int32_t *d_moves,
                          const int32_t *d_colors, uint32_t *d_out, const int32_t *d_out_idx, uint32_t *d_legal,
                          int32_t *d_status, void *stream);
/* Kernel form behind the non-aliasing board_advance launches (sgo_advance_legal_dev with disjoint dense in / out, the
 * engine's leaf step): 0 = history stream + one lane per position (two launches), 1 = the same two in one launch,
 * 2 = one half-wavefront per position (row per lane; csrc/sgo_rows.hpp), -1 = by batch size (default: 2 up to 32 768
 * positions, 1 up to 65 536, 0 above).  Returns the previous mode; other values only query.  All forms are bit-identical. */
int sgo_advance_mode(int mode);
int sgo_legal_dev(int S, int n, const uint32_t *d_packed, const int32_t *d_idx, uint32_t *d_legal, void *stream);
/* d_result[i] = {winner, black, white_stones_and_territory (without komi)} as 3 x int32 */
int sgo_score_dev(int S, int n, const uint32_t *d_packed, const int32_t *d_idx, double komi, int32_t *d_result,
                  void *stream);
/* nn_input_pack (+ fused sym_apply): network input for positions d_packed[d_idx[i]], transformed by
 * symmetry k.  layout 0: NHWC [n][S][S][17], 1: NCHW [n][17][S][S], 2: NHWC with the channels zero-padded
 * to 32 [n][S][S][32] (MFMA-friendly K for the stem convolution); dtype 0: fp16, 1: fp32. */
int sgo_nn_pack_dev(int S, int n, const uint32_t *d_packed, const int32_t *d_idx, int k, int layout, int dtype,
                    void *d_out, void *stream);

/* Fused convolution epilogue of the resident net (model.py:37-46 BatchNorm folded into the conv, then
 * Activation('relu') / Add()): out = relu(x + bias[c] (+ skip)) on NHWC fp16, in place allowed.
 * n_elems and channels must be multiples of 8. */
int sgo_bias_act_dev(long n_elems, int channels, const void *d_x, const void *d_bias, const void *d_skip, void *d_out,
                     void *stream);

/* The 3x3 convolutions of the resident net with the epilogue fused: y = relu(conv3x3(x, w) + bias[k] (+ skip)),
 * stride 1, pad 0 or 1, NHWC fp16 (x [n][h][w][c], w [k][3][3][c] = PyTorch channels_last weight storage,
 * y / skip [n][ho][wo][k]), fp32 accumulation on MFMA.  Dispatches to the hand-written kernels below (the tower's and the
 * stem's; together with sgo_stem_packed_dev and sgo_heads_dev they are every layer of the resident net); any other shape
 * returns SGO_ERR_UNSUPPORTED (net.FusedInferenceNet then runs that layer through the framework's convolution and
 * sgo_bias_act_dev). */
int sgo_conv3x3_bias_act_dev(int n, int h, int w, int c, int k, int pad, const void *d_x, const void *d_w,
                             const void *d_bias, const void *d_skip, void *d_y, void *stream);

/* The hand-written CDNA4 kernel for the tower shape (c = k = 256, pad 1, w <= 19; csrc/sgo_conv4w.hpp, sgo_conv8w.hpp).  Same layouts. */
int sgo_conv3x3_tower_dev(int n, int h, int w, const void *d_x, const void *d_w, const void *d_bias, const void *d_skip,
                          void *d_y, void *stream);
/* The same convolution fed from a filter bank in MFMA-FRAGMENT ORDER (csrc/sgo_conv4r.hpp, k_conv4r: the weights go L2 -> registers,
 * one 1-KB contiguous load per fragment, and never touch the LDS; the resident net's route since round 3).  A bank is
 * sgo_conv3x3_tower_packed_bytes() bytes, 16-byte aligned, and is written ONCE per layer from the OHWI weights d_w
 * [256][3][3][256] fp16 by sgo_conv3x3_tower_prepack_dev (again after every weight update); x / bias / skip / y as above.
 * Results equal sgo_conv3x3_tower_dev's bit for bit (same MFMA order per output). */
long sgo_conv3x3_tower_packed_bytes(void);
int sgo_conv3x3_tower_prepack_dev(const void *d_w, void *d_wp, void *stream);
int sgo_conv3x3_tower_packed_dev(int n, int h, int w, const void *d_x, const void *d_wp, const void *d_bias, const void *d_skip,
                                 void *d_y, void *stream);
/* Schedule variant of k_conv4r (A/B builds with -DSGO_CONV4W_VARIANTS: 0, 3, 17; 1 = the product, which any other value and
 * every product build runs).  Returns the previous one; negative = query. */
int sgo_conv_packed_variant(int v);
/* The hand-written CDNA4 kernel for the stem (c = 32: the 17 input planes zero-padded, k = 256, pad 0, no skip;
 * csrc/sgo_stem.hpp; model.py:57-60).  x [n][h][w][32] is layout 2 of sgo_nn_pack_dev: the route of callers that hold board
 * TENSORS (put_predict_request); the self-play engine feeds the net through sgo_stem_packed_dev below instead. */
int sgo_conv3x3_stem_dev(int n, int h, int w, const void *d_x, const void *d_w, const void *d_bias, void *d_y, void *stream);
/* The stem straight from PACKED POSITION RECORDS (csrc/sgo_stem_packed.hpp; model.py:57-60 + symmetry.py:127-132): row i of the
 * output is relu(conv3x3_valid(planes of sym_k(record d_index[i])) + bias), y [n][S-2][S-2][256] fp16.  The 16 stone planes are
 * expanded from the record's bit-planes in LDS (relative to the side to move, symmetry on the gather side); the colour plane
 * (+-1 over the whole board, 'valid' convolution) is the per-position constant c * d_wcol[k] added to the bias.
 * d_w10: [256][10][16] fp16 -- taps 0..8 (dy * 3 + dx) of the 16 stone planes, tap 9 zero; d_bias fp16 [256];
 * d_wcol float [256] = sum over the 9 taps of the colour plane's weights.  d_index NULL = records 0..n-1; d_sym_k (device
 * int, optional) overrides sym_k when the kernel runs.  No network-input tensor exists on this route. */
int sgo_stem_packed_dev(int S, int n, const uint32_t *d_records, const int32_t *d_index, int sym_k, const int32_t *d_sym_k,
                        const void *d_w10, const void *d_bias, const float *d_wcol, void *d_y, void *stream);
/* Which hand-written kernel sgo_conv3x3_tower_dev launches: 1 = k_conv4w (csrc/sgo_conv4w.hpp: two 256-thread workgroups per
 * CU, 256 pixels x 128 channels each; the default), 0 = k_conv8w (csrc/sgo_conv8w.hpp: one 512-thread workgroup per CU,
 * 256 pixels x 256 channels); 16 + v = k_conv4w's schedule variant v (A/B builds with -DSGO_CONV4W_VARIANTS: 0, 4, 5, 6; any other
 * v and every product build run the product's 7).  Same results bit for bit.  Returns the previous choice; other values only query. */
int sgo_conv_tower_kernel(int mode);
/* Tile order of the tower kernel's launches: 1 = every XCD walks a contiguous range of pixel tiles (default: the halo rows
 * a tile shares with its neighbour are then in that XCD's L2), 0 = identity.  Returns the previous mode; other values query. */
int sgo_conv_tile_order(int mode);
/* Test hook: cap the samples per launch of sgo_conv3x3_tower_dev / _stem_dev (0 = no cap) so that the slice loop, which
 * otherwise needs tensors beyond 2^31 bytes, can be exercised on small inputs.  Returns the previous cap; negative = query. */
long sgo_conv_tower_slice_cap(long cap);

/* ---- the heads of the resident net as ONE kernel (csrc/sgo_heads.hpp, k_heads; model.py:62-95) -------------------------- */
/* Policy head Conv1x1(->2) + ReLU + Flatten + Dense(S*S+1, softmax) and value head Conv1x1(->2) + ReLU + Flatten + Dense(256,
 * relu) + Dense(1, tanh), BatchNorm folded, on the tower's output.  Weights in the layouts net.FusedInferenceNet holds:
 * head_w [4][256] fp16 (rows p0 p1 v0 v1), head_b [4], p_fc_w [A][2 t t], v_fc1_w [256][2 t t] with the K index in Keras'
 * flatten order pixel * 2 + channel (t = S - 2, A = S*S + 1).  The two wide FC layers are read from a BANK in MFMA fragment
 * order (K zero-padded to a multiple of 32, N to a multiple of 16), sgo_heads_packed_bytes(S) bytes, 16-byte aligned, written
 * once per weight update by sgo_heads_prepack_dev.
 * Arithmetic: every accumulation is fp32; h = relu(conv1x1 + bias) is rounded to fp16 once (an MFMA operand); logits, v1, the
 * pre-tanh value, the softmax (row maximum subtracted) and the tanh stay fp32.
 * sgo_heads_dev: y [n][t][t][256] fp16 NHWC -> policy [n][A] f32, value [n] f32: the shapes sgo_step consumes.  One launch, no
 * allocation, no synchronisation (capturable); n == 0 is a no-op; rows >= n are neither read nor written.  y, head_w and the
 * bank must be 16-byte aligned. */
long sgo_heads_packed_bytes(int S);
int sgo_heads_prepack_dev(int S, const void *d_p_fc_w, const void *d_v_fc1_w, void *d_bank, void *stream);
int sgo_heads_dev(int S, int n, const void *d_y, const void *d_head_w, const void *d_head_b, const void *d_bank,
                  const void *d_p_fc_b, const void *d_v_fc1_b, const void *d_v_fc2_w, const void *d_v_fc2_b, float *d_policy,
                  float *d_value, void *stream);

/* ---- the resident net as an object of this library: positions in, policy / value out (model.py:55-95) ----------------- */
/* 256 channels, 'valid' stem, n_blocks residual blocks.  With sgo_eval_list and sgo_step a self-play loop needs this header
 * alone ("A loop without a framework"). */
typedef struct sgo_net sgo_net;
/* Every pointer may be a HOST or a DEVICE pointer (copied with hipMemcpyDefault).  Layouts as net.FusedInferenceNet holds them:
 * stem_w10 [256][10][16] fp16, stem_b [256] fp16, stem_wcol [256] f32 (see sgo_stem_packed_dev); block_*: n_blocks entries each,
 * w OHWI [256][3][3][256] fp16, b [256] fp16; the head tensors as sgo_heads_dev / sgo_heads_prepack_dev take them. */
typedef struct sgo_net_weights {
    const void *stem_w10, *stem_b;
    const float *stem_wcol;
    const void *const *block_w1, *const *block_b1, *const *block_w2, *const *block_b2;
    const void *head_w, *head_b, *p_fc_w, *p_fc_b, *v_fc1_w, *v_fc1_b, *v_fc2_w, *v_fc2_b;
} sgo_net_weights;
/* Allocates the weights, the heads bank and three activation buffers of max_batch * t * t * 256 fp16 (y, z, y'), once.
 * NULL + sgo_last_error() for an unsupported S, n_blocks < 1, max_batch < 1 or when memory runs out. */
sgo_net *sgo_net_create(int S, int n_blocks, int max_batch, int device_id);
/* Copies the weights with hipMemcpyAsync on `stream` and prepacks the heads bank, and the k_conv4r filter banks when that tower
 * kernel is selected.  PAGEABLE host sources have been read when the call returns; PINNED host sources and device sources are
 * read when the stream reaches the copies and must stay valid and unchanged until then.  Call again after every weight update.
 * The calling thread's current device is left as it was (also by sgo_net_create / sgo_net_packed_tower / sgo_net_destroy). */
int sgo_net_set_weights(sgo_net *net, const sgo_net_weights *w, void *stream);
/* Tower kernel of this net: on = 0: sgo_conv3x3_tower_dev (default), on = 1: sgo_conv3x3_tower_packed_dev (k_conv4r; the filter
 * banks are allocated on the first selection and written here, on `stream`, when the net already has weights).  Same bits
 * either way.  Returns SGO_OK or a negative error (the route is then unchanged; a later call allocates only what is missing). */
int sgo_net_packed_tower(sgo_net *net, int on, void *stream);
/* Row i of the outputs = the net on sym_k(record d_index[i]) (d_index NULL: records 0..n-1; d_sym_k, a device int, overrides
 * sym_k when the kernels run): queues sgo_stem_packed_dev, 2 * n_blocks tower launches and sgo_heads_dev on `stream` and nothing
 * else -- no allocation, no synchronisation, capturable.  n > max_batch runs in slices.  d_policy [n][A] f32 and d_value [n]
 * f32 are what sgo_step / sgo_step_enqueue consume.  The tower output is bit-identical to net.FusedInferenceNet's. */
int sgo_net_predict_packed_dev(sgo_net *net, int n, const uint32_t *d_records, const int32_t *d_index, int sym_k,
                               const int32_t *d_sym_k, float *d_policy, float *d_value, void *stream);
void sgo_net_destroy(sgo_net *net);

/* ---- self-play engine: virtual-loss PUCT + game loop, many games resident on one GPU ------------ */
/* Replaces nomodel_self_play.py:59-82 async_simulate2, :114-140 select_play, :142-271 play_game_async,
 * tree_util.py:4-32, play.py:308-323/376-421, simulation_workers.py:42-54 basic_tasks2 and the request
 * side of predicting_queue_worker.py:40-102.  One ctx per GPU; not thread-safe. */
typedef struct sgo_ctx sgo_ctx;

typedef struct sgo_config {
    int32_t size;             /* conf['SIZE'] */
    int32_t n_games;          /* concurrent game slots */
    int32_t sims;             /* conf['MCTS_SIMULATIONS'] */
    int32_t energy;           /* conf['ENERGY'] (<= 64) */
    int32_t stop_exploration; /* conf['STOP_EXPLORATION'] */
    int32_t num_moves;        /* play_game_async(num_moves); <0 => 2*S*S */
    int32_t blocks_per_game;  /* PRIVATE tree blocks per game; <=0 => 8*sims + 128 (and the default shared pool, below) */
    int32_t self_play;        /* add Dirichlet noise when a tree is created (play.py:400-403) */
    double komi;              /* conf['KOMI'] */
    double dirichlet_epsilon; /* conf['DIRICHLET_EPSILON'] */
    int32_t device_id;
    int32_t two_model;        /* 1: evaluation games between two nets (evaluate_worker.py:137): one tree per player, the tree of
                                 the side not to move follows the move when it holds it (nomodel_self_play.py:203-218);
                                 requires self_play = 0.  Every row of a step's evaluation list belongs to one model:
                                 sgo_eval_models() */
    int32_t shared_blocks;    /* tree blocks SHARED by all games of the context: a game whose tree outgrows its private blocks
                                 takes more from here, one at a time, and gives them back when a move prunes its tree.
                                 > 0: that many; < 0: the default (2*sims per game, at least 12*sims + 128); 0: the default when
                                 blocks_per_game <= 0, none otherwise (a fixed per-game pool).  All bounded by 60 % of the free
                                 device memory and, per game, by the id space of k_search's LDS work queue (~38 000 blocks). */
    int32_t reserved;
} sgo_config;

typedef struct sgo_status {
    int32_t n_eval;       /* positions waiting for a network evaluation after this step */
    int32_t n_records;    /* move records waiting in the record buffer */
    int32_t n_active;     /* game slots still playing */
    int32_t n_done;       /* game slots finished and not yet restarted */
    int32_t error;        /* first error raised by any game (SGO_ERR_*) or 0 */
    int32_t error_game;
    int64_t total_moves;  /* moves played since ctx creation (a session's resign record counts, an analysis record does not) */
    int64_t total_evals;  /* network evaluations consumed since ctx creation */
    int64_t none_events;  /* "No best leaf" events (nomodel_self_play.py:70-75) */
} sgo_status;

/* one record per move played = the reference's move_data (nomodel_self_play.py:187-194) */
typedef struct sgo_move_record {
    int32_t game;      /* slot */
    int32_t game_seq;  /* how many games this slot had finished before this one */
    int32_t move_n;
    int32_t action;    /* y*S + x, S*S = pass; -1 = a session resigned, SGO_ACTION_ANALYSIS (-2) = a search-only record */
    int32_t player;    /* 'player' exactly as the reference records it */
    float value;       /* raw network value at the root */
} sgo_move_record;

typedef struct sgo_game_result {
    int32_t winner;      /* +1 black, -1 white, 0 draw (play.py:274-284) */
    int32_t black;       /* black points */
    double white;        /* white points incl. komi */
    int32_t end_reason;  /* 0 PLAYED ALL MOVES, 1 resign, 2 BOTH_PASSED */
    int32_t n_moves;
    int32_t last_player; /* 'player' when the loop ended (used for "X+R") */
    int32_t done;
    int32_t first_model; /* two_model games: which model moved first = plays black (0 = model1, 1 = model2) */
    int32_t blocks_high_water; /* most tree blocks the game ever held at once (private + shared) */
} sgo_game_result;

sgo_ctx *sgo_ctx_create(const sgo_config *cfg);
void sgo_ctx_destroy(sgo_ctx *ctx);
int sgo_blocks_per_game(sgo_ctx *ctx);   /* the private tree blocks per game this context was created with */
/* out[0..n): {private blocks per game, local ids per game (private + overflow ids), shared pool blocks, shared blocks free now,
 * fewest shared blocks ever free, games}.  n <= 6.  Synchronises the device. */
int sgo_pool_info(sgo_ctx *ctx, int64_t *out, int n);
/* (Re)start game slots.  noise: [n][A] float64 Dirichlet draws (np.random.dirichlet stand-in, consumed
 * when a tree is created); uniforms: [n][n_uniforms] float64 in [0,1) consumed one per sampled move
 * (np.random.choice stand-in); resign: [n] thresholds, NaN or 0 = None.  HOST pointers; they are copied before the call
 * returns.  The batch reaches the device in ONE host-to-device copy followed by one kernel, both queued on `stream`
 * (use the stream the steps run on): no device-wide synchronisation. */
int sgo_start_games(sgo_ctx *ctx, int n, const int32_t *slots, const double *noise, const double *uniforms,
                    int n_uniforms, const float *resign, void *stream);
/* (Re)start slots of a two_model context: no Dirichlet noise (self_play is off), one resign threshold per model
 * (nomodel_self_play.py:170: `resign_model1 if current == model1 else resign_model2`), and who moves first
 * (first_model[i] = 0: model1 plays black; play.py:301-306 choose_first_player is the caller's coin). */
int sgo_start_games2(sgo_ctx *ctx, int n, const int32_t *slots, const double *uniforms, int n_uniforms,
                     const float *resign_model1, const float *resign_model2, const int32_t *first_model, void *stream);
/* Which model (0 / 1) must evaluate each row of the evaluation list of the last step (all 0 unless two_model).  HOST buffer
 * models[cap]; returns the number of rows. */
int sgo_eval_models(sgo_ctx *ctx, int cap, int32_t *models);
/* One engine step.  Consumes the evaluations of the positions listed by the previous step
 * (d_policy [n_eval][A] float32, d_value [n_eval] float32, produced from inputs transformed by
 * symmetry sym_k; NULL on the first call), back-propagates, selects the next leaves, plays moves whose
 * search is complete, computes the new leaf positions, and reports what must be evaluated next.
 * Synchronises `stream` once to return `st`. */
int sgo_step(sgo_ctx *ctx, const float *d_policy, const float *d_value, int sym_k, void *stream, sgo_status *st);
/* The same step in two halves, for launch chains that must not wait for the host (hipGraph capture, two half-populations
 * alternating on two streams): sgo_step_enqueue queues k_search / k_compact / board_advance and the copy of the status words to
 * pinned host memory on `stream` and returns at once; the symmetry the consumed evaluations were produced under is read from
 * DEVICE memory (*d_sym_k, 0..7) when the kernel runs, so one captured chain serves every symmetry.  d_policy / d_value must
 * stay valid until the chain has run (rows beyond the listed count are ignored).  After the caller has synchronised the stream
 * (or an event behind the enqueue), sgo_step_status returns what that step reported.  No board_advance timing in this form. */
int sgo_step_enqueue(sgo_ctx *ctx, const float *d_policy, const float *d_value, const int32_t *d_sym_k, void *stream);
int sgo_step_status(sgo_ctx *ctx, sgo_status *st);
/* Where the evaluation list of the last step lives ON THE DEVICE, for consumers that read packed records directly
 * (sgo_stem_packed_dev): *d_records = the context's record array (sgo_packed_words(S) words per record), *d_index = the
 * record index of every row of the list (n_eval of them valid, in the order results are expected), *d_models = which model
 * evaluates each row (two_model contexts).  The pointers stay valid for the life of the context; the contents change with
 * every step.  Returns the capacity of the list (n_games * energy). */
int sgo_eval_list(sgo_ctx *ctx, const uint32_t **d_records, const int32_t **d_index, const int32_t **d_models);
/* Network input for the positions listed by the last sgo_step (same order as the results expected). */
int sgo_collect(sgo_ctx *ctx, int sym_k, int layout, int dtype, void *d_nn_in, void *stream);
/* Move records produced so far (HOST buffers): recs[cap], boards packed [cap][packed_words],
 * policy targets [cap][A] float64.  Returns the number written (>=0) and clears the buffer. */
int sgo_drain_records(sgo_ctx *ctx, int cap, sgo_move_record *recs, uint32_t *packed, double *policy);
int sgo_game_results(sgo_ctx *ctx, int n, const int32_t *slots, sgo_game_result *out);

/* ---- interactive games: session slots that take external moves and answer genmove on demand ----------------------------- */
/* Replaces sejonggo_nomodel.py:20-100 SejongGoEngine (play / genmove on a persistent tree), for 1..n_games resident games at
 * once.  A slot becomes a SESSION by sgo_session_open; between commands it HOLDS: it keeps its board and tree, sgo_step skips
 * it, and sgo_status counts it neither in n_active nor in n_done.  Session and ordinary slots may share one context (not a
 * two_model one); sgo_start_games on a session slot turns it back into an ordinary game.  Every sgo_session_* call on a slot
 * that runs an ordinary game fails with SGO_ERR_STATE.  slots / actions / colors / status / resign are HOST arrays of n entries
 * (a slot may be listed once per call); all three calls wait for `stream` (use the stream the steps run on).
 *
 * sgo_session_open: as sgo_start_games without noise or draws -- empty board, empty tree, whatever the slot held (shared-pool
 * blocks included) released -- but the slot is a session, holds, and plays at temperature 0 without Dirichlet noise for its
 * whole life (sejonggo_nomodel.py:22 defaults).  It never ends by num_moves or by two passes: a GTP game goes on after both
 * players pass.  resign: thresholds as in sgo_start_games (NULL, NaN or 0 = never).  Also serves clear_board (:135-140). */
int sgo_session_open(sgo_ctx *ctx, int n, const int32_t *slots, const float *resign, void *stream);
/* SejongGoEngine.play (sejonggo_nomodel.py:45-56) as ONE launch, one wavefront per listed slot.  actions[i] = y*S + x, pass = S*S;
 * colors[i] = 0 for the side to move, or +1 / -1.  status[i] receives SGO_OK, SGO_ERR_STATE (not a session, or not holding),
 * SGO_ERR_RANGE (action outside [0, S*S]) or SGO_ERR_OCCUPIED (play.py:233-234); a slot with a non-zero status is left
 * untouched in every word.  Otherwise move_n is incremented and
 *   - the move is in turn and the root holds an evaluated child for it: the tree is re-rooted onto that child (:49-51), its
 *     statistics become the root's, every block that is no longer reachable is recycled (shared blocks go back to the pool);
 *   - any other in-turn move (the child was never evaluated, the root is unexpanded, or the move is playable by make_play but
 *     not in the legal set -- a suicide, which play.py:200-215 executes): the tree is dropped, the root holds
 *     make_play(position, action, colour) (play.py:226-242) and the next genmove builds its tree from the root evaluation
 *     (play.py:376-389 new_tree);
 *   - an out-of-turn colour: the board is exactly make_play(x, y, board, color) and the tree is dropped.  DEVIATION: the
 *     reference keeps the subtree's statistics there and replays them over the changed board; tree blocks store positions.
 * Returns SGO_OK when the batch ran. */
int sgo_session_play(sgo_ctx *ctx, int n, const int32_t *slots, const int32_t *actions, const int32_t *colors, int32_t *status,
                     void *stream);
/* SejongGoEngine.genmove (sejonggo_nomodel.py:58-76): ARMS the listed holding slots; the ordinary sgo_step loop then runs, per
 * armed slot, one turn of play_game_async's loop body (nomodel_self_play.py:165-216): root evaluation; the resign test (value <=
 * resign: a move record with action = -1 and a zero policy row; board, tree and move_n unchanged); new_tree without noise when
 * the root is unexpanded; the search; the sgo_move_record with policy target and packed board; the re-root; move_n + 1 -- and
 * then the slot holds again instead of asking for its next root evaluation.  The move is read from sgo_drain_records.
 * A listed slot that is not a holding session (an ordinary game, a session that is still searching, a failed slot) gives
 * SGO_ERR_STATE, and then NO slot of the call is armed. */
int sgo_session_genmove(sgo_ctx *ctx, int n, const int32_t *slots, void *stream);
/* A position instead of the empty board (GTP undo, loadsgf, handicap stones; a game record under review): for every listed slot
 * what sgo_session_open followed by the slot's move list through sgo_session_play does -- the empty board, then the moves, with
 * make_play's rules (play.py:226-242: suicide executed; colors 0 = the side to move, +1 / -1 explicit, an out-of-turn colour is
 * how set-up and handicap stones are placed, played as sgo_session_play plays it and with its DEVIATION: no tree survives) -- in
 * ONE launch for all slots, one wavefront per slot, and one host-to-device copy of all lists (a staging buffer of the context
 * that only grows: no allocation per call once it has).  Slot i replays actions / colors [moves_off[i], moves_off[i] +
 * n_moves[i]) (colors NULL: all 0).  The slot is left holding with an unexpanded root; everything else it held, shared-pool
 * blocks included, is released; move_n and player are as the chain of plays leaves them; the slot's resign threshold is KEPT
 * (a list of zero moves is sgo_session_open without a change of the threshold).
 * ATOMIC PER SLOT: the list is replayed into a private copy of the record and the slot is written after the last move only.
 * status[i] = SGO_OK and fail_at[i] = -1, or SGO_ERR_RANGE / SGO_ERR_OCCUPIED with fail_at[i] = the index of the refused move, or
 * SGO_ERR_STATE (not a holding session; fail_at -1); a refused slot is unchanged in every word, the other slots of the call go
 * through.  A slot listed twice, a negative length or a list longer than SGO_SETUP_MAX_MOVES(size) returns SGO_ERR_ARG and
 * nothing runs.  Waits for `stream`. */
#define SGO_SETUP_MAX_MOVES(size) (4 * (size) * (size))
int sgo_session_setup(sgo_ctx *ctx, int n, const int32_t *slots, const int32_t *n_moves, const int32_t *moves_off,
                      const int32_t *actions, const int32_t *colors, int32_t *status, int32_t *fail_at, void *stream);
/* Search without moving: ARMS the listed holding slots as sgo_session_genmove does (all or none, SGO_ERR_STATE otherwise); the
 * ordinary sgo_step loop then runs, per armed slot: the root evaluation; NO resign test; new_tree without noise when the root is
 * unexpanded (play.py:376-389); sims / energy rounds of async_simulate2 (nomodel_self_play.py:59-82; sims <= 0: the context's,
 * 0 < sims < energy: SGO_ERR_ARG) -- select_play's simulation loop (:114-124) without its choice.  Instead of a move the slot
 * writes ONE sgo_move_record with action = SGO_ACTION_ANALYSIS, the root's net value, the packed root position and the prior row
 * a genmove from this root would record, and holds.  Board, tree and move_n stay; the searched tree is KEPT: a second analyze
 * deepens it (one more root evaluation, then its rounds), a following genmove searches on top of it as the reference does with
 * a kept subtree (sejonggo_nomodel.py:63), a following play follows into it when it can.  A search that outgrows the slot's
 * blocks fails the slot with SGO_ERR_CAPACITY, as any search does; sgo_game_results then shows done = the error and, for a slot
 * that failed inside an analysis, end_reason = 2 (the engine's mark of a search-only search, not BOTH_PASSED): a failed session
 * slot has no result to read, reopen it. */
#define SGO_ACTION_ANALYSIS (-2)
int sgo_session_analyze(sgo_ctx *ctx, int n, const int32_t *slots, int sims, void *stream);
/* The result of many slots at once: ONE launch (one wavefront per slot) and one copy back; waits for `stream`.  HOST outputs,
 * each may be NULL except status: status[n] (SGO_OK, or SGO_ERR_STATE for a slot that is not a holding session: its rows are left
 * as the caller filled them), to_play[n] (+1 black), root_count[n], root_value[n], root_mean[n], n_children[n]; the root's child
 * tables N[n][A] (-1 = no child), Q[n][A], P[n][A] float32 -- the values sgo_root_table gives, raw; top_action[n][K]: the K best
 * children in select_play's temperature-0 order (nomodel_self_play.py:138: count, then mean, then the HIGHER index), -1 padded;
 * pv[n][K][D]: below each, the principal variation -- the child itself, then the same rule applied down the tree while the
 * node is expanded and has a visited child, at most D moves, -1 padded.  K <= SGO_REPORT_MAX_TOP, D <= SGO_REPORT_MAX_DEPTH,
 * SGO_ERR_ARG beyond. */
#define SGO_REPORT_MAX_TOP 16
#define SGO_REPORT_MAX_DEPTH 32
int sgo_session_report(sgo_ctx *ctx, int n, const int32_t *slots, int K, int D, int32_t *status, int32_t *to_play,
                       int32_t *root_count, float *root_value, float *root_mean, int32_t *n_children, int32_t *N, float *Q,
                       float *P, int32_t *top_action, int32_t *pv, void *stream);

/* ---- policy rollouts: ownership, final score and dead stones from many policy-sampled play-outs -------------------------- */
/* How did the game end?  sgo_score_dev / get_winner (play.py:274-292) count every stone on the board as alive.  A ROLLOUT object
 * plays a position out many times with the net's policy -- thousands of tree-less games, one sampled move per net call -- and
 * counts who ends up holding each point (csrc/sgo_rollout.hip).  The caller's loop is
 *     sgo_rollout_start*;  while (n_live) { sgo_rollout_list -> the net on those rows -> sgo_rollout_step; }  sgo_rollout_result
 * (INTEGRATION.md shows it with sgo_net_predict_packed_dev).  One object per caller; not thread-safe.
 *
 * Semantics, all integer.  A rollout is a packed record, a ply counter, a consecutive-pass counter and a global id
 * g = src * per_src + j (j < per_src).  One step does, for every live rollout: the legal set of its position (play.py:71-104
 * legal_moves, ko approximation included).  No legal board point: it passes (pass counter + 1; its policy row is ignored).
 * Otherwise every legal point a < S*S weighs w[a] = floor(clamp(p[a]) * 2^20) + 1, where clamp(p) = p for 0 < p <= 1, 1 for p > 1
 * or +inf, 0 for anything not > 0 (NaN, negatives, +-0); illegal points weigh 0 and the row's pass entry is never used (while a
 * board move exists a rollout does not pass); total = sum of w (< 2^29); t = (uint64(r) * total) >> 32 with r = draw(seed, g,
 * ply); the move is the smallest a with w[0] + ... + w[a] > t, and the pass counter returns to 0.  The move is played with
 * make_play's rules (play.py:226-242) and ply is incremented.  The rollout ENDS when the pass counter reaches 2 or ply ==
 * max_plies (<= 0: 2*S*S, the reference's num_moves); passes in the starting position's history do not count; one that ends
 * with fewer than two passes in a row is CAPPED.
 *   mix(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (uint32)
 *   draw(seed, g, ply) = mix(mix(seed ^ (g * 0x9E3779B9)) + ply * 0x85EBCA6B)
 * At its end a rollout is scored as play.py:244-292 does: a point is black's if it holds a black stone or is empty and reached
 * by black only, the same for white; empty points reached by both or by neither are nobody's.  Its source receives +1 in
 * black_own / white_own for each owned point and one entry of the sums (below), with integer atomics: results do not depend on
 * the order in which rollouts are listed or finish.
 * A policy row is what the net produced from the input transformed by sym_k, the convention of sgo_step; the step maps it back. */
typedef struct sgo_rollout sgo_rollout;
typedef struct sgo_rollout_status { int32_t n_live, n_done, steps, error; } sgo_rollout_status;

/* Allocates everything once: 2 * max_rollouts records, the lists, the accumulators of max_sources sources, pinned host blocks.
 * NULL + sgo_last_error() for an unsupported S, max_sources outside [1, max_rollouts] or when memory runs out. */
sgo_rollout *sgo_rollout_create(int S, int max_rollouts, int max_sources, int device_id);
void sgo_rollout_destroy(sgo_rollout *);
/* Start n_src * per_src rollouts, per_src from each source record; counters and accumulators are zeroed; whatever ran before is
 * abandoned.  One kernel (after one host-to-device copy for HOST records: sgo_rollout_start) queued on `stream`, no
 * synchronisation.  sgo_rollout_start_dev: DEVICE records, source s = record d_index[s] (d_index NULL: record s), read when the
 * stream reaches the kernel.  Afterwards n_live = n_src * per_src, and every live rollout is on the list every step.
 * SGO_ERR_ARG (nothing runs, state and results untouched): n_src * per_src > max_rollouts, n_src > max_sources, n_src < 1 or
 * per_src < 1. */
int sgo_rollout_start(sgo_rollout *, int n_src, const uint32_t *records, int per_src, uint32_t seed, int max_plies, void *stream);
int sgo_rollout_start_dev(sgo_rollout *, int n_src, const uint32_t *d_records, const int32_t *d_index, int per_src, uint32_t seed,
                          int max_plies, void *stream);
/* The sources are the root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), copied on the
 * device; the context is only read.  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is not a holding session: the call then
 * returns SGO_ERR_STATE and nothing starts.  Waits for `stream` once (the verdict comes back); use the stream the steps run on. */
int sgo_rollout_start_sessions(sgo_rollout *, sgo_ctx *ctx, int n, const int32_t *slots, int per_src, uint32_t seed, int max_plies,
                               int32_t *status, void *stream);
/* What the net must evaluate now: *d_records = the object's record array, *d_index = the record index of every live rollout
 * (n_live rows valid; row i of the policy handed to the next step belongs to entry i), for sgo_stem_packed_dev /
 * sgo_net_predict_packed_dev / sgo_nn_pack_dev.  Records ping-pong and the step fills a second list: ask again after every
 * step.  Returns the capacity of the list (max_rollouts). */
int sgo_rollout_list(sgo_rollout *, const uint32_t **d_records, const int32_t **d_index);
/* One ply of every live rollout from d_policy [n_live][S*S+1] float32 (device): ONE kernel, then the count of the next list goes
 * to pinned host memory and `stream` is synchronised once to return *st.  No allocation, no device-wide synchronisation.
 * SGO_ERR_STATE (nothing runs): before a start, or after n_live reached 0. */
int sgo_rollout_step(sgo_rollout *, const float *d_policy, int sym_k, void *stream, sgo_rollout_status *st);
/* HOST outputs of the first n_src sources, each may be NULL: black_own / white_own int32 [n_src][S*S]; sums int64 [n_src][8] =
 * {black_wins, white_wins, draws (by the komi-free area counts), score_sum (sum of black - white), score_sq_sum, plies_sum,
 * capped, rollouts}.  SGO_ERR_STATE while rollouts are live or before a start; SGO_ERR_ARG for more sources than were started. */
int sgo_rollout_result(sgo_rollout *, int n_src, int32_t *black_own, int32_t *white_own, int64_t *sums);

/* ---- game records: whole move lists replayed into one packed record per ply, and a net scored on the recorded moves ---------- */
/* A RECORDS object turns a collection of game records into device data without an engine context (csrc/sgo_records.hip).  The
 * caller's loop is
 *     sgo_records_replay;  for slices of its list of record indices { sgo_net_predict_packed_dev -> sgo_records_score_dev; }
 * (INTEGRATION.md shows it).  One object per caller; not thread-safe.
 *
 * Replay.  Game g is a list of n_entries[g] entries, actions / colors [off[g], off[g] + n_entries[g]): action = y * S + x, S * S =
 * pass; colors 0 = the side to move, +1 black / -1 white explicit (colors NULL: all 0), exactly what sgo_session_setup takes and
 * played as it plays them: from the empty board with black to move, make_play's rules (play.py:226-242: suicide executed, passes
 * are moves; a recorded move is PLAYED, not filtered by the legal set, so a ko recapture goes through), an out-of-turn colour is
 * how set-up and handicap stones are placed.  The lists lie BACK TO BACK: off[g] = n_entries[0] + ... + n_entries[g-1].
 * Game g owns the records base_g .. base_g + n_entries[g] with base_g = off[g] + g: record base_g + j is the position BEFORE
 * entry j (record base_g is the empty board), record base_g + n_entries[g] is the final position.  Every record has its legal
 * bitset (play.py:71-104, sgo_plane_words(S) words, bit a = action a is legal, the pass bit always set) at the same index of a
 * parallel array.  The records are what sgo_stem_packed_dev / sgo_net_predict_packed_dev / sgo_nn_pack_dev / sgo_unpack_dev read.
 * REFUSAL: entry j off the board (outside [0, S*S]) gives status[g] = SGO_ERR_RANGE, on a stone SGO_ERR_OCCUPIED, with fail_at[g]
 * = j; game g ends there: records base_g .. base_g + j are valid, nothing after them is written, and every other game of the call
 * goes through.  Otherwise status[g] = SGO_OK and fail_at[g] = -1.
 *
 * Score.  Per listed row i: the record index d_index[i], the recorded action t = d_target[i], z = d_z[i] in {+1, -1, 0} (the
 * result seen from the mover; 0 = unknown), a bucket d_bucket[i] in [0, n_buckets), row i of d_policy [n][S*S+1] and d_value [n]
 * as the net produced them from the record transformed by sym_k (sgo_step's convention; the row is mapped back as
 * sgo_sym_invert_policy does: p[a] = d_policy[i][SWAP_k[a]]).  With key(a) = p[a], a NaN taken as -inf, and the candidates = the
 * legal set of the record (pass included) united with {t}:
 *     rank     = #{candidates a != t : key(a) > key(t) or (key(a) == key(t) and a < t)}
 *     best     = the legal action with the largest key, the lowest index among equals
 *     p_target = p[t], the float copied
 *     flags    bit 0: t is in the legal set
 * and the int64 counters [n_buckets][8] of the row's bucket grow (integer atomics) by {1, rank == 0, rank < 5, t not legal,
 * z != 0, z != 0 and the value agrees (v > 0 and z > 0, or v < 0 and z < 0), 0, 0}.  A row whose record index, target or bucket is
 * out of range is SKIPPED: rank = best = -1, p_target = 0, flags = 2, no counter moves.  Nothing depends on the order of the rows;
 * sums of floats (cross-entropy, squared error) are the caller's, from p_target and the values. */
typedef struct sgo_records sgo_records;
/* Allocates everything once: max_entries + max_games records and legal bitsets, the staging block of the move lists and its
 * pinned host twin (verdicts included).  NULL + sgo_last_error() for an unsupported S, max_games < 1, max_entries < 0 or when
 * memory runs out. */
sgo_records *sgo_records_create(int S, int max_games, int max_entries, int device_id);
void sgo_records_destroy(sgo_records *);
/* ONE host-to-device copy of all lists and ONE launch (one half-wavefront per game), then `stream` is waited for once to return
 * status[n_games] and fail_at[n_games] (HOST).  Whatever an earlier call left in the records is overwritten from record 0 on.
 * SGO_ERR_ARG (nothing runs, records and legal bitsets untouched): a negative length, a list longer than
 * SGO_SETUP_MAX_MOVES(S), offsets that are not back to back, more games than max_games or more entries than max_entries.
 * n_games == 0 is a no-op. */
int sgo_records_replay(sgo_records *, int n_games, const int32_t *n_entries, const int32_t *off, const int32_t *actions,
                       const int32_t *colors, int32_t *status, int32_t *fail_at, void *stream);
/* *d_records = the record array (sgo_packed_words(S) words each), *d_legal = the legal bitsets (sgo_plane_words(S) words each);
 * either may be NULL.  Returns the capacity in records (max_entries + max_games). */
int sgo_records_list(sgo_records *, const uint32_t **d_records, const uint32_t **d_legal);
/* ONE launch on `stream` (one half-wavefront per row), no allocation, no synchronisation; every pointer is DEVICE memory, outputs
 * [n] each, d_counters int64 [n_buckets][8], zeroed by the caller (launches accumulate).  n == 0 is a no-op.  SGO_ERR_ARG: sym_k
 * outside [0, 7], n < 0, n_buckets < 1, a NULL pointer. */
int sgo_records_score_dev(sgo_records *, int n, const int32_t *d_index, const int32_t *d_target, const int32_t *d_z,
                          const int32_t *d_bucket, int n_buckets, const float *d_policy, const float *d_value, int sym_k,
                          int32_t *d_rank, int32_t *d_best, float *d_p_target, int32_t *d_flags, int64_t *d_counters, void *stream);

/* ---- position keys: which position does a record hold?  A 64-bit key that rotations and reflections do not change ------------- */
/* What an opening book, duplicate detection and every later "have I seen this position" stand on (csrc/sgo_keys.hip).  All
 * arithmetic is unsigned 64-bit and wraps.
 *   sm(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *           x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  x ^= x >> 31                                      (uint64)
 *   z(S, c, a) = sm((uint64(S) << 24) | (uint64(c) << 16) | a)      c: 0 black, 1 white, 2 = "white to play" (a = 0)
 * Inputs of a record, N = S * S: black = the bits a < N of plane 0, white = the bits a < N of plane 1 (ABSOLUTE colours, the
 * current position only), w = the to-play flag, the top bit of the last word of plane 0.  The flag is NOT a stone (at S = 5 it
 * shares the plane's only word with the stones); bits a >= N other than the flag and planes 2..15 are never read as stones.
 * L_k is the table sgo_sym_lut(S, k) writes, k = 0..7: together the whole symmetry group of the square.  For k = 4 and k = 6 the
 * table is the INVERSE of where sgo_sym_apply moves a stone, which is why the definition goes through the tables:
 *   key_k  = XOR over a in black of z(S, 0, L_k[a])  ^  XOR over a in white of z(S, 1, L_k[a])  ^  (w ? z(S, 2, 0) : 0)
 *   key0   = key_0
 *   canon  = the unsigned minimum of key_0 .. key_7
 *   mask   = bit k set  <=>  key_k == canon            (the empty board: 255; never 0 for a valid row)
 *   canon_action(t) = min over k in mask of L_k[t]     for t in [0, N]  (L_k[N] = N: a pass stays a pass);  -1 for any other t
 * INVARIANCE: for every g among the eight tables, the record of the position moved by g with the target moved by g has the same
 * (canon, canon_action).
 * LEFT OUT: ko status and history are no part of the key, so two positions that differ only in what the ko approximation
 * (play.py:78-80) forbids share a key; so do positions reached by different move orders.  Colours are not swapped.
 *
 * sgo_keys_dev: row i keys record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], read in place;
 * d_target[i] is the action to map (d_target NULL: no targets; d_canon_action is then not written and may be NULL, and only
 * then).  Outputs [n] each.  A row whose record index is outside [0, n_records) gives key0 = canon = 0, mask = 0, canon_action
 * = -1.  ONE launch on `stream` (one half-wavefront per row), no allocation, no synchronisation, capturable; n == 0 is a no-op;
 * rows >= n are not written.  SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0, a NULL d_records or output. */
int sgo_keys_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_target,
                 uint64_t *d_key0, uint64_t *d_canon, int32_t *d_mask, int32_t *d_canon_action, void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order (copy in, run, copy back): for drop-in use and parity tests. */
int sgo_keys(int S, int n, const uint32_t *records, const int32_t *target, uint64_t *key0, uint64_t *canon, int32_t *mask,
             int32_t *canon_action);
/* The root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), keyed in place: one launch and one
 * copy back; waits for `stream`.  HOST arrays of n entries.  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is not a holding
 * session: that row's outputs are left as the caller filled them.  The context is only read; a slot may be listed repeatedly. */
int sgo_session_keys(sgo_ctx *ctx, int n, const int32_t *slots, int32_t *status, uint64_t *key0, uint64_t *canon, int32_t *mask,
                     void *stream);
/* Where sgo_keys_dev / sgo_keys take z from: 0 = a table z[2][N] in LDS, written once per workgroup (default), 1 = computed where
 * it is used (for A/B timing).  Same bits.  Returns the previous mode; other values only query. */
int sgo_keys_mode(int mode);

/* ---- chains and ladders: which stones are short of liberties, and can they be caught? ------------------------------------------- */
/* Per packed record: the liberty count of the chain on every point, the table of the chains with one or two liberties, and for
 * each of them the verdict of a small exhaustive reader (csrc/sgo_tactics.hip).  Everything is integer.
 * Inputs of a record, N = S * S: black / white = the bits a < N of planes 0 / 1; the to-play flag is read as sgo_keys_dev reads
 * it (the top bit of the last word of plane 0; NOT a stone); planes 2 / 3 = black / white one ply ago, bits a < N, used only for
 * the ko test at the root; padding bits and planes 4..15 are never read.
 * RULES: the project's.  A move is one ply of sgo_make_play (captures first, then suicide is executed).  A move of a side is
 * ALLOWED iff sgo_legal_moves allows it in the position with that side to move and `prev` = that side's stones one ply ago: a
 * point without an empty neighbour only if it captures, and the one-stone ko approximation (play.py:78-80) on `prev`.
 * LIBERTY MAP: libs[a] = min(255, liberties of the chain on a); 0 on an empty point.
 * CHAIN TABLE: the chains of either colour with 1 or 2 liberties in ascending order of their ANCHOR, the lowest point index of
 * the chain.  n_chains = their true number; the first max_chains (1..SGO_TACTICS_MAX_CHAINS) get a row
 *   int32[8] = {anchor, colour (+1 black, -1 white), size, liberties, status, attack_move, defend_move, nodes}.
 * THE READER: read(pos, t, attacker_to_move, prev, depth) -> captured | escaped.  t = the anchor, the DEFENDER is the colour on t,
 * the ATTACKER the other colour; the root has depth 0, a child depth + 1.  On entry: nodes += 1; if nodes >
 * SGO_TACTICS_MAX_NODES or depth > SGO_TACTICS_MAX_DEPTH the WHOLE QUERY ends unknown at once, whatever the branches above had
 * found.  L = the liberties of the chain on t.
 *   Attacker to move:  L >= 3: escaped.  L == 1: captured iff that liberty is allowed for the attacker.  L == 2: for each liberty
 *     a in ascending index order that is allowed: play it; the chain on t is gone: captured; else the stone just played was
 *     removed (suicide): next liberty; else recurse with the defender to move: captured if that returns captured.  No liberty
 *     gives captured: escaped.
 *   Defender to move:  candidates = the liberties of the chain on t, plus the single liberty of every attacker chain that touches
 *     it and has exactly one liberty; merged, ascending, duplicates dropped.  For each candidate that is allowed: play it; the
 *     chain on t is gone or has <= 1 liberty: next candidate; >= 3 liberties: escaped; exactly 2: recurse with the attacker to
 *     move: escaped if that returns escaped.  No candidate escapes: captured.
 *   A pass is never considered.  `prev` of a child = the child's mover's stones BEFORE the parent's move.  `prev` at the root =
 *   plane 2 (black) / 3 (white) of the record when the root's mover is the record's side to move; otherwise there is no ko
 *   restriction at the root.
 * QUERIES per chain row:  A = the attacker moves first, always run;  D = the defender moves first, run when L == 1, or L == 2 and
 * A returned captured.  status bits: 1 = A captured, 2 = D ran and returned captured, 4 = A unknown, 8 = D unknown, 16 = D ran.
 * attack_move = the first liberty by which A captures (L == 1: that liberty), -1 otherwise and when A is unknown; defend_move =
 * the first candidate by which D escapes, -1 otherwise.  nodes = the sum of the node counts of the queries that ran; the counter
 * restarts per query, and a query that ends unknown contributes its count at the moment it ended.  The traversal order is fixed,
 * so `nodes` pins it.
 *
 * sgo_tactics_dev: row i reads record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], in place.
 * d_libs uint8 [n][N], d_n_chains int32 [n], d_chains int32 [n][max_chains][8]; of a row's chain rows only the first
 * min(n_chains, max_chains) are written.  A row whose record index is outside [0, n_records) gives zero libs, n_chains = 0 and
 * untouched chain rows.  TWO launches on `stream` (k_tactics_chains, k_tactics_read), no allocation, no synchronisation,
 * capturable; n == 0 is a no-op; rows >= n are not written.  SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0, max_chains
 * outside [1, SGO_TACTICS_MAX_CHAINS], a NULL d_records or output. */
#define SGO_TACTICS_MAX_CHAINS 128
#define SGO_TACTICS_MAX_NODES 512
#define SGO_TACTICS_MAX_DEPTH 80
#define SGO_TACTICS_A_CAPTURED 1
#define SGO_TACTICS_D_CAPTURED 2
#define SGO_TACTICS_A_UNKNOWN 4
#define SGO_TACTICS_D_UNKNOWN 8
#define SGO_TACTICS_D_RAN 16
int sgo_tactics_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int max_chains, uint8_t *d_libs,
                    int32_t *d_n_chains, int32_t *d_chains, void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order (copy in, run, copy back): for drop-in use and parity
 * tests.  Chain rows beyond min(n_chains, max_chains) come back as the caller filled them. */
int sgo_tactics(int S, int n, const uint32_t *records, int max_chains, uint8_t *libs, int32_t *n_chains, int32_t *chains);
/* The root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), read in place; waits for `stream`.
 * HOST arrays: status [n], libs [n][N], n_chains [n], chains [n][max_chains][8].  status[i] = SGO_OK, or SGO_ERR_STATE for a slot
 * that is not a holding session: that row's outputs are left as the caller filled them.  The context is only read; a slot may be
 * listed repeatedly. */
int sgo_session_tactics(sgo_ctx *ctx, int n, const int32_t *slots, int max_chains, int32_t *status, uint8_t *libs, int32_t *n_chains,
                        int32_t *chains, void *stream);
/* Which of the two launches the calls above make: 0 = both (default), 1 = k_tactics_chains only (chain rows listed, not read
 * out), 2 = k_tactics_read only, on the table an earlier call left in the same buffers (for timing the kernels apart).  Returns
 * the previous stage; other values only query. */
int sgo_tactics_stage(int stage);

/* ---- unconditional life: which stones can never be captured, and which points are therefore settled? ------------------------------ */
/* Per packed record: the stones of either colour that no sequence of opponent moves captures even when their owner always passes
 * (Benson's pass-alive chains), and the points those chains enclose (csrc/sgo_life.hip).  Everything is integer; there are no
 * search caps and no "unknown".
 * Inputs of a record, N = S * S: black / white = the bits a < N of planes 0 / 1.  The to-play flag (the top bit of the last word
 * of plane 0) is NOT a stone and influences no output: the answer is the same for either side to move.  Padding bits and planes
 * 2..15 are never read.
 * For a colour X, the other colour called O:
 *   A CHAIN of X is a maximal 4-connected set of X stones.
 *   A REGION of X is a maximal 4-connected set of points that are NOT X: empty points and O stones together.
 *   Region R is VITAL to chain C iff R holds at least one empty point and EVERY empty point of R is 4-adjacent to a stone of C.
 *     O stones inside R do not matter.  A region without an empty point is vital to no chain (that occurs only in an illegal
 *     record).
 *   Let CC = all chains of X and RR = all regions of X.  Repeat until nothing is removed: remove from CC every chain that has
 *     fewer than two vital regions in RR; remove from RR every region that is 4-adjacent to a stone of a chain removed so far.
 *     The fixed point does not depend on the order of the removals; how many passes an implementation takes is not part of the
 *     interface.
 *   alive_X = the stones of the chains left in CC.
 *   terr_X  = the points (empty or O stones) of the regions left in RR that are vital to at least one chain left in CC.  A region
 *     that survives in RR without being vital to anyone is not territory: the open board next to a living wall is such a region.
 *   safe_X  = alive_X | terr_X.
 * The two colours are computed independently.  Illegal records (a chain without a liberty) go through the same definitions
 * without special cases.
 * OUTPUTS per listed row:
 *   sets   uint32 [4][sgo_plane_words(S)] = alive_black, alive_white, terr_black, terr_white; bit order as the legal bitsets of
 *          sgo_legal_dev; all bits a >= N are zero.
 *   counts int32 [8] = |alive_black|, |alive_white|, |terr_black|, |terr_white|, dead_white (white stones in terr_black),
 *          dead_black (black stones in terr_white), unsettled = N - |safe_black | safe_white|, margin = |safe_black| - |safe_white|.
 *
 * sgo_life_dev: row i reads record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], in place.
 * d_sets uint32 [n][4][sgo_plane_words(S)], d_counts int32 [n][8].  A row whose record index is outside [0, n_records) gets
 * all-zero sets and counts.  ONE launch on `stream` (one wavefront per row: a half per colour), no allocation, no synchronisation,
 * capturable; n == 0 is a no-op; rows >= n are not written.  SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0, a NULL
 * d_records or output. */
int sgo_life_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, uint32_t *d_sets, int32_t *d_counts,
                 void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order (copy in, run, copy back): for drop-in use and parity tests. */
int sgo_life(int S, int n, const uint32_t *records, uint32_t *sets, int32_t *counts);
/* The root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), read in place; waits for `stream`.
 * HOST arrays: status [n], sets [n][4][sgo_plane_words(S)], counts [n][8].  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is
 * not a holding session: that row's outputs are left as the caller filled them.  The context is only read; a slot may be listed
 * repeatedly. */
int sgo_session_life(sgo_ctx *ctx, int n, const int32_t *slots, int32_t *status, uint32_t *sets, int32_t *counts, void *stream);

/* ---- shape search: where does a local pattern occur in a position? ---------------------------------------------------------------- */
/* Per packed record: every place at which a small grid of black / white / empty / don't-care cells occurs, in any of its sixteen
 * variants (the eight symmetries of the grid, colours as drawn or exchanged), anchored to the board edges the shape names
 * (csrc/sgo_shapes.hip).  What a search for a joseki or a side shape in a game collection stands on.  Everything is integer.
 * N = S * S, NW = sgo_plane_words(S).
 * Inputs of a record: black / white = the bits a < N of planes 0 / 1.  The to-play flag (the top bit of the last word of plane 0) is
 * NOT a stone; at S = 5 it shares the only word with the stones.  Padding bits and planes 2..15 are never read.  A point is EMPTY
 * iff it is on the board and in neither set.
 * A SHAPE is a grid of w columns and h rows, 1 <= w, h <= S.  Each cell c[j][i] (row j < h counted from the top, column i < w
 * counted from the left, as board rows y and columns x are) is one of X, O, empty, don't-care.  Bit i of x[j] / o[j] / e[j] says
 * that cell (i, j) is X / O / must be empty; a cell in none of the three is don't-care.  `edges` is a bit set of the sides of the
 * grid that must lie on the board's edge: L = 1, T = 2, R = 4, B = 8.  `reserved` is 0. */
typedef struct sgo_shape { int32_t w, h, edges, reserved; uint32_t x[19], o[19], e[19]; } sgo_shape;
/* VARIANTS: sixteen, v = 8 * c + g.  c = 1 exchanges X and O (empty and don't-care cells stay).  g transforms the grid; the new
 * grid has w' columns and h' rows:
 *   g   w', h'   c'[j][i] =            new L, T, R, B = old
 *   0   w, h     c[j][i]               L, T, R, B
 *   1   h, w     c[i][j]               T, L, B, R
 *   2   w, h     c[j][w-1-i]           R, T, L, B
 *   3   w, h     c[h-1-j][i]           L, B, R, T
 *   4   h, w     c[h-1-i][j]           B, L, T, R
 *   5   w, h     c[h-1-j][w-1-i]       R, B, L, T
 *   6   h, w     c[i][w-1-j]           T, R, B, L
 *   7   h, w     c[h-1-i][w-1-j]       B, R, T, L
 * An edge flag stays with the side of the grid it was attached to (the column or row of cells that lay on that side is carried to
 * a side of the new grid, and the flag goes with it); should the last column of the table ever disagree with that rule, the rule
 * holds.  Variant v is DROPPED when an earlier variant v' < v has the same w', h', cells and edges: a symmetric shape is counted
 * once per place.  The others are KEPT.
 * MATCHING: a kept variant matches the record at (x0, y0), 0 <= x0 <= S - w', 0 <= y0 <= S - h', iff every X / O / empty cell
 * (i, j) finds the point (y0 + j) * S + x0 + i black / white / empty, and every edge flag of the variant holds: L: x0 == 0,
 * T: y0 == 0, R: x0 + w' == S, B: y0 + h' == S.  Don't-care cells ask nothing of their points, but the whole window lies on the
 * board, don't-care cells included.
 * OUTPUTS per listed row:
 *   hits  int32 [4] = n_hits  the number of triples (kept v, x0, y0) that match,
 *                     first   the smallest (v * S + y0) * S + x0 among them, -1 when there is none,
 *                     vmask   bit v set iff variant v matches somewhere,
 *                     n_cover the number of bits set in cover.
 *   cover uint32 [NW] = the union over all matches of the board points under cells that are not don't-care; bit order as the legal
 *         bitsets of sgo_legal_dev; all bits a >= N are zero.
 * A row whose record index is outside [0, n_records) gives {0, -1, 0, 0} and a zero cover.
 *
 * sgo_shape_compile: pure HOST arithmetic like sgo_sym_lut (no device is needed).  Writes the table the kernels read,
 * SGO_SHAPE_TABLE_WORDS words: words 0..15 = {S, n_kept, kept_mask (bit v: variant v is kept), w, h, edges, 0 ...}; the t-th kept
 * variant in ascending v occupies the 64 words from 16 + 64 * t: {v, w', h', edges', x'[19], o'[19], e'[19], 0, 0, 0}, where bit i
 * of x'[j] / o'[j] / e'[j] says that cell (i, j) of the variant must be black / white / empty (the exchange of c = 1 is already
 * made); unused slots and unused rows are zero.  SGO_ERR_ARG (nothing written): an unsupported S, w or h outside [1, S], a bit at a
 * column >= w or in a row >= h, a cell in two of the three sets, edges outside [0, 15], reserved != 0, a NULL argument. */
#define SGO_SHAPE_TABLE_WORDS (16 + 16 * 64)
int sgo_shape_compile(int S, const sgo_shape *shape, uint32_t *table);
/* Row i reads record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], in place, and matches the
 * table d_table [SGO_SHAPE_TABLE_WORDS] (DEVICE memory, as sgo_shape_compile wrote it for the same S).  d_hits int32 [n][4],
 * d_cover uint32 [n][sgo_plane_words(S)].  ONE launch on `stream` (one half-wavefront per row), no allocation, no synchronisation,
 * capturable; n == 0 is a no-op; rows >= n are not written.  The table is not read on the host: a table compiled for another size
 * is the caller's error here (the two entry points below compile it themselves and refuse a word 0 that is not S).  SGO_ERR_ARG:
 * an unsupported S, n < 0, n_records < 0, a NULL d_records, d_table or output. */
int sgo_shapes_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const uint32_t *d_table, int32_t *d_hits,
                   uint32_t *d_cover, void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order (compile, copy in, run, copy back): for drop-in use and
 * parity tests.  SGO_ERR_ARG as both of the above. */
int sgo_shapes(int S, int n, const uint32_t *records, const sgo_shape *shape, int32_t *hits, uint32_t *cover);
/* The root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), read in place; waits for `stream`.
 * HOST arrays: status [n], hits [n][4], cover [n][sgo_plane_words(S)].  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is not a
 * holding session: that row's outputs are left as the caller filled them.  The context is only read; a slot may be listed
 * repeatedly.  SGO_ERR_ARG: a shape sgo_shape_compile refuses at the context's size, a slot outside the context, a NULL argument. */
int sgo_session_shapes(sgo_ctx *ctx, int n, const int32_t *slots, const sgo_shape *shape, int32_t *status, int32_t *hits, uint32_t *cover,
                       void *stream);

/* ---- move outcomes: what would a stone on each point do? -------------------------------------------------------------------------- */
/* Per packed record and per point of the board: what ONE ply by a chosen side on that point captures, how large the mover's new
 * chain is and how many liberties it is left with, which of the mover's chains it joins, which opponent chains it puts in atari;
 * and a per-record summary (csrc/sgo_moves.hip).  What a review tool, a record statistic and a GTP front end ask of a move
 * without playing it.  Everything is integer.  N = S * S.
 * Inputs of a record: black / white = the bits a < N of planes 0 / 1; the to-play flag is read as sgo_keys_dev reads it (the top
 * bit of the last word of plane 0; NOT a stone, at S = 5 it shares the only word with the stones); planes 2 / 3 = black / white
 * one ply ago, bits a < N, used only for the ko test; padding bits and planes 4..15 are never read.
 * `side` chooses the MOVER M.  side = 0: M is the record's side to move (white iff the flag is set), and `prev` = M's stones one
 * ply ago (plane 2 for black, plane 3 for white).  side = 1: M is the other colour; there is no `prev` and so no ko restriction
 * (the convention of the tactics reader's root).  "own" = M's stones, "opp" = the other colour's.  A CHAIN is a maximal
 * 4-connected set of stones of one colour; its LIBERTIES are the empty points 4-adjacent to it.
 * PER POINT a (index y * S + x) a row int16[8] = {flags, captured, size, libs, joined, weakest, ataris, atari_stones}:
 *   flags & SGO_MOVES_OCCUPIED: a holds a stone.  Words 1..7 are then 0, and ALLOWED and SUICIDE are never set.
 *   flags & SGO_MOVES_KO: `prev` exists, prev & ~own is exactly one point, and that point is a.  Stated literally: in a constructed
 *     record it may coincide with OCCUPIED (an opp stone on a).
 *   flags & SGO_MOVES_ALLOWED: bit a of sgo_legal_moves for M to move with that `prev` -- the project's rule: a point without an
 *     empty neighbour only if it captures, and the one-stone ko approximation (play.py:78-80), i.e. never a KO point.
 *   For an EMPTY a let P' be the position after one ply of sgo_make_play by M on a (captures first, then suicide is executed); the
 *   ply is played whether or not it is ALLOWED.
 *   captured = the number of opp stones of the record that are gone in P'.
 *   flags & SGO_MOVES_SUICIDE: a is empty in P'.  Then size = libs = ataris = atari_stones = 0.
 *   size = the stones of M's chain on a in P';  libs = its liberties in P' (no saturation).
 *   joined = the number of DISTINCT own chains of the position BEFORE the ply that have a stone 4-adjacent to a (0..4).
 *   weakest = the smallest liberty count among those chains BEFORE the ply (a itself counts as a liberty of theirs); 0 when
 *     joined is 0.
 *   ataris = the number of DISTINCT opp chains of P' that have a stone 4-adjacent to a and exactly one liberty in P';
 *   atari_stones = the stones of those chains together.
 *   (So an empty point with no stone among its neighbours has {ALLOWED unless KO, 0, 1, its on-board neighbours, 0, 0, 0, 0}.)
 * PER RECORD counts int32[8]; entries 0..6 are taken over the ALLOWED points only:
 *   0 allowed           the number of ALLOWED points
 *   1 capturing         points with captured > 0
 *   2 max_captured      the largest captured
 *   3 max_capture_move  the lowest a that reaches it; -1 when nothing captures
 *   4 self_atari        points with libs == 1 and captured == 0
 *   5 atari_giving      points with ataris > 0
 *   6 escapes           points with weakest == 1 and libs >= 2
 *   7 forbidden_sound   EMPTY points with none of ALLOWED, KO and SUICIDE: the moves the inherited rule forbids although the stone
 *                       would stand (no empty neighbour, captures nothing, joins a chain that keeps a liberty)
 *
 * sgo_moves_dev: row i reads record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], in place.
 * d_moves int16 [n][N][8] (16-byte aligned: a point's row is one store), d_counts int32 [n][8].  A row whose record index is outside
 * [0, n_records) gets all-zero rows and counts.  ONE launch on `stream` (one half-wavefront per row), no allocation, no
 * synchronisation, capturable; n == 0 is a no-op; rows >= n are not written.  SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0,
 * side outside {0, 1}, a NULL d_records or output, a d_moves that is not 16-byte aligned. */
#define SGO_MOVES_ALLOWED 1
#define SGO_MOVES_OCCUPIED 2
#define SGO_MOVES_KO 4
#define SGO_MOVES_SUICIDE 8
int sgo_moves_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int side, int16_t *d_moves,
                  int32_t *d_counts, void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order (copy in, run, copy back): for drop-in use and parity tests.
 * No alignment is asked of host buffers. */
int sgo_moves(int S, int n, const uint32_t *records, int side, int16_t *moves, int32_t *counts);
/* The root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), read in place; waits for `stream`.
 * HOST arrays: status [n], moves [n][N][8], counts [n][8].  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is not a holding
 * session: that row's outputs are left as the caller filled them.  The context is only read; a slot may be listed repeatedly.
 * No alignment is asked of the host arrays: the kernel writes into the context's own staging block, at a 16-byte boundary, and the
 * rows are copied out of it.  SGO_ERR_ARG: side outside {0, 1}, a slot outside the context, a NULL argument. */
int sgo_session_moves(sgo_ctx *ctx, int n, const int32_t *slots, int side, int32_t *status, int16_t *moves, int32_t *counts,
                      void *stream);

/* ---- securing moves: what does one more stone make pass-alive? ----------------------------------------------------------------------- */
/* Per packed record and per point of the board: the unconditional life of the position after ONE ply by a chosen side on that point,
 * and a per-record summary with the life sets before and after the best such ply (csrc/sgo_secure.hip).  The question a player asks
 * of a group -- is it safe, and if not, which move makes it safe -- in its exact one-ply form: play the stone, then prove what can
 * never be captured.  Everything is integer; there are no search caps and no "unknown".  N = S * S.
 * Inputs of a record and `side` are read exactly as sgo_moves_dev reads them ("move outcomes" above): black / white = the bits a < N
 * of planes 0 / 1; the to-play flag is the top bit of the last word of plane 0 (NOT a stone); planes 2 / 3 = black / white one ply
 * ago, bits a < N, used only for the ko test; padding bits and planes 4..15 are never read.  side = 0: the MOVER M is the record's
 * side to move (white iff the flag is set), and `prev` = M's stones one ply ago.  side = 1: M is the other colour; there is no `prev`
 * and so no ko restriction.  "own" = M's stones, "opp" = the other colour's.
 * alive_X, terr_X and safe_X of a position are those of the "unconditional life" section above, with X = M and O = the other colour;
 * the position's side to move plays no part in them.
 * PER POINT a (index y * S + x) a row int16[4] = {flags, alive, terr, dead}:
 *   flags: SGO_MOVES_OCCUPIED, SGO_MOVES_KO, SGO_MOVES_ALLOWED and SGO_MOVES_SUICIDE with the meanings of the "move outcomes" section
 *     (the same constants).  On an OCCUPIED point words 1..3 are 0, and ALLOWED and SUICIDE are never set.
 *   For an EMPTY a let P' be the position after one ply of sgo_make_play by M on a (captures first, then suicide is executed); the
 *   ply is played whether or not it is ALLOWED.
 *   alive = |alive_M(P')|;  terr = |terr_M(P')|;  dead = the number of opp stones of P' inside terr_M(P').
 *   These are literally the life definitions on P': there are no special cases for a suicide (P' then lacks the stone and the
 *   mover's chain it killed) or for an illegal record.
 * PER RECORD counts int32[8], with P the record's position, base = |alive_M(P)| + |terr_M(P)| and gain(a) = alive + terr - base:
 *   0 base_alive   |alive_M(P)|
 *   1 base_terr    |terr_M(P)|
 *   2 base_dead    the opp stones of P inside terr_M(P)
 *   3 allowed      the number of ALLOWED points
 *   4 securing     ALLOWED points with gain > 0
 *   5 best_gain    the largest gain over the ALLOWED points; 0 when there are none; may be negative
 *   6 best_move    the lowest ALLOWED a that reaches best_gain; -1 when allowed == 0
 *   7 harmful      ALLOWED points with gain < 0
 * PER RECORD sets uint32 [4][sgo_plane_words(S)] = alive_M(P), terr_M(P), alive_M(P*), terr_M(P*), where P* is P' of best_move, or P
 *   itself when best_move is -1; bit order as the life sets; all bits a >= N are zero.
 *
 * sgo_secure_dev: row i reads record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], in place.
 * d_table int16 [n][N][4] (8-byte aligned: a point's row is one store), d_sets uint32 [n][4][sgo_plane_words(S)], d_counts int32
 * [n][8].  A row whose record index is outside [0, n_records) gets all-zero table rows, sets and counts (best_move 0 too).  TWO
 * launches on `stream` (a half-wavefront per row and empty point, then a wavefront per row), no allocation, no synchronisation,
 * capturable; n == 0 is a no-op; rows >= n are not written.  SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0, side outside
 * {0, 1}, a NULL d_records or output, a d_table that is not 8-byte aligned. */
int sgo_secure_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int side, int16_t *d_table,
                   uint32_t *d_sets, int32_t *d_counts, void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order (copy in, run, copy back): for drop-in use and parity tests.
 * No alignment is asked of host buffers. */
int sgo_secure(int S, int n, const uint32_t *records, int side, int16_t *table, uint32_t *sets, int32_t *counts);
/* The root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), read in place; waits for `stream`.
 * HOST arrays: status [n], table [n][N][4], sets [n][4][sgo_plane_words(S)], counts [n][8].  status[i] = SGO_OK, or SGO_ERR_STATE
 * for a slot that is not a holding session: that row's outputs are left as the caller filled them.  The context is only read; a
 * slot may be listed repeatedly.  No alignment is asked of the host arrays.  SGO_ERR_ARG: side outside {0, 1}, a slot outside the
 * context, a NULL argument. */
int sgo_session_secure(sgo_ctx *ctx, int n, const int32_t *slots, int side, int32_t *status, int16_t *table, uint32_t *sets,
                       int32_t *counts, void *stream);
/* How the first launch deals a row's empty points to workgroups, for A/B timing; the words written are the same.  Bits 0..15: the
 * workgroups per row (0 = chosen from n, the default; capped at ceil(N / 2)).  Bit 16: 0 = half h of pair k takes the (2k + h)-th
 * EMPTY point (default), 1 = it takes point 2k + h and idles on a stone.  Returns the previous mode; a negative value, or one with
 * other bits set or more than 1024 workgroups, only queries. */
int sgo_secure_mode(int mode);

/* ---- life and death: can an enclosed chain be killed when both sides play? ---------------------------------------------------------- */
/* Per packed record: the table of the enclosed chains (or the one chain asked for), the region each is read in, and for each the
 * verdict of an exhaustive reader bounded by that region in which BOTH sides play, with unconditional life as the terminal for
 * "lives" (csrc/sgo_solve.hip).  Everything is integer.  N = S * S.
 * Inputs of a record: as sgo_tactics_dev reads them ("chains and ladders" above): black / white = the bits a < N of planes 0 / 1; the
 * to-play flag is the top bit of the last word of plane 0 (NOT a stone); planes 2 / 3 = black / white one ply ago, bits a < N, used
 * only for the ko test at the root; padding bits and planes 4..15 are never read.
 * TARGET: a chain (a maximal 4-connected set of stones of one colour), named by any of its points.  Its ANCHOR t is its lowest point
 * index.  The DEFENDER is its colour X, the ATTACKER the other colour O.
 * DEFAULT REGION M of a target: R = the maximal 4-connected set of points that are NOT O stones and that contains the target (the
 * REGION of O of the "unconditional life" section that holds it: X stones and empty points together).  M = R plus every O chain that
 * has at least one liberty and whose EVERY liberty lies in R.  (Without these the points of attacker stones captured inside an eye
 * would become unplayable, and every nakade would be misread.  An O chain without a liberty occurs only in an illegal record and is
 * not added.)  A caller may give M explicitly instead; it is masked to the board and otherwise taken as it is.  Moves of both
 * sides are confined to the points of M that are empty at the time of the move.  region_empty = the empty points of M at the root.
 * ALLOWED, for the side to move with `prev` = that side's stones one ply ago:  rules = 0: exactly the ALLOWED of the "chains and
 * ladders" section (sgo_legal_moves).  rules = 1 ("sound"): additionally the points the "move outcomes" section calls
 * forbidden_sound: EMPTY points that are not the KO point (prev & ~own is exactly one point, and it is that point) and on which the
 * stone stands after one ply of sgo_make_play.  The inherited rule forbids a point without an empty neighbour that captures nothing
 * even when it joins a chain that keeps a liberty, and that is otherwise the connecting move that saves a group.  EVERY VERDICT HOLDS
 * FOR THE CHOSEN RULE SET.
 * THE READER: read(pos, mover, prev, depth) -> DEAD | ALIVE; the root has depth 0, a child depth + 1.  On entry: nodes += 1; if nodes >
 * max_nodes or depth > SGO_SOLVE_MAX_DEPTH the WHOLE QUERY ends unknown at once, whatever the branches above had found.  Then, if
 * the stone on t belongs to alive_X(pos) of the "unconditional life" section (computed on the whole board of pos): ALIVE.
 *   Attacker to move:  for every ALLOWED empty point a of M in ascending index order: play it (one ply of sgo_make_play); the stone on
 *     t is gone: DEAD; else the stone just played is gone: next point; else recurse with the defender to move: DEAD if that returns
 *     DEAD.  Then, ONLY while the ko test forbids the attacker an empty point of M (prev & ~own is exactly one point, and that point
 *     is an empty point of M), the WAIT, encoded as move N: the same stones, the defender to move, depth + 1: DEAD if that returns
 *     DEAD.  Otherwise ALIVE.  The attacker never passes otherwise (a pass could only be answered by a pass).  The wait is not a
 *     convenience: the ko test forbids the replay on a point where exactly ONE stone was just captured whether or not that is a ko,
 *     and the kill of a straight three, a bulky five or a square four ends with such a replay when no other point of M is left.
 *   Defender to move:  for every ALLOWED empty point a of M in ascending index order: play it; the stone on t or the stone just played
 *     is gone: next point; else recurse with the attacker to move: ALIVE if that returns ALIVE.  Then the PASS, encoded as move N: the
 *     same stones, the attacker to move, depth + 1: ALIVE if that returns ALIVE.  Otherwise DEAD.  The pass is what reads a seki as
 *     "not killable".
 *   `prev` of a child = the child's mover's stones BEFORE the parent's move, and `prev` at the root = plane 2 (black) / 3 (white) of the
 *   record when the root's mover is the record's side to move, otherwise no ko restriction: exactly as the tactics reader.  After a pass
 *   the child's `prev` equals its stones, so the formula leaves no ko restriction.
 * WHAT IS LEFT OUT.  No transposition table and no move-ordering heuristics: the traversal order is fixed, so the node counts pin it,
 * and a region of a dozen empty points is about what the budgets reach.  Ko is the one-ply approximation: the defender may pass and
 * retake, and the attacker has no ko threats -- its wait is no threat: the defender may use that ply to settle the ko, and only a
 * defender that passes too lets the ban lapse.  A chain is judged ALONE, not its group: a neighbour chain of the same colour may die
 * while the target lives.  An ALIVE verdict means "the attacker cannot capture it inside M"; it does not mean "two eyes" -- an
 * attacker move outside M is not read, so M must be closed for the verdict to say something about the game.
 * QUERIES per row:  A = the attacker moves first, always run;  D = the defender moves first, run only when A returned DEAD.  The node
 * counter restarts per query, and a query that ends unknown reports its count at the moment it ended.
 * RESULT ROW int32[8] = {anchor, colour (+1 black, -1 white), region_empty, status, kill_move, live_move, nodes_A, nodes_D}.
 *   kill_move = the first root move by which A kills (N = the wait), -1 otherwise and when A is unknown.
 *   live_move = the first root candidate by which
 *   D lives (N = the pass), -1 otherwise.  status bits: 1 = A returned DEAD, 2 = D ran and returned DEAD, 4 = A unknown, 8 = D unknown,
 *   16 = D ran, 32 = SGO_SOLVE_OPEN: region_empty is 0 or greater than max_region, no query runs (moves -1, nodes 0),
 *   64 = SGO_SOLVE_NO_STONE: an asked point is empty or outside the board; anchor and moves are -1, the other words 0, the region empty.
 *
 * sgo_solve_dev: row i reads record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], in place.
 * d_n_targets int32 [n], d_rows int32 [n][max_targets][8], d_regions uint32 [n][max_targets][sgo_plane_words(S)]: the M used, in the
 * bit order of the legal bitsets, bits a >= N zero.  Of a row's table rows and region sets only the first min(n_targets, max_targets)
 * are written.  d_ask NULL, or d_ask[i] < 0: ENUMERATE for that row: the table lists, in ascending anchor order, the chains of either
 * colour that are not in alive_X of the record and whose default region has 1..max_region empty points; n_targets = their true number.
 * d_ask[i] >= 0: exactly one table row, for the chain on that point (n_targets = 1), read in row i of d_region [n][sgo_plane_words(S)]
 * when d_region is not NULL, otherwise in its default region.  A row whose record index is outside [0, n_records) gives n_targets = 0
 * and untouched rows.  TWO launches on `stream` (k_solve_targets, k_solve_read), no allocation, no synchronisation, capturable; n ==
 * 0 is a no-op; rows >= n are not written.  SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0, rules outside {0, 1}, max_region
 * outside [1, SGO_SOLVE_MAX_REGION], max_nodes outside [1, SGO_SOLVE_MAX_NODES], max_targets outside [1, SGO_SOLVE_MAX_TARGETS], a NULL
 * d_records or output.  SGO_SOLVE_MAX_NODES bounds the longest launch a single query can cause: measured on one MI355X
 * (profiles/solve_ab.json) a node takes 4.4 us at 19x19, a query that spends all 65 536 nodes 0.29 s, so the cap stands as it is. */
#define SGO_SOLVE_MAX_REGION 32
#define SGO_SOLVE_MAX_NODES 65536
#define SGO_SOLVE_MAX_TARGETS 64
#define SGO_SOLVE_MAX_DEPTH 80
#define SGO_SOLVE_A_DEAD 1
#define SGO_SOLVE_D_DEAD 2
#define SGO_SOLVE_A_UNKNOWN 4
#define SGO_SOLVE_D_UNKNOWN 8
#define SGO_SOLVE_D_RAN 16
#define SGO_SOLVE_OPEN 32
#define SGO_SOLVE_NO_STONE 64
int sgo_solve_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask,
                  const uint32_t *d_region, int rules, int max_region, int max_nodes, int max_targets, int32_t *d_n_targets,
                  int32_t *d_rows, uint32_t *d_regions, void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order (copy in, run, copy back): for drop-in use and parity tests.
 * ask (or NULL) int32 [n], region (or NULL) uint32 [n][sgo_plane_words(S)].  Table rows and region sets beyond min(n_targets,
 * max_targets) come back as the caller filled them. */
int sgo_solve(int S, int n, const uint32_t *records, const int32_t *ask, const uint32_t *region, int rules, int max_region, int max_nodes,
              int max_targets, int32_t *n_targets, int32_t *rows, uint32_t *regions);
/* The root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), read in place; waits for `stream`.
 * HOST arrays: ask (or NULL) [n], region (or NULL) [n][sgo_plane_words(S)], status [n], n_targets [n], rows [n][max_targets][8],
 * regions [n][max_targets][sgo_plane_words(S)].  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is not a holding session: that
 * row's outputs are left as the caller filled them, as are the table rows beyond min(n_targets, max_targets) of every row.  The
 * context is only read; a slot may be listed repeatedly.  SGO_ERR_ARG: the bounds of sgo_solve_dev, a slot outside the context, a
 * NULL slot list or output. */
int sgo_session_solve(sgo_ctx *ctx, int n, const int32_t *slots, const int32_t *ask, const uint32_t *region, int rules, int max_region,
                      int max_nodes, int max_targets, int32_t *status, int32_t *n_targets, int32_t *rows, uint32_t *regions, void *stream);

/* ---- capturing races: which of two chains in contact falls first? ------------------------------------------------------------------ */
/* Per packed record: the table of the pairs of a black and a white chain that lean on each other short of liberties (or the one pair
 * asked for), the region each pair is read in, and for EACH of the two chains the verdict of an exhaustive reader bounded by that
 * region in which both sides play and the other chain can be captured back (csrc/sgo_race.hip).  Everything is integer.  N = S * S.
 * Inputs of a record: exactly as sgo_solve_dev reads them ("life and death" above): black / white = the bits a < N of planes 0 / 1;
 * the to-play flag is NOT a stone; planes 2 / 3 are used only for the ko test at the root; padding bits and planes 4..15 are never
 * read.  rules in {0, 1} and ALLOWED have the meaning of the "life and death" section.
 * PAIR: a black chain B and a white chain W (maximal 4-connected sets of stones of one colour).  Their ANCHORS are the lowest point
 * index of each; lib(B), lib(W) are their liberties (the empty points 4-adjacent to a stone of the chain).  They are IN CONTACT when a
 * stone of one is 4-adjacent to a stone of the other, or when lib(B) & lib(W) is not empty (a race across a shared liberty without
 * touching stones is a race too).
 * DEFAULT REGION M of a pair: M0 = lib(B) | lib(W).  M1 = M0 plus every empty point 4-adjacent to a point of M0 (the second-order
 * liberties, so that an extension along a corridor stays readable).  M = M1 plus every chain other than B and W, of either colour,
 * that has at least one liberty and whose EVERY liberty lies in M1 (the rule of the "life and death" section, for its reason: without
 * it the points of stones captured inside an eye become unplayable and every nakade race is misread; the test is against M1, in one
 * pass, not iterated).  A caller may give M explicitly instead; it is masked to the board and otherwise taken as it is.
 * region_empty = the empty points of M at the root.  Moves of both sides are confined to the points of M that are empty at the time
 * of the move.
 * THE READER: read(pos, mover, prev, depth) -> CAUGHT | SAFE, for one DEFENDER racer, the stone on point tD (the anchor of its chain at
 * the root); the ATTACKER's racer is the stone on point tA (the other anchor).  Node counting, the rule that ends the WHOLE QUERY
 * unknown (nodes > max_nodes or depth > SGO_RACE_MAX_DEPTH), the ascending candidate order, the `prev` of a child and of the root and
 * the pass after which no ko restriction is left are word for word those of the "life and death" reader.  On entry, after the node
 * is counted: L = the liberties of the chain on tD on the whole board.  If L has a point outside M, or |L| > max_libs: SAFE (the
 * racer has escaped).  The unconditional-life test of the "life and death" reader is NOT made here.
 *   Attacker to move:  for every ALLOWED empty point a of M in ascending index order: play it; the stone on tD is gone: CAUGHT; else
 *     the stone just played is gone: next point; else recurse with the defender to move: CAUGHT if that returns CAUGHT.  Then the WAIT
 *     (move N) under exactly the condition of the "life and death" reader (the ko test forbids the attacker an empty point of M):
 *     CAUGHT if that returns CAUGHT.  Otherwise SAFE.  The attacker never passes otherwise.
 *   Defender to move:  for every ALLOWED empty point a of M in ascending index order: play it; the stone on tD or the stone just played
 *     is gone: next point; else the stone on tA is gone (the defender captured the attacker's racer): SAFE with move a; else recurse
 *     with the attacker to move: SAFE if that returns SAFE.  Then the PASS (move N): SAFE if that returns SAFE; this is what reads a
 *     seki as SAFE for both.  Otherwise CAUGHT.
 * WHAT IS LEFT OUT.  No transposition table and no move ordering: the traversal is fixed and the node counts pin it.  Ko is the
 * one-ply approximation.  A racer whose stone on tA is captured has lost: a snapback under the captured stones is not read.  Moves
 * outside M are not read.  Helper chains matter only through the inner-chain rule.  A verdict is about the two CHAINS, not their groups.
 * QUERIES per pair, for each racer as the defender:  A = the attacker moves first, always run;  D = the defender moves first, run only
 * when A returned CAUGHT.  The node counter restarts per query; a pair costs up to four queries.
 * RESULT ROW int32[16] = {anchor_b, anchor_w, |lib(B)|, |lib(W)|, |lib(B) & lib(W)|, region_empty, status, 0 (reserved, written),
 *   catch_b, save_b, catch_w, save_w, nodes of A and of D for the black racer, nodes of A and of D for the white racer}.
 *   catch_b = the first root move by which white, moving first, catches the black racer (N = the wait); save_b = the first root
 *   candidate by which black, moving first, saves it (N = the pass); catch_w / save_w the same with the colours exchanged.  Moves are
 *   -1 and nodes 0 under the conditions of the solve row (no such move, the query unknown or not run).
 *   status: for the black racer SGO_RACE_A_CAUGHT 1, SGO_RACE_D_CAUGHT 2, SGO_RACE_A_UNKNOWN 4, SGO_RACE_D_UNKNOWN 8, SGO_RACE_D_RAN 16;
 *   for the white racer the same five shifted left by SGO_RACE_WHITE_SHIFT = 8.  SGO_RACE_OPEN: region_empty is 0 or above max_region,
 *   no query runs.  SGO_RACE_NO_PAIR: an asked point is empty or off the board, or the two asked stones have one colour; anchors and
 *   moves are -1, the other words 0, the region empty.
 *   A racer is `safe` when A is not CAUGHT, `unsettled` when A is CAUGHT and D is not, `caught` when both are, `unknown` when a query
 *   of it ended unknown.
 *
 * sgo_race_dev: row i reads record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], in place.
 * d_n_pairs int32 [n], d_rows int32 [n][max_pairs][16], d_regions uint32 [n][max_pairs][sgo_plane_words(S)]: the M used, bits a >= N
 * zero.  d_ask NULL, or d_ask[i][0] < 0 (d_ask int32 [n][2]): ENUMERATE: every pair in contact with 1 <= |lib(B)| <= max_libs, 1 <=
 * |lib(W)| <= max_libs and region_empty in 1..max_region, in ascending (anchor_b, anchor_w) order; n_pairs = their true number; only
 * min(n_pairs, max_pairs) rows and region sets are written and everything behind them stays untouched.  d_ask[i] = {p, q} with p >=
 * 0: exactly one row (n_pairs = 1), for the chains on p and q in either colour order; contact and the liberty bounds are not required
 * (the reader's own terminal speaks when a racer has more than max_libs liberties); read in row i of d_region
 * [n][sgo_plane_words(S)] when that is not NULL.  A row whose record index is outside [0, n_records) gives n_pairs = 0 and untouched
 * rows.  TWO launches on `stream` (k_race_pairs, k_race_read), no allocation, no synchronisation, capturable; n == 0 is a no-op; rows
 * >= n are not written.  SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0, rules outside {0, 1}, max_libs outside [1,
 * SGO_RACE_MAX_LIBS], max_region outside [1, SGO_RACE_MAX_REGION], max_nodes outside [1, SGO_RACE_MAX_NODES], max_pairs outside [1,
 * SGO_RACE_MAX_PAIRS], a NULL d_records or output.  SGO_RACE_MAX_NODES bounds the longest launch a single query can cause: measured on
 * one MI355X (profiles/race_ab.json) a node takes 3.7 us at 19x19 with one racer of the pair reading and 5.2 us at 9x9 with both, and
 * a query that spends 65 536 nodes took 0.32 s there, longer than the 0.29 s the "life and death" cap allows; so the cap is HALF of
 * that section's, 32 768 nodes. */
#define SGO_RACE_MAX_LIBS 8
#define SGO_RACE_MAX_REGION 32
#define SGO_RACE_MAX_NODES 32768
#define SGO_RACE_MAX_PAIRS 64
#define SGO_RACE_MAX_DEPTH 80
#define SGO_RACE_A_CAUGHT 1
#define SGO_RACE_D_CAUGHT 2
#define SGO_RACE_A_UNKNOWN 4
#define SGO_RACE_D_UNKNOWN 8
#define SGO_RACE_D_RAN 16
#define SGO_RACE_WHITE_SHIFT 8
#define SGO_RACE_OPEN (1 << 16)
#define SGO_RACE_NO_PAIR (1 << 17)
int sgo_race_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask,
                 const uint32_t *d_region, int rules, int max_libs, int max_region, int max_nodes, int max_pairs, int32_t *d_n_pairs,
                 int32_t *d_rows, uint32_t *d_regions, void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order (copy in, run, copy back): for drop-in use and parity tests.
 * ask (or NULL) int32 [n][2], region (or NULL) uint32 [n][sgo_plane_words(S)].  Table rows and region sets beyond min(n_pairs,
 * max_pairs) come back as the caller filled them. */
int sgo_race(int S, int n, const uint32_t *records, const int32_t *ask, const uint32_t *region, int rules, int max_libs, int max_region,
             int max_nodes, int max_pairs, int32_t *n_pairs, int32_t *rows, uint32_t *regions);
/* The root positions of the listed HOLDING session slots of `ctx`, read in place; waits for `stream`.  HOST arrays: ask (or NULL)
 * [n][2], region (or NULL) [n][sgo_plane_words(S)], status [n], n_pairs [n], rows [n][max_pairs][16], regions
 * [n][max_pairs][sgo_plane_words(S)].  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is not a holding session: that row's
 * outputs are left as the caller filled them, as are the table rows beyond min(n_pairs, max_pairs) of every row.  The context is only
 * read; a slot may be listed repeatedly.  SGO_ERR_ARG: the bounds of sgo_race_dev, a slot outside the context, a NULL slot list or
 * output. */
int sgo_session_race(sgo_ctx *ctx, int n, const int32_t *slots, const int32_t *ask, const uint32_t *region, int rules, int max_libs,
                     int max_region, int max_nodes, int max_pairs, int32_t *status, int32_t *n_pairs, int32_t *rows, uint32_t *regions,
                     void *stream);

/* ---- connections: can two chains of one colour be cut apart? ------------------------------------------------------------------------ */
/* Per packed record: the table of the pairs of two chains of ONE colour that are near each other (or the one pair asked for), the
 * region each pair is read in, the verdict of an exhaustive reader bounded by that region on whether the other colour can keep the two
 * from becoming one chain, and the map of the GROUPS the connected pairs tie the chains into (csrc/sgo_connect.hip).  This is what
 * turns the chains of the three sections above into groups.  Everything is integer.  N = S * S.
 * Inputs of a record, rules in {0, 1}, ALLOWED, `prev` and the ko test: word for word those of the "life and death" and "capturing
 * races" sections: black / white = the bits a < N of planes 0 / 1; the to-play flag is NOT a stone; planes 2 / 3 are used only for the
 * ko test at the root; padding bits and planes 4..15 are never read.  Node counting, the rule that ends the WHOLE QUERY unknown (nodes
 * > max_nodes or depth > SGO_CONNECT_MAX_DEPTH) and the ascending candidate order are those sections' too.
 * PAIR: two different chains X and Y of the SAME colour C; their ANCHORS are their lowest points, anchor_x < anchor_y.  The DEFENDER
 * is C and wants to make them one chain; the ATTACKER is the other colour.  lib(X), lib(Y) are their liberties; nbr(s) is the set of
 * points 4-adjacent to a point of s.
 * LINK POINTS K = (lib(X) & lib(Y)) | (lib(X) & nbr(lib(Y))) | (lib(Y) & nbr(lib(X))): the common liberties, and the liberties of one
 * chain that are 4-adjacent to a liberty of the other.  That covers the diagonal, the one-point jump, the bamboo joint, the knight's
 * move and the two-point jump.  A CUTTING CHAIN is an attacker chain Z that is 4-adjacent to a stone of X and to a stone of Y with 1
 * <= |lib(Z)| <= cut_libs; its liberties join K, and Z itself joins M, so that the points it leaves when captured are playable.  The
 * pair is NEAR when K is not empty.
 * DEFAULT REGION M: M1 = K plus the empty points 4-adjacent to K.  M = M1 plus the cutting chains plus every chain other than X, Y and
 * the cutting chains, of either colour, that has at least one liberty and whose EVERY liberty lies in M1 (the inner-chain rule of the
 * two sections above: one pass, tested against M1).  A caller may give M explicitly instead; it is masked to the board and otherwise
 * taken as it is.  region_empty = the empty points of M at the root.  Moves of both sides are confined to the points of M that are
 * empty at the time of the move.
 * THE READER: read(pos, mover, prev, depth) -> JOINED | CUT, for the stones on tx and ty (the two anchors at the root).  On entry,
 * after the node is counted: if the chain on tx holds ty: JOINED.
 *   Attacker to move:  for every ALLOWED empty point a of M in ascending index order: play it; the stone on tx or on ty is gone: CUT
 *     with move a; else the stone just played is gone: next point; else recurse with the defender to move: CUT if that returns CUT.
 *     Then the attacker's PASS (move N), ALWAYS tried, last: the same stones, the defender to move, `prev` as after a pass: CUT if that
 *     returns CUT.  Otherwise JOINED.  The pass is always allowed, not only under a ko ban: a cutter must not be forced into a
 *     self-atari that the defender captures to connect.  The wait of the "life and death" reader is the special case of this pass.
 *   Defender to move:  for every ALLOWED empty point a of M in ascending index order: play it; the stone on tx, on ty or on a is gone:
 *     next point; else recurse with the attacker to move: JOINED if that returns JOINED.  Otherwise CUT.  The defender never passes:
 *     its pass could be answered by a pass, and two chains that are not one chain are not joined.
 *   So JOINED means "the defender can force ONE standing chain inside M whatever the attacker plays there, a tenuki included".
 * QUERIES per pair:  A = the attacker moves first, always run;  D = the defender moves first, run only when A returned CUT.  The node
 * counter restarts per query.  A pair is `connected` when A is JOINED, `unsettled` when A is CUT and D is JOINED, `cut` when both are
 * CUT, `unknown` when a query ended unknown, `open` when region_empty is 0 or above max_region (no query runs), `no_pair` see below.
 * RESULT ROW int32[12] = {anchor_x, anchor_y, colour (+1 black, -1 white), |lib(X) & lib(Y)|, |K|, region_empty, status,
 *   n_cutting_chains, cut_move, join_move, nodes_A, nodes_D}.  cut_move = the first root move by which A cuts (N = the pass);
 *   join_move = the first root candidate by which D joins.  Moves are -1 and nodes 0 under the conditions of the solve row (no such
 *   move, the query unknown or not run).  status bits: SGO_CONNECT_A_CUT 1, SGO_CONNECT_D_CUT 2, SGO_CONNECT_A_UNKNOWN 4,
 *   SGO_CONNECT_D_UNKNOWN 8, SGO_CONNECT_D_RAN 16, SGO_CONNECT_OPEN, SGO_CONNECT_NO_PAIR: an asked point is empty or off the board, the
 *   two stones differ in colour, or they are one chain already; anchors and moves are then -1, the other words 0, the region empty.
 * GROUPS: d_groups int16 [n][N]: for a stone the lowest anchor among the chains its chain is tied to through `connected` pairs -- the
 *   transitive closure over the WRITTEN table rows of that row; for an empty point -1.  Both colours stand in the one map.
 *   d_group_counts int32 [n][4] = {chains, groups, connected pairs among the written rows, flags}; flag 1: n_pairs > max_pairs, the table
 *   was cut, so the partition may be too fine; flag 2: some written pair is `unknown` or `open`; such pairs do NOT tie.
 * WHAT IS LEFT OUT.  No transposition table and no move ordering: the traversal is fixed and the node counts pin it.  Ko is the
 * one-ply approximation.  Moves outside M are not read, so a cut that works only through a ladder running out of M reads `unsettled`
 * or `cut`, not `connected`.  Connection by capturing a cutting chain with more than cut_libs liberties is not seen.  `connected` is
 * about making one chain inside M; it is not about whether the joined chain lives.  The knight's move and the two-point jump usually
 * have region_empty above the default max_region of the Python layer (8) and read `open`.
 *
 * sgo_connect_dev: row i reads record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], in place.
 * d_n_pairs int32 [n], d_rows int32 [n][max_pairs][12], d_regions uint32 [n][max_pairs][sgo_plane_words(S)]: the M used, bits a >= N
 * zero.  d_ask NULL, or d_ask[i][0] < 0 (d_ask int32 [n][2]): ENUMERATE: the NEAR pairs of either colour whose region_empty lies in
 * 1..max_region, in ascending (anchor_x, anchor_y) order; n_pairs = their true number; only min(n_pairs, max_pairs) rows and region
 * sets are written and everything behind them stays untouched.  d_ask[i] = {p, q} with p >= 0: exactly one row (n_pairs = 1), for the
 * chains on p and q in either order; the pair need not be NEAR (K empty: region_empty 0, `open`); read in row i of d_region
 * [n][sgo_plane_words(S)] when that is not NULL.  A row whose record index is outside [0, n_records) gives n_pairs = 0, untouched rows,
 * an untouched group map and untouched counts.  THREE launches on `stream` (k_connect_pairs, k_connect_read, k_connect_groups), no
 * allocation, no synchronisation, capturable; n == 0 is a no-op; rows >= n are not written.  SGO_ERR_ARG: an unsupported S, n < 0,
 * n_records < 0, rules outside {0, 1}, cut_libs outside [0, SGO_CONNECT_MAX_CUT_LIBS], max_region outside [1, SGO_CONNECT_MAX_REGION],
 * max_nodes outside [1, SGO_CONNECT_MAX_NODES], max_pairs outside [1, SGO_CONNECT_MAX_PAIRS], a NULL d_records or output.
 * SGO_CONNECT_MAX_NODES bounds the longest launch a single query can cause: measured on one MI355X (profiles/connect_ab.json) a node
 * takes 1.9 us with one half of the wave reading and 2.1 us with both, at 9x9 and at 19x19 alike, and a query that spends all 32 768
 * nodes 62 to 70 ms, under the 0.29 s the "life and death" cap allows; so the cap stands at that of the "capturing races" section. */
#define SGO_CONNECT_MAX_CUT_LIBS 4
#define SGO_CONNECT_MAX_REGION 32
#define SGO_CONNECT_MAX_NODES 32768
#define SGO_CONNECT_MAX_PAIRS 64
#define SGO_CONNECT_MAX_DEPTH 80
#define SGO_CONNECT_A_CUT 1
#define SGO_CONNECT_D_CUT 2
#define SGO_CONNECT_A_UNKNOWN 4
#define SGO_CONNECT_D_UNKNOWN 8
#define SGO_CONNECT_D_RAN 16
#define SGO_CONNECT_OPEN (1 << 16)
#define SGO_CONNECT_NO_PAIR (1 << 17)
int sgo_connect_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask,
                    const uint32_t *d_region, int rules, int cut_libs, int max_region, int max_nodes, int max_pairs, int32_t *d_n_pairs,
                    int32_t *d_rows, uint32_t *d_regions, int16_t *d_groups, int32_t *d_group_counts, void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order (copy in, run, copy back): for drop-in use and parity tests.
 * ask (or NULL) int32 [n][2], region (or NULL) uint32 [n][sgo_plane_words(S)].  Table rows and region sets beyond min(n_pairs,
 * max_pairs) come back as the caller filled them. */
int sgo_connect(int S, int n, const uint32_t *records, const int32_t *ask, const uint32_t *region, int rules, int cut_libs, int max_region,
                int max_nodes, int max_pairs, int32_t *n_pairs, int32_t *rows, uint32_t *regions, int16_t *groups, int32_t *group_counts);
/* The root positions of the listed HOLDING session slots of `ctx`, read in place; waits for `stream`.  HOST arrays: ask (or NULL)
 * [n][2], region (or NULL) [n][sgo_plane_words(S)], status [n], n_pairs [n], rows [n][max_pairs][12], regions
 * [n][max_pairs][sgo_plane_words(S)], groups int16 [n][N], group_counts [n][4].  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that
 * is not a holding session: that row's outputs are left as the caller filled them, as are the table rows beyond min(n_pairs,
 * max_pairs) of every row.  The context is only read; a slot may be listed repeatedly.  SGO_ERR_ARG: the bounds of sgo_connect_dev, a
 * slot outside the context, a NULL slot list or output. */
int sgo_session_connect(sgo_ctx *ctx, int n, const int32_t *slots, const int32_t *ask, const uint32_t *region, int rules, int cut_libs,
                        int max_region, int max_nodes, int max_pairs, int32_t *status, int32_t *n_pairs, int32_t *rows, uint32_t *regions,
                        int16_t *groups, int32_t *group_counts, void *stream);

/* ---- influence: who holds what right now, and by how much?  (an ESTIMATE, not a proof) --------------------------------------------- */
/* Per packed record: Bouzy's dilation / erosion map of the stones, the territory and moyo sets read off it, and an area-score
 * estimate (csrc/sgo_influence.hip).  The heuristic counterpart of the "unconditional life" section: that one is proved and says
 * little before the endgame, this one answers for every position and can be wrong.  Everything is integer, a fixed number of steps,
 * no loop depends on the data.  N = S * S.
 * Inputs of a record: black / white = the bits a < N of planes 0 / 1.  The to-play flag (the top bit of the last word of plane 0;
 * at S = 5 it shares the only word with the stones) is NOT a stone and changes no output.  Planes 2..15 and padding bits are never
 * read.
 * `dead` (optional), per ROW a bitset uint32 [sgo_plane_words(S)] in the bit order of the legal bitsets: a stone whose bit is set is
 * LIFTED before anything else, its point is treated as empty.  Bits on empty points and bits a >= N are ignored.  NULL: nothing is
 * lifted.  The LIVE stones are the stones that are not lifted.  (A point in both planes occurs only in an illegal record; it is
 * read as a black stone.)
 * PARAMETERS: dilate in [0, SGO_INFLUENCE_MAX_DILATE], erode_moyo <= erode_terr, both in [0, SGO_INFLUENCE_MAX_ERODE].  The
 * classical triples (dilate, erode_moyo, erode_terr) are territory / moyo = (5, 10, 21) and area = (4, 0, 0).
 * THE MAP: v[a] starts at +128 on a live black stone, -128 on a live white one, 0 elsewhere.  A NEIGHBOUR of a is one of the at
 * most four ON-BOARD 4-adjacent points; off-board points do not exist: they are neither positive, negative nor zero.  Every step
 * reads the previous map and writes a new one (Jacobi: all points at once).
 *   DILATION step: pos(a) = the number of neighbours with v > 0, neg(a) = the number with v < 0.
 *     if v[a] >= 0 and neg(a) == 0: v'[a] = v[a] + pos(a);   if v[a] <= 0 and pos(a) == 0: v'[a] = v[a] - neg(a);
 *     otherwise v'[a] = v[a].  (When both conditions hold, both add 0.)
 *   EROSION step: if v[a] > 0: v'[a] = max(0, v[a] - #{neighbours with v <= 0});
 *     if v[a] < 0: v'[a] = min(0, v[a] + #{neighbours with v >= 0});   if v[a] == 0 it stays 0.
 *   SCHEDULE: `dilate` dilation steps, then `erode_terr` erosion steps.  The map after the first `erode_moyo` erosion steps is the
 *     MOYO map (erode_moyo == 0: the dilated map itself), the final one the TERRITORY map.
 *   BOUNDS: |v| <= 128 + 4 * 8 = 160; a live stone keeps at least 128 - 4 * 31 = 4, so its sign never changes (hence the cap 31).
 * OUTPUTS per listed row:
 *   values int16 [N] = the territory map.
 *   sets   uint32 [4][sgo_plane_words(S)] = terr_black, terr_white, moyo_black, moyo_white: the points WITHOUT a live stone whose
 *          value is > 0 / < 0 in the territory map / in the moyo map (a lifted stone's point can be territory); bit order as the
 *          legal bitsets of sgo_legal_dev; all bits a >= N are zero.
 *   counts int32 [8] = |terr_black|, |terr_white|, |moyo_black|, |moyo_white|, live black stones, live white stones,
 *          neutral = N - live stones - |terr_black| - |terr_white|,
 *          margin = (live_black + |terr_black|) - (live_white + |terr_white|): the area-score estimate before komi.
 *
 * sgo_influence_dev: row i reads record d_index[i] (d_index NULL: record i) of d_records [n_records][sgo_packed_words(S)], in place.
 * d_dead uint32 [n][sgo_plane_words(S)] per ROW (not per record) or NULL; d_values int16 [n][N], d_sets uint32
 * [n][4][sgo_plane_words(S)], d_counts int32 [n][8].  A row whose record index is outside [0, n_records) gets all-zero outputs.
 * ONE launch on `stream` (one half-wavefront per row), no allocation, no synchronisation, capturable; n == 0 is a no-op; rows >= n
 * are not written.  SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0, dilate / erode_moyo / erode_terr out of range,
 * erode_moyo > erode_terr, a NULL d_records or output. */
#define SGO_INFLUENCE_MAX_DILATE 8
#define SGO_INFLUENCE_MAX_ERODE 31
int sgo_influence_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const uint32_t *d_dead, int dilate,
                      int erode_moyo, int erode_terr, int16_t *d_values, uint32_t *d_sets, int32_t *d_counts, void *stream);
/* The same for HOST buffers, records [n][sgo_packed_words(S)] in order, dead [n][sgo_plane_words(S)] or NULL (copy in, run, copy
 * back): for drop-in use and parity tests. */
int sgo_influence(int S, int n, const uint32_t *records, const uint32_t *dead, int dilate, int erode_moyo, int erode_terr, int16_t *values,
                  uint32_t *sets, int32_t *counts);
/* The root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), read in place; waits for `stream`.
 * HOST arrays: dead [n][sgo_plane_words(S)] or NULL, status [n], values [n][N], sets [n][4][sgo_plane_words(S)], counts [n][8].
 * status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is not a holding session: that row's outputs are left as the caller filled
 * them.  The context is only read; a slot may be listed repeatedly.  SGO_ERR_ARG: parameters as above, a slot outside the context,
 * a NULL argument other than dead. */
int sgo_session_influence(sgo_ctx *ctx, int n, const int32_t *slots, const uint32_t *dead, int dilate, int erode_moyo, int erode_terr,
                          int32_t *status, int16_t *values, uint32_t *sets, int32_t *counts, void *stream);

/* ---- superko: which moves would repeat an earlier position of the game? ------------------------------------------------------------ */
/* The one analysis that needs a record AND the game behind it (csrc/sgo_superko.hip).  Everything is integer.  N = S * S,
 * W = sgo_plane_words(S).
 * Row i names a record r = d_index[i] (d_index NULL: r = i) of d_records [n_records][sgo_packed_words(S)] and the first record
 * f = d_first[i] of its game.  The HISTORY of the row is the records f .. r in order, the current one included: what
 * sgo_records_replay writes for one game (f = base_g).  Nothing asks that the history come from a real game: it is a list of
 * positions.
 * A POSITION is the set of stones of planes 0 / 1, bits a < N, exactly as the "position keys" section reads them (the flag is not a
 * stone; padding bits and planes 2..15 are no part of it); its side to move is the to-play flag.
 * `rule` selects the comparison: 0 POSITIONAL, two positions are equal when their stones are equal; 1 SITUATIONAL, their stones are
 * equal and the same side is to move.
 * For every EMPTY point a of record r the side to move plays a by one ply of sgo_make_play (captures removed, then suicide
 * executed); the result is P' with the OTHER side to move.  The ply is played whether or not it is legal.
 *   a REPEATS when some h in [f, r] holds a position equal to P' under `rule`;
 *   back[a] = r - h for the LARGEST such h.  A simple ko gives 1; a single-stone suicide gives 0 under rule 0 (P' is the current
 *   position) and can never match h = r under rule 1.
 * d_sets uint32 [n][3][W], padding bits zero:
 *   0 repeat          the empty points that repeat
 *   1 extra           repeat AND the record's own legal set (sgo_legal_moves with `prev` from plane 2 / 3, what sgo_moves_dev calls
 *                     ALLOWED at side 0): the points superko forbids and the inherited rule (play.py:78-80) allows
 *   2 legal_superko   the legal set without repeat, with the pass bit N always set: a drop-in legal bitset
 * A pass is never in set 0 or 1.
 * d_back int16 [n][N]: back[a] for the points of repeat, -1 everywhere else (stones included).
 * d_counts int32 [n][8]:
 *   0 |repeat|     1 |extra|
 *   2 the largest back over extra, 0 when it is empty     3 the lowest point that has it, -1 when extra is empty
 *   4 seen = r - h for the largest h in [f, r - 1] whose position equals the CURRENT position of r under `rule`, 0 when there is
 *     none: the game has already cycled when it reaches this record
 *   5 the number of history records looked at
 *   6 key matches that the exact comparison refuted (below)
 *   7 1 when the history was longer than SGO_SUPERKO_MAX_HISTORY(S) and only its most recent part was read, else 0
 * A row with r outside [0, n_records), f < 0 or f > r gives the ZERO ROW: sets 0, back all -1, counts 0.
 * KEYS.  Stage 1 writes key_0 of the "position keys" section (with the flag term under rule 1, without it under rule 0) of every
 * record [0, n_records) into the work array d_keys; stage 2 compares the key of P' with the keys of the history.  A verdict NEVER
 * rests on a key alone: every key match is confirmed by comparing the stones of P' with planes 0 / 1 of record h (and the flag under
 * rule 1); a match the comparison refutes is counted in counts[6] and the search goes on with the next smaller h.
 *
 * sgo_superko_dev: TWO launches on `stream` (the keys; one half-wavefront per row), no allocation, no synchronisation, capturable;
 * n == 0 is a no-op; rows >= n are not written.  d_keys is uint64 [n_records], overwritten.  SGO_ERR_ARG: an unsupported S, n < 0,
 * n_records < 0, rule outside {0, 1}, a NULL d_records, d_first, d_keys or output.
 * LEFT OUT: superko inside the search, self-play and rollouts (the engine keeps the reference's one-ply rule); natural situational
 * superko; colour-swapped and symmetric repetition; histories longer than SGO_SUPERKO_MAX_HISTORY(S), beyond the flag.
 * There is NO session form: a session slot holds its root record and seven positions of history, not the game.  A caller that
 * holds a game replays its move list (sgo_records_replay) and asks for the last record with f = 0. */
#define SGO_SUPERKO_MAX_HISTORY(size) (SGO_SETUP_MAX_MOVES(size) + 1)   /* the longest game a replay can write */
int sgo_superko_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_first,
                    int rule, uint64_t *d_keys, uint32_t *d_sets, int16_t *d_back, int32_t *d_counts, void *stream);
/* The same for HOST buffers: records [n_records][sgo_packed_words(S)], index [n] or NULL, first [n] (copy in, run, copy back). */
int sgo_superko(int S, int n_records, const uint32_t *records, int n, const int32_t *index, const int32_t *first, int rule,
                uint32_t *sets, int16_t *back, int32_t *counts);
/* 1: stage 2 compares only the low 6 bits of the keys, so that the confirmation path is taken often (for tests); every output
 * but counts[6] stays the same.  0: all 64 bits (default).  Returns the previous mode; other values only query. */
int sgo_superko_mode(int mode);

/* ---- light playouts: ownership, score and move values from uniformly random games, no net -------------------------------------------- */
/* Per listed record `per_row` random games that refuse to fill their own eyes, each played to its end inside one kernel
 * (csrc/sgo_playout.hip): who ends up holding each point, the score distribution and an all-moves-as-first table.  An ESTIMATE of how
 * the position ends, not a proof; no net, no host loop.  Everything is integer.  N = S * S.
 * Row i names a record r = d_index[i] (d_index NULL: r = i) of d_records [n_records][sgo_packed_words(S)], read in place.  Per row
 * per_row PLAYOUTS j run, each with the global id g = i * per_row + j as uint32: the position in the CALL, not the record index, as
 * sgo_rollout_* numbers its sources.
 * START of a playout = the start of a rollout: black / white = the bits a < N of planes 0 / 1; the side to move is the to-play flag
 * (the top bit of the last word of plane 0; NOT a stone); `prev` of the first ply = plane 2 (black to move) or 3 (white), bits a < N,
 * as sgo_rollout_step reads it; from the second ply on `prev` = the mover's stones one ply ago in the playout itself (so after a pass
 * nothing is forbidden).  Passes in the record's history do not count: ply = 0, passes = 0.  touched = the points that hold a stone at
 * the start; first = the empty set.  Padding bits and planes 4..15 are never read.
 * EACH PLY, mover X, other colour O:
 *   ALLOWED is exactly the set of the "life and death" section for the given `rules`: 0 = sgo_legal_moves, 1 = sound; the ko test is
 *     word for word that section's (prev & ~own is exactly one point, and it is that point).
 *   EYE = the EMPTY points whose every on-board 4-neighbour holds an X stone and of whose on-board diagonal neighbours fewer than T
 *     hold an O stone; T = 2 when all four diagonals are on the board, else T = 1.  Empty diagonals do not count.
 *   cand = ALLOWED minus EYE, k = |cand|.  k = 0: the playout passes, passes += 1.  Otherwise t = (uint64(draw(seed, g, ply)) * k) >> 32
 *     with draw and mix exactly those of the "policy rollouts" section; the move is the (t + 1)-th lowest point of cand, played with one
 *     ply of sgo_make_play; passes returns to 0; a point not in touched enters touched and, when X is also the side that was to move
 *     at the start, first.
 *   ply += 1.
 * END: passes == 2 or ply == max_plies.  One that ends with fewer than two passes in a row is CAPPED.  max_plies <= 0 means 3 * N; a
 * value above 4 * N is refused.  (Under rules = 0 random playouts need not end on their own: a ko can never be connected, because the
 * connecting point has no empty neighbour and captures nothing; the cap ends them.  Under rules = 1 the cap is rarely reached.)
 * SCORING is that of the "policy rollouts" section (play.py:244-292): a point is black's if it holds a black stone or is empty and
 * reached by black only, the same for white; diff = black - white, komi-free.
 * OUTPUTS per row, written and not added to:
 *   own  int32 [2][N]   the number of playouts that end with the point black's, and with it white's
 *   amaf int32 [2][N]   for the side to move at the start: [0][a] = the playouts with a in first, [1][a] = the sum over those of diff
 *                       seen from that side (-diff for white).  Points occupied at the start have 0 in both.
 *   sums int64 [8]      {black_wins, white_wins, draws, score_sum, score_sq_sum, plies_sum, capped, playouts}, the order of
 *                       sgo_rollout_result
 * Results do not depend on how playouts are dealt to the machine or in which order they finish: accumulation is integer adds only.
 * A row whose record index is outside [0, n_records) gets all-zero outputs.  Illegal records go through the same definitions.
 *
 * sgo_playout_dev: d_own [n][2][N], d_amaf [n][2][N] or NULL, d_sums [n][8].  TWO launches on `stream` (the outputs are zeroed, then the
 * playouts add into them), no allocation, no synchronisation, capturable; n == 0 is a no-op; rows >= n are not written.
 * SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0, rules outside {0, 1}, per_row outside [1, SGO_PLAYOUT_MAX_PER_ROW] (so that
 * amaf [1][a] fits int32 at 19x19), n * per_row beyond int32, max_plies above 4 * N, a NULL d_records, d_own or d_sums. */
#define SGO_PLAYOUT_MAX_PER_ROW 65536
int sgo_playout_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int per_row, uint32_t seed, int rules,
                    int max_plies, int32_t *d_own, int32_t *d_amaf, int64_t *d_sums, void *stream);
/* The same for HOST buffers: records [n_records][sgo_packed_words(S)], index [n] or NULL, amaf or NULL (copy in, run, copy back). */
int sgo_playout(int S, int n_records, const uint32_t *records, int n, const int32_t *index, int per_row, uint32_t seed, int rules,
                int max_plies, int32_t *own, int32_t *amaf, int64_t *sums);
/* The root positions of the listed HOLDING session slots of `ctx` (what sgo_game_board shows), read in place; waits for `stream`.
 * HOST arrays: status [n], own [n][2][N], amaf [n][2][N] or NULL, sums [n][8].  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is
 * not a holding session: that row's outputs are left as the caller filled them.  g counts the listed slots, not the slot ids.  The
 * context is only read; a slot may be listed repeatedly.  SGO_ERR_ARG: the bounds of sgo_playout_dev, a slot outside the context, a
 * NULL slot list, status, own or sums. */
int sgo_session_playout(sgo_ctx *ctx, int n, const int32_t *slots, int per_row, uint32_t seed, int rules, int max_plies, int32_t *status,
                        int32_t *own, int32_t *amaf, int64_t *sums, void *stream);

/* ---- playout tree search: which move?  Monte-Carlo tree search with RAVE on the light playouts, no net ------------------------------- */
/* Per listed record `trees` independent tree searches of `sims` simulations each, every search run from first to last inside one
 * kernel (csrc/sgo_uct.hip): selection by a RAVE-blended value, expansion, a light playout below the tree, back-propagation.  What
 * comes out is the root's move table summed over the trees and the move it favours.  An ESTIMATE, not a proof; no net, no host
 * loop.  Everything is integer.  N = S * S; the pass is the move N.
 * ROWS, TREES, SIMULATIONS.  Rows, records, d_index, `rules` and the START of a game (stones, side to move, `prev` of the first ply)
 * are exactly those of the "light playouts" section.  Per row `trees` searches run (root parallelisation); tree t of row i has the id
 * g = i * trees + t.  A tree runs its simulations s = 0 .. sims - 1 one after another; simulation s of tree g draws with the playout id
 * gs = g * sims + s as uint32, that is draw(seed, gs, ply) of the "policy rollouts" section with ply counted from the root.  A tree
 * never sees another tree, and what a row reports is the integer sum over its trees: results do not depend on scheduling.
 * CANDIDATES.  At every ply, in the tree and below it, cand = ALLOWED minus EYE of the "light playouts" section for the given `rules`;
 * cand empty means the only move is the pass.  A simulation ENDS at two passes in a row or at ply == max_plies; max_plies <= 0 means
 * 3 * N, a value above 4 * N is refused, and a simulation that ends with fewer than two passes in a row is CAPPED, as there.
 * NODES.  A node is a position reached by a move sequence from the root (no transpositions).  When it is created it takes cand of its
 * position as its child set ({N} when cand is empty) and keeps per child a the counters n[a], w[a], rn[a], rw[a], all zero, and a link
 * to the child's node, none at first.  w counts 2 per win and 1 per draw from the view of the node's mover.  The root is node 0 and
 * is created before simulation 0.  A position in which the game has ended gets no node.
 * SELECTION at a node with mover X, ply `ply`, with P = prior and E = rave_equiv; all values unsigned, all divisions floor divisions:
 *   rn' = rn + P, rw' = rw + P
 *   rq = (E != 0 and rn' != 0) ? (rw' << 16) / rn' : 65536
 *   q = n ? (w << 16) / n : rq
 *   beta = n == 0 ? 65536 : (E != 0 and rn' != 0) ? (rn' << 16) / (rn' + n + rn' * n / E) : 0
 *   v = (beta * rq + (65536 - beta) * q) >> 16                       (the products in 64 bits; everything else fits 32)
 * The child chosen has the largest v; among equals the largest h(a) = mix(draw(seed, gs, ply) + a) (mod 2^32); among equals the lowest
 * a.  There is no exploration term: the prior and the hash tie-break do that work.
 * DESCENT.  The chosen child is played with one ply of sgo_make_play.  If the child has a node the simulation goes on there.
 * Otherwise the tree part ends with D = the number of tree plies taken, and a node for the new position is created and linked when
 * all of these hold: the child's n before this simulation was at least expand_at; D < SGO_UCT_MAX_DEPTH; the game has not ended; the
 * tree has fewer than max_nodes nodes.  (When only the last fails the tree was REFUSED a node.)  From ply D on the moves are the
 * playouts' uniform picks with draw(seed, gs, ply).
 * RESULT.  Scoring is that of the "policy rollouts" section; diff = black - white.  result2 = 2, 1 or 0 for 2 * diff greater than,
 * equal to or less than komi2, seen from black; from white's view it is 2 - result2.
 * During the plies >= D two sets are kept: a point played at such a ply enters Fb (black moved) or Fw (white moved) unless it is
 * already in one of them.
 * BACK-PROPAGATION walks the path from d = D - 1 down to 0.  With c the mover of ply d, a_d its move, its node, and r = result2 from
 * c's view:  (1) if a_d is a point it enters F_c and leaves the other set;  (2) n[a_d] += 1, w[a_d] += r;  (3) for every a in F_c
 * that is a child of the node: rn[a] += 1, rw[a] += r.
 * OUTPUTS per row, written and not added to:
 *   visits int32 [N + 1]      the root's n, summed over the trees; index N is the pass
 *   wins2  int32 [N + 1]      the root's w, summed over the trees (seen from the side to move)
 *   rave   int32 [2][N + 1]   the root's rn and rw, summed over the trees; may be NULL
 *   own    int32 [2][N]       the number of simulations that end with the point black's, and with it white's; may be NULL
 *   sums   int64 [8]          the eight sums of the "light playouts" section over all simulations (komi-free; plies from the root)
 *   info   int32 [4]          {nodes created, roots included; the largest D; the trees that were refused a node at least once; best}
 *   trace  int32 [n * trees][sims], indexed [g][s]; may be NULL: a_0 | D << 9 | result2 << 16 | capped << 18 of every simulation,
 *                             a_0 the move of ply 0
 * best = the child of the largest visits; among equals the larger wins2; among equals the lower point.  A row whose record index is
 * outside [0, n_records) gets all-zero outputs (its trace words included) and best = -1.
 *
 * sgo_uct_dev: THREE launches on `stream` (the outputs are zeroed, the trees add into them, best is written), no allocation, no
 * synchronisation, capturable; n == 0 is a no-op; rows >= n are not written.  d_work is device memory of at least
 * sgo_uct_workspace bytes (S, n, trees, max_nodes), 4-byte aligned, whose content means nothing before or after the call.
 * SGO_ERR_ARG: an unsupported S, n < 0, n_records < 0, trees outside [1, SGO_UCT_MAX_TREES], sims outside [1, SGO_UCT_MAX_SIMS],
 * n * trees * sims beyond int32, rules outside {0, 1}, max_plies above 4 * N, |komi2| above 4 * N, expand_at outside [0, sims],
 * rave_equiv outside [0, 1 << 20], prior outside [0, 1024], max_nodes outside [1, sims + 1], a NULL d_records, d_visits, d_wins2,
 * d_sums or d_info, and for n > 0 a NULL d_work or a work_bytes below the workspace size.  Nothing is written then.
 * sgo_uct_workspace returns the bytes, or SGO_ERR_ARG (negative) for an unsupported S, n < 0, trees or max_nodes out of range. */
#define SGO_UCT_MAX_TREES 4096
#define SGO_UCT_MAX_SIMS 4096
#define SGO_UCT_MAX_DEPTH 64
int64_t sgo_uct_workspace(int S, int n, int trees, int max_nodes);
int sgo_uct_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int trees, int sims, uint32_t seed, int rules,
                int max_plies, int komi2, int expand_at, int rave_equiv, int prior, int max_nodes, int32_t *d_visits, int32_t *d_wins2,
                int32_t *d_rave, int32_t *d_own, int64_t *d_sums, int32_t *d_info, int32_t *d_trace, void *d_work, int64_t work_bytes,
                void *stream);
/* The same for HOST buffers: records [n_records][sgo_packed_words(S)], index [n] or NULL; rave, own and trace or NULL (copy in,
 * allocate the workspace, run, copy back). */
int sgo_uct(int S, int n_records, const uint32_t *records, int n, const int32_t *index, int trees, int sims, uint32_t seed, int rules, int max_plies,
            int komi2, int expand_at, int rave_equiv, int prior, int max_nodes, int32_t *visits, int32_t *wins2, int32_t *rave, int32_t *own,
            int64_t *sums, int32_t *info, int32_t *trace);
/* The root positions of the listed HOLDING session slots of `ctx`, read in place; waits for `stream`; allocates and frees its
 * workspace for the call.  HOST arrays: status [n], visits [n][N + 1], wins2 [n][N + 1], rave [n][2][N + 1] or NULL, own [n][2][N] or
 * NULL, sums [n][8], info [n][4].  status[i] = SGO_OK, or SGO_ERR_STATE for a slot that is not a holding session: that row's outputs
 * are left as the caller filled them.  g counts the listed slots, not the slot ids.  The context is only read; a slot may be listed
 * repeatedly.  SGO_ERR_ARG: the bounds of sgo_uct_dev, a slot outside the context, a NULL slot list, status, visits, wins2, sums or
 * info. */
int sgo_session_uct(sgo_ctx *ctx, int n, const int32_t *slots, int trees, int sims, uint32_t seed, int rules, int max_plies, int komi2,
                    int expand_at, int rave_equiv, int prior, int max_nodes, int32_t *status, int32_t *visits, int32_t *wins2, int32_t *rave,
                    int32_t *own, int64_t *sums, int32_t *info, void *stream);

/* Introspection for parity tests: root child table of a slot's current tree and the canonical
 * serialisation of the whole tree (32-byte records, see oracle/sgo_oracle.c ora_game_tree_serialize). */
int sgo_root_table(sgo_ctx *ctx, int slot, int32_t *N, float *W, float *Q, double *P, int8_t *EX, int32_t *root_count,
                   float *root_value);
int64_t sgo_tree_serialize(sgo_ctx *ctx, int slot, uint8_t *buf, int64_t cap, int64_t *n_nodes, int64_t *n_expanded);
/* Same walk with 40-byte records <i action, i count, f value, f mean, d p, i vloss, i expanded, i depth, i pad>, from
 * which a host rebuilds the reference's nested dict nodes (play.py:376-421) -- see engine.SelfPlayEngine.tree_dict. */
int64_t sgo_tree_dump(sgo_ctx *ctx, int slot, uint8_t *buf, int64_t cap, int64_t *n_nodes);
int sgo_game_board(sgo_ctx *ctx, int slot, int32_t *board17);
/* test hook: stop slot right before the move choice of move_n == k (phase becomes done, error 0) */
int sgo_set_halt(sgo_ctx *ctx, int slot, int move_n);
/* Diagnostic: cycles per phase of k_search (csrc/sgo_search.hpp), summed over games and calls (zeros unless the library was built
 * with -DSGO_KSEARCH_PROFILE): [0] consuming evaluations, [1] round set-up, [2] selection, [7] round back-propagation,
 * [3] move step, [4] wave-calls. */
int sgo_debug_counters(sgo_ctx *ctx, unsigned long long *out, int n);
/* Test hook: the PUCT selector of the search (play.py:308-323 top_one_with_virtual_loss) on caller-supplied child tables.
 * DEVICE pointers to flat [n_cases][A] arrays: priors as float32 and, when f64 != 0, as the float64 root priors (P64 may be
 * NULL otherwise); counts; means; busy (> 0 = virtual loss set); legal (!= 0 = the child exists).  out[n_cases] receives the
 * chosen slot or -1.  Each case is written into the root block of a game slot and handed to the very function the descent
 * calls; cases run in chunks of n_games, all queued on `stream`.  Refuses (SGO_ERR_STATE) a context with games in flight;
 * the root blocks of all slots are overwritten. */
int sgo_debug_top_one(sgo_ctx *ctx, int n_cases, const float *P32, const double *P64, const int32_t *N, const float *Q,
                      const int8_t *busy, const uint8_t *legal, int f64, int32_t *out, void *stream);
/* Test hooks (tests/block_audit.py): the raw tree-block accounting, copied to HOST buffers and not interpreted.  Both
 * synchronise the device.  Every array pointer may be NULL; a first call with hdr alone gives the sizes.
 * Slot: hdr[20] = {phase, error, root_blk, other_root, free_top, min_free, ovf_hi, fifo_head, fifo_tail, cap, L, ovf_cap, APAD,
 * NW, E, rows, A, F = FIFO ring length, 0, 0}; free_list[L]; ovf_map[ovf_cap]; per local id of [0, rows): b_parent[rows],
 * b_slot[rows], c_b[rows][APAD], legal[rows][NW], where rows = cap + 1 + the highest backed overflow index (rows of overflow
 * ids that are not backed are left as the caller filled them); fifo[4][F] = the ring arrays parent, slot, block, evaluated.
 * A failed slot gives hdr (rows = 0) and ovf_map only.
 * Context: hdr[4] = {top of the free stack, returned entries, low-water mark, pool blocks}; pool_free / pool_ret[pool blocks]. */
int sgo_debug_block_state(sgo_ctx *ctx, int slot, int32_t *hdr, int32_t *free_list, int32_t *ovf_map, int32_t *b_parent,
                          int32_t *b_slot, int32_t *c_b, uint32_t *legal, int32_t *fifo);
int sgo_debug_pool_state(sgo_ctx *ctx, int32_t *hdr, int32_t *pool_free, int32_t *pool_ret);

/* average duration (ms) and launch count of the board_advance kernel inside sgo_step since the last
 * call (HIP events on the step's stream); used by bench.py for the roofline object */
int sgo_advance_timing(sgo_ctx *ctx, double *total_ms, int64_t *launches, int64_t *positions);

#ifdef __cplusplus
}
#endif
#endif
