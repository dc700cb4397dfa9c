// sgo_engine_state.hpp -- the engine's device data model: what lives in HBM between two kernels of a step, and the sizes
// derived from it.  Included by sgo_engine.hip (the one engine translation unit) before sgo_search.hpp; no kernels here.
//   GameState   one per game slot: the state machine's registers (k_search loads it, runs, stores it back)
//   Ctx         the context: configuration, geometry, every device array; passed BY VALUE to every engine kernel
//   Counters / DevStatus   running totals; the status words k_compact folds for the host
//   StageLayout staging area of sgo_start_games (one host-to-device copy per batch of restarts)
//   search_lds  the ONLY statement of k_search's dynamic LDS size, and the id-space limit that follows from it
//   HostSide / sgo_ctx   what the host keeps per context beside Ctx (shared by sgo_engine.hip and sgo_session.hip)
#pragma once
#include "sgo_bits.hpp"
#include "sgo_common.hpp"

namespace sgo {

// PH_HOLD: a SESSION slot (sgo_session_open) between two commands -- it keeps its board and tree, takes external moves
// (sgo_session_play) and waits to be armed (sgo_session_genmove); k_search skips it like PH_DONE, k_compact counts it neither as
// active nor as done
enum { PH_IDLE = 0, PH_WAIT_ROOT = 1, PH_SEARCH = 2, PH_DONE = 3, PH_HOLD = 4 };
#define MAXE 64

struct GameState {
    int32_t phase, root_blk, move_n, player;
    int32_t temperature, skipped_last, has_value, end_reason;
    float value, last_value, resign;
    int32_t has_resign;
    int32_t error, rounds_left, e_left, pre_bp;
    int32_t need_bp, original_player, fifo_head, fifo_tail;
    int32_t free_top, root_f64, root_count, halt_at;
    float root_value, root_mean;
    int32_t i_uniform, n_uniform;
    int32_t noise_used, game_seq, n_req, req_kind;
    int32_t eval_base, root_requested, winner, black;
    int32_t list_base;                     // k_compact: base of the game's requests in the leaf list (or among the root requests)
    int32_t session;                       // 1: an interactive slot (csrc/sgo_session.hpp): a move ends in PH_HOLD, the game never ends by itself
    double white;
    int32_t n_moves, last_player;
    int64_t n_predict, none_events;
    // two-model (evaluation) games, nomodel_self_play.py:203-218: the side NOT to move keeps its own tree
    int32_t cur_model, first_model;       // 0 = model1, 1 = model2: who searches now / who moved first (plays black)
    int32_t other_root, other_count;      // the other player's tree: root block (-1: none) and root statistics
    float other_value, other_mean;
    float resign2;
    int32_t has_resign2;
    int32_t min_free;                     // fewest free local ids the game ever had (high-water mark = L - min_free)
    int32_t ovf_hi;                       // overflow local ids [cap, cap + ovf_hi) have been backed at some time in this game
    // sgo_session_analyze (csrc/sgo_session.hpp), written by the arming kernel: the search this slot was armed for is search-only
    // (no resign test, no move: one record with action SGO_ACTION_ANALYSIS, then PH_HOLD) and runs an_rounds rounds
    int32_t analysis, an_rounds;
};

struct Counters {
    int32_t rec_count;
    int32_t pad;
    unsigned long long total_moves, total_evals, none_events;
    unsigned long long dbg[8];   // diagnostic build (-DSGO_KSEARCH_PROFILE): cycles per phase of k_search, summed over games
};

struct DevStatus {  // written by k_compact, copied to the host once per step
    int32_t n_eval, n_leaf, n_records, n_active, n_done, error, error_game, n_root;
    unsigned long long total_moves, total_evals, none_events;
};

struct Ctx {
    sgo_config cfg;
    int S, A, APAD, NW, RW, G, E, cap;
    // Block ids of a game are LOCAL: [0, cap) live in the game's private region (physical block g * cap + id), [cap, L) are
    // overflow ids, backed on demand by blocks of a pool SHARED by all games of the context (physical block G * cap + ovfMap).
    int ovf_cap, L;
    long pool_blocks;
    int max_moves;       // effective num_moves
    int rec_cap;
    // device arrays
    GameState *gs;
    uint32_t *pos;        // [G*cap][RW]
    uint32_t *legal;      // [G*cap][NW]
    float *cP, *cW, *cQ;  // [G*cap][APAD]
    int32_t *cN, *cB;     // counts, child block (local index, -1 = not expanded)
    uint8_t *cBusy;
    int32_t *bParent;     // [G*cap] local parent block (-1 root)
    int32_t *bSlot;       // [G*cap] slot in parent
    int32_t *freeList;    // [G][L] stack of free local ids: the private ones on top, overflow ids (largest first) at the bottom
    int32_t *ovfMap;      // [G][ovf_cap] shared block behind overflow id cap + j, -1 = not backed
    int32_t *poolFree;    // [pool_blocks] stack of free shared blocks: popped inside k_search, refilled by k_compact only
    int32_t *poolRet;     // [pool_blocks] shared blocks released by re-roots / restarts since the last k_compact
    int32_t *poolCtl;     // [0] top of poolFree, [1] entries of poolRet, [2] low-water mark of [0]
    double *rootP64;      // [G][APAD]
    double *noise;        // [G][APAD]
    double *uniforms;     // [G][max_moves]
    // fifo
    int32_t *fParent, *fSlot, *fBlk, *fEvalLocal, *fEvaluated;  // [G][2E]
    float *fValue;
    // requests of the current step
    int32_t *reqBlk, *reqParent, *reqMove;  // [G][E]; block ids are GLOBAL (g*cap + local)
    // compacted lists
    int32_t *evalIdx, *leafIn, *leafMv, *leafOut;  // [G*E]
    int32_t *evalModel;   // [G*E] which model evaluates each row of the evaluation list (two-model games; 0 otherwise)
    // records
    sgo_move_record *recs;
    uint32_t *recPacked;
    double *recPolicy;
    Counters *counters;
    DevStatus *dstatus;
    DevStatus *hstatus;   // pinned host
    int32_t *symLut;      // [8][A]
    uint8_t *stage;       // device staging area of sgo_start_games (one H2D copy per call)
    int last_n_eval;      // positions listed by the previous step
};

struct StageLayout {  // byte offsets into the staging area for a batch of n restarts (all 8-byte aligned)
    size_t slots, resign, resign2, first, noise, uniforms, total;
    int nu;
};
static inline size_t al8(size_t v) { return (v + 7) & ~(size_t)7; }
static StageLayout stage_layout(int n, int APAD, int nu, bool has_noise) {
    StageLayout L;
    L.nu = nu;
    L.slots = 0;
    L.resign = al8(sizeof(int32_t) * (size_t)n);
    L.resign2 = L.resign + al8(sizeof(float) * (size_t)n);
    L.first = L.resign2 + al8(sizeof(float) * (size_t)n);
    L.noise = L.first + al8(sizeof(int32_t) * (size_t)n);
    L.uniforms = L.noise + (has_noise ? sizeof(double) * (size_t)n * APAD : 0);
    L.total = L.uniforms + sizeof(double) * (size_t)n * nu;
    return L;
}

// a session slot between two commands: the state every sgo_session_* call and every reader of a session's root asks for
__device__ __forceinline__ bool holding(const GameState &s) { return s.session && s.phase == PH_HOLD && !s.error; }

// physical block behind local id `blk` of game g: the private region, or one dependent load for an overflow id.  gb0 = g * cap is
// passed in by Eng<S>, which keeps it: recomputed here, k_search's listing changes
__device__ __forceinline__ size_t phys_block(const Ctx &c, int g, size_t gb0, int blk) {
    if (blk < c.cap) return gb0 + blk;
    return (size_t)c.G * c.cap + (size_t)c.ovfMap[(size_t)g * c.ovf_cap + (blk - c.cap)];
}
__device__ __forceinline__ size_t phys_block(const Ctx &c, int g, int blk) { return phys_block(c, g, (size_t)g * c.cap, blk); }

// csrc/sgo_session.hip: k_session_roots on device pointers -- per listed slot the record index (physical block) of a holding
// session's root position and SGO_OK, or -1 and SGO_ERR_STATE.  The records are c.pos, G * cap + pool_blocks of them.
int launch_session_roots(const Ctx &c, int n, const int32_t *d_slots, int32_t *d_status, int32_t *d_index, hipStream_t st);
static inline int ctx_records(const Ctx &c) {
    const long blocks = (long)c.G * c.cap + c.pool_blocks;
    return blocks < 0x7fffffffl ? (int)blocks : 0x7fffffff;
}

// Give the shared block behind one entry of the overflow map (index mi = g * ovf_cap + j: overflow id cap + j of game g) back
// to the pool, if it is backed.  Releases go to poolRet; k_compact merges them into poolFree between two k_search launches, so
// a pop never meets a push.
__device__ __forceinline__ void pool_release(const Ctx &c, size_t mi) {
    const int ob = c.ovfMap[mi];
    if (ob >= 0) {
        c.poolRet[atomicAdd(&c.poolCtl[1], 1)] = ob;
        c.ovfMap[mi] = -1;
    }
}

// Dynamic LDS of k_search, in 4-byte words: queue[L] (the parent copy of the re-root's mark pass), sN[APAD], sQ[APAD] (the
// root's counts and means for the move choice), then (L + 31) / 32 + 4 tail words that are RESERVED AND UNUSED (once a mark
// bitmap).  They stay in the count: the id-space limit below and the occupancy figures in sgo_ctx_create's comments depend on it.
static const size_t SEARCH_LDS_LIMIT = 160 * 1024;   // bytes of LDS per CU on gfx950
static inline size_t search_lds_bytes(int L, int APAD) {
    return sizeof(int32_t) * ((size_t)L + 2 * (size_t)APAD + (L + 31) / 32 + 4);
}
// an id space L that is certain to fit: L * 33 / 32 + 32 + 2 * APAD + 4 words <= SEARCH_LDS_LIMIT
static inline long search_lds_max_ids(int APAD) { return ((long)(SEARCH_LDS_LIMIT / 4) - 2L * APAD - 4) * 32 / 33 - 32; }
template <int S>
static size_t search_lds(const Ctx &c) {
    return search_lds_bytes(c.L, Geo<S>::APAD);
}

struct HostSide {  // not passed to kernels
    uint8_t *stage = nullptr;                  // pinned host twin of Ctx::stage
    size_t stage_cap = 0;
    hipEvent_t ev_stage = nullptr;             // k_start has consumed the staged batch (host block and device twin)
    bool stage_busy = false;
    hipStream_t last_stream = nullptr;         // stream of the last sgo_step (records are drained behind it)
    bool lds_attr_set = false;                 // k_search's > 64 KiB dynamic-LDS attribute has been set
    bool lds_attr_session = false;             // ... and k_session_play's
    // sgo_session_setup / sgo_session_report: a grow-only pair of buffers (pinned host block and its device twin) for move
    // lists going in and reports coming out; both calls wait for their stream, so the pair is free again on return
    uint8_t *sess_h = nullptr, *sess_d = nullptr;
    size_t sess_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // bracket board_advance inside sgo_step
    double adv_ms = 0;
    long long adv_launches = 0, adv_positions = 0;
};

}  // namespace sgo

struct sgo_ctx {
    sgo::Ctx c;
    sgo::HostSide h;
};
