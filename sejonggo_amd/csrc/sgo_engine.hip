// sgo_engine.hip -- device-resident self-play engine: virtual-loss PUCT search + game loop for many
// concurrent games on one MI355X.  Second half of the C ABI in include/sgo.h.  One translation unit, four files:
//   sgo_engine_state.hpp    the device data model (GameState, Ctx, DevStatus, StageLayout) and k_search's LDS size
//   sgo_search.hpp          the search itself: Eng<S>, k_search (one wavefront per game), k_debug_top_one -- the part that
//                           restates the reference's play.py / tree_util.py / nomodel_self_play.py
//   sgo_engine.hip          (this file) the step plumbing: k_compact, k_start, context sizing / allocation, sgo_start_games*,
//                           step_enqueue / sgo_step*, the evaluation list, records and results
//   sgo_engine_inspect.hpp  host introspection used by tests and tools only (tree / board snapshots, debug entry points)
//
// Per engine step: k_search (consume evaluations -> back-propagate -> select the next leaves, or play a move) -> k_compact
// (prefix sums over games: dense evaluation list + leaf list + status words) -> board_advance for the new leaves
// (k_board_advance_rows, one half-wavefront per leaf, up to 32 768 leaves; k_board_advance, one lane per leaf + history-stream
// blocks, above; the grid is sized for the worst case and guarded by the device-side leaf count, so no host round trip sits in
// between) -> [host runs the network] -> next step.
// What it replaces of the reference (drsagitn/sejonggo): the request side of predicting_queue_worker.py:40-102 and the process /
// queue plumbing around nomodel_self_play.py:142-271 play_game_async; the search's own citations are in sgo_search.hpp.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "sgo_engine_state.hpp"
#include "sgo_search.hpp"

namespace sgo {

// ---------------------------------------------------------------------------------------- k_compact
// One block.  Exclusive prefix sums of the per-game request counts -> dense evaluation list (block ids
// in game-major order) and dense leaf list for board_advance; also folds the status words.
// The six block-wide scans (evaluation / leaf / root counts, active, done, first failing game) run as wave-level shuffles
// + one pass over the 16 wave totals: two block barriers instead of the twenty of a Hillis-Steele scan over LDS arrays.
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
__global__ __launch_bounds__(1024) void k_compact(Ctx c) {
    __shared__ int wE[16], wL[16], wR[16], wAct[16], wDone[16], wErr[16];
    __shared__ int tot[6];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int per = (c.G + 1023) / 1024;
    const int g0 = t * per, g1 = min(c.G, g0 + per);
    int ne = 0, nl = 0, nr = 0, act = 0, done = 0, err = 0x7fffffff;
    for (int g = g0; g < g1; g++) {
        const GameState &s = c.gs[g];
        ne += s.n_req;
        if (s.req_kind == 1) nl += s.n_req;
        else nr += s.n_req;
        if (s.phase == PH_WAIT_ROOT || s.phase == PH_SEARCH) act++;
        if (s.phase == PH_DONE) done++;
        if (s.error && err == 0x7fffffff) err = g;
    }
    // inclusive scans inside the wave
    int iE = wave_incl_scan(ne, lane), iL = wave_incl_scan(nl, lane), iR = wave_incl_scan(nr, lane);
    int sAct = act, sDone = done, sErr = err;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sAct += __shfl_xor(sAct, o);
        sDone += __shfl_xor(sDone, o);
        sErr = min(sErr, __shfl_xor(sErr, o));
    }
    if (lane == 63) { wE[w] = iE; wL[w] = iL; wR[w] = iR; }
    if (lane == 0) { wAct[w] = sAct; wDone[w] = sDone; wErr[w] = sErr; }
    __syncthreads();
    if (w == 0) {
        // exclusive scan of the 16 wave totals (lanes 0..15), totals of everything in tot[]
        const int vE = lane < 16 ? wE[lane] : 0, vL = lane < 16 ? wL[lane] : 0, vR = lane < 16 ? wR[lane] : 0;
        const int xE = wave_incl_scan(vE, lane), xL = wave_incl_scan(vL, lane), xR = wave_incl_scan(vR, lane);
        int a = lane < 16 ? wAct[lane] : 0, d = lane < 16 ? wDone[lane] : 0, e = lane < 16 ? wErr[lane] : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o);
            d += __shfl_xor(d, o);
            e = min(e, __shfl_xor(e, o));
        }
        if (lane < 16) { wE[lane] = xE - vE; wL[lane] = xL - vL; wR[lane] = xR - vR; }
        if (lane == 15) { tot[0] = xE; tot[1] = xL; tot[2] = xR; }
        if (lane == 0) { tot[3] = a; tot[4] = d; tot[5] = e; }
    }
    __syncthreads();
    // phase 1: every game's bases (thread t owns games [g0, g1))
    int be = wE[w] + iE - ne, bl = wL[w] + iL - nl, br = wR[w] + iR - nr;
    for (int g = g0; g < g1; g++) {
        GameState &s = c.gs[g];
        s.eval_base = be;
        s.list_base = (s.req_kind == 1) ? bl : br;
        be += s.n_req;
        if (s.req_kind == 1) bl += s.n_req;
        else br += s.n_req;
    }
    __syncthreads();
    // phase 2: one (game, request) pair per thread and pass -- all loads of a pair are independent of every other pair's, so
    // the 8 192 pairs of a 1 024-game step are a few memory round trips instead of eight dependent ones per game
    const int pairs = c.G * c.E;
    for (int e = t; e < pairs; e += 1024) {
        const int g = e / c.E, j = e - g * c.E;
        const GameState &s = c.gs[g];
        if (j >= s.n_req) continue;
        const int row = s.eval_base + j, blk = c.reqBlk[e];
        c.evalIdx[row] = blk;
        c.evalModel[row] = s.cur_model;
        if (s.req_kind == 1) {
            const int li = s.list_base + j;
            c.leafIn[li] = c.reqParent[e];
            c.leafMv[li] = c.reqMove[e];
            c.leafOut[li] = blk;
        }
    }
    // shared blocks released during this step's k_search (and by k_start since the previous step) go back on the free stack
    // here, between two k_search launches: pops and pushes never run concurrently
    {
        const int nret = c.poolCtl[1], top = c.poolCtl[0];
        for (int i = t; i < nret; i += 1024) c.poolFree[top + i] = c.poolRet[i];
        __syncthreads();
        if (t == 0 && nret > 0) { c.poolCtl[0] = top + nret; c.poolCtl[1] = 0; }
    }
    if (t == 1023) {
        DevStatus d;
        d.n_eval = tot[0]; d.n_leaf = tot[1]; d.n_records = c.counters->rec_count;
        d.n_active = tot[3]; d.n_done = tot[4];
        int eg = tot[5];
        d.error_game = (eg == 0x7fffffff) ? -1 : eg;
        d.error = (eg == 0x7fffffff) ? 0 : c.gs[eg].error;
        d.n_root = tot[2];
        d.total_moves = c.counters->total_moves; d.total_evals = c.counters->total_evals;
        d.none_events = c.counters->none_events;
        *c.dstatus = d;
    }
}

// (re)start listed game slots: empty board in block 0, everything else free
// Inputs come from the staging area filled by ONE host-to-device copy: slots[n], resign[n] (NaN = None), then
// (optionally) noise[n][APAD] and uniforms[n][nu].  session != 0 (sgo_session_open): the same empty board and empty tree, but the
// slot is a session that holds (PH_HOLD) at temperature 0 until a command arrives.
template <int S>
__global__ __launch_bounds__(64) void k_start(Ctx c, int n, StageLayout L, int has_noise, int has_uniforms, int session) {
    using G = Geo<S>;
    const int k = blockIdx.x;
    if (k >= n) return;
    const int g = reinterpret_cast<const int32_t *>(c.stage + L.slots)[k];
    const float *resign = reinterpret_cast<const float *>(c.stage + L.resign);
    const int lane = threadIdx.x;
    if (has_noise) {
        const double *src = reinterpret_cast<const double *>(c.stage + L.noise) + (size_t)k * c.APAD;
        for (int i = lane; i < c.APAD; i += 64) c.noise[(size_t)g * c.APAD + i] = src[i];
    }
    if (has_uniforms) {
        const double *src = reinterpret_cast<const double *>(c.stage + L.uniforms) + (size_t)k * L.nu;
        for (int i = lane; i < L.nu; i += 64) c.uniforms[(size_t)g * c.max_moves + i] = src[i];
    }
    const size_t gb0 = (size_t)g * c.cap;
    GameState st;
    memset(&st, 0, sizeof st);
    st.phase = PH_WAIT_ROOT;
    st.root_blk = 0;
    st.player = 1;
    st.temperature = (0 == c.cfg.stop_exploration) ? 0 : 1;
    st.e_left = -1;
    st.halt_at = -1;
    st.n_uniform = has_uniforms ? L.nu : 0;   // a game that samples a move without a supplied draw fails with SGO_ERR_DRAWS
    st.game_seq = c.gs[g].phase == PH_IDLE && c.gs[g].game_seq == 0 && c.gs[g].n_predict == 0 ? 0 : c.gs[g].game_seq + 1;
    float r = resign[k];
    st.has_resign = !(r != r) && r != 0.f;   // `if resign and ...` (nomodel_self_play.py:171): None and 0.0 never resign
    st.resign = st.has_resign ? r : 0.f;
    const float r2 = reinterpret_cast<const float *>(c.stage + L.resign2)[k];
    st.has_resign2 = !(r2 != r2) && r2 != 0.f;
    st.resign2 = st.has_resign2 ? r2 : 0.f;
    st.first_model = c.cfg.two_model ? (reinterpret_cast<const int32_t *>(c.stage + L.first)[k] & 1) : 0;
    st.cur_model = st.first_model;
    st.other_root = -1;
    if (c.max_moves == 0) st.phase = PH_DONE;
    if (session) { st.session = 1; st.phase = PH_HOLD; st.temperature = 0; }
    for (int i = lane; i < G::RW; i += 64) c.pos[gb0 * G::RW + i] = 0;
    for (int i = lane; i < G::NW; i += 64) c.legal[gb0 * G::NW + i] = empty_legal_word<S>(i);
    // whatever the slot's previous game still holds of the shared pool goes back to it
    for (int j = lane; j < c.ovf_cap; j += 64) pool_release(c, (size_t)g * c.ovf_cap + j);
    for (int b = lane; b < c.L - 1; b += 64) c.freeList[(size_t)g * c.L + b] = c.L - 1 - b;  // pops give 1,2,3,...: private ids first
    st.free_top = c.L - 1;
    st.min_free = c.L - 1;
    st.ovf_hi = 0;
    if (lane == 0) {
        c.bParent[gb0] = -1;
        c.bSlot[gb0] = -2;  // no children yet
        c.gs[g] = st;
    }
}

}  // namespace sgo

using namespace sgo;

#define CK(call)                      \
    do {                              \
        int _r = (call);              \
        if (_r != SGO_OK) return _r;  \
    } while (0)

template <typename T>
static int dalloc(T **p, size_t n) {
    SGO_HIP(hipMalloc((void **)p, sizeof(T) * (n ? n : 1)));
    SGO_HIP(hipMemset(*p, 0, sizeof(T) * (n ? n : 1)));
    return SGO_OK;
}

static int ctx_alloc(Ctx &c) {
    const size_t nb = (size_t)c.G * c.cap + (size_t)c.pool_blocks;       // private regions, then the shared pool
    CK(dalloc(&c.gs, c.G));
    CK(dalloc(&c.pos, nb * c.RW));
    CK(dalloc(&c.legal, nb * c.NW));
    CK(dalloc(&c.cP, nb * c.APAD));
    CK(dalloc(&c.cW, nb * c.APAD));
    CK(dalloc(&c.cQ, nb * c.APAD));
    CK(dalloc(&c.cN, nb * c.APAD));
    CK(dalloc(&c.cB, nb * c.APAD));
    CK(dalloc(&c.cBusy, nb * c.APAD));
    CK(dalloc(&c.bParent, nb));
    CK(dalloc(&c.bSlot, nb));
    CK(dalloc(&c.freeList, (size_t)c.G * c.L));
    CK(dalloc(&c.ovfMap, (size_t)c.G * c.ovf_cap));
    CK(dalloc(&c.poolFree, (size_t)c.pool_blocks));
    CK(dalloc(&c.poolRet, (size_t)c.pool_blocks));
    CK(dalloc(&c.poolCtl, 4));
    if (c.ovf_cap > 0) SGO_HIP(hipMemset(c.ovfMap, 0xff, sizeof(int32_t) * (size_t)c.G * c.ovf_cap));   // -1: not backed
    {
        std::vector<int32_t> ids((size_t)c.pool_blocks);
        for (size_t i = 0; i < ids.size(); i++) ids[i] = (int32_t)(ids.size() - 1 - i);                  // pops give 0, 1, 2, ...
        if (!ids.empty()) SGO_HIP(hipMemcpy(c.poolFree, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice));
        const int32_t ctl[4] = {(int32_t)c.pool_blocks, 0, (int32_t)c.pool_blocks, 0};
        SGO_HIP(hipMemcpy(c.poolCtl, ctl, sizeof ctl, hipMemcpyHostToDevice));
    }
    CK(dalloc(&c.rootP64, (size_t)c.G * c.APAD));
    CK(dalloc(&c.noise, (size_t)c.G * c.APAD));
    CK(dalloc(&c.uniforms, (size_t)c.G * (c.max_moves ? c.max_moves : 1)));
    const size_t nf = (size_t)c.G * 2 * MAXE;
    CK(dalloc(&c.fParent, nf));
    CK(dalloc(&c.fSlot, nf));
    CK(dalloc(&c.fBlk, nf));
    CK(dalloc(&c.fEvalLocal, nf));
    CK(dalloc(&c.fEvaluated, nf));
    CK(dalloc(&c.fValue, nf));
    const size_t nr = (size_t)c.G * c.E;
    CK(dalloc(&c.reqBlk, nr));
    CK(dalloc(&c.reqParent, nr));
    CK(dalloc(&c.reqMove, nr));
    CK(dalloc(&c.evalIdx, nr));
    CK(dalloc(&c.leafIn, nr));
    CK(dalloc(&c.leafMv, nr));
    CK(dalloc(&c.leafOut, nr));
    CK(dalloc(&c.evalModel, nr));
    CK(dalloc(&c.recs, (size_t)c.rec_cap));
    CK(dalloc(&c.recPacked, (size_t)c.rec_cap * c.RW));
    CK(dalloc(&c.recPolicy, (size_t)c.rec_cap * c.A));
    CK(dalloc(&c.counters, 1));
    CK(dalloc(&c.dstatus, 1));
    CK(dalloc(&c.symLut, (size_t)8 * c.A));
    {
        const StageLayout L = stage_layout(c.G, c.APAD, c.max_moves, true);
        CK(dalloc(&c.stage, L.total));
    }
    SGO_HIP(hipHostMalloc((void **)&c.hstatus, sizeof(DevStatus), hipHostMallocDefault));
    memset(c.hstatus, 0, sizeof(DevStatus));
    SGO_HIP(upload_sym_luts(c.S, c.symLut));
    return SGO_OK;
}

static void ctx_free(Ctx &c) {
    void *ptrs[] = {c.gs, c.pos, c.legal, c.cP, c.cW, c.cQ, c.cN, c.cB, c.cBusy, c.bParent, c.bSlot, c.freeList, c.ovfMap, c.poolFree, c.poolRet, c.poolCtl,
                    c.rootP64, c.noise, c.uniforms, c.fParent, c.fSlot, c.fBlk, c.fEvalLocal, c.fEvaluated, c.fValue,
                    c.reqBlk, c.reqParent, c.reqMove, c.evalIdx, c.leafIn, c.leafMv, c.leafOut, c.evalModel, c.recs, c.recPacked,
                    c.recPolicy, c.counters, c.dstatus, c.symLut, c.stage};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (c.hstatus) (void)hipHostFree(c.hstatus);
}

extern "C" {

sgo_ctx *sgo_ctx_create(const sgo_config *cfg) {
    if (!cfg || !size_ok(cfg->size) || cfg->n_games < 1 || cfg->energy < 1 || cfg->energy > MAXE || cfg->sims < 0) {
        set_error("sgo_ctx_create: bad config");
        return nullptr;
    }
    if (hipSetDevice(cfg->device_id) != hipSuccess) { set_error("sgo_ctx_create: hipSetDevice failed (no HIP device?)"); return nullptr; }
    sgo_ctx *x = new sgo_ctx();
    Ctx &c = x->c;
    memset((void *)&c.cfg, 0, sizeof c.cfg);
    c.cfg = *cfg;
    if (c.cfg.two_model && c.cfg.self_play) { set_error("sgo_ctx_create: two_model games are not self-play games"); delete x; return nullptr; }
    c.S = cfg->size; c.A = c.S * c.S + 1; c.NW = sgo_plane_words(c.S); c.RW = sgo_packed_words(c.S);
    c.APAD = 32 * c.NW; c.G = cfg->n_games; c.E = cfg->energy;
    // Tree blocks.  A search adds <= sims blocks and a move keeps the chosen child's subtree, so a tree settles at sims / (1 - f)
    // blocks, f = the share of the visits under the chosen child; over 512 full-length 19x19 / 400-sim games (20-block net) the
    // high-water mark was 4.2 sims in the median, 9.9 sims at the 99th percentile, 12.1 sims at most
    // (profiles/r03_fullgame_headline.json).  Sizing every game for the worst tree wastes four fifths of the memory (round 2:
    // 20 sims + 128 per game = 74 GB at 1 024 games) and still loses games where memory forces less (config 5 at 1 024 games:
    // 11.8 sims).  So: a PRIVATE region per game that covers most games (8 sims + 128), local ids beyond it backed on demand
    // from a pool SHARED by the context (2 sims per game, at least 12 sims), up to the id space k_search's LDS work queue
    // allows.  blocks_per_game > 0 fixes the private region; shared_blocks: > 0 fixes the pool, 0 = the default pool when the
    // private region is the default too and none otherwise (the round-2 behaviour: a fixed per-game pool), < 0 = default pool.
    const long lds_max = search_lds_max_ids(c.APAD);
    const size_t per_block = sizeof(uint32_t) * ((size_t)c.RW + c.NW) + (size_t)c.APAD * (4 * 5 + 1) + 3 * sizeof(int32_t);
    long priv = cfg->blocks_per_game > 0 ? cfg->blocks_per_game : 8L * cfg->sims + 128;
    long pool = cfg->shared_blocks > 0 ? cfg->shared_blocks
                : (cfg->shared_blocks < 0 || cfg->blocks_per_game <= 0) ? std::max(2L * cfg->sims * c.G, 12L * cfg->sims + 128) : 0;
    if (cfg->blocks_per_game <= 0 && priv > lds_max) priv = lds_max;
    {
        size_t free_b = 0, total_b = 0;
        if ((cfg->blocks_per_game <= 0 || cfg->shared_blocks <= 0) && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
            const double fit = (double)(free_b / 10 * 6) / (double)per_block;        // blocks that fit in 60 % of the free memory
            const double want = (double)priv * c.G + (double)pool;
            if (want > fit) {
                const double r = fit / want;
                if (cfg->blocks_per_game <= 0) priv = (long)(priv * r);
                if (cfg->shared_blocks <= 0) pool = (long)(pool * r);
            }
        }
    }
    if (priv < cfg->energy + 2) priv = cfg->energy + 2;
    long L = priv + pool;
    // default id space per game: 20 sims + 128 (the most any game has needed is 12.1 sims); at 19x19 / 400 sims that keeps
    // k_search's LDS work queue at 36 KB, i.e. four games per CU resident at once (at 40 sims: 65 KB, two per CU, +25 % per call)
    if (L > 20L * cfg->sims + 128 && cfg->shared_blocks <= 0) L = std::max(priv, 20L * cfg->sims + 128);
    if (L > lds_max) L = std::max(priv, lds_max);
    c.cap = (int)priv;
    c.L = (int)L;
    c.ovf_cap = (int)(L - priv);
    c.pool_blocks = c.ovf_cap > 0 ? pool : 0;
    c.max_moves = cfg->num_moves < 0 ? 2 * c.S * c.S : cfg->num_moves;
    c.rec_cap = 2 * c.G + 16;
    c.last_n_eval = 0;
    c.gs = nullptr; c.hstatus = nullptr;
    // LDS budget of k_search (blocks_per_game fixed by the caller can exceed lds_max)
    if (search_lds_bytes(c.L, c.APAD) > SEARCH_LDS_LIMIT) { set_error("sgo_ctx_create: blocks_per_game too large for the LDS work queue"); delete x; return nullptr; }
    if (ctx_alloc(c) != SGO_OK) { ctx_free(c); delete x; return nullptr; }
    x->h.stage_cap = stage_layout(c.G, c.APAD, c.max_moves, true).total;
    if (hipHostMalloc((void **)&x->h.stage, x->h.stage_cap, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&x->h.ev_stage, hipEventDisableTiming) != hipSuccess) {
        set_error("sgo_ctx_create: staging allocation failed");
        ctx_free(c); delete x; return nullptr;
    }
    if (hipEventCreate(&x->h.ev0) != hipSuccess || hipEventCreate(&x->h.ev1) != hipSuccess) {
        set_error("sgo_ctx_create: hipEventCreate failed");
        ctx_free(c); delete x; return nullptr;
    }
    return x;
}

int sgo_blocks_per_game(sgo_ctx *x) {
    if (!x) { set_error("sgo_blocks_per_game: bad argument"); return SGO_ERR_ARG; }
    return x->c.cap;
}

int sgo_pool_info(sgo_ctx *x, int64_t *out, int n) {
    if (!x || !out || n < 0) { set_error("sgo_pool_info: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    int32_t ctl[4] = {0, 0, 0, 0};
    SGO_HIP(hipDeviceSynchronize());
    SGO_HIP(hipMemcpy(ctl, c.poolCtl, sizeof ctl, hipMemcpyDeviceToHost));
    const int64_t v[6] = {c.cap, c.L, c.pool_blocks, (int64_t)ctl[0] + ctl[1], ctl[2], c.G};
    for (int i = 0; i < n && i < 6; i++) out[i] = v[i];
    return SGO_OK;
}

void sgo_ctx_destroy(sgo_ctx *x) {
    if (!x) return;
    (void)hipSetDevice(x->c.cfg.device_id);
    (void)hipDeviceSynchronize();
    ctx_free(x->c);
    if (x->h.stage) (void)hipHostFree(x->h.stage);
    if (x->h.sess_h) (void)hipHostFree(x->h.sess_h);
    if (x->h.sess_d) (void)hipFree(x->h.sess_d);
    if (x->h.ev_stage) (void)hipEventDestroy(x->h.ev_stage);
    if (x->h.ev0) (void)hipEventDestroy(x->h.ev0);
    if (x->h.ev1) (void)hipEventDestroy(x->h.ev1);
    delete x;
}

static int start_games_impl(sgo_ctx *x, int n, const int32_t *slots, const double *noise, const double *uniforms, int n_uniforms,
                            const float *resign, const float *resign2, const int32_t *first_model, void *stream, int session = 0);

int sgo_start_games(sgo_ctx *x, int n, const int32_t *slots, const double *noise, const double *uniforms, int n_uniforms,
                    const float *resign, void *stream) {
    return start_games_impl(x, n, slots, noise, uniforms, n_uniforms, resign, nullptr, nullptr, stream);
}

int sgo_start_games2(sgo_ctx *x, int n, const int32_t *slots, const double *uniforms, int n_uniforms, const float *resign_model1,
                     const float *resign_model2, const int32_t *first_model, void *stream) {
    if (!x || !x->c.cfg.two_model) { set_error("sgo_start_games2: the context was not created with two_model = 1"); return SGO_ERR_STATE; }
    return start_games_impl(x, n, slots, nullptr, uniforms, n_uniforms, resign_model1, resign_model2, first_model, stream);
}

static int start_games_impl(sgo_ctx *x, int n, const int32_t *slots, const double *noise, const double *uniforms, int n_uniforms,
                            const float *resign, const float *resign2, const int32_t *first_model, void *stream, int session) {
    if (!x || n < 0 || (n && !slots)) { set_error("sgo_start_games: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    if (n == 0) return SGO_OK;
    if (n > c.G || n_uniforms < 0) { set_error("sgo_start_games: too many slots"); return SGO_ERR_ARG; }
    for (int i = 0; i < n; i++)
        if (slots[i] < 0 || slots[i] >= c.G) { set_error("sgo_start_games: slot out of range"); return SGO_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    SGO_HIP(hipSetDevice(c.cfg.device_id));
    // the pinned staging area is reused: wait (host side, this one copy only) until the previous batch has left it
    if (x->h.stage_busy) { SGO_HIP(hipEventSynchronize(x->h.ev_stage)); x->h.stage_busy = false; }
    const int nu = uniforms ? (n_uniforms < c.max_moves ? n_uniforms : c.max_moves) : 0;
    const StageLayout L = stage_layout(n, c.APAD, nu, noise != nullptr);
    uint8_t *h = x->h.stage;
    memcpy(h + L.slots, slots, sizeof(int32_t) * n);
    float *hr = reinterpret_cast<float *>(h + L.resign), *hr2 = reinterpret_cast<float *>(h + L.resign2);
    int32_t *hf = reinterpret_cast<int32_t *>(h + L.first);
    for (int i = 0; i < n; i++) {
        hr[i] = resign ? resign[i] : NAN;
        hr2[i] = resign2 ? resign2[i] : NAN;
        hf[i] = first_model ? first_model[i] : 0;
    }
    if (noise) {
        double *hn = reinterpret_cast<double *>(h + L.noise);
        for (int i = 0; i < n; i++) {
            memcpy(hn + (size_t)i * c.APAD, noise + (size_t)i * c.A, sizeof(double) * c.A);
            memset(hn + (size_t)i * c.APAD + c.A, 0, sizeof(double) * (c.APAD - c.A));
        }
    }
    if (nu > 0) {
        double *hu = reinterpret_cast<double *>(h + L.uniforms);
        for (int i = 0; i < n; i++) memcpy(hu + (size_t)i * nu, uniforms + (size_t)i * n_uniforms, sizeof(double) * nu);
    }
    // one host-to-device copy, then one kernel, both on the caller's stream: ordered against the steps before and after
    SGO_HIP(hipMemcpyAsync(c.stage, h, L.total, hipMemcpyHostToDevice, st));
    SGO_DISPATCH(c.S, k_start<kS><<<dim3(n), dim3(64), 0, st>>>(c, n, L, noise != nullptr, nu > 0, session));
    SGO_HIP(hipGetLastError());
    // recorded BEHIND k_start: the event guards the pinned block and its device twin `c.stage` alike, so the next batch
    // (whatever stream it arrives on) is staged only after this one's kernel has read its slots / draws
    SGO_HIP(hipEventRecord(x->h.ev_stage, st));
    x->h.stage_busy = true;
    return SGO_OK;
}

// sejonggo_nomodel.py:20-35 SejongGoEngine.__init__ and GTPEngine.clear_board (:135-140): the listed slots become sessions on the
// empty board.  The other two session entry points are in sgo_session.hip.
int sgo_session_open(sgo_ctx *x, int n, const int32_t *slots, const float *resign, void *stream) {
    if (!x || n < 0 || (n && !slots)) { set_error("sgo_session_open: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    if (c.cfg.two_model) { set_error("sgo_session_open: a two_model context has no sessions"); return SGO_ERR_STATE; }
    if (n == 0) return SGO_OK;
    hipStream_t st = (hipStream_t)stream;
    SGO_HIP(hipSetDevice(c.cfg.device_id));
    std::vector<GameState> all(c.G);
    SGO_HIP(hipMemcpyAsync(all.data(), c.gs, sizeof(GameState) * c.G, hipMemcpyDeviceToHost, st));
    SGO_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= c.G) { set_error("sgo_session_open: slot out of range"); return SGO_ERR_ARG; }
        const GameState &s = all[slots[i]];
        if (!s.session && (s.phase == PH_WAIT_ROOT || s.phase == PH_SEARCH)) {
            set_error("sgo_session_open: the slot is running an ordinary game");
            return SGO_ERR_STATE;
        }
    }
    return start_games_impl(x, n, slots, nullptr, nullptr, 0, resign, nullptr, nullptr, stream, 1);
}

// Everything a step runs on the GPU, queued on `st` without waiting: k_search (consumes the evaluations of the list the previous
// step produced, selects / moves), k_compact (dense evaluation list + leaf list + status words), board_advance for the new
// leaves, and the copy of the status words to pinned host memory.  No host synchronisation, no host-side shape dependence: the
// chain can be captured in a hipGraph and replayed (timing = false then: event timestamps do not exist inside a graph).
static int step_enqueue(sgo_ctx *x, const float *d_policy, const float *d_value, int sym_k, const int32_t *d_sym_k, hipStream_t st,
                        bool timing) {
    Ctx &c = x->c;
    x->h.last_stream = st;
    SGO_DISPATCH(c.S, {
        const size_t lds = search_lds<kS>(c);
        if (lds > 64 * 1024 && !x->h.lds_attr_set) {
            SGO_HIP(hipFuncSetAttribute((const void *)k_search<kS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            x->h.lds_attr_set = true;
        }
        k_search<kS><<<dim3(c.G), dim3(64), lds, st>>>(c, d_policy, d_value, sym_k, d_sym_k);
    });
    SGO_HIP(hipGetLastError());
    k_compact<<<dim3(1), dim3(1024), 0, st>>>(c);
    SGO_HIP(hipGetLastError());
    // board_advance for the new leaves (parents = leafIn and freshly allocated blocks = leafOut are disjoint block sets => the
    // split form), bracketed by HIP events on this stream when timing
    if (timing) SGO_HIP(hipEventRecord(x->h.ev0, st));
    CK(launch_advance_split(c.S, c.G * c.E, &c.dstatus->n_leaf, c.pos, c.leafIn, c.leafMv, nullptr, c.pos, c.leafOut, c.legal,
                            c.leafOut, nullptr, st));
    if (timing) SGO_HIP(hipEventRecord(x->h.ev1, st));
    SGO_HIP(hipMemcpyAsync(c.hstatus, c.dstatus, sizeof(DevStatus), hipMemcpyDeviceToHost, st));
    return SGO_OK;
}

static void read_status(sgo_ctx *x, sgo_status *out) {
    Ctx &c = x->c;
    const DevStatus &d = *c.hstatus;
    out->n_eval = d.n_eval; out->n_records = d.n_records; out->n_active = d.n_active; out->n_done = d.n_done;
    out->error = d.error; out->error_game = d.error_game; out->total_moves = (int64_t)d.total_moves;
    out->total_evals = (int64_t)d.total_evals; out->none_events = (int64_t)d.none_events;
    c.last_n_eval = d.n_eval;
}

int sgo_step(sgo_ctx *x, const float *d_policy, const float *d_value, int sym_k, void *stream, sgo_status *out) {
    if (!x || !out || sym_k < 0 || sym_k > 7) { set_error("sgo_step: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    if (c.last_n_eval > 0 && (!d_policy || !d_value)) {
        set_error("sgo_step: the previous step listed positions to evaluate; policy/value are required");
        return SGO_ERR_STATE;
    }
    const int rc = step_enqueue(x, d_policy, d_value, sym_k, nullptr, st, true);
    if (rc != SGO_OK) return rc;
    SGO_HIP(hipStreamSynchronize(st));
    if (c.hstatus->n_leaf > 0) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, x->h.ev0, x->h.ev1) == hipSuccess) {
            x->h.adv_ms += ms; x->h.adv_launches += 1; x->h.adv_positions += c.hstatus->n_leaf;
        }
    }
    read_status(x, out);
    return SGO_OK;
}

int sgo_step_enqueue(sgo_ctx *x, const float *d_policy, const float *d_value, const int32_t *d_sym_k, void *stream) {
    if (!x || !d_policy || !d_value || !d_sym_k) { set_error("sgo_step_enqueue: bad argument"); return SGO_ERR_ARG; }
    return step_enqueue(x, d_policy, d_value, 0, d_sym_k, (hipStream_t)stream, false);
}

int sgo_step_status(sgo_ctx *x, sgo_status *out) {
    if (!x || !out) { set_error("sgo_step_status: bad argument"); return SGO_ERR_ARG; }
    read_status(x, out);
    return SGO_OK;
}

int sgo_eval_list(sgo_ctx *x, const uint32_t **d_records, const int32_t **d_index, const int32_t **d_models) {
    if (!x) { set_error("sgo_eval_list: bad argument"); return SGO_ERR_ARG; }
    if (d_records) *d_records = x->c.pos;
    if (d_index) *d_index = x->c.evalIdx;
    if (d_models) *d_models = x->c.evalModel;
    return x->c.G * x->c.E;
}

int sgo_eval_models(sgo_ctx *x, int cap, int32_t *models) {
    if (!x || !models || cap < 0) { set_error("sgo_eval_models: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    const int n = c.last_n_eval;
    if (n > cap) { set_error("sgo_eval_models: caller buffer too small"); return SGO_ERR_ARG; }
    if (n > 0) {
        SGO_HIP(hipMemcpyAsync(models, c.evalModel, sizeof(int32_t) * n, hipMemcpyDeviceToHost, x->h.last_stream));
        SGO_HIP(hipStreamSynchronize(x->h.last_stream));
    }
    return n;
}

int sgo_collect(sgo_ctx *x, int sym_k, int layout, int dtype, void *d_nn_in, void *stream) {
    if (!x || !d_nn_in) { set_error("sgo_collect: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    if (sym_k < 0 || sym_k > 7 || layout < 0 || layout > 2 || dtype < 0 || dtype > 1) { set_error("sgo_collect: bad argument"); return SGO_ERR_ARG; }
    return launch_nn_pack(c.S, c.last_n_eval, c.pos, c.evalIdx, sym_k, layout, dtype, d_nn_in, (hipStream_t)stream);
}

int sgo_drain_records(sgo_ctx *x, int cap, sgo_move_record *recs, uint32_t *packed, double *policy) {
    if (!x || cap < 0) { set_error("sgo_drain_records: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    // sgo_step has synchronised its stream before returning, so the records (and the count in the status it returned)
    // are complete; everything here is queued behind that stream and waited for once
    hipStream_t st = x->h.last_stream;
    int n = c.hstatus->n_records;
    if (n > c.rec_cap) n = c.rec_cap;
    if (n > cap) { set_error("sgo_drain_records: caller buffer too small"); return SGO_ERR_ARG; }
    if (n > 0) {
        if (recs) SGO_HIP(hipMemcpyAsync(recs, c.recs, sizeof(sgo_move_record) * n, hipMemcpyDeviceToHost, st));
        if (packed) SGO_HIP(hipMemcpyAsync(packed, c.recPacked, sizeof(uint32_t) * (size_t)n * c.RW, hipMemcpyDeviceToHost, st));
        if (policy) SGO_HIP(hipMemcpyAsync(policy, c.recPolicy, sizeof(double) * (size_t)n * c.A, hipMemcpyDeviceToHost, st));
    }
    SGO_HIP(hipMemsetAsync(&c.counters->rec_count, 0, sizeof(int32_t), st));
    SGO_HIP(hipStreamSynchronize(st));
    c.hstatus->n_records = 0;
    return n;
}

int sgo_game_results(sgo_ctx *x, int n, const int32_t *slots, sgo_game_result *out) {
    if (!x || n < 0 || !out) { set_error("sgo_game_results: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    std::vector<GameState> all(c.G);
    SGO_HIP(hipMemcpyAsync(all.data(), c.gs, sizeof(GameState) * c.G, hipMemcpyDeviceToHost, x->h.last_stream));
    SGO_HIP(hipStreamSynchronize(x->h.last_stream));
    for (int i = 0; i < n; i++) {
        int g = slots ? slots[i] : i;
        if (g < 0 || g >= c.G) { set_error("sgo_game_results: slot out of range"); return SGO_ERR_ARG; }
        const GameState &s = all[g];
        out[i].winner = s.winner; out[i].black = s.black; out[i].white = s.white; out[i].end_reason = s.end_reason;
        out[i].n_moves = s.n_moves; out[i].last_player = s.last_player; out[i].done = (s.phase == PH_DONE) ? 1 : 0;
        out[i].first_model = s.first_model;
        out[i].blocks_high_water = c.L - s.min_free;
        if (s.error) out[i].done = s.error;
    }
    return SGO_OK;
}

int sgo_set_halt(sgo_ctx *x, int slot, int move_n) {
    if (!x || slot < 0 || slot >= x->c.G) { set_error("sgo_set_halt: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    SGO_HIP(hipDeviceSynchronize());
    GameState s;
    SGO_HIP(hipMemcpy(&s, c.gs + slot, sizeof s, hipMemcpyDeviceToHost));
    s.halt_at = move_n;
    SGO_HIP(hipMemcpy(c.gs + slot, &s, sizeof s, hipMemcpyHostToDevice));
    return SGO_OK;
}

}  // extern "C"

// host introspection for tests and tools (tree / board snapshots, the debug entry points): no part of a step
#include "sgo_engine_inspect.hpp"
