// sgo_search.hpp -- the search: virtual-loss PUCT descent, expansion, back-propagation, and the game's state machine.
// Included by sgo_engine.hip only.  This is the part of the engine that restates the reference (drsagitn/sejonggo, file:line):
//   play.py:308-323 top_one_with_virtual_loss, tree_util.py:4-24 find_best_leaf_virtual_loss,
//   play.py:376-421 new_tree/new_subtree, simulation_workers.py:42-54 basic_tasks2,
//   nomodel_self_play.py:40-56 back_propagation, :59-82 async_simulate2, :114-140 select_play,
//   :142-271 play_game_async.
//
// Execution model
//   * ONE WAVEFRONT PER GAME runs the game's state machine (k_search): the descent does a 64-lane
//     argmax over the <=362 child slots of a node (6 slots per lane at 19x19, butterfly reduce), busy
//     flags and back-off exactly as the reference; expansion and garbage collection use wave ballots +
//     prefix popcounts.  Games never talk to each other, so there is no inter-workgroup hand-off.
//   * Tree storage: every game owns `cap` fixed-size BLOCKS.  A block = one expanded node: its packed
//     position, legal bitset, and APAD child slots in struct-of-arrays form (P, N, W, Q, child block,
//     busy) so that the lanes of the selecting wave read consecutive slots (coalesced).  Child slot i
//     is only ever touched by lane (i & 63) of the game's wave.  Blocks are recycled by a
//     mark-and-rebuild pass when the tree is re-rooted after a move.
//
// Float regime (must match oracle/sgo_oracle.c, i.e. the reference under numpy>=2): W/Q/score in
// float32; at a root whose priors were mixed with Dirichlet noise priors and score are float64.
//
// THE INLINING RULE.  The design rests on three things the compiler must deliver: one wavefront per game, the whole GameState
// in registers for the length of a launch, and no calls.  So every device function that k_search or k_debug_top_one reaches is
// `__forceinline__` (a lambda, should one return: `__attribute__((always_inline))`), and nothing is left to the inliner's cost
// model.  Measured on this file's code for gfx950: with ONE stage out of line (the move step as a plain lambda, which also
// un-inlined finish()) the listing had 9 s_swappc_b64 calls, GameState went to memory -- 768 B of scratch per lane in every
// k_search<S> -- and k_search<19> rose from 196 to 248 VGPRs; with everything forced inline: no call, no scratch, 196 VGPRs.
// The golden games pass either way, only slower, so tests/test_engine_isa.py holds the structure: no call instruction, no
// non-kernel function emitted, no scratch, and no static LDS in k_search.
#pragma once
#include "sgo_engine_state.hpp"

namespace sgo {

// ---------------------------------------------------------------------------------------- device helpers
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// argmax over the wave with "higher score, then lower index"; idx < 0 = no candidate
template <typename F>
__device__ __forceinline__ void wave_argmax(F &score, int &idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        F os = __shfl_xor(score, o);
        int oi = __shfl_xor(idx, o);
        bool take = (oi >= 0) && (idx < 0 || os > score || (os == score && oi < idx));
        if (take) { score = os; idx = oi; }
    }
}

// select_play's choice at temperature 0 (nomodel_self_play.py:138 `max((count, mean_value, index))`): child (n, q, i) beats the
// best so far (bn, bq, bi; bi < 0 = none yet) on count, then mean, then the HIGHER index.  Shared by Search<S>::choose_move and
// k_session_report (csrc/sgo_session.hpp).
__device__ __forceinline__ bool child_beats(int n, float q, int i, int bn, float bq, int bi) {
    return bi < 0 || n > bn || (n == bn && (q > bq || (q == bq && i > bi)));
}

template <int S>
struct Eng {
    using G = Geo<S>;
    const Ctx &c;
    int g, lane;
    size_t gb0;  // g * cap
    __device__ __forceinline__ Eng(const Ctx &cc, int gg) : c(cc), g(gg), lane(threadIdx.x & 63), gb0((size_t)gg * cc.cap) {}

    // physical block behind local id `blk` (uniform over the wave): private region, or one dependent load for an overflow id
    __device__ __forceinline__ size_t ph(int blk) const { return phys_block(c, g, gb0, blk); }
    __device__ __forceinline__ size_t slot_base(int blk) const { return ph(blk) * (size_t)G::APAD; }
    __device__ __forceinline__ bool legal_bit(int blk, int i) const {
        return (c.legal[ph(blk) * G::NW + (i >> 5)] >> (i & 31)) & 1u;
    }
    // a block for overflow id `blk` from the shared pool (all lanes call; false = the pool is empty)
    __device__ __forceinline__ bool back(int blk, GameState &st) const {
        int phys = -1;
        if (lane == 0) {
            const int t = atomicSub(&c.poolCtl[0], 1);
            if (t > 0) {
                phys = c.poolFree[t - 1];
                atomicMin(&c.poolCtl[2], t - 1);
                c.ovfMap[(size_t)g * c.ovf_cap + (blk - c.cap)] = phys;
            } else {
                atomicAdd(&c.poolCtl[0], 1);
            }
        }
        phys = __shfl(phys, 0);
        if (blk - c.cap + 1 > st.ovf_hi) st.ovf_hi = blk - c.cap + 1;
        return phys >= 0;
    }
    // pop a free local id, backed; -1 = out of blocks (private region used up and the shared pool empty, or the id space)
    __device__ __forceinline__ int alloc(GameState &st) const {
        if (st.free_top <= 0) return -1;
        const int nb = c.freeList[(size_t)g * c.L + st.free_top - 1];
        if (nb >= c.cap && !back(nb, st)) return -1;
        st.free_top--;
        if (st.free_top < st.min_free) st.min_free = st.free_top;
        return nb;
    }

    // play.py:308-323 on block `blk`; returns chosen slot or -1, and in `child` the chosen slot's child block (-1: a leaf).
    // Every array of the block is loaded UNCONDITIONALLY for all slots (expand() initialises all APAD slots, illegal ones with
    // zeros), so that the ~30 loads of a node are in flight together: one memory round trip per tree level instead of four
    // (legal word -> N / busy under that mask -> P / Q under the not-busy mask -> the winner's child pointer), which is what a
    // descent through a late-game tree spent its time on (k_search averaged 0.9 ms per call over a full 19x19 game, 0.2 ms at
    // the first plies).
    __device__ __forceinline__ int top_one(int blk, bool f64, int &child) const {
        const size_t pb = ph(blk), sb = pb * (size_t)G::APAD;
        constexpr int J = (G::APAD + 63) / 64;
        int n_[J], cb_[J];
        float p_[J], q_[J];
        bool ex[J], busy[J];
        int sum = 0;
#pragma unroll
        for (int j = 0; j < J; j++) {
            const int i = lane + 64 * j;
            const bool in = i < G::APAD;
            const uint32_t lw = in ? c.legal[pb * G::NW + (i >> 5)] : 0u;
            const int nv = in ? c.cN[sb + i] : 0;
            const int bz = in ? (int)c.cBusy[sb + i] : 1;
            p_[j] = in ? c.cP[sb + i] : 0.f;
            q_[j] = in ? c.cQ[sb + i] : 0.f;
            cb_[j] = in ? c.cB[sb + i] : -1;
            ex[j] = in && ((lw >> (i & 31)) & 1u);
            n_[j] = ex[j] ? nv : 0;
            busy[j] = ex[j] ? (bz > 0) : true;
            sum += n_[j];
        }
        // A position whose only legal move is the pass (the endgame's pass-pass chains, hundreds of levels deep: the reference's
        // search has no terminal test) needs no scores: its single child is chosen unless it is busy -- what the general path
        // below computes too (any finite score beats -100), minus two wave reductions and the score arithmetic.
        {
            constexpr int jN = G::N >> 6, lN = G::N & 63;
            bool only_pass = true;
#pragma unroll
            for (int j = 0; j < J; j++) {
                const unsigned long long m = __ballot(ex[j]);
                only_pass = only_pass && (m == (j == jN ? (1ull << lN) : 0ull));
            }
            if (only_pass) {
                const int bz = __shfl((int)busy[jN], lN);
                child = bz ? -1 : __shfl(cb_[jN], lN);
                return bz ? -1 : G::N;
            }
        }
        sum = wave_sum_i(sum);
        double tn = sqrt((double)sum);
        if (tn == 0) tn = 1;
        int best = -1;
        if (!f64) {
            float bs = -100.0f;
            const float tnf = (float)tn;
#pragma unroll
            for (int j = 0; j < J; j++) {
                int i = lane + 64 * j;
                if (!busy[j]) {
                    float u = p_[j] * tnf;
                    u = u / (float)(1.0 + (double)n_[j]);
                    float v = q_[j] + u;
                    if (v > bs) { bs = v; best = i; }
                }
            }
            wave_argmax<float>(bs, best);
        } else {
            double bs = -100.0;
            const double *p64 = c.rootP64 + (size_t)g * G::APAD;
#pragma unroll
            for (int j = 0; j < J; j++) {
                int i = lane + 64 * j;
                if (!busy[j]) {
                    double u = p64[i] * tn / (1. + (double)n_[j]);
                    double v = (double)q_[j] + u;
                    if (v > bs) { bs = v; best = i; }
                }
            }
            wave_argmax<double>(bs, best);
        }
        int cb = -1;
        if (best >= 0) {
#pragma unroll
            for (int j = 0; j < J; j++)
                if ((best >> 6) == j) cb = cb_[j];
            cb = __shfl(cb, best & 63);
        }
        child = cb;
        return best;
    }

    // tree_util.py:4-24.  Returns true and (pblk, slot) of the leaf (flagged busy), or false ("None").
    // `start` >= 0 resumes below the root: between two selections of one round nothing changes but busy flags at and below
    // the previous leaf's parent (no statistics move until the round's back-propagation), so a walk from the root would make
    // the same choices down to that parent -- the descent continues there instead of re-walking a path that, in the endgame's
    // deep pass-pass chains, is hundreds of levels long (k_search: 0.08 ms per call up to move 250, 0.8 ms at move 325).
    __device__ __forceinline__ bool find_best_leaf(const GameState &st, int &pblk, int &slot, int start) const {
        int node = start >= 0 ? start : st.root_blk;
        for (;;) {
            int cb = -1;
            int a = top_one(node, st.root_f64 && node == st.root_blk, cb);
            if (a < 0) {
                const size_t pn = ph(node);
                int par = c.bParent[pn];
                if (par < 0) return false;
                int ps = c.bSlot[pn];
                if (lane == (ps & 63)) c.cBusy[slot_base(par) + ps] = 2;
                node = par;
                continue;
            }
            if (cb < 0) {
                if (lane == (a & 63)) c.cBusy[slot_base(node) + a] = 2;
                pblk = node;
                slot = a;
                return true;
            }
            node = cb;
        }
    }

    // children of block `blk` from a policy row (play.py:391-421); legal[] of the block must be valid
    __device__ __forceinline__ void expand(int blk, const float *policy, const int32_t *lut, const double *noise, double eps) const {
        const size_t pb = ph(blk), sb = pb * (size_t)G::APAD;
        double *p64 = c.rootP64 + (size_t)g * G::APAD;
        // all loads of the node first (legal words, the symmetry LUT, then the gathered priors: two dependent round trips for the
        // whole node), then the stores: the slot-by-slot loop paid three dependent round trips per 64 slots -- 43 % of k_search
        constexpr int J = (G::APAD + 63) / 64;
        bool ex[J];
        int src[J];
        float pr[J];
#pragma unroll
        for (int j = 0; j < J; j++) {
            const int i = lane + 64 * j;
            ex[j] = i < G::APAD && ((c.legal[pb * G::NW + ((i < G::APAD ? i : 0) >> 5)] >> (i & 31)) & 1u);
            src[j] = i < G::A ? lut[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < J; j++) {
            const int i = lane + 64 * j;
            pr[j] = i < G::A ? policy[src[j]] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < J; j++) {
            const int i = lane + 64 * j;
            if (i >= G::APAD) continue;
            float p = (ex[j] && i < G::A) ? pr[j] : 0.0f;
            if (noise) {
                double t = (1.0 - eps) * (double)p;
                double pd = ex[j] ? t + eps * noise[i] : 0.0;
                p64[i] = pd;
                p = (float)pd;
            }
            c.cP[sb + i] = p;
            c.cN[sb + i] = 0;
            c.cW[sb + i] = 0.f;
            c.cQ[sb + i] = 0.f;
            c.cB[sb + i] = -1;
            c.cBusy[sb + i] = 0;
        }
    }

    // nomodel_self_play.py:40-56 + the stats part of simulation_workers.py:50-53
    __device__ __forceinline__ void back_propagate(GameState &st, int fi) const {
        const size_t fo = (size_t)g * (2 * MAXE) + fi;
        const int pb = c.fParent[fo], slot = c.fSlot[fo], nb = c.fBlk[fo];
        const float vraw = c.fValue[fo];
        const int leaf_player = white_to_play<S>(c.pos + ph(nb) * G::RW) ? -1 : 1;
        const float v = (leaf_player == st.original_player) ? vraw : -vraw;
        float leaf_value = 0.f;
        if (lane == (slot & 63)) {
            const size_t o = slot_base(pb) + slot;
            int n = c.cN[o] + 1;
            float w = c.cW[o] + v;
            c.cN[o] = n;
            c.cW[o] = w;
            c.cQ[o] = w / (float)n;
            c.cBusy[o] = 0;
            c.cB[o] = nb;
            leaf_value = w;
        }
        leaf_value = __shfl(leaf_value, slot & 63);
        // Walk to the root.  One memory round trip per level: the next level's parent / slot are requested together with this
        // level's statistics (the walk was three dependent round trips per level: parent, then slot, then N / W).
        const size_t ppb = ph(pb);
        int par = c.bParent[ppb], ps = c.bSlot[ppb];
        while (par >= 0) {
            const size_t pp = ph(par);
            const int npar = c.bParent[pp], nps = c.bSlot[pp];
            if (lane == (ps & 63)) {
                const size_t o = slot_base(par) + ps;
                int n = c.cN[o] + 1;
                float w = c.cW[o] + leaf_value;
                c.cN[o] = n;
                c.cW[o] = w;
                c.cQ[o] = w / (float)n;
                c.cBusy[o] = 0;
            }
            par = npar;
            ps = nps;
        }
        st.root_count += 1;
        st.root_value += leaf_value;
        st.root_mean = st.root_value / (float)st.root_count;
    }
};

// ---------------------------------------------------------------------------------------- test hook: the selector alone
// sgo_debug_top_one: one wave per case writes a flat child table into the root block of game slot blockIdx.x -- every array
// top_one() reads: counts, busy flags, priors (float32 and the slot's float64 root priors), means, child pointers (-1), the
// legal words -- and then runs Eng<S>::top_one itself on it, the function every descent step of k_search calls.
template <int S>
__global__ void __launch_bounds__(64) k_debug_top_one(Ctx c, int n, const float *P32, const double *P64, const int32_t *N,
                                                      const float *Q, const int8_t *busy, const uint8_t *legal, int f64,
                                                      int32_t *out) {
    using G = Geo<S>;
    const int g = blockIdx.x, lane = threadIdx.x & 63;
    if (g >= n || g >= c.G) return;
    Eng<S> e(c, g);
    int blk = c.gs[g].root_blk;
    if (blk < 0 || blk >= c.cap) blk = 0;
    const size_t pb = e.ph(blk), sb = pb * (size_t)G::APAD, t = (size_t)g * G::A;
    for (int i = lane; i < G::APAD; i += 64) {                 // slot i by lane i & 63, as everywhere in the engine
        const bool in = i < G::A;
        c.cP[sb + i] = in ? P32[t + i] : 0.f;
        c.cN[sb + i] = in ? N[t + i] : 0;
        c.cW[sb + i] = 0.f;
        c.cQ[sb + i] = in ? Q[t + i] : 0.f;
        c.cB[sb + i] = -1;
        c.cBusy[sb + i] = (in && busy[t + i] > 0) ? 2 : 0;
        c.rootP64[(size_t)g * G::APAD + i] = (in && f64) ? P64[t + i] : 0.0;
    }
    for (int w = lane; w < G::NW; w += 64) {
        uint32_t m = 0;
        for (int b = 0; b < 32; b++) {
            const int i = 32 * w + b;
            if (i < G::A && legal[t + i]) m |= 1u << b;
        }
        c.legal[pb * G::NW + w] = m;
    }
    __threadfence();                                           // the legal words are read by other lanes than their writers
    __syncthreads();
    int child = -1;
    const int a = e.top_one(blk, f64 != 0, child);
    if (lane == 0) out[g] = a;
}

// ---------------------------------------------------------------------------------------- the stages of one k_search launch
// What one launch of k_search holds for its game: the GameState copy (in registers, see the inlining rule at the top of this
// file), the `run` flag -- false = the launch is over for this game: it waits for evaluations, has failed or is done -- and the
// launch's pointers.  Every member is one stage of play_game_async (nomodel_self_play.py:142-271); k_search below is the state
// machine that orders them.  Inside a stage the order of memory and float operations is part of the contract (trees are compared
// byte for byte).
template <int S>
struct Search {
    using G = Geo<S>;
    const Ctx &c;
    const Eng<S> e;
    const int g, lane;                  // e.g, e.lane: the game slot and the lane (one wavefront per game)
    GameState st;
    bool run = true;
    int32_t *const queue;               // LDS [L]: reroot's copy of the parent array
    int32_t *const sN;                  // LDS [APAD]: the root's counts for choose_move (-1: no such child)
    float *const sQ;                    // LDS [APAD]: the root's means
    const float *const policy, *const value;
    const int32_t *const lut;           // the step's symmetry: policy row index of every action
    const size_t fbase, rbase;          // the game's rows of the FIFO and of the request arrays

    // sym_k: the immediate, or a device-side value so that one captured launch chain serves every symmetry
    __device__ __forceinline__ Search(const Ctx &cc, int gg, int32_t *lds, const float *pol, const float *val, int sym_k_imm,
                                      const int32_t *sym_k_dev)
        : c(cc), e(cc, gg), g(e.g), lane(e.lane), st(cc.gs[gg]), queue(lds), sN(lds + cc.L), sQ((float *)(lds + cc.L + G::APAD)),
          policy(pol), value(val), lut(cc.symLut + (size_t)(sym_k_dev ? (*sym_k_dev & 7) : sym_k_imm) * G::A),
          fbase((size_t)gg * (2 * MAXE)), rbase((size_t)gg * cc.E) {}

    // the game is over (get_winner at play_game_async's tail, nomodel_self_play.py:227-233): score the root position, set the result
    __device__ __forceinline__ void finish(int reason) {
        st.end_reason = reason;
        int bp = 0, wp = 0;
        if (lane == 0) score_record<S>(c.pos + e.ph(st.root_blk) * G::RW, bp, wp);
        bp = __shfl(bp, 0);
        wp = __shfl(wp, 0);
        double white = (double)wp + c.cfg.komi;
        st.winner = ((double)bp > white) ? 1 : (((double)bp == white) ? 0 : -1);
        st.black = bp;
        st.white = white;
        st.n_moves = st.move_n;
        st.last_player = st.player;
        st.phase = PH_DONE;
        run = false;
    }
    // the first error wins; the slot waits for a restart
    __device__ __forceinline__ void fail(int code) {
        if (!st.error) st.error = code;
        st.phase = PH_DONE;
        run = false;
    }
    // ask for the evaluation of the root position; the launch is over for this game
    __device__ __forceinline__ void request_root() {
        st.root_requested = 1;
        if (lane == 0) c.reqBlk[rbase] = (int32_t)e.ph(st.root_blk);
        st.n_req = 1;
        st.req_kind = 0;
        run = false;
    }

    // PH_WAIT_ROOT, nomodel_self_play.py:165-178: the root's value, the resign test, new_tree (play.py:376-389) with or without
    // Dirichlet noise, and the round budget of the move's search
    __device__ __forceinline__ void consume_root_eval() {
        if (!st.root_requested) { request_root(); return; }
        st.root_requested = 0;
        const float *prow = policy + (size_t)st.eval_base * G::A;
        st.value = value[st.eval_base];
        st.has_value = 1;
        st.n_predict++;
        if (lane == 0) atomicAdd(&c.counters->total_evals, 1ull);
        // resign = resign_model1 if current == model1 else resign_model2 (nomodel_self_play.py:170-173)
        const bool use2 = c.cfg.two_model && st.cur_model == 1;
        // a search-only slot (sgo_session_analyze) has no resign test
        if (!st.analysis && (use2 ? (st.has_resign2 && st.value <= st.resign2) : (st.has_resign && st.value <= st.resign))) {
            // a session slot resigns without ending (sejonggo_nomodel.py:58-60 genmove): play_move records action -1 and holds
            if (st.session) { st.end_reason = 1; st.rounds_left = 0; st.phase = PH_SEARCH; }
            else finish(1);
            return;
        }
        // "if not mcts_tree or not mcts_tree['subtree']": the root block carries children iff flag set
        bool expanded = c.bSlot[e.ph(st.root_blk)] != -2;  // -2 marks "block holds no children yet"
        if (!expanded) {
            const double *noise = nullptr;
            if (c.cfg.self_play && !st.session) {      // a session's tree never gets noise (sejonggo_nomodel.py:22 add_noise=False)
                if (st.noise_used) fail(SGO_ERR_DRAWS);
                noise = c.noise + (size_t)g * G::APAD;
                st.noise_used = 1;
            }
            if (run) {
                e.expand(st.root_blk, prow, lut, noise, c.cfg.dirichlet_epsilon);
                if (lane == 0) c.bSlot[e.ph(st.root_blk)] = -1;
                st.root_f64 = noise ? 1 : 0;
                st.root_count = 0;
                st.root_value = 0.f;
                st.root_mean = 0.f;
            }
        }
        if (run) {
            st.rounds_left = st.analysis ? st.an_rounds : c.cfg.sims / c.cfg.energy;
            // search-only: play_move finds end_reason set, as for a session that resigns, and records and holds without choosing
            if (st.analysis) st.end_reason = 2;
            st.e_left = -1;
            st.original_player = white_to_play<S>(c.pos + e.ph(st.root_blk) * G::RW) ? -1 : 1;
            st.phase = PH_SEARCH;
            if (c.cfg.sims < c.cfg.energy) fail(SGO_ERR_STATE);  // zero simulations: the reference cannot pick a move
        }
    }

    // PH_SEARCH: every not-yet-evaluated FIFO entry was evaluated by the previous step -- new_subtree for each
    // (simulation_workers.py:42-54), then the back-propagation a blocked select_round left for this launch
    __device__ __forceinline__ void consume_leaf_evals() {
        for (int fi = st.fifo_head; fi < st.fifo_tail; fi++) {
            const size_t fo = fbase + (fi % (2 * MAXE));
            if (c.fEvaluated[fo]) continue;
            const int row = st.eval_base + c.fEvalLocal[fo];
            e.expand(c.fBlk[fo], policy + (size_t)row * G::A, lut, nullptr, 0.0);
            if (lane == 0) {
                c.fValue[fo] = value[row];
                c.fEvaluated[fo] = 1;
                atomicAdd(&c.counters->total_evals, 1ull);
            }
            st.n_predict++;
        }
        __syncthreads();
        if (st.need_bp) {
            st.need_bp = 0;
            e.back_propagate(st, st.fifo_head % (2 * MAXE));
            st.fifo_head++;
            st.pre_bp++;
        }
    }

    // One round of async_simulate2 (nomodel_self_play.py:59-82): up to `energy` leaves, each flagged busy, given a block and
    // queued for evaluation.  Returns true when the round is blocked on an evaluation that this step has yet to deliver.
    __device__ __forceinline__ bool select_round() {
        bool blocked = false;
        int resume = -1;                         // parent of the leaf selected last in this round; -1 = walk from the root
        while (st.e_left > 0) {
            int pb = -1, slot = -1;
            bool found = e.find_best_leaf(st, pb, slot, resume);
            resume = found ? pb : -1;
            if (found) {
                int n = 0;
                if (lane == (slot & 63)) n = c.cN[e.slot_base(pb) + slot];
                n = __shfl(n, slot & 63);
                if (n > 0) { st.e_left--; st.pre_bp++; continue; }   // "already simulated leaf node"
            } else {
                st.none_events++;
                if (lane == 0) atomicAdd(&c.counters->none_events, 1ull);
                if (st.fifo_tail == st.fifo_head) { fail(SGO_ERR_STATE); break; }  // the reference would block forever
                if (!c.fEvaluated[fbase + (st.fifo_head % (2 * MAXE))]) { st.need_bp = 1; blocked = true; break; }
                e.back_propagate(st, st.fifo_head % (2 * MAXE));   // statistics moved: the next walk starts at the root (resume = -1)
                st.fifo_head++;
                st.pre_bp++;
                continue;
            }
            const int nb = e.alloc(st);
            if (nb < 0) { fail(SGO_ERR_CAPACITY); break; }
            const size_t fo = fbase + (st.fifo_tail % (2 * MAXE));
            if (lane == 0) {
                c.bParent[e.ph(nb)] = pb;
                c.bSlot[e.ph(nb)] = slot;
                c.fParent[fo] = pb; c.fSlot[fo] = slot; c.fBlk[fo] = nb;
                c.fEvalLocal[fo] = st.n_req; c.fEvaluated[fo] = 0;
                c.reqBlk[rbase + st.n_req] = (int32_t)e.ph(nb);
                c.reqParent[rbase + st.n_req] = (int32_t)e.ph(pb);
                c.reqMove[rbase + st.n_req] = slot;
            }
            st.fifo_tail++;
            st.n_req++;
            st.req_kind = 1;
            st.e_left--;
        }
        return blocked;
    }

    // The round's back-propagations in FIFO order (nomodel_self_play.py:73-82), once every leaf of the round is evaluated.
    // Returns false when the launch ends here: evaluations are pending, or the FIFO ran dry (an error).
    __device__ __forceinline__ bool close_round() {
        bool pending = false;
        for (int fi = st.fifo_head; fi < st.fifo_tail; fi++)
            if (!c.fEvaluated[fbase + (fi % (2 * MAXE))]) pending = true;
        if (pending) return false;
        const int nbp = c.cfg.energy - st.pre_bp;
        bool bad = false;
        for (int i = 0; i < nbp; i++) {
            if (st.fifo_head == st.fifo_tail) { bad = true; break; }
            e.back_propagate(st, st.fifo_head % (2 * MAXE));
            st.fifo_head++;
        }
        if (bad) { fail(SGO_ERR_STATE); return false; }
        st.e_left = -1;
        st.rounds_left--;
        return true;
    }

    // select_play (nomodel_self_play.py:114-140) on the root block whose slots start at `sb`: lane 0 samples the visit counts
    // through a float64 cdf at temperature 1 (np.cumsum / searchsorted) or takes the argmax with the reference's tie rule (count,
    // then mean, then the HIGHER index).  Returns 0 and the action in `selected`, or an error code.
    __device__ __forceinline__ int choose_move(size_t sb, int &selected) {
        for (int i = lane; i < G::APAD; i += 64) {
            bool ex = e.legal_bit(st.root_blk, i);
            sN[i] = ex ? c.cN[sb + i] : -1;
            sQ[i] = ex ? c.cQ[sb + i] : 0.f;
        }
        __syncthreads();
        selected = -1;
        int err = 0;
        if (lane == 0) {
            if (st.temperature == 1) {
                long total = 0;
                for (int i = 0; i < G::A; i++) if (sN[i] > 0) total += sN[i];
                double last = 0;
                for (int i = 0; i < G::A; i++) if (sN[i] > 0) last += (double)sN[i] / (double)total;  // np.cumsum
                if (total == 0 || st.i_uniform >= st.n_uniform) err = SGO_ERR_DRAWS;
                else {
                    double u = c.uniforms[(size_t)g * c.max_moves + st.i_uniform];
                    double acc = 0;
                    int lastmv = -1;
                    for (int i = 0; i < G::A; i++) {
                        if (sN[i] <= 0) continue;
                        acc += (double)sN[i] / (double)total;
                        lastmv = i;
                        if (acc / last > u) { selected = i; break; }   // searchsorted(cdf/cdf[-1], u, 'right')
                    }
                    if (selected < 0) selected = lastmv;
                }
            } else {
                int bc = -1, ba = -1;
                float bm = 0;
                for (int i = 0; i < G::A; i++) {
                    if (sN[i] < 0) continue;
                    if (child_beats(sN[i], sQ[i], i, bc, bm, ba)) { bc = sN[i]; bm = sQ[i]; ba = i; }
                }
                selected = ba;
            }
        }
        selected = __shfl(selected, 0);
        err = __shfl(err, 0);
        return err;
    }

    // the move_data row of the move (nomodel_self_play.py:183-195): the record, the packed root position and the prior vector.
    // Returns false (failed) when the record buffer is full.
    __device__ __forceinline__ bool record_move(size_t sb, int selected) {
        int ri = 0;
        if (lane == 0) ri = atomicAdd(&c.counters->rec_count, 1);
        ri = __shfl(ri, 0);
        if (ri >= c.rec_cap) { fail(SGO_ERR_CAPACITY); return false; }
        if (lane == 0) {
            sgo_move_record r;
            r.game = g; r.game_seq = st.game_seq; r.move_n = st.move_n; r.action = selected;
            r.player = st.player; r.value = st.value;
            c.recs[ri] = r;
            if (selected != SGO_ACTION_ANALYSIS) atomicAdd(&c.counters->total_moves, 1ull);   // a search-only record is no move
        }
        for (int i = lane; i < G::RW; i += 64) c.recPacked[(size_t)ri * G::RW + i] = c.pos[e.ph(st.root_blk) * G::RW + i];
        for (int i = lane; i < G::A; i += 64) {
            double p = 0;
            if (selected != -1 && e.legal_bit(st.root_blk, i)) p = st.root_f64 ? c.rootP64[(size_t)g * G::APAD + i] : (double)c.cP[sb + i];
            c.recPolicy[(size_t)ri * G::A + i] = p;
        }
        return true;
    }

    // Two-model games (self_play == False, nomodel_self_play.py:203-208): the other player's tree follows the move when
    // it holds it ("if other_mcts and index in other_mcts['subtree']"); a child that was never evaluated there has an
    // empty subtree, i.e. the tree is rebuilt by new_tree() when its owner moves next -- here: no block, -1 is returned.
    __device__ __forceinline__ int other_tree_follows(int selected) {
        int onr = -1;
        if (c.cfg.two_model && st.other_root >= 0 && c.bSlot[e.ph(st.other_root)] != -2) {
            const size_t osb = e.slot_base(st.other_root);
            int ocb = -1, oc = 0; float ov = 0, om = 0;
            if (lane == (selected & 63) && e.legal_bit(st.other_root, selected)) {
                ocb = c.cB[osb + selected]; oc = c.cN[osb + selected]; ov = c.cW[osb + selected]; om = c.cQ[osb + selected];
            }
            onr = __shfl(ocb, selected & 63);
            st.other_count = __shfl(oc, selected & 63);
            st.other_value = __shfl(ov, selected & 63);
            st.other_mean = __shfl(om, selected & 63);
        }
        return onr;
    }

    // the block behind the chosen slot: the next root (-1: the slot was never expanded, which a searched root's choice cannot be)
    __device__ __forceinline__ int chosen_child(size_t sb, int selected) {
        int nr = 0;
        if (lane == (selected & 63)) nr = c.cB[sb + selected];
        return __shfl(nr, selected & 63);
    }

    // Re-root onto the chosen child `nr` (nomodel_self_play.py:212-213, "Cut the tree"): its statistics become the root's, and
    // every block that is no longer reachable is recycled.  Returns the colour that made the move; `onr` = the root block of the
    // other player's tree after the move (-1: none).  It cannot fail: the one test (nr >= 0) stays in play_move, because a
    // failing return from in here cost 3 VGPRs in every k_search<S> (measured).
    __device__ __forceinline__ int reroot(size_t sb, int selected, int nr, int &onr) {
        float rv = 0, rm = 0; int rc = 0;
        if (lane == (selected & 63)) { rc = c.cN[sb + selected]; rv = c.cW[sb + selected]; rm = c.cQ[sb + selected]; }
        st.root_count = __shfl(rc, selected & 63);
        st.root_value = __shfl(rv, selected & 63);
        st.root_mean = __shfl(rm, selected & 63);
        const int mover = white_to_play<S>(c.pos + e.ph(st.root_blk) * G::RW) ? -1 : 1;
        onr = other_tree_follows(selected);
        st.root_blk = nr;
        st.root_f64 = 0;
        if (lane == 0) {
            c.bParent[e.ph(nr)] = -1; c.bSlot[e.ph(nr)] = -1;
            if (onr >= 0) { c.bParent[e.ph(onr)] = -1; c.bSlot[e.ph(onr)] = -1; }
        }
        // mark: which blocks hang below the new root(s)?  Every allocated block is linked from its parent exactly once (the
        // graft in back_propagate) and carries that parent in bParent, so "reachable from the new root" = "the parent chain
        // ends in it".  All chains are resolved together by pointer jumping on a copy of the parent array in LDS:
        // O(log depth) passes of cap / 64 coalesced steps, instead of a breadth-first walk that paid one dependent memory
        // round trip per CHILD ARRAY of every kept block (22 ms for a late-game tree, measured; now tens of microseconds).
        constexpr int KEEP = -3, DROP = -4;
        int *par = queue;
        // local ids in use or used before: the private region plus the overflow ids backed so far in this game; ids beyond
        // Lu have never left the bottom of the free stack (entries [0, L - Lu), untouched here)
        const int Lu = c.cap + st.ovf_hi, base = c.L - Lu;
        for (int b = lane; b < Lu; b += 64) {
            int pv = DROP;
            if (b < c.cap) pv = c.bParent[e.gb0 + b];
            else {
                const int ob = c.ovfMap[(size_t)g * c.ovf_cap + (b - c.cap)];      // -1: not backed = free
                if (ob >= 0) pv = c.bParent[(size_t)c.G * c.cap + ob];
            }
            par[b] = pv < 0 ? DROP : pv;                       // other roots (the old one): dropped
        }
        __syncthreads();
        for (int i = base + lane; i < st.free_top; i += 64) par[c.freeList[(size_t)g * c.L + i]] = DROP;   // stale parents of free blocks
        __syncthreads();
        if (lane == 0) { par[nr] = KEEP; if (onr >= 0) par[onr] = KEEP; }
        __syncthreads();
        for (;;) {
            bool open = false;
            for (int b = lane; b < Lu; b += 64) {
                const int pv = par[b];
                if (pv >= 0) {
                    const int pp = par[pv];                    // KEEP / DROP resolve b; otherwise jump to the grandparent
                    par[b] = pp;
                    open |= pp >= 0;
                }
            }
            __syncthreads();
            if (!__any(open)) break;
        }
        // rebuild the stack above `base`, ids DESCENDING so that the private ids pop before the overflow ids; an overflow id
        // that is free now gives its block back to the shared pool (poolRet: merged into poolFree by k_compact, so a pop in
        // this launch never meets a push)
        int ft = base;
        for (int b1 = ((Lu + 63) & ~63); b1 > 0; b1 -= 64) {
            const int b = b1 - 1 - lane;
            const bool fr = b < Lu && par[b] != KEEP;
            const unsigned long long m = __ballot(fr);
            if (fr) {
                c.freeList[(size_t)g * c.L + ft + __popcll(m & ((1ull << lane) - 1ull))] = b;
                if (b >= c.cap) pool_release(c, (size_t)g * c.ovf_cap + (b - c.cap));
            }
            ft += __popcll(m);
        }
        st.free_top = ft;
        __syncthreads();
        return mover;
    }

    // Two-model games: the other player's tree becomes the tree that is searched next.  Returns false (failed) when there is
    // no block for its root.
    __device__ __forceinline__ bool adopt_other_tree(int onr) {
        const int nr = st.root_blk;
        if (onr < 0) {
            // the other player's tree is empty: a fresh root block holding the position after the move (a copy of the
            // mover's new root), unexpanded -- new_tree() fills it when that player's root evaluation arrives
            onr = e.alloc(st);
            if (onr < 0) { fail(SGO_ERR_CAPACITY); return false; }
            for (int i = lane; i < G::RW; i += 64) c.pos[e.ph(onr) * G::RW + i] = c.pos[e.ph(nr) * G::RW + i];
            for (int i = lane; i < G::NW; i += 64) c.legal[e.ph(onr) * G::NW + i] = c.legal[e.ph(nr) * G::NW + i];
            if (lane == 0) { c.bParent[e.ph(onr)] = -1; c.bSlot[e.ph(onr)] = -2; }
            st.other_count = 0; st.other_value = 0.f; st.other_mean = 0.f;
            __syncthreads();
        }
        // mcts_tree, other_mcts = other_mcts, mcts_tree (:218) and the models swap (:217)
        const int tb = st.root_blk, tc = st.root_count; const float tv = st.root_value, tm = st.root_mean;
        st.root_blk = onr; st.root_count = st.other_count; st.root_value = st.other_value; st.root_mean = st.other_mean;
        st.other_root = tb; st.other_count = tc; st.other_value = tv; st.other_mean = tm;
        st.cur_model ^= 1;
        return true;
    }

    // The round budget is spent: select_play's tail + the body of play_game_async's loop (nomodel_self_play.py:125-138,
    // :180-216).  Every path ends the launch for this game: it failed, finished, halted, or waits for its new root's evaluation.
    __device__ __forceinline__ void play_move() {
        if (st.halt_at == st.move_n) { st.phase = PH_DONE; run = false; return; }
        const size_t sb = e.slot_base(st.root_blk);
        // end_reason is set here only by a session slot: 1 = it resigns (action -1, a zero policy row), 2 = its search was an
        // analysis (action SGO_ACTION_ANALYSIS = -2, the root's prior row).  No move is chosen then.
        int selected = -st.end_reason;
        if (!st.end_reason) {
            const int err = choose_move(sb, selected);
            if (err) { fail(err); return; }
        }
        if (st.temperature == 1) st.i_uniform++;
        if (!record_move(sb, selected)) return;
        // the resign / analysis record is all that happens: board, tree and move_n stay, the slot holds again
        if (selected < 0) { st.end_reason = 0; st.phase = PH_HOLD; run = false; return; }
        st.n_moves = st.move_n + 1;
        const bool is_pass = (selected == G::N);
        if (st.skipped_last && is_pass && !st.session) { finish(2); st.n_moves = st.move_n + 1; return; }   // BOTH_PASSED (:197-199)
        st.skipped_last = is_pass ? 1 : 0;
        const int nr = chosen_child(sb, selected);
        if (nr < 0) { fail(SGO_ERR_STATE); return; }
        int onr = -1;
        const int mover = reroot(sb, selected, nr, onr);
        if (c.cfg.two_model && !adopt_other_tree(onr)) return;
        // board, player = make_play(...): the new root block already holds the position after the move
        st.player = mover;
        st.move_n++;
        // a session slot (csrc/sgo_session.hpp) never ends by itself -- a GTP game goes on after two passes and has no move limit
        // -- and HOLDS after its move instead of asking for its next root evaluation.  The hold is three selects on the common
        // path, not an exit of its own: a separate `if (st.session) return` cost 11 VGPRs in every k_search<S> (measured).
        if (st.move_n >= c.max_moves && !st.session) { finish(0); return; }
        st.last_value = st.value;
        if (st.move_n == c.cfg.stop_exploration) st.temperature = 0;
        request_root();
        st.phase = st.session ? PH_HOLD : PH_WAIT_ROOT;
        st.root_requested = st.session ? 0 : 1;
        st.n_req = st.session ? 0 : 1;
    }

    // a game that has just failed (its tree is abandoned; the slot waits for a restart) hands its shared blocks back at once,
    // so that one starved game does not starve its neighbours for the steps until the host reacts
    __device__ __forceinline__ void release_on_error() {
        if (st.error && st.ovf_hi > 0) {
            for (int j = lane; j < st.ovf_hi; j += 64) pool_release(c, (size_t)g * c.ovf_cap + j);
            st.ovf_hi = 0;
        }
    }
};

// ---------------------------------------------------------------------------------------- k_search
// The game's state machine, one wavefront per game and launch: play_game_async (nomodel_self_play.py:142-271) cut where it
// would wait for the network.  load state -> consume the evaluations the previous step requested -> rounds of async_simulate2
// (or the move, when the budget is spent) until evaluations are needed -> release on error -> store state.
// Diagnostic build (-DSGO_KSEARCH_PROFILE): cycles per phase summed into Counters::dbg -- [0] consuming evaluations, [7] the
// round's back-propagation (loop turn-around), [1] round set-up, [2] selection, [3] the move step, [4] launches (waves).
#ifdef SGO_KSEARCH_PROFILE
#define SGO_TICK(k) do { tq1 = clock64(); if (s.lane == 0) atomicAdd(&c.counters->dbg[k], (unsigned long long)(tq1 - tq0)); tq0 = tq1; } while (0)
#else
#define SGO_TICK(k) do { } while (0)
#endif
template <int S>
__global__ __launch_bounds__(64) void k_search(Ctx c, const float *policy, const float *value, int sym_k_imm, const int32_t *sym_k_dev) {
    extern __shared__ int32_t lds[];            // search_lds<S>(c) bytes: queue[L], sN[APAD], sQ[APAD], reserved tail
    const int g = blockIdx.x;
    Search<S> s(c, g, lds, policy, value, sym_k_imm, sym_k_dev);
    GameState &st = s.st;
    st.n_req = 0;
    if (st.phase == PH_IDLE || st.phase == PH_DONE || st.phase == PH_HOLD) {
        if (s.lane == 0) c.gs[g].n_req = 0;
        return;
    }
#ifdef SGO_KSEARCH_PROFILE
    long long tq0 = clock64(), tq1;
#endif
    if (st.phase == PH_WAIT_ROOT) s.consume_root_eval();
    else s.consume_leaf_evals();
    SGO_TICK(0);
    while (s.run && st.phase == PH_SEARCH) {
        SGO_TICK(7);
        if (st.rounds_left == 0) { s.play_move(); break; }
        if (st.e_left < 0) { st.e_left = c.cfg.energy; st.pre_bp = 0; }
        SGO_TICK(1);
        const bool blocked = s.select_round();
        SGO_TICK(2);
        __syncthreads();
        if (!s.run || blocked) break;
        if (!s.close_round()) break;
    }
    SGO_TICK(3);
#ifdef SGO_KSEARCH_PROFILE
    if (s.lane == 0) atomicAdd(&c.counters->dbg[4], 1ull);
#endif
    s.release_on_error();
    if (s.lane == 0) c.gs[g] = st;
}
#undef SGO_TICK

}  // namespace sgo
