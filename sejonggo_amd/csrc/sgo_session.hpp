// sgo_session.hpp -- interactive (session) slots: the kernels behind sgo_session_play, sgo_session_genmove / _analyze (the arming),
// sgo_session_setup and sgo_session_report.
// Included by sgo_session.hip only, after sgo_search.hpp: k_session_play re-roots with Search<S>::reroot itself, so it shares
// k_search's dynamic-LDS layout (search_lds) and its inlining rule.  It lives in a translation unit of its own because
// tests/test_engine_isa.py pins the kernel set of sgo_engine.hip; k_search is instantiated in sgo_engine.hip alone.
// What it restates of the reference (drsagitn/sejonggo): sejonggo_nomodel.py:20-100 SejongGoEngine -- :45-56 play, :58-76
// genmove -- on device trees.
//
// A session slot (GameState::session, set by sgo_session_open) waits in PH_HOLD between commands.  sgo_session_play changes its
// board, sgo_session_genmove arms it (PH_WAIT_ROOT); the ordinary sgo_step loop then runs one move's search and k_search puts
// the slot back into PH_HOLD (Search<S>::play_move, resign_hold).
#pragma once
#include "sgo_search.hpp"

namespace sgo {

// SejongGoEngine.play for the listed slots, one wavefront per slot.  The staging area holds slots[n], actions[n], colors[n]
// (0 = the side to move, +1 black, -1 white) and receives status[n].  A slot whose status is not SGO_OK is not written at all.
//   follow  the move is in turn and the root holds an evaluated child for it: the tree is re-rooted onto that child
//           (`mcts_tree = mcts_tree['subtree'][index]`, :49-51), unreachable blocks are recycled
//   fresh   anything else: the tree is dropped (`mcts_tree = None`, or a child with an empty subtree, which genmove replaces by
//           new_tree): block 0 becomes an unexpanded root holding make_play(position, action, colour) (play.py:226-242 -- suicide
//           executed, an out-of-turn colour played as the reference plays it) and its legal bits; every other block is free
// DEVIATION: with an out-of-turn colour the reference keeps the followed subtree's statistics and replays them over the changed
// board; device blocks store positions, so the tree is dropped there.
template <int S>
__global__ __launch_bounds__(64) void k_session_play(Ctx c, int n, StageLayout L) {
    extern __shared__ int32_t lds[];            // search_lds<S>(c) bytes, as k_search: reroot's parent copy lives in it
    using G = Geo<S>;
    const int k = blockIdx.x;
    if (k >= n) return;
    const int g = reinterpret_cast<const int32_t *>(c.stage + L.slots)[k];
    const int a = reinterpret_cast<const int32_t *>(c.stage + L.resign)[k];
    const int col = reinterpret_cast<const int32_t *>(c.stage + L.resign2)[k];
    int32_t *status = reinterpret_cast<int32_t *>(c.stage + L.first);
    Search<S> s(c, g, lds, nullptr, nullptr, 0, nullptr);
    GameState &st = s.st;
    const int lane = s.lane;
    // every test below is uniform over the wave
    const bool holds = holding(st);
    const uint32_t *rpos = c.pos + s.e.ph(holds ? st.root_blk : 0) * G::RW;
    const int rc = holds ? external_move_status<S>(rpos, a) : SGO_ERR_STATE;
    if (rc) {
        if (lane == 0) status[k] = rc;
        return;
    }
    int to_play;
    const bool in_turn = moves_in_turn<S>(rpos, col, to_play);
    const size_t sb = s.e.slot_base(st.root_blk);
    int nr = -1;
    if (in_turn && c.bSlot[s.e.ph(st.root_blk)] != -2 && s.e.legal_bit(st.root_blk, a)) nr = s.chosen_child(sb, a);
    if (nr >= 0) {
        int onr = -1;
        st.player = s.reroot(sb, a, nr, onr);
    } else {
        const size_t gb0 = s.e.gb0;
        // block 0 is private, so the new root never sits on a shared block; in == out (the root is block 0) is the in-place form
        if (lane == 0) (void)advance_record<S>(rpos, c.pos + gb0 * G::RW, a, !in_turn, c.legal + gb0 * G::NW);
        // the allocator as k_start leaves it (min_free, the game's high-water mark, stays)
        for (int j = lane; j < st.ovf_hi; j += 64) pool_release(c, (size_t)g * c.ovf_cap + j);
        for (int b = lane; b < c.L - 1; b += 64) c.freeList[(size_t)g * c.L + b] = c.L - 1 - b;
        st.free_top = c.L - 1;
        st.ovf_hi = 0;
        st.root_blk = 0;
        st.root_f64 = 0;
        st.root_count = 0;
        st.root_value = 0.f;
        st.root_mean = 0.f;
        st.fifo_head = st.fifo_tail = 0;
        if (lane == 0) { c.bParent[gb0] = -1; c.bSlot[gb0] = -2; }
        st.player = in_turn ? to_play : -to_play;
    }
    st.move_n++;
    if (lane == 0) {
        // the fields a play changes (reroot: the root and its statistics, free_top; the fresh path: the allocator and the FIFO too),
        // stored one by one: storing the struct whole put it into scratch memory in this kernel (160 B per lane)
        GameState &d = c.gs[g];
        d.move_n = st.move_n; d.player = st.player;
        d.root_blk = st.root_blk; d.root_f64 = st.root_f64;
        d.root_count = st.root_count; d.root_value = st.root_value; d.root_mean = st.root_mean;
        d.free_top = st.free_top; d.ovf_hi = st.ovf_hi;
        d.fifo_head = st.fifo_head; d.fifo_tail = st.fifo_tail;
        status[k] = SGO_OK;
    }
}

// sgo_session_genmove / sgo_session_analyze: arm the listed slots -- all of them, or none when one is not a holding session.  One
// block; the slot list is in the staging area, the verdict goes to its status word.  analysis != 0: the armed search is
// search-only and runs `rounds` rounds (GameState::analysis, an_rounds; Search<S>::consume_root_eval and play_move read them).
__global__ __launch_bounds__(1024) void k_session_arm(Ctx c, int n, StageLayout L, int analysis, int rounds) {
    const int32_t *slots = reinterpret_cast<const int32_t *>(c.stage + L.slots);
    int32_t *status = reinterpret_cast<int32_t *>(c.stage + L.first);
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        if (!holding(c.gs[slots[i]])) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (!bad) {
        for (int i = threadIdx.x; i < n; i += 1024) {
            GameState &s = c.gs[slots[i]];
            s.phase = PH_WAIT_ROOT;         // the next k_search asks for the root's evaluation (consume_root_eval)
            s.root_requested = 0;
            s.rounds_left = 0;
            s.e_left = -1;
            s.pre_bp = 0;
            s.need_bp = 0;
            s.analysis = analysis;
            s.an_rounds = rounds;
        }
    }
    if (threadIdx.x == 0) status[0] = bad ? SGO_ERR_STATE : SGO_OK;
}

// One thread per listed slot: the record index (physical block of c.pos) of the root position of a holding session, what
// sgo_game_board shows; anything else gets SGO_ERR_STATE and index -1.  The context is only read.  sgo_session_keys,
// sgo_session_tactics and sgo_rollout_start_sessions run their ordinary record kernels over c.pos with this index.
__global__ __launch_bounds__(64) void k_session_roots(Ctx c, int n, const int32_t *slots, int32_t *status, int32_t *index) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int g = slots[i];
    const GameState &s = c.gs[g];
    const int idx = holding(s) ? (int)phys_block(c, g, s.root_blk) : -1;
    status[i] = idx >= 0 ? SGO_OK : SGO_ERR_STATE;
    index[i] = idx;
}

// ---------------------------------------------------------------------------------------- sgo_session_setup
// Byte offsets into the session buffer (HostSide::sess_d) of one sgo_session_setup call: per listed slot its id, the length of
// its move list and where the list starts in actions / colors; status and fail_at come back from the front of the buffer.
struct SetupLayout {
    size_t status, fail_at, slots, n_moves, off, actions, colors, total;
};
static inline SetupLayout setup_layout(int n, size_t n_total) {
    SetupLayout L;
    const size_t w = al8(sizeof(int32_t) * (size_t)n), t = al8(sizeof(int32_t) * n_total);
    L.status = 0; L.fail_at = w; L.slots = 2 * w; L.n_moves = 3 * w; L.off = 4 * w; L.actions = 5 * w; L.colors = 5 * w + t;
    L.total = 5 * w + 2 * t;
    return L;
}

// sgo_session_open followed by the slot's move list through k_session_play, for every listed slot in one launch: one wavefront
// per slot.  The list is replayed into a copy of the record in LDS by lane 0 with k_session_play's own tests and its
// advance_record call (play.py:226-242 make_play: suicide executed, an out-of-turn colour played as the reference plays it), and
// the slot is written only after the last move went through: a refused slot (not a holding session; move j out of range or on
// an occupied point -> status, fail_at = j) is unchanged in every word.  A slot that went through is what k_start(session)
// and the fresh path of k_session_play leave: block 0 an unexpanded root with the position and its legal bits, every other
// block free, the shared blocks returned; the resign threshold of the slot stays.
template <int S>
__global__ __launch_bounds__(64) void k_session_setup(Ctx c, int n, uint8_t *buf, SetupLayout L) {
    using G = Geo<S>;
    __shared__ __attribute__((aligned(16))) uint32_t rec[G::RW];
    __shared__ __attribute__((aligned(16))) uint32_t lg[G::NW];
    __shared__ int32_t verdict[4];              // status, fail_at, player (who moved last), moves played
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= n) return;
    const int g = reinterpret_cast<const int32_t *>(buf + L.slots)[k];
    const int nm = reinterpret_cast<const int32_t *>(buf + L.n_moves)[k];
    const int off = reinterpret_cast<const int32_t *>(buf + L.off)[k];
    const int32_t *actions = reinterpret_cast<const int32_t *>(buf + L.actions) + off;
    const int32_t *colors = reinterpret_cast<const int32_t *>(buf + L.colors) + off;
    int32_t *status = reinterpret_cast<int32_t *>(buf + L.status), *fail_at = reinterpret_cast<int32_t *>(buf + L.fail_at);
    const GameState &old = c.gs[g];
    if (!holding(old)) {                                          // uniform over the wave
        if (lane == 0) { status[k] = SGO_ERR_STATE; fail_at[k] = -1; }
        return;
    }
    // the empty board and its legal set, as k_start writes them
    for (int i = lane; i < G::RW; i += 64) rec[i] = 0;
    for (int i = lane; i < G::NW; i += 64) lg[i] = empty_legal_word<S>(i);
    __syncthreads();
    if (lane == 0) {
        int rc = SGO_OK, j = 0, player = 1;
        for (; j < nm; j++) {
            const int a = actions[j], col = colors[j];
            rc = external_move_status<S>(rec, a);
            if (rc) break;
            int to_play;
            const bool in_turn = moves_in_turn<S>(rec, col, to_play);
            rc = advance_record<S>(rec, rec, a, !in_turn, lg);    // in == out: the in-place form, as k_session_play
            if (rc) break;
            player = in_turn ? to_play : -to_play;
        }
        verdict[0] = rc; verdict[1] = rc ? j : -1; verdict[2] = player; verdict[3] = j;
    }
    __syncthreads();
    if (verdict[0]) {
        if (lane == 0) { status[k] = verdict[0]; fail_at[k] = verdict[1]; }
        return;
    }
    // commit.  The state is k_start's for a session, with the threshold kept and the counters of the chain of plays.
    const size_t gb0 = (size_t)g * c.cap;
    for (int i = lane; i < G::RW; i += 64) c.pos[gb0 * G::RW + i] = rec[i];
    for (int i = lane; i < G::NW; i += 64) c.legal[gb0 * G::NW + i] = lg[i];
    for (int j = lane; j < c.ovf_cap; j += 64) pool_release(c, (size_t)g * c.ovf_cap + j);
    for (int b = lane; b < c.L - 1; b += 64) c.freeList[(size_t)g * c.L + b] = c.L - 1 - b;
    if (lane == 0) {
        GameState st;
        memset(&st, 0, sizeof st);
        st.phase = PH_HOLD;
        st.session = 1;
        st.player = verdict[2];
        st.move_n = verdict[3];
        st.e_left = -1;
        st.halt_at = -1;
        st.game_seq = old.game_seq + 1;
        st.has_resign = old.has_resign;
        st.resign = old.resign;
        st.has_resign2 = old.has_resign2;       // a session is never a two-model game (sgo_session_open refuses such a context):
        st.resign2 = old.resign2;               // carried for the record, first_model / cur_model stay 0 as k_start sets them
        st.other_root = -1;
        st.free_top = c.L - 1;
        st.min_free = c.L - 1;
        c.bParent[gb0] = -1;
        c.bSlot[gb0] = -2;
        c.gs[g] = st;
        status[k] = SGO_OK;
        fail_at[k] = -1;
    }
}

// ---------------------------------------------------------------------------------------- sgo_session_report
// One slot's report in the session buffer, in 4-byte words: hdr[8] = {status, to_play, root_count, root_value, root_mean,
// n_children, 0, 0}, N[A], Q[A], P[A], top[K], pv[K][D].
static inline __host__ __device__ size_t report_words(int A, int K, int D) { return 8 + 3 * (size_t)A + (size_t)K + (size_t)K * D; }

// the best child of block `blk` in choose_move's temperature-0 order (child_beats) among the children whose bit in `taken` is
// clear (bit j of a lane = slot lane + 64 * j); returns its slot or -1, its count in `bn` and its child block in `bcb`
template <int S>
__device__ __forceinline__ int best_child(const Ctx &c, const Eng<S> &e, int blk, uint32_t taken, int &bn, int &bcb) {
    using G = Geo<S>;
    constexpr int J = (G::APAD + 63) / 64;
    const size_t pb = e.ph(blk), sb = pb * (size_t)G::APAD;
    int bi = -1, cb = -1;
    float bq = 0.f;
    bn = -1;
#pragma unroll
    for (int j = 0; j < J; j++) {
        const int i = e.lane + 64 * j;
        if (i >= G::A || ((taken >> j) & 1u)) continue;
        if (!((c.legal[pb * G::NW + (i >> 5)] >> (i & 31)) & 1u)) continue;
        const int nv = c.cN[sb + i];
        const float qv = c.cQ[sb + i];
        if (child_beats(nv, qv, i, bn, bq, bi)) { bn = nv; bq = qv; bi = i; cb = c.cB[sb + i]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int on = __shfl_xor(bn, o), oi = __shfl_xor(bi, o), ocb = __shfl_xor(cb, o);
        const float oq = __shfl_xor(bq, o);
        if (oi >= 0 && child_beats(on, oq, oi, bn, bq, bi)) { bn = on; bq = oq; bi = oi; cb = ocb; }
    }
    bcb = cb;
    return bi;
}

// The listed holding sessions, one wavefront per slot: the root's statistics, its raw child tables (what sgo_root_table gives;
// N = -1: no such child), the K best children in choose_move's temperature-0 order and, below each, the principal variation: the
// same rule applied down the tree while the node is expanded and has a visited child, at most D moves.  Reads only.
template <int S>
__global__ __launch_bounds__(64) void k_session_report(Ctx c, int n, const int32_t *slots, int32_t *out, int K, int D) {
    using G = Geo<S>;
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= n) return;
    const int g = slots[k];
    int32_t *o = out + (size_t)k * report_words(G::A, K, D);
    const GameState &s = c.gs[g];
    if (!holding(s)) {                                            // uniform over the wave
        if (lane == 0) o[0] = SGO_ERR_STATE;
        return;
    }
    const Eng<S> e(c, g);
    const int rb = s.root_blk, f64 = s.root_f64;
    const size_t pb = e.ph(rb), sb = pb * (size_t)G::APAD;
    const bool expanded = c.bSlot[pb] != -2;
    int32_t *oN = o + 8, *top = o + 8 + 3 * G::A, *pv = top + K;
    float *oQ = reinterpret_cast<float *>(o + 8 + G::A), *oP = reinterpret_cast<float *>(o + 8 + 2 * G::A);
    int nc = 0;
    for (int i = lane; i < G::A; i += 64) {
        const bool ex = expanded && e.legal_bit(rb, i);
        oN[i] = ex ? c.cN[sb + i] : -1;
        oQ[i] = ex ? c.cQ[sb + i] : 0.f;
        oP[i] = ex ? (f64 ? (float)c.rootP64[(size_t)g * G::APAD + i] : c.cP[sb + i]) : 0.f;
        nc += ex ? 1 : 0;
    }
    nc = wave_sum_i(nc);
    for (int i = lane; i < K + K * D; i += 64) top[i] = -1;
    if (lane == 0) {
        o[0] = SGO_OK;
        o[1] = white_to_play<S>(c.pos + pb * G::RW) ? -1 : 1;
        o[2] = s.root_count;
        reinterpret_cast<float *>(o)[3] = s.root_value;
        reinterpret_cast<float *>(o)[4] = s.root_mean;
        o[5] = nc; o[6] = 0; o[7] = 0;
    }
    if (!expanded) return;
    __syncthreads();                                               // the -1 padding is written before the moves
    uint32_t taken = 0;
    for (int t = 0; t < K; t++) {
        int bn, node;
        const int a = best_child<S>(c, e, rb, taken, bn, node);
        if (a < 0) break;
        if (lane == (a & 63)) taken |= 1u << (a >> 6);
        if (lane == 0) { top[t] = a; if (D > 0) pv[(size_t)t * D] = a; }
        for (int d = 1; d < D && node >= 0; d++) {
            int nn;
            const int m = best_child<S>(c, e, node, 0u, bn, nn);
            if (m < 0 || bn <= 0) break;                           // no visited child
            if (lane == 0) pv[(size_t)t * D + d] = m;
            node = nn;
        }
    }
}

}  // namespace sgo
