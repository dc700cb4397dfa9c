// sgo_session.hpp -- interactive (session) slots: the kernels behind sgo_session_play and sgo_session_genmove.
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
    int rc = SGO_OK;
    if (!st.session || st.phase != PH_HOLD || st.error) rc = SGO_ERR_STATE;
    else if (a < 0 || a >= G::A) rc = SGO_ERR_RANGE;
    const uint32_t *rpos = c.pos + s.e.ph(rc ? 0 : st.root_blk) * G::RW;
    if (!rc && a < G::N && (((rpos[a >> 5] | rpos[G::NW + (a >> 5)]) >> (a & 31)) & 1u)) rc = SGO_ERR_OCCUPIED;
    if (rc) {
        if (lane == 0) status[k] = rc;
        return;
    }
    const int to_play = white_to_play<S>(rpos) ? -1 : 1;
    const bool in_turn = col == 0 || col == to_play;
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

// sgo_session_genmove: arm the listed slots -- all of them, or none when one is not a holding session.  One block; the slot list
// is in the staging area, the verdict goes to its status word.
__global__ __launch_bounds__(1024) void k_session_arm(Ctx c, int n, StageLayout L) {
    const int32_t *slots = reinterpret_cast<const int32_t *>(c.stage + L.slots);
    int32_t *status = reinterpret_cast<int32_t *>(c.stage + L.first);
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const GameState &s = c.gs[slots[i]];
        if (!s.session || s.phase != PH_HOLD || s.error) bad = 1;
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
        }
    }
    if (threadIdx.x == 0) status[0] = bad ? SGO_ERR_STATE : SGO_OK;
}

}  // namespace sgo
