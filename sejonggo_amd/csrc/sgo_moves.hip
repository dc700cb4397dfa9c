// sgo_moves.hip -- move outcomes on the device (include/sgo.h "move outcomes"): per packed record and per point of the board what
// one ply by the chosen side on that point does (captures, the new chain's size and liberties, the chains it joins, the ataris it
// gives), and a per-record summary.  A translation unit of its own, like sgo_tactics.hip and sgo_life.hip:
// tests/test_engine_isa.py pins the kernel set of sgo_engine.hip.
//
//   k_moves<S>   per listed record: the table int16 [N][8] and the eight counts
//
// sgo_session_moves runs the same kernel over the context's records, with the root index k_session_roots (sgo_session.hpp) writes.
//
// Kernel form: one 32-lane HALF of a wavefront per listed row, one board row per lane (sgo_rows.hpp), one wavefront per workgroup:
// the form of k_tactics_chains.  The rules are rows::Board<S>::advance / legal / flood: nothing is restated.
//   QUIET points (empty, no stone among the four neighbours) are all done at once with row bit operations: the stone stands alone
//     with one liberty per on-board neighbour, nothing is captured, joined or put in atari, and Board::legal has them in its e1
//     set.  They cost no flood; on an opening board that is almost every point.
//   CONTACT points (empty, next to a stone) are walked one by one in ascending order: one advance on a copy of the rows, one flood
//     for the mover's new chain, and one flood per distinct chain on the (at most four) neighbouring stones, for the opponent in
//     P' (ataris) and for the mover before the ply (joined, weakest).
//   joined / weakest are measured PER CANDIDATE, not from a chain pass per record.  A chain pass would have to keep the liberty
//     count (9 bits at 19x19, there is no saturation) and a chain number (8 bits) of every point as 17 row bit-planes in registers
//     and pick the four neighbours' values out of three lanes with a shuffle per plane; the direct form is at most four short
//     floods that the whole wave skips when neither half's candidate touches a stone of the mover, and it shares its loop with the
//     atari count.
// LOCKSTEP: the floods vote over the whole wave, so both halves run every loop in lockstep; the trip count of the candidate loop
// is the wave's, the larger of its two halves'.  A half that is done, idle or out of range goes on with an EMPTY board (its floods
// end at once) and only its stores differ.  No flood, advance or cross-lane operation sits under a per-half branch.  Everything
// lives in registers: no LDS, no scratch, no atomics (the counts are ballots and half_sum).
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_rows.hpp"

namespace sgo {

typedef uint32_t moves_u32x4 __attribute__((ext_vector_type(4)));

// one row of the table, int16[8] little-endian in four words: one 16-byte store
SGO_DEV moves_u32x4 moves_row(int flags, int captured, int size, int libs, int joined, int weakest, int ataris, int atari_stones) {
    moves_u32x4 v;
    v.x = (uint32_t)flags | ((uint32_t)captured << 16);
    v.y = (uint32_t)size | ((uint32_t)libs << 16);
    v.z = (uint32_t)joined | ((uint32_t)weakest << 16);
    v.w = (uint32_t)ataris | ((uint32_t)atari_stones << 16);
    return v;
}

// TRIPS: the candidate loop takes one trip per contact point of the half with more of them, at most N (every trip clears at
// least the seed from `rest`; a half without candidates left plays a pass on an empty board).  A trip makes one advance (at most
// four floods), one flood for the new chain, and two neighbour loops of at most four trips each (every trip clears at least one
// of the four neighbouring stones from `cand`) with one flood per trip: at most 13 floods per trip, 13 * N per launch and wave,
// plus what Board::legal takes once.  Termination does not depend on the data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_moves(int n, const uint32_t *records, int n_records, const int32_t *index, int side,
                                              moves_u32x4 *moves, int32_t *counts) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long i = (long)blockIdx.x * 2 + half;
    const bool valid = i < n;
    const int r = valid ? (index ? index[i] : (int)i) : -1;
    const bool ok = r >= 0 && r < n_records;                         // uniform over the half
    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    const rows::Board<S> bd(half, y);
    const uint32_t rb = rec ? rows::load_row<S>(rec, y) : 0u, rw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
    const bool mover_white = rec ? (((rec[G::META_WORD] & G::META_BIT) != 0) != (side != 0)) : false;
    const uint32_t own = mover_white ? rw : rb, opp = mover_white ? rb : rw;
    // prev exists only for the record's side to move; without it prev = own, which forbids nothing
    const uint32_t prev = (rec && side == 0) ? rows::load_row<S>(rec + (mover_white ? 3 : 2) * G::NW, y) : own;
    const uint32_t emp = ok ? (~(own | opp) & bd.M) : 0u;
    const uint32_t gone = prev & ~own;
    const uint32_t ko = rows::half_one_bit(gone, half) ? gone : 0u;
    const uint32_t lg_all = bd.legal(own, opp, prev);                // every half calls it: an out-of-range half has an empty board
    const uint32_t lg = ok ? lg_all : 0u;
    const uint32_t near = bd.nbr4(own | opp);
    const uint32_t contact = emp & near;

    int n_cap = 0, max_cap = 0, max_mv = -1, n_self = 0, n_atari = 0, n_esc = 0, n_fs = 0;
    moves_u32x4 *out = valid ? moves + (size_t)i * G::N : nullptr;
    uint32_t rest = contact;
    while (__any(rest != 0)) {
        const int a = lowest_point<S>(rest, half);                   // -1: this half has no candidate left
        const bool live = a >= 0;
        const int ay = live ? a / S : -1, ax = live ? a - ay * S : 0;
        const uint32_t pb = (y == ay) ? (1u << ax) : 0u;
        rest &= ~pb;
        const uint32_t own0 = live ? own : 0u, opp0 = live ? opp : 0u, emp0 = live ? emp : 0u;
        uint32_t o2 = own0, p2 = opp0;
        // advance returns early, ahead of its floods, for an OCCUPIED point.  That would be a per-half branch; it is never taken
        // here because every candidate comes from `emp` (and a pass places no stone).  Walking occupied points would break lockstep.
        (void)bd.advance(o2, p2, live ? a : G::N);                   // a pass on an empty board for a finished half
        const uint32_t taken = opp0 & ~p2;
        const int captured = __any(taken != 0) ? half_sum(__popc(taken)) : 0;            // most plies capture nothing: one vote
        const bool suicide = live && !rows::half_any(o2 & pb, half);
        const uint32_t emp2 = live ? (~(o2 | p2) & bd.M) : 0u;
        const uint32_t g = bd.flood(pb & o2, o2);
        // two counts of at most N = 361 in one sum: stones in the low half-word, liberties in the high one
        const int sl = half_sum(__popc(g) | (__popc(bd.nbr4(g) & emp2) << 16));
        const int size = sl & 0xffff, libs = sl >> 16;
        const uint32_t np = bd.nbr4(pb);
        // the opponent's chains of P' on the neighbours with exactly one liberty there
        int ataris = 0, atari_stones = 0;
        uint32_t cand = np & p2;
        while (__any(cand != 0)) {
            const int c0 = lowest_point<S>(cand, half);
            const uint32_t cb = (c0 >= 0 && y == c0 / S) ? (1u << (c0 % S)) : 0u;
            const uint32_t C = bd.flood(cb, p2);
            const int cs = half_sum(__popc(C) | (__popc(bd.nbr4(C) & emp2) << 16));
            if (c0 >= 0 && (cs >> 16) == 1) { ataris++; atari_stones += cs & 0xffff; }
            cand &= ~C;
        }
        // the mover's chains BEFORE the ply on the neighbours; the point itself is one of their liberties
        int joined = 0, weakest = 0;
        cand = np & own0;
        while (__any(cand != 0)) {
            const int c0 = lowest_point<S>(cand, half);
            const uint32_t cb = (c0 >= 0 && y == c0 / S) ? (1u << (c0 % S)) : 0u;
            const uint32_t C = bd.flood(cb, own0);
            const int L = half_sum(__popc(bd.nbr4(C) & emp0));
            if (c0 >= 0) { weakest = (joined == 0 || L < weakest) ? L : weakest; joined++; }
            cand &= ~C;
        }
        if (suicide) { ataris = 0; atari_stones = 0; }
        const bool allowed = rows::half_any(lg & pb, half), is_ko = rows::half_any(ko & pb, half);
        if (live) {
            if (allowed) {
                if (captured > 0) n_cap++;
                if (captured > max_cap) { max_cap = captured; max_mv = a; }
                if (libs == 1 && captured == 0) n_self++;
                if (ataris > 0) n_atari++;
                if (weakest == 1 && libs >= 2) n_esc++;
            } else if (!is_ko && !suicide) n_fs++;
            if (valid && y == ay) {
                const int flags = (allowed ? SGO_MOVES_ALLOWED : 0) | (is_ko ? SGO_MOVES_KO : 0) | (suicide ? SGO_MOVES_SUICIDE : 0);
                out[a] = moves_row(flags, captured, size, libs, joined, weakest, ataris, atari_stones);
            }
        }
    }

    // every lane takes part in the sum; only the stores are conditional
    const int n_allowed = half_sum(__popc(lg));
    if (valid) {
        if (y < S) {
            // the other points of this lane's row: stones, quiet points, and everything of an out-of-range row
            const int edge_y = (y == 0 ? 1 : 0) + (y == S - 1 ? 1 : 0);
#pragma unroll
            for (int x = 0; x < S; x++) {
                const uint32_t bit = 1u << x;
                if (contact & bit) continue;
                const int kf = (ko & bit) ? SGO_MOVES_KO : 0;
                moves_u32x4 v = moves_row(0, 0, 0, 0, 0, 0, 0, 0);
                if ((own | opp) & bit) v = moves_row(SGO_MOVES_OCCUPIED | kf, 0, 0, 0, 0, 0, 0, 0);
                else if (ok) v = moves_row(((lg & bit) ? SGO_MOVES_ALLOWED : 0) | kf, 0, 1, 4 - edge_y - (x == 0 ? 1 : 0) - (x == S - 1 ? 1 : 0), 0, 0, 0, 0);
                out[y * S + x] = v;
            }
        }
        if (y == 0) {
            int32_t *co = counts + (size_t)i * 8;
            co[0] = n_allowed; co[1] = n_cap; co[2] = max_cap; co[3] = ok ? max_mv : 0;
            co[4] = n_self; co[5] = n_atari; co[6] = n_esc; co[7] = n_fs;
        }
    }
}

int launch_moves(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int side, int16_t *d_moves,
                 int32_t *d_counts, hipStream_t st) {
    SGO_DISPATCH(S, k_moves<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(n, d_records, n_records, d_index, side,
                                                                         reinterpret_cast<moves_u32x4 *>(d_moves), d_counts));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_moves_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int side, int16_t *d_moves,
                  int32_t *d_counts, void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || (side != 0 && side != 1) || !d_records || !d_moves || !d_counts ||
        (reinterpret_cast<uintptr_t>(d_moves) & 15) != 0) {
        set_error("sgo_moves_dev: bad argument (unsupported size, n < 0, n_records < 0, side outside {0, 1}, a NULL record array or output, "
                  "d_moves not 16-byte aligned)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_moves(S, n, d_records, n_records, d_index, side, d_moves, d_counts, (hipStream_t)stream);
}

int sgo_moves(int S, int n, const uint32_t *records, int side, int16_t *moves, int32_t *counts) {
    if (!size_ok(S) || n < 0 || (side != 0 && side != 1) || !records || !moves || !counts) {
        set_error("sgo_moves: bad argument (unsupported size, n < 0, side outside {0, 1}, a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    // every row is written whole, so nothing of the caller's goes in
    const HostArray a[] = {{(size_t)n * S * S * 8 * sizeof(int16_t), nullptr, moves}, {(size_t)n * 8 * sizeof(int32_t), nullptr, counts}};
    return host_entry("sgo_moves", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_moves(S, n, d_records, n, nullptr, side, reinterpret_cast<int16_t *>(d[0]), reinterpret_cast<int32_t *>(d[1]), nullptr);
    });
}

}  // extern "C"
