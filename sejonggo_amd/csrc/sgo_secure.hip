// sgo_secure.hip -- securing moves on the device (include/sgo.h "securing moves"): per packed record and per empty point what ONE
// more stone of the chosen side makes pass-alive -- the ply of the rules, then unconditional life on the position after it -- and a
// per-record summary with the life sets before and after the best such stone.  A translation unit of its own, like sgo_moves.hip
// and sgo_life.hip: tests/test_engine_isa.py pins the kernel set of sgo_engine.hip.
//
//   k_secure<S>      per (listed record, EMPTY point): the table row {flags, alive, terr, dead}
//   k_secure_sum<S>  per listed record: the rows of the occupied points, the eight counts, the four sets
//
// sgo_session_secure runs the same kernels over the context's records, with the root index k_session_roots (sgo_session.hpp) writes.
//
// No rule is restated: the ply is rows::Board<S>::advance, ALLOWED is Board::legal with the `prev` handling of k_moves, and the
// fixed point is life_core (sgo_life_core.hpp), which k_life runs too.
//
// Kernel form of k_secure: one 32-lane HALF of a wavefront per (row, candidate), one board row per lane (sgo_rows.hpp), one wavefront
// per workgroup: the form k_tactics_read uses for (row, chain slot).  A candidate costs one advance and one fixed point, and there
// is no cheap class as k_moves' quiet points are (a lone stone can make a region vital by taking the one point that touched no
// chain), so the work is parallel over candidates.  A row's candidates are dealt to `ch` workgroups: workgroup c of the row takes
// the pairs c, c + ch, c + 2 ch, ... and its half h the (2k + h)-th EMPTY point of pair k, found by a popcount rank over the rows, so
// no half idles on a stone (only the last pair of a row with an odd number of empty points has an idle half).  The record, `prev`
// and Board::legal are read once per workgroup.  `ch` and the dealing are launch parameters (sgo_secure_mode) because DESIGN.md
// measures them; the words written do not depend on either.
// LOCKSTEP: the floods vote over the whole wave, so both halves run every loop in lockstep; both halves of a wave read the SAME row,
// so the trip count of the pair loop is the same for both.  A half without a candidate runs a pass and the fixed point on an EMPTY
// board (its floods end at once) and only its stores differ.  No flood, advance or cross-lane operation sits under a per-half
// branch.  Everything lives in registers: no LDS, no scratch, no atomics (the counts are ballots and half_sum).
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_life_core.hpp"
#include "sgo_rows.hpp"

namespace sgo {

typedef uint32_t secure_u32x2 __attribute__((ext_vector_type(2)));

// the launch shape of k_secure (secure_ch below): the waves a call should put on the chip before a workgroup takes more than one
// pair of candidates, the fewest workgroups per row, and the grid cap behind which workgroups stride over (row, workgroup) units
constexpr long SECURE_WAVES = 16384, SECURE_CH_MIN = 8, SECURE_GRID_CAP = 1L << 24;

// one row of the table, int16[4] little-endian in two words: one 8-byte store
SGO_DEV secure_u32x2 secure_row(int flags, int alive, int terr, int dead) {
    secure_u32x2 v;
    v.x = (uint32_t)flags | ((uint32_t)alive << 16);
    v.y = (uint32_t)terr | ((uint32_t)dead << 16);
    return v;
}

// What both kernels read of a record: the mover's rows, the opponent's, and the ko point (a set of at most one bit).
struct SecureSide {
    uint32_t own, opp, prev, ko;
};
template <int S>
SGO_DEV SecureSide secure_side(const uint32_t *rec, int side, int half, int y) {
    using G = Geo<S>;
    SecureSide s;
    const uint32_t rb = rec ? rows::load_row<S>(rec, y) : 0u, rw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
    const bool mover_white = rec ? (((rec[G::META_WORD] & G::META_BIT) != 0) != (side != 0)) : false;
    s.own = mover_white ? rw : rb;
    s.opp = mover_white ? rb : rw;
    // prev exists only for the record's side to move; without it prev = own, which forbids nothing
    s.prev = (rec && side == 0) ? rows::load_row<S>(rec + (mover_white ? 3 : 2) * G::NW, y) : s.own;
    const uint32_t gone = s.prev & ~s.own;
    s.ko = rows::half_one_bit(gone, half) ? gone : 0u;
    return s;
}

// the three counts of a position's life, each at most N = 361, in one sum: 10 bits apiece
SGO_DEV int secure_sums(uint32_t alive, uint32_t terr, uint32_t opp) {
    return half_sum(__popc(alive) | (__popc(terr) << 10) | (__popc(terr & opp) << 20));
}

// TRIPS: the outer loop takes cdiv(n * ch, gridDim.x) trips (one unless n * ch passes the grid cap); the pair loop at most
// cdiv(cdiv(N, 2), ch) trips, the same for both halves (they read the same row).  A trip makes one advance (at most four floods) and
// one life_core call ((chains + 1) * (5 N + 1) floods at most, sgo_life_core.hpp); Board::legal runs once per outer trip.  The rank
// walk clears one bit of a row per trip, at most S - 1.  Termination does not depend on the data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_secure(int n, const uint32_t *records, int n_records, const int32_t *index, int side, int ch,
                                               int by_point, secure_u32x2 *table) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const rows::Board<S> bd(half, y);
    const long units = (long)n * ch;
    for (long u = blockIdx.x; u < units; u += gridDim.x) {           // the whole workgroup
        const long i = u / ch;
        const int c = (int)(u - i * ch);
        const int r = index ? index[i] : (int)i;
        if (r < 0 || r >= n_records) continue;                       // uniform over the wave: k_secure_sum writes the zero rows
        const uint32_t *rec = records + (size_t)r * G::RW;
        const SecureSide s = secure_side<S>(rec, side, half, y);
        const uint32_t emp = ~(s.own | s.opp) & bd.M;
        const uint32_t lg = bd.legal(s.own, s.opp, s.prev);
        // the rank of this lane's first empty point among the empty points of the board
        const int cnt = __popc(emp);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const int v = __shfl_up(incl, o, 32);
            if (y >= o) incl += v;
        }
        const int excl = incl - cnt;
        const int n_emp = __shfl(incl, half * 32 + 31, 64);
        const int pairs = by_point ? (G::N + 1) / 2 : (n_emp + 1) / 2;
        secure_u32x2 *out = table + (size_t)i * G::N;
        for (int k = c; k < pairs; k += ch) {
            const int t = 2 * k + half;
            int mine = -1;                                           // the candidate, in the lane that holds its row
            if (by_point) {
                if (t < G::N && y == t / S && ((emp >> (t % S)) & 1u)) mine = t;
            } else if (t >= excl && t < incl) {
                uint32_t v = emp;
                for (int j = t - excl; j > 0; j--) v &= v - 1;       // no cross-lane operation in here
                mine = y * S + __builtin_ctz(v);
            }
            const uint32_t has = rows::half_ballot(mine >= 0, half);
            const int a = has ? __shfl(mine, half * 32 + (__ffs((int)has) - 1), 64) : -1;
            const bool live = a >= 0;                                // -1: this half has no candidate in this pair
            const int ay = live ? a / S : -1, ax = live ? a - ay * S : 0;
            const uint32_t pb = (y == ay) ? (1u << ax) : 0u;
            uint32_t o2 = live ? s.own : 0u, p2 = live ? s.opp : 0u;
            // advance returns early, ahead of its floods, for an OCCUPIED point.  That would be a per-half branch; it is never
            // taken here because every candidate comes from `emp` (and a pass places no stone).
            (void)bd.advance(o2, p2, live ? a : G::N);               // a pass on an empty board for an idle half
            uint32_t alive, terr;
            life_core<S>(bd, half, y, o2, p2, live, alive, terr);
            const int sums = secure_sums(alive, terr, p2);
            const bool suicide = live && !rows::half_any(o2 & pb, half);
            const bool allowed = rows::half_any(lg & pb, half), is_ko = rows::half_any(s.ko & pb, half);
            if (live && y == ay) {
                const int flags = (allowed ? SGO_MOVES_ALLOWED : 0) | (is_ko ? SGO_MOVES_KO : 0) | (suicide ? SGO_MOVES_SUICIDE : 0);
                out[a] = secure_row(flags, sums & 1023, (sums >> 10) & 1023, sums >> 20);
            }
        }
    }
}

// One wavefront per listed row, after k_secure on the same stream.  Both halves read the table row (lane y the points of board row
// y) and reduce it alike, so each has the summary without a cross-half exchange; then half 0 runs the fixed point on P and half 1
// the ply of best_move and the fixed point on P*.  best_move needs no base (it is the arg-max of alive + terr), so the table is
// read once; the totals stay in S registers per lane for the two counts that do need it.
// TRIPS: one advance and one life_core call per wave; everything else is unrolled over the S points of a board row.
template <int S>
__global__ __launch_bounds__(64) void k_secure_sum(int n, const uint32_t *records, int n_records, const int32_t *index, int side,
                                                   secure_u32x2 *table, uint32_t *sets, int32_t *counts) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long i = blockIdx.x;
    if (i >= n) return;                                              // the whole workgroup
    const int r = index ? index[i] : (int)i;
    const bool ok = r >= 0 && r < n_records;                         // uniform over the wave
    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    const rows::Board<S> bd(half, y);
    const SecureSide s = secure_side<S>(rec, side, half, y);
    const uint32_t stones = s.own | s.opp;
    secure_u32x2 *tb = table + (size_t)i * G::N;

    // the table row: the occupied points (and every point of an out-of-range row) are written here, the empty ones read
    int tot[S];                                                      // alive + terr of an ALLOWED point, -1 otherwise
    int n_allowed = 0, key = -1;                                     // key = total << 9 | (511 - a): the largest total, the lowest a
#pragma unroll
    for (int x = 0; x < S; x++) {
        const uint32_t bit = 1u << x;
        tot[x] = -1;
        if (y < S) {
            const int a = y * S + x;
            if (!ok) {
                if (half == 0) tb[a] = secure_row(0, 0, 0, 0);
            } else if (stones & bit) {
                if (half == 0) tb[a] = secure_row(SGO_MOVES_OCCUPIED | ((s.ko & bit) ? SGO_MOVES_KO : 0), 0, 0, 0);
            } else {
                const secure_u32x2 v = tb[a];
                if (v.x & SGO_MOVES_ALLOWED) {
                    tot[x] = (int)(v.x >> 16) + (int)(v.y & 0xffffu);
                    n_allowed++;
                    const int kx = (tot[x] << 9) | (511 - a);
                    key = kx > key ? kx : key;
                }
            }
        }
    }
    n_allowed = half_sum(n_allowed);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        const int v = __shfl_xor(key, o, 32);
        key = v > key ? v : key;
    }
    const int best_move = key >= 0 ? 511 - (key & 511) : -1, best_total = key >= 0 ? (key >> 9) : 0;

    // half 0: P.  half 1: P* = P after best_move, or P itself without one.  A pass leaves the rows as they are.
    uint32_t o2 = s.own, p2 = s.opp;
    (void)bd.advance(o2, p2, (half == 1 && best_move >= 0) ? best_move : G::N);   // best_move is ALLOWED, hence empty
    uint32_t alive, terr;
    life_core<S>(bd, half, y, o2, p2, ok, alive, terr);
    const uint32_t wa = rows::gather_word<S>(alive, half, y), wt = rows::gather_word<S>(terr, half, y);
    const int sums = secure_sums(alive, terr, p2);
    const int base = (sums & 1023) + ((sums >> 10) & 1023);          // in half 0; half 1 holds P*'s and stores none of it
    int sec = 0, harm = 0;
#pragma unroll
    for (int x = 0; x < S; x++) {
        sec += (tot[x] >= 0 && tot[x] > base) ? 1 : 0;
        harm += (tot[x] >= 0 && tot[x] < base) ? 1 : 0;
    }
    const int sh = half_sum(sec | (harm << 10));
    uint32_t *so = sets + (size_t)i * 4 * G::NW;
    if (y < G::NW) {
        so[(size_t)(2 * half) * G::NW + y] = wa;                     // alive(P) | alive(P*)
        so[(size_t)(2 * half + 1) * G::NW + y] = wt;                 // terr(P) | terr(P*)
    }
    if (half == 0 && y == 0) {
        int32_t *co = counts + (size_t)i * 8;
        co[0] = sums & 1023; co[1] = (sums >> 10) & 1023; co[2] = sums >> 20; co[3] = n_allowed;
        co[4] = sh & 1023; co[5] = best_move >= 0 ? best_total - base : 0; co[6] = ok ? best_move : 0; co[7] = sh >> 10;
    }
}

// How k_secure deals a row's candidates (sgo_secure_mode): the workgroups per row (0: chosen from n) and the dealing.
static int g_secure_ch = 0, g_secure_by_point = 0;

// Workgroups per row when none is forced: as many as keep a small call (one GTP position) spread over the chip, as few as amortise
// the record read and Board::legal once the rows alone fill it.  DESIGN.md "Securing moves" has the measurement behind the numbers.
static int secure_ch(int S, int n) {
    const int pairs = (S * S + 1) / 2;
    if (g_secure_ch > 0) return g_secure_ch < pairs ? g_secure_ch : pairs;
    const long want = cdiv(SECURE_WAVES, n);
    return (int)(want < SECURE_CH_MIN ? (SECURE_CH_MIN < pairs ? SECURE_CH_MIN : pairs) : (want < pairs ? want : pairs));
}

int launch_secure(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int side, int16_t *d_table,
                  uint32_t *d_sets, int32_t *d_counts, hipStream_t st) {
    const int ch = secure_ch(S, n);
    const long units = (long)n * ch;
    const unsigned grid = (unsigned)(units < SECURE_GRID_CAP ? units : SECURE_GRID_CAP);
    secure_u32x2 *table = reinterpret_cast<secure_u32x2 *>(d_table);
    SGO_DISPATCH(S, k_secure<kS><<<dim3(grid), dim3(64), 0, st>>>(n, d_records, n_records, d_index, side, ch, g_secure_by_point, table));
    SGO_HIP(hipGetLastError());
    SGO_DISPATCH(S, k_secure_sum<kS><<<dim3(n), dim3(64), 0, st>>>(n, d_records, n_records, d_index, side, table, d_sets, d_counts));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_secure_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int side, int16_t *d_table,
                   uint32_t *d_sets, int32_t *d_counts, void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || (side != 0 && side != 1) || !d_records || !d_table || !d_sets || !d_counts ||
        (reinterpret_cast<uintptr_t>(d_table) & 7) != 0) {
        set_error("sgo_secure_dev: bad argument (unsupported size, n < 0, n_records < 0, side outside {0, 1}, a NULL record array or output, "
                  "d_table not 8-byte aligned)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_secure(S, n, d_records, n_records, d_index, side, d_table, d_sets, d_counts, (hipStream_t)stream);
}

int sgo_secure(int S, int n, const uint32_t *records, int side, int16_t *table, uint32_t *sets, int32_t *counts) {
    if (!size_ok(S) || n < 0 || (side != 0 && side != 1) || !records || !table || !sets || !counts) {
        set_error("sgo_secure: bad argument (unsupported size, n < 0, side outside {0, 1}, a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    // every row is written whole, so nothing of the caller's goes in
    const HostArray a[] = {{(size_t)n * S * S * 4 * sizeof(int16_t), nullptr, table},
                           {(size_t)n * 4 * sgo_plane_words(S) * sizeof(uint32_t), nullptr, sets},
                           {(size_t)n * 8 * sizeof(int32_t), nullptr, counts}};
    return host_entry("sgo_secure", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_secure(S, n, d_records, n, nullptr, side, reinterpret_cast<int16_t *>(d[0]), reinterpret_cast<uint32_t *>(d[1]),
                             reinterpret_cast<int32_t *>(d[2]), nullptr);
    });
}

int sgo_secure_mode(int mode) {
    const int prev = g_secure_ch | (g_secure_by_point << 16);
    if (mode >= 0 && (mode & 0xffff) <= 1024 && (mode >> 17) == 0) {
        g_secure_ch = mode & 0xffff;
        g_secure_by_point = (mode >> 16) & 1;
    }
    return prev;
}

}  // extern "C"
