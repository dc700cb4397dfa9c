// sgo_playout.hip -- light playouts on the device (include/sgo.h "light playouts"): per listed record `per_row` uniformly random
// games that refuse to fill their own eyes, each played to its end inside ONE kernel, with no net and no host loop; what comes out is
// who ends up holding each point, the score distribution and an all-moves-as-first table.  A translation unit of its own, like
// sgo_moves.hip: tests/test_engine_isa.py pins the kernel set of sgo_engine.hip, and nothing here touches k_search or the legal set.
//
//   k_playout_zero      zeroes own / amaf / sums of the n rows (the playing kernel adds into them)
//   k_playout<S>        plays the units and adds what they found, one round of integer atomics per unit
//
// Kernel form: the form of k_life / k_superko.  One 32-lane HALF of a wavefront per playout, one board row per lane (sgo_rows.hpp),
// one wavefront per workgroup.  The WHOLE GAME lives in registers: the mover's and the other colour's row, the ko row `prev`,
// `touched`, `first`, the ply and pass counters; nothing is written per ply, there is no LDS and no scratch.
// Nothing of the rules is restated: the legal set is Board::legal, the ply Board::advance, the score area_owners (sgo_draw.hpp, the
// two floods of k_rollout_step), the draw draw32 of the rollouts.
//   `prev` of the next ply is the next mover's row as it was before this ply (what advance_record_rows hands to legal): after a pass
//     it equals that colour's stones, so the ko test forbids nothing.
//   SOUND (rules = 1), EYE and PICK -- the candidate set of a ply and the uniform pick -- are in sgo_playout_core.hpp, which the
//     playout tree search (sgo_uct.hip) inlines as well: the points Board::legal leaves out and on which the stone would stand, found
//     with floods; two neighbour-row shifts of the opponent row for the four diagonals; popcount per row, inclusive scan over the
//     half, the owning row resolves the bit.  A unit that starts from a record with a chain without a liberty (found once per unit)
//     pays one more flood per ply.
// UNITS: a unit is SGO_PLAYOUT_UNIT consecutive playouts j of one row, played by one half from first to last; a half whose playout
// has ended takes the next one of its unit in the same trip.  Ownership, AMAF and sums accumulate in registers across the unit (at
// 19x19 four tables of 19 VGPRs per lane) and leave with one round of integer atomics at its end.  The grid is capped and walks
// the remaining units in a stride loop.
// LOCKSTEP: the floods of legal / advance / area_owners, the ballots and the shuffles vote over the whole wave, so both halves run
// every loop in lockstep; trip counts are the wave's.  A half without a live playout goes on with an EMPTY board and passes; only
// what it keeps differs.  Nothing cross-lane sits under a per-half branch.  No scratch, no calls.
// TRIPS: one trip of the ply loop is one ply of every live half, and a playout ends at ply == max_plies at the latest, so a unit
// takes at most SGO_PLAYOUT_UNIT * max_plies trips; the sound loop retires one point per trip, at most N; the stride loop takes
// ceil(units / (2 * grid)) trips.  Termination does not depend on the data beyond that.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_draw.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_playout_core.hpp"
#include "sgo_rows.hpp"

namespace sgo {

constexpr int PLAYOUT_UNIT = 16;
constexpr int PLAYOUT_MAX_BLOCKS = 1 << 15;     // two units per workgroup and trip

__global__ __launch_bounds__(256) void k_playout_zero(long n_own, int32_t *own, int32_t *amaf, long n_sums, unsigned long long *sums) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n_own; t += stride) {
        own[t] = 0;
        if (amaf) amaf[t] = 0;
        if (t < n_sums) sums[t] = 0ull;
    }
}

template <int S>
__global__ __launch_bounds__(64) void k_playout(int n, const uint32_t *records, int n_records, const int32_t *index, int per_row, int upr,
                                                uint32_t seed, int rules, int max_plies, int32_t *own_out, int32_t *amaf_out,
                                                unsigned long long *sums_out) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const rows::Board<S> bd(half, y);
    const long n_units = (long)n * upr;
    const PlayoutCore<S> core(bd);

    for (long u0 = (long)blockIdx.x * 2; u0 < n_units; u0 += (long)gridDim.x * 2) {    // the trip count is the workgroup's
        const long u = u0 + half;
        const bool valid = u < n_units;
        const int i = valid ? (int)(u / upr) : 0;
        const int j0 = valid ? (int)(u - (long)i * upr) * PLAYOUT_UNIT : 0;
        const int r = valid ? (index ? index[i] : i) : -1;
        const bool ok = r >= 0 && r < n_records;                     // uniform over the half
        const int cnt = ok ? ((per_row - j0 < PLAYOUT_UNIT) ? per_row - j0 : PLAYOUT_UNIT) : 0;
        const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
        const uint32_t sb = rec ? rows::load_row<S>(rec, y) : 0u, sw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
        const bool start_white = rec ? ((rec[G::META_WORD] & G::META_BIT) != 0) : false;
        const uint32_t sprev = rec ? rows::load_row<S>(rec + (start_white ? 3 : 2) * G::NW, y) : 0u;
        const uint32_t g0 = (uint32_t)i * (uint32_t)per_row + (uint32_t)j0;
        const bool weird = playout_weird<S>(bd, sb, sw);             // the record holds a chain without a liberty

        int bacc[S], wacc[S], acnt[S], asum[S];
#pragma unroll
        for (int x = 0; x < S; x++) { bacc[x] = 0; wacc[x] = 0; acnt[x] = 0; asum[x] = 0; }
        int s_bw = 0, s_ww = 0, s_dr = 0, s_sc = 0, s_sq = 0, s_pl = 0, s_cap = 0, s_n = 0;

        bool active = cnt > 0, mover_white = start_white;
        uint32_t own = active ? (start_white ? sw : sb) : 0u, opp = active ? (start_white ? sb : sw) : 0u, prev = active ? sprev : 0u;
        uint32_t touched = sb | sw, first = 0u;
        int j = 0, ply = 0, passes = 0;

        for (int trip = 0; trip < PLAYOUT_UNIT * max_plies; trip++) {
            if (!__any(active)) break;
            const uint32_t cand = core.cand(own, opp, prev, rules, weird);
            uint32_t k;                                              // the (t + 1)-th lowest candidate
            const int a_pick = core.pick(cand, draw32(seed, g0 + (uint32_t)j, (uint32_t)ply), k);
            const int a = (active && k != 0) ? a_pick : G::N;        // no candidate: a pass

            const uint32_t before_opp = opp;
            (void)bd.advance(own, opp, a);                           // a candidate is never occupied: no early return
            const uint32_t pb = (a < G::N && y == a / S) ? (1u << (a % S)) : 0u;
            if (mover_white == start_white) first |= pb & ~touched;
            touched |= pb;
            {   // the other colour moves next; its stones one ply ago are its row before this ply
                const uint32_t t2 = own;
                own = opp; opp = t2; prev = before_opp;
                mover_white = !mover_white;
            }
            ply++;
            passes = (a == G::N) ? passes + 1 : 0;

            const bool ended = active && (passes >= 2 || ply >= max_plies);
            if (__any(ended)) {                                      // uniform over the wave: the fills below vote over it
                const uint32_t nb = ended ? (mover_white ? opp : own) : 0u, nw = ended ? (mover_white ? own : opp) : 0u;
                uint32_t bo, wo;
                area_owners<S>(bd, nb, nw, bo, wo);
                const int diff = half_sum(__popc(bo)) - half_sum(__popc(wo));
                if (ended) {
                    const int mine_diff = start_white ? -diff : diff;
#pragma unroll
                    for (int x = 0; x < S; x++) {
                        bacc[x] += (int)((bo >> x) & 1u);
                        wacc[x] += (int)((wo >> x) & 1u);
                        acnt[x] += (int)((first >> x) & 1u);
                        asum[x] += ((first >> x) & 1u) ? mine_diff : 0;
                    }
                    s_bw += diff > 0; s_ww += diff < 0; s_dr += diff == 0;
                    s_sc += diff; s_sq += diff * diff; s_pl += ply; s_cap += passes < 2; s_n++;
                    j++;
                    active = j < cnt;                                // the next playout of the unit, or an empty board
                    mover_white = start_white;
                    own = active ? (start_white ? sw : sb) : 0u;
                    opp = active ? (start_white ? sb : sw) : 0u;
                    prev = active ? sprev : 0u;
                    touched = sb | sw; first = 0u; ply = 0; passes = 0;
                }
            }
        }

        if (cnt > 0 && y < S) {
            int32_t *ob = own_out + (size_t)i * 2 * G::N + y * S, *am = amaf_out ? amaf_out + (size_t)i * 2 * G::N + y * S : nullptr;
#pragma unroll
            for (int x = 0; x < S; x++) {
                if (bacc[x]) atomicAdd(ob + x, bacc[x]);
                if (wacc[x]) atomicAdd(ob + G::N + x, wacc[x]);
                if (am && acnt[x]) { atomicAdd(am + x, acnt[x]); atomicAdd(am + G::N + x, asum[x]); }
            }
            if (y == 0) {
                unsigned long long *sm = sums_out + (size_t)i * 8;
                const int v[8] = {s_bw, s_ww, s_dr, s_sc, s_sq, s_pl, s_cap, s_n};
#pragma unroll
                for (int q = 0; q < 8; q++)
                    if (v[q]) atomicAdd(sm + q, (unsigned long long)(long long)v[q]);   // two's complement: read back as int64
            }
        }
    }
}

bool playout_params_ok(int S, int n, int per_row, int rules, int max_plies) {
    return size_ok(S) && n >= 0 && per_row >= 1 && per_row <= SGO_PLAYOUT_MAX_PER_ROW && (rules == 0 || rules == 1) &&
           max_plies <= 4 * S * S && (long)n * per_row <= 0x7fffffffL;
}

int launch_playout(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int per_row, uint32_t seed, int rules,
                   int max_plies, int32_t *d_own, int32_t *d_amaf, int64_t *d_sums, hipStream_t st) {
    const int N = S * S, upr = cdiv(per_row, PLAYOUT_UNIT);
    const long n_own = (long)n * 2 * N, n_units = (long)n * upr, wg = (n_units + 1) / 2;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(d_sums);
    k_playout_zero<<<dim3(cdiv(n_own, 256) < 4096 ? cdiv(n_own, 256) : 4096), dim3(256), 0, st>>>(n_own, d_own, d_amaf, (long)n * 8, sums);
    SGO_HIP(hipGetLastError());
    const int blocks = wg < PLAYOUT_MAX_BLOCKS ? (int)wg : PLAYOUT_MAX_BLOCKS;
    const int plies = max_plies > 0 ? max_plies : 3 * N;
    SGO_DISPATCH(S, k_playout<kS><<<dim3(blocks), dim3(64), 0, st>>>(n, d_records, n_records, d_index, per_row, upr, seed, rules, plies, d_own,
                                                                       d_amaf, sums));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_playout_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int per_row, uint32_t seed, int rules,
                    int max_plies, int32_t *d_own, int32_t *d_amaf, int64_t *d_sums, void *stream) {
    if (!playout_params_ok(S, n, per_row, rules, max_plies) || n_records < 0 || !d_records || !d_own || !d_sums) {
        set_error("sgo_playout_dev: bad argument (unsupported size, n < 0, n_records < 0, per_row outside [1, SGO_PLAYOUT_MAX_PER_ROW], "
                  "n * per_row beyond int32, rules outside {0, 1}, max_plies above 4 * S * S, a NULL d_records, d_own or d_sums)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_playout(S, n, d_records, n_records, d_index, per_row, seed, rules, max_plies, d_own, d_amaf, d_sums, (hipStream_t)stream);
}

int sgo_playout(int S, int n_records, const uint32_t *records, int n, const int32_t *index, int per_row, uint32_t seed, int rules,
                int max_plies, int32_t *own, int32_t *amaf, int64_t *sums) {
    if (!playout_params_ok(S, n, per_row, rules, max_plies) || n_records < 0 || !records || !own || !sums) {
        set_error("sgo_playout: bad argument (unsupported size, n < 0, n_records < 0, per_row outside [1, SGO_PLAYOUT_MAX_PER_ROW], "
                  "n * per_row beyond int32, rules outside {0, 1}, max_plies above 4 * S * S, a NULL record array, own or sums)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const size_t tb = (size_t)n * 2 * S * S * sizeof(int32_t);
    // every row is written whole, so nothing of the caller's outputs goes in
    const HostArray a[] = {{tb, nullptr, own}, {amaf ? tb : 0, nullptr, amaf}, {(size_t)n * 8 * sizeof(int64_t), nullptr, sums},
                           {index ? (size_t)n * sizeof(int32_t) : 0, index, nullptr}};
    return host_entry("sgo_playout", records, (size_t)n_records * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_playout(S, n, d_records, n_records, index ? reinterpret_cast<const int32_t *>(d[3]) : nullptr, per_row, seed, rules,
                              max_plies, reinterpret_cast<int32_t *>(d[0]), amaf ? reinterpret_cast<int32_t *>(d[1]) : nullptr,
                              reinterpret_cast<int64_t *>(d[2]), nullptr);
    });
}

}  // extern "C"
