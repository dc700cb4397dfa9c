// sgo_life.hip -- unconditional life on the device (include/sgo.h "unconditional life"): per packed record the stones of either
// colour that no sequence of opponent moves can capture (Benson's pass-alive chains) and the points those chains enclose.  A
// translation unit of its own, like sgo_tactics.hip: tests/test_engine_isa.py pins the kernel set of sgo_engine.hip.
//
//   k_life<S>   per listed record: the four sets (alive_black, alive_white, terr_black, terr_white) and the eight counts
//
// sgo_session_life runs the same kernel over the context's records, with the root index k_session_roots (sgo_session.hpp) writes.
//
// Kernel form: one 32-lane HALF of a wavefront per (row, colour) -- half 0 reads the record for black, half 1 for white -- one board
// row per lane (sgo_rows.hpp), one wavefront per workgroup.  Chains and regions are rows::Board<S>::flood / nbr4: nothing is
// restated.  The floods vote over the whole wave, so both halves run every loop in lockstep: a half that has reached its fixed
// point, or whose row is out of range, goes on with an EMPTY board (its floods end at once) and only its stores differ.  No flood
// or shuffle sits under a per-half branch.  Everything lives in registers: no LDS, no scratch.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_life_core.hpp"
#include "sgo_rows.hpp"

namespace sgo {

// The fixed point itself is life_core (sgo_life_core.hpp), which states the iteration and its TRIPS bound; k_secure shares it.
template <int S>
__global__ __launch_bounds__(64) void k_life(int n, const uint32_t *records, int n_records, const int32_t *index, uint32_t *sets,
                                             int32_t *counts) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long i = blockIdx.x;                                       // the row: both halves of the wave
    if (i >= n) return;                                              // the whole workgroup
    const int r = index ? index[i] : (int)i;
    const bool ok = r >= 0 && r < n_records;                         // uniform over the wave
    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    const rows::Board<S> bd(half, y);
    const uint32_t rb = rec ? rows::load_row<S>(rec, y) : 0u, rw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
    const uint32_t own = half ? rw : rb, opp = half ? rb : rw;
    uint32_t alive, terr;
    life_core<S>(bd, half, y, own, opp, ok, alive, terr);

    // every lane takes part in the gathers and the sums; only the stores are conditional
    const uint32_t safe = alive | terr;
    const uint32_t wa = rows::gather_word<S>(alive, half, y), wt = rows::gather_word<S>(terr, half, y);
    const int n_alive = half_sum(__popc(alive)), n_terr = half_sum(__popc(terr)), n_dead = half_sum(__popc(terr & opp));
    const int n_safe = half_sum(__popc(safe));
    const uint32_t other = (uint32_t)__shfl((int)safe, (int)(threadIdx.x ^ 32), 64);     // the cross-half exchange
    const int n_other = __shfl(n_safe, (int)(threadIdx.x ^ 32), 64);
    const int n_union = half_sum(__popc(safe | other));
    uint32_t *so = sets + (size_t)i * 4 * G::NW;
    if (y < G::NW) {
        so[(size_t)half * G::NW + y] = wa;                           // alive_black | alive_white
        so[(size_t)(2 + half) * G::NW + y] = wt;                     // terr_black | terr_white
    }
    if (y == 0) {
        int32_t *co = counts + (size_t)i * 8;
        co[half] = n_alive;
        co[2 + half] = n_terr;
        co[4 + half] = n_dead;                                       // black's half: white stones in terr_black
        if (half == 0) {
            co[6] = ok ? G::N - n_union : 0;
            co[7] = n_safe - n_other;
        }
    }
}

int launch_life(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, uint32_t *d_sets, int32_t *d_counts,
                hipStream_t st) {
    SGO_DISPATCH(S, k_life<kS><<<dim3(n), dim3(64), 0, st>>>(n, d_records, n_records, d_index, d_sets, d_counts));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_life_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, uint32_t *d_sets, int32_t *d_counts,
                 void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || !d_records || !d_sets || !d_counts) {
        set_error("sgo_life_dev: bad argument (unsupported size, n < 0, n_records < 0, a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_life(S, n, d_records, n_records, d_index, d_sets, d_counts, (hipStream_t)stream);
}

int sgo_life(int S, int n, const uint32_t *records, uint32_t *sets, int32_t *counts) {
    if (!size_ok(S) || n < 0 || !records || !sets || !counts) {
        set_error("sgo_life: bad argument (unsupported size, n < 0, a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    // every row is written whole, so nothing of the caller's goes in
    const HostArray a[] = {{(size_t)n * 4 * sgo_plane_words(S) * sizeof(uint32_t), nullptr, sets}, {(size_t)n * 8 * sizeof(int32_t), nullptr, counts}};
    return host_entry("sgo_life", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_life(S, n, d_records, n, nullptr, reinterpret_cast<uint32_t *>(d[0]), reinterpret_cast<int32_t *>(d[1]), nullptr);
    });
}

}  // extern "C"
