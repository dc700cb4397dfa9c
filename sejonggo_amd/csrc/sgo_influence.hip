// sgo_influence.hip -- influence and territory estimate on the device (include/sgo.h "influence"): per packed record Bouzy's
// dilation / erosion map of the live stones, the territory and moyo sets read off it, and the area-score estimate.  A heuristic,
// kept apart from the proved sgo_life.hip.  A translation unit of its own, like sgo_life.hip and sgo_shapes.hip:
// tests/test_engine_isa.py pins the kernel set of sgo_engine.hip.
//
//   k_influence<S>   per listed record: the territory map, the four sets (terr_black, terr_white, moyo_black, moyo_white), the counts
//
// sgo_session_influence runs the same kernel over the context's records, with the root index k_session_roots (sgo_session.hpp) writes.
//
// Kernel form: one 32-lane HALF of a wavefront per listed row, one board row per lane (sgo_rows.hpp), two rows per 64-thread
// workgroup, as k_keys and k_shapes.  Lane y holds the S values of board row y as one int per column, in registers: every loop over
// the columns is fully unrolled with constant indices.  A step needs of its neighbours only the SIGN of their values, so what
// crosses lanes is two row masks per step (P: columns with v > 0, Q: columns with v < 0), moved with the DPP shifts of row_above /
// row_below; left / right are shifts of the lane's own masks.  Which neighbours exist is decided by four ON-BOARD masks (up, down,
// left, right), never by a value: a padding lane (y >= S) has all four empty, so it stays 0 through every step and isolates the two
// halves of the wave; the 0 a DPP shift delivers at the wave's edge, a padding lane's 0 and the missing columns -1 and S are never
// counted as "<= 0" neighbours in erosion.  The step counts are kernel arguments (wave-uniform): no loop or branch depends on the
// data.  A half whose row is out of range or does not exist (odd n) runs the same steps on an empty board; only its stores differ.
// Everything lives in registers: no LDS, no scratch, no atomics.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_rows.hpp"

namespace sgo {

// the number of the four row masks that have bit x set
SGO_DEV int bits4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, int x) {
    return (int)(((a >> x) & 1u) + ((b >> x) & 1u) + ((c >> x) & 1u) + ((d >> x) & 1u));
}

template <int S>
__global__ __launch_bounds__(64) void k_influence(int n, const uint32_t *__restrict__ records, int n_records, const int32_t *__restrict__ index,
                                                  const uint32_t *__restrict__ dead, int dilate, int erode_moyo, int erode_terr,
                                                  int16_t *__restrict__ values, uint32_t *__restrict__ sets, int32_t *__restrict__ counts) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long i = (long)blockIdx.x * 2 + half;
    const bool valid = i < n;
    const int r = valid ? (index ? index[i] : (int)i) : -1;
    const bool ok = r >= 0 && r < n_records;                         // uniform over the half
    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    const rows::Board<S> bd(half, y);
    const uint32_t lift = (rec && dead) ? rows::load_row<S>(dead + (size_t)i * G::NW, y) : 0u;
    const uint32_t lb = (rec ? rows::load_row<S>(rec, y) : 0u) & ~lift, lw = (rec ? rows::load_row<S>(rec + G::NW, y) : 0u) & ~lift & ~lb;
    const uint32_t live = lb | lw;
    // the neighbours that exist, per direction: rows 1 .. S-1 have one above, rows 0 .. S-2 one below (padding rows none), columns
    // 1 .. S-1 one to the left, columns 0 .. S-2 one to the right
    const uint32_t ON_U = (y > 0) ? bd.M : 0u, ON_D = (y < S - 1) ? bd.M : 0u, ON_L = bd.M & ~1u, ON_R = bd.M >> 1;

    int v[S];
#pragma unroll
    for (int x = 0; x < S; x++) v[x] = (int)((lb >> x) & 1u) * 128 - (int)((lw >> x) & 1u) * 128;
    uint32_t P = lb, Q = lw;                                         // the columns with v > 0 / v < 0, kept current after every step

    for (int s = 0; s < dilate; s++) {
        const uint32_t Pu = rows::row_above(P) & ON_U, Pd = rows::row_below(P) & ON_D, Pl = (P << 1) & ON_L, Pr = (P >> 1) & ON_R;
        const uint32_t Qu = rows::row_above(Q) & ON_U, Qd = rows::row_below(Q) & ON_D, Ql = (Q << 1) & ON_L, Qr = (Q >> 1) & ON_R;
        // a column takes its positive neighbours only when v >= 0 and no neighbour is negative, and the other way round
        const uint32_t tp = ~Q & ~(Qu | Qd | Ql | Qr), tq = ~P & ~(Pu | Pd | Pl | Pr);
        const uint32_t au = Pu & tp, ad = Pd & tp, al = Pl & tp, ar = Pr & tp, su = Qu & tq, sd = Qd & tq, sl = Ql & tq, sr = Qr & tq;
        uint32_t p = 0u, q = 0u;
#pragma unroll
        for (int x = 0; x < S; x++) {
            v[x] += bits4(au, ad, al, ar, x) - bits4(su, sd, sl, sr, x);
            p |= (v[x] > 0 ? 1u : 0u) << x;
            q |= (v[x] < 0 ? 1u : 0u) << x;
        }
        P = p;
        Q = q;
    }
    uint32_t mp = P, mq = Q;                                         // the moyo checkpoint: the dilated map when erode_moyo == 0
    for (int s = 0; s < erode_terr; s++) {
        // the neighbours that EXIST and are <= 0 (for a positive column) / >= 0 (for a negative one)
        const uint32_t cu = ON_U & ~rows::row_above(P) & P, cd = ON_D & ~rows::row_below(P) & P, cl = ON_L & ~(P << 1) & P, cr = ON_R & ~(P >> 1) & P;
        const uint32_t eu = ON_U & ~rows::row_above(Q) & Q, ed = ON_D & ~rows::row_below(Q) & Q, el = ON_L & ~(Q << 1) & Q, er = ON_R & ~(Q >> 1) & Q;
        uint32_t p = 0u, q = 0u;
#pragma unroll
        for (int x = 0; x < S; x++) {
            const int down = bits4(cu, cd, cl, cr, x), up = bits4(eu, ed, el, er, x);
            v[x] = v[x] > 0 ? max(v[x] - down, 0) : min(v[x] + up, 0);
            p |= (v[x] > 0 ? 1u : 0u) << x;
            q |= (v[x] < 0 ? 1u : 0u) << x;
        }
        P = p;
        Q = q;
        if (s + 1 == erode_moyo) {                                   // uniform over the grid
            mp = P;
            mq = Q;
        }
    }

    // every lane takes part in the gathers and the sums; only the stores are conditional
    const uint32_t tb = P & ~live, tw = Q & ~live, yb = mp & ~live, yw = mq & ~live;
    const uint32_t w0 = rows::gather_word<S>(tb, half, y), w1 = rows::gather_word<S>(tw, half, y);
    const uint32_t w2 = rows::gather_word<S>(yb, half, y), w3 = rows::gather_word<S>(yw, half, y);
    const int n_tb = half_sum(__popc(tb)), n_tw = half_sum(__popc(tw)), n_yb = half_sum(__popc(yb)), n_yw = half_sum(__popc(yw));
    const int n_lb = half_sum(__popc(lb)), n_lw = half_sum(__popc(lw));
    if (!valid) return;
    if (y < G::NW) {
        uint32_t *so = sets + (size_t)i * 4 * G::NW;
        so[y] = w0;
        so[G::NW + y] = w1;
        so[2 * G::NW + y] = w2;
        so[3 * G::NW + y] = w3;
    }
    if (y < S) {                                                     // the lane that owns the row; 2-byte aligned only (S is odd)
        int16_t *vo = values + (size_t)i * G::N + y * S;
#pragma unroll
        for (int x = 0; x < S; x++) vo[x] = (int16_t)v[x];
    }
    if (y == 0) {
        int32_t *co = counts + (size_t)i * 8;
        co[0] = n_tb;
        co[1] = n_tw;
        co[2] = n_yb;
        co[3] = n_yw;
        co[4] = n_lb;
        co[5] = n_lw;
        co[6] = ok ? G::N - n_lb - n_lw - n_tb - n_tw : 0;
        co[7] = (n_lb + n_tb) - (n_lw + n_tw);
    }
}

bool influence_params_ok(int dilate, int erode_moyo, int erode_terr) {
    return dilate >= 0 && dilate <= SGO_INFLUENCE_MAX_DILATE && erode_moyo >= 0 && erode_terr >= 0 && erode_terr <= SGO_INFLUENCE_MAX_ERODE &&
           erode_moyo <= erode_terr;
}

int launch_influence(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const uint32_t *d_dead, int dilate,
                     int erode_moyo, int erode_terr, int16_t *d_values, uint32_t *d_sets, int32_t *d_counts, hipStream_t st) {
    SGO_DISPATCH(S, k_influence<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(n, d_records, n_records, d_index, d_dead, dilate, erode_moyo,
                                                                         erode_terr, d_values, d_sets, d_counts));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_influence_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const uint32_t *d_dead, int dilate,
                      int erode_moyo, int erode_terr, int16_t *d_values, uint32_t *d_sets, int32_t *d_counts, void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || !influence_params_ok(dilate, erode_moyo, erode_terr) || !d_records || !d_values || !d_sets ||
        !d_counts) {
        set_error("sgo_influence_dev: bad argument (unsupported size, n < 0, n_records < 0, dilate outside [0, 8], an erosion count outside "
                  "[0, 31], erode_moyo > erode_terr, a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_influence(S, n, d_records, n_records, d_index, d_dead, dilate, erode_moyo, erode_terr, d_values, d_sets, d_counts,
                            (hipStream_t)stream);
}

int sgo_influence(int S, int n, const uint32_t *records, const uint32_t *dead, int dilate, int erode_moyo, int erode_terr, int16_t *values,
                  uint32_t *sets, int32_t *counts) {
    if (!size_ok(S) || n < 0 || !influence_params_ok(dilate, erode_moyo, erode_terr) || !records || !values || !sets || !counts) {
        set_error("sgo_influence: bad argument (unsupported size, n < 0, dilate outside [0, 8], an erosion count outside [0, 31], "
                  "erode_moyo > erode_terr, a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    // every row is written whole, so nothing of the caller's goes in
    const size_t db = (size_t)n * sgo_plane_words(S) * sizeof(uint32_t);
    const HostArray a[] = {{db, dead, nullptr}, {4 * db, nullptr, sets}, {(size_t)n * 8 * sizeof(int32_t), nullptr, counts}, {(size_t)n * S * S * sizeof(int16_t), nullptr, values}};
    return host_entry("sgo_influence", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_influence(S, n, d_records, n, nullptr, dead ? reinterpret_cast<const uint32_t *>(d[0]) : nullptr, dilate, erode_moyo, erode_terr,
                                reinterpret_cast<int16_t *>(d[3]), reinterpret_cast<uint32_t *>(d[1]), reinterpret_cast<int32_t *>(d[2]), nullptr);
    });
}

}  // extern "C"
