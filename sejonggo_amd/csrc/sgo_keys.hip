// sgo_keys.hip -- position keys on the device (include/sgo.h "position keys"): per packed record a 64-bit Zobrist-style key, its
// minimum over the eight symmetries of the square (the canonical key), the mask of the symmetries that reach the minimum, and a
// recorded action mapped into the canonical frame.  What an opening book and duplicate detection stand on.  A translation unit
// of its own: tests/test_engine_isa.py pins the kernel set of sgo_engine.hip, and nothing here touches k_search.
//
//   k_keys<S, INLINE>     per listed record: key0, canon, mask, canon_action
//
// sgo_session_keys runs the same launcher over the context's records, with the root index k_session_roots (sgo_session.hpp) writes.
//
// Kernel form: one 32-lane HALF of a wavefront per record, one board row per lane (sgo_rows.hpp load_row), as k_records_score.
// A record gives 2 of its 16 planes; they are read in place through the index list, no record is copied.  Each lane walks the
// set bits of its black and its white row and XORs z(S, c, L_k[a]) into eight 64-bit accumulators; L_k of a point is plain
// arithmetic on (x, y) -- per lane a base and a step per symmetry -- so no symmetry table is read.  Five butterfly steps XOR
// the 32 lanes together; lane 0 adds the to-play word, takes the minimum and writes the outputs with plain stores.
//
// z comes from a table z[2][N] in LDS (5.8 KB at 19x19), written once per 256-thread workgroup, which then strides over the
// records (INLINE = false, the product), or is computed where it is needed (INLINE = true: eight splitmix rounds per stone;
// sgo_keys_mode selects it for A/B timing).  Same bits either way.
//
// z and the row walk stone_keys are in sgo_zkeys.hpp, which sgo_superko.hip shares.
//
// Nothing branches around a shuffle on a per-record condition: a half whose row is out of range or does not exist reads no
// stones and only its final stores differ.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_rows.hpp"
#include "sgo_zkeys.hpp"

namespace sgo {

// L_k[y * S + x], the table sgo_sym_lut(S, k) writes (build_sym_lut's rotations and reflections, in integers)
template <int S>
SGO_DEV int sym_point(int k, int x, int y) {
    constexpr int m = S - 1;
    switch (k) {
    case 0: return y * S + x;
    case 1: return x * S + y;                  // left diagonal
    case 2: return y * S + (m - x);            // vertical axis
    case 3: return (m - y) * S + x;            // horizontal axis
    case 4: return x * S + (m - y);            // rotation 90
    case 5: return (m - y) * S + (m - x);      // rotation 180
    case 6: return (m - x) * S + y;            // rotation 270
    default: return (m - x) * S + (m - y);     // right diagonal
    }
}

// canon, mask and canon_action(t) from the eight keys (to-play word included)
template <int S>
SGO_DEV void canonical(const uint64_t (&key)[8], int t, uint64_t &canon, int &mask, int &action) {
    using G = Geo<S>;
    canon = key[0];
#pragma unroll
    for (int k = 1; k < 8; k++) canon = key[k] < canon ? key[k] : canon;
    mask = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) mask |= (key[k] == canon) ? (1 << k) : 0;
    action = -1;
    if (t == G::N) action = G::N;                          // a pass stays a pass
    else if (t >= 0 && t < G::N) {
        const int x = t % S, y = t / S;
        action = G::N;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int a = sym_point<S>(k, x, y);
            if (((mask >> k) & 1) && a < action) action = a;
        }
    }
}

template <int S, bool INLINE>
__global__ __launch_bounds__(256) void k_keys(int n, const uint32_t *records, int n_records, const int32_t *index, const int32_t *target,
                                              uint64_t *key0, uint64_t *canon_out, int32_t *mask_out, int32_t *action_out) {
    using G = Geo<S>;
    __shared__ uint64_t zt[INLINE ? 1 : 2 * G::N];
    if (!INLINE) {
        for (int i = threadIdx.x; i < 2 * G::N; i += 256) zt[i] = zkey(S, i >= G::N ? 1 : 0, i >= G::N ? i - G::N : i);
        __syncthreads();
    }
    const int hw = threadIdx.x >> 5, y = threadIdx.x & 31;
    // the trip count is the workgroup's: every half of a wave runs every shuffle
    for (long i0 = (long)blockIdx.x * 8; i0 < n; i0 += (long)gridDim.x * 8) {
        const long i = i0 + hw;
        const bool valid = i < n;
        const int r = valid ? (index ? index[i] : (int)i) : -1;
        const bool ok = r >= 0 && r < n_records;                         // uniform over the half
        const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
        uint64_t key[8];
        stone_keys<S, INLINE>(rec, zt, y, key);
        if (valid && y == 0) {
            uint64_t canon = 0ull;
            int mask = 0, action = -1;
            if (ok) {
                if (rec[G::META_WORD] & G::META_BIT) {
                    const uint64_t zw = zkey(S, 2, 0);
#pragma unroll
                    for (int k = 0; k < 8; k++) key[k] ^= zw;
                }
                canonical<S>(key, target ? target[i] : -1, canon, mask, action);
            }
            key0[i] = ok ? key[0] : 0ull;
            canon_out[i] = canon;
            mask_out[i] = mask;
            if (target) action_out[i] = action;
        }
    }
}

static int g_keys_mode = 0;       // 0: the LDS table, 1: splitmix inline

int launch_keys(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_target,
                uint64_t *d_key0, uint64_t *d_canon, int32_t *d_mask, int32_t *d_action, hipStream_t st) {
    const int blocks = cdiv(n, 8) < 4096 ? cdiv(n, 8) : 4096;
    if (g_keys_mode == 1) {
        SGO_DISPATCH(S, k_keys<kS, true><<<dim3(blocks), dim3(256), 0, st>>>(n, d_records, n_records, d_index, d_target, d_key0, d_canon,
                                                                              d_mask, d_action));
    } else {
        SGO_DISPATCH(S, k_keys<kS, false><<<dim3(blocks), dim3(256), 0, st>>>(n, d_records, n_records, d_index, d_target, d_key0, d_canon,
                                                                               d_mask, d_action));
    }
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_keys_mode(int mode) {
    const int prev = g_keys_mode;
    if (mode == 0 || mode == 1) g_keys_mode = mode;
    return prev;
}

int sgo_keys_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_target,
                 uint64_t *d_key0, uint64_t *d_canon, int32_t *d_mask, int32_t *d_canon_action, void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || !d_records || !d_key0 || !d_canon || !d_mask || (d_target && !d_canon_action)) {
        set_error("sgo_keys_dev: bad argument (unsupported size, n < 0, a NULL record array or output, targets without d_canon_action)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_keys(S, n, d_records, n_records, d_index, d_target, d_key0, d_canon, d_mask, d_canon_action, (hipStream_t)stream);
}

int sgo_keys(int S, int n, const uint32_t *records, const int32_t *target, uint64_t *key0, uint64_t *canon, int32_t *mask,
             int32_t *canon_action) {
    if (!size_ok(S) || n < 0 || !records || !key0 || !canon || !mask || (target && !canon_action)) {
        set_error("sgo_keys: bad argument (unsupported size, n < 0, a NULL record array or output, targets without canon_action)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const size_t kb = (size_t)n * sizeof(uint64_t), ib = (size_t)n * sizeof(int32_t);
    const HostArray a[] = {{kb, nullptr, key0}, {kb, nullptr, canon}, {ib, nullptr, mask}, {ib, target, nullptr}, {ib, nullptr, target ? canon_action : nullptr}};
    return host_entry("sgo_keys", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_keys(S, n, d_records, n, nullptr, target ? reinterpret_cast<const int32_t *>(d[3]) : nullptr, reinterpret_cast<uint64_t *>(d[0]),
                           reinterpret_cast<uint64_t *>(d[1]), reinterpret_cast<int32_t *>(d[2]), reinterpret_cast<int32_t *>(d[4]), nullptr);
    });
}

}  // extern "C"
