// sgo_zkeys.hpp -- the words z(S, c, a) of the position keys (include/sgo.h "position keys") and the row walk that folds them over
// one record, shared by the two translation units that key positions: sgo_keys.hip (the eight symmetric keys, canonical form)
// and sgo_superko.hip (the identity key of every record of a game).  splitmix is stated here and nowhere else.
#pragma once
#include "sgo_rows.hpp"

namespace sgo {

__host__ __device__ __forceinline__ uint64_t sm64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// c: 0 black, 1 white, 2 = "white to play" (a = 0)
__host__ __device__ __forceinline__ uint64_t zkey(int S, int c, int a) {
    return sm64(((uint64_t)S << 24) | ((uint64_t)c << 16) | (uint64_t)a);
}

// XOR of a 64-bit word over the 32 lanes of the half, delivered to every lane of it
SGO_DEV uint64_t half_xor(uint64_t v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v ^= (uint64_t)__shfl_xor((unsigned long long)v, o, 32);
    return v;
}

// The first K of the eight keys of one record WITHOUT the to-play word, XOR-reduced over the half: every lane of the half returns
// them all (K = 1: the identity key alone).  rec == nullptr (uniform over the half): no stones.
template <int S, bool INLINE, int K = 8>
SGO_DEV void stone_keys(const uint32_t *rec, const uint64_t *zt, int y, uint64_t (&key)[K]) {
    using G = Geo<S>;
    constexpr int m = S - 1;
    uint32_t row[2] = {0u, 0u};
    if (rec) { row[0] = rows::load_row<S>(rec, y); row[1] = rows::load_row<S>(rec + G::NW, y); }
    // L_k[y * S + x] = base[k] + x * step[k]
    const int base[8] = {y * S, y, y * S + m, (m - y) * S, m - y, (m - y) * S + m, m * S + y, m * S + (m - y)};
    constexpr int step[8] = {1, S, -1, 1, S, -1, -S, -S};
#pragma unroll
    for (int k = 0; k < K; k++) key[k] = 0ull;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        uint32_t bits = row[c];
        while (bits) {
            const int x = __builtin_ctz(bits);
            bits &= bits - 1u;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int a = base[k] + x * step[k];
                key[k] ^= INLINE ? zkey(S, c, a) : zt[c * G::N + a];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < K; k++) key[k] = half_xor(key[k]);
}

}  // namespace sgo
