// sgo_half.hpp -- half-wide reductions the record readers share (sgo_tactics.hip, sgo_life.hip): one 32-lane half of a wavefront
// owns one item, one board row per lane (sgo_rows.hpp).
#pragma once
#include "sgo_rows.hpp"

namespace sgo {

// sum of a per-lane count over the 32 lanes of the half, delivered to every lane of it
SGO_DEV int half_sum(int v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
    return v;
}
// index y * S + x of the lowest set bit of a set (rows per lane), the same in every lane of the half; -1 for the empty set
template <int S>
SGO_DEV int lowest_point(uint32_t v, int half) {
    const uint32_t nz = rows::half_ballot(v != 0, half);
    const int first = nz ? (__ffs((int)nz) - 1) : 0;
    const int x = __shfl(v ? __builtin_ctz(v) : 0, half * 32 + first, 64);
    return nz ? first * S + x : -1;
}

}  // namespace sgo
