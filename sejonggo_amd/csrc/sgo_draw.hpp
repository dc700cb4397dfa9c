// sgo_draw.hpp -- what the policy rollouts (sgo_rollout.hip) and the light playouts (sgo_playout.hip) share on the device: the
// integer draw of include/sgo.h "policy rollouts" and the area scoring at a game's end, so that each stands in one place.
#pragma once
#include "sgo_half.hpp"

namespace sgo {

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t draw32(uint32_t seed, uint32_t g, uint32_t ply) {
    return mix32(mix32(seed ^ (g * 0x9E3779B9u)) + ply * 0x85EBCA6Bu);
}

// play.py:244-292: a point is black's if it holds a black stone or is empty and reached by black only, the same for white.
// Two floods, which vote over the whole wave: every lane of the wave calls it.
template <int S>
__device__ __forceinline__ void area_owners(const rows::Board<S> &bd, uint32_t nb, uint32_t nw, uint32_t &bo, uint32_t &wo) {
    const uint32_t emp = ~(nb | nw) & bd.M;
    const uint32_t rb = bd.flood(bd.nbr4(nb) & emp, emp), rw = bd.flood(bd.nbr4(nw) & emp, emp);
    bo = nb | (rb & ~rw);
    wo = nw | (rw & ~rb);
}

}  // namespace sgo
