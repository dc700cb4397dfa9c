// sgo_life_core.hpp -- the fixed point of unconditional life (include/sgo.h "unconditional life") for ONE colour of one position, as
// a device function over row bitboards: what k_life (sgo_life.hip) runs per (record, colour) and k_secure / k_secure_sum
// (sgo_secure.hip) per (record, candidate) on the position after a ply.  The rule lives here and nowhere else.
//
// Form: one 32-lane HALF of a wavefront per position, one board row per lane (sgo_rows.hpp).  Chains and regions are
// rows::Board<S>::flood / nbr4.  The floods vote over the whole wave, so both halves run every loop in lockstep: a half that has
// reached its fixed point, or that has no position (`ok` false, its rows all zero), goes on with an EMPTY board (its floods end at
// once).  The CALLER keeps the call out of any per-half branch.  Everything lives in registers: no LDS, no scratch.
#pragma once
#include "sgo_half.hpp"
#include "sgo_rows.hpp"

namespace sgo {

// X = the half's colour (`own`), O = the other (`opp`).  Three row-bitboards carry the header's iteration: `live` (the stones of
// the chains still in C), `reg` (the points of the regions still in R), and per round v1 / v2 (the stones of the chains with >= 1 /
// >= 2 vital regions found so far).  A region that is still in R touches live chains only (a region next to a removed chain was
// removed with it), so the chains a region can be vital to are the at most four live chains on the neighbours of ONE of its
// empty points -- the lowest -- since a vital region has every empty point next to the chain.
// TRIPS: a round that is not the last removes at least one chain, so a half takes at most chains + 1 rounds; a round takes one
// trip per region still in R (at most N: every trip clears at least the seed from `rest`), and a trip one flood for the region
// and at most four for the chains (every trip of the inner loop clears at least one of the four neighbours from `cand`): at
// most 5 floods per region, (chains + 1) * N * 5 floods per call and half, plus one per round for the removal.  Termination
// does not depend on the data beyond that.
template <int S>
SGO_DEV void life_core(const rows::Board<S> &bd, int half, int y, uint32_t own, uint32_t opp, bool ok, uint32_t &alive, uint32_t &terr) {
    const uint32_t emp = ~(own | opp) & bd.M;
    uint32_t live = own, reg = ok ? (~own & bd.M) : 0u;
    alive = 0u;
    terr = 0u;
    bool done = !ok;
    do {
        uint32_t v1 = 0u, v2 = 0u, t = 0u, rest = reg;
        while (__any(rest != 0)) {                                   // the regions still in R, by lowest point
            const int lo = lowest_point<S>(rest, half);
            const uint32_t seed = (lo >= 0 && y == lo / S) ? (1u << (lo % S)) : 0u;
            const uint32_t R = bd.flood(seed, rest);
            rest &= ~R;
            const uint32_t E = R & emp;
            const int e0 = lowest_point<S>(E, half);
            const uint32_t eb = (e0 >= 0 && y == e0 / S) ? (1u << (e0 % S)) : 0u;
            uint32_t cand = bd.nbr4(eb) & live;                      // at most four stones
            bool vital = false;
            while (__any(cand != 0)) {                               // the distinct live chains on them
                const int c0 = lowest_point<S>(cand, half);
                const uint32_t cb = (c0 >= 0 && y == c0 / S) ? (1u << (c0 % S)) : 0u;
                const uint32_t C = bd.flood(cb, live);
                const bool is_vital = c0 >= 0 && !rows::half_any(E & ~bd.nbr4(C), half);
                if (is_vital) {
                    v2 |= C & v1;
                    v1 |= C;
                    vital = true;
                }
                cand &= ~C;
            }
            if (vital) t |= R;
        }
        const uint32_t removed = live & ~v2;
        const bool fixed = !rows::half_any(removed, half);           // the same in every lane of the half
        const uint32_t gone = bd.flood(bd.nbr4(removed) & reg, reg); // the regions next to a removed chain
        if (!done && fixed) {
            alive = live;
            terr = t;
            done = true;
        }
        live = done ? 0u : v2;
        reg = done ? 0u : (reg & ~gone);
    } while (__any(!done));
}

}  // namespace sgo
