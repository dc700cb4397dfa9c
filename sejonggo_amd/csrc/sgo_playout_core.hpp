// sgo_playout_core.hpp -- what the light playouts (sgo_playout.hip) and the playout tree search (sgo_uct.hip) share on the device: the
// candidate set of a ply (ALLOWED minus EYE of include/sgo.h "light playouts") and the uniform pick, in the half-per-game form of
// sgo_rows.hpp.  Nothing of the rules is restated: ALLOWED is Board::legal, completed to the sound set of rules = 1 with floods.
// Every function votes over the whole wave (floods, ballots, shuffles): every lane of the wave calls it, a half without a live game
// with an empty board.
#pragma once
#include "sgo_half.hpp"
#include "sgo_rows.hpp"

namespace sgo {

// the record holds a chain without a liberty (an illegal record: found once per game; a legal position never turns into one)
template <int S>
SGO_DEV bool playout_weird(const rows::Board<S> &bd, uint32_t sb, uint32_t sw) {
    const uint32_t e0 = ~(sb | sw) & bd.M, l0 = bd.nbr4(e0);
    const uint32_t ab = bd.flood(sb & l0, sb), aw = bd.flood(sw & l0, sw);
    return rows::half_any((sb & ~ab) | (sw & ~aw), bd.half);
}

template <int S>
struct PlayoutCore {
    using G = Geo<S>;
    const rows::Board<S> &bd;
    // the masks of the eye test: a neighbour beyond the edge counts as the mover's; T = 1 on the edge, 2 inside
    uint32_t off_u, off_d, edge;
    SGO_DEV explicit PlayoutCore(const rows::Board<S> &b)
        : bd(b), off_u((b.y == 0) ? G::ROWMASK : 0u), off_d((b.y == S - 1) ? G::ROWMASK : 0u),
          edge((b.y == 0 || b.y == S - 1) ? G::ROWMASK : (1u | (1u << (S - 1)))) {}

    // EYE: every on-board neighbour is the mover's, and fewer than T diagonals are the other colour's
    SGO_DEV uint32_t eye(uint32_t own, uint32_t opp, uint32_t emp) const {
        const uint32_t a4 = (rows::row_above(own) | off_u) & (rows::row_below(own) | off_d) & ((own << 1) | 1u) & ((own >> 1) | (1u << (S - 1)));
        const uint32_t oa = rows::row_above(opp), ob = rows::row_below(opp);
        const uint32_t d1 = (oa << 1) & bd.M, d2 = oa >> 1, d3 = (ob << 1) & bd.M, d4 = ob >> 1;
        const uint32_t ge1 = d1 | d2 | d3 | d4, ge2 = ((d1 | d2) & (d3 | d4)) | (d1 & d2) | (d3 & d4);
        return emp & a4 & ~((edge & ge1) | ge2);
    }

    // cand = ALLOWED minus EYE for the mover `own`.  rules is uniform over the launch, weird over the half.
    // SOUND (rules = 1): the points Board::legal leaves out and on which the stone would stand.  Such a point has no empty neighbour
    // and captures nothing (else it were legal, or it is the ko point, which stays out), so its stone stands exactly when an adjacent
    // own chain keeps a liberty elsewhere.  Own chains with a liberty that HAS an empty neighbour are found with one flood for all
    // points at once; what is left is decided one point at a time with one flood each (at most N trips).  Only points outside EYE
    // are looked at.  A game that started from a record with a chain without a liberty pays one more flood per ply for the opponent
    // chains any neighbouring stone captures and Board::legal does not count.
    SGO_DEV uint32_t cand(uint32_t own, uint32_t opp, uint32_t prev, int rules, bool weird) const {
        const int half = bd.half, y = bd.y;
        const uint32_t emp = ~(own | opp) & bd.M;
        const uint32_t ey = eye(own, opp, emp);
        uint32_t allowed = bd.legal(own, opp, prev);
        if (rules) {
            const uint32_t t0 = bd.nbr4(emp), e1 = emp & t0;
            const uint32_t gone = prev & ~own;
            const uint32_t ko = rows::half_one_bit(gone, half) ? gone : 0u;
            const uint32_t cx = emp & ~t0 & ~allowed & ~ko & ~ey;
            if (__any(cx != 0)) {
                const uint32_t safe = bd.flood(own & bd.nbr4(e1), own);
                uint32_t ex = cx & bd.nbr4(safe);
                if (__any(weird)) {
                    const uint32_t live = bd.flood(opp & t0, opp);
                    ex |= weird ? (cx & bd.nbr4(opp & ~live)) : 0u;
                }
                uint32_t rem = cx & ~ex;
                for (int q = 0; q < G::N; q++) {
                    if (!__any(rem != 0)) break;
                    const int a = lowest_point<S>(rem, half);        // -1: this half has none left
                    const uint32_t pb = (a >= 0 && y == a / S) ? (1u << (a % S)) : 0u;
                    rem &= ~pb;
                    const uint32_t g = bd.flood(bd.nbr4(pb) & own, own);
                    if (rows::half_any(bd.nbr4(g) & emp & ~pb, half)) ex |= pb;
                }
                allowed |= ex;
            }
        }
        return allowed & ~ey;
    }

    // PICK: the (t + 1)-th lowest point of cand, t = (uint64(r) * k) >> 32 with k = |cand|: popcount per row, inclusive scan over the
    // half, the owning row resolves the bit.  k == 0: no candidate (the value returned means nothing).
    SGO_DEV int pick(uint32_t cand, uint32_t r, uint32_t &k) const {
        const int half = bd.half, y = bd.y;
        const int rc = __popc(cand);
        int incl = rc;
#pragma unroll
        for (int s = 1; s < 32; s <<= 1) {
            const int t = __shfl_up(incl, s, 32);
            if (y >= s) incl += t;
        }
        k = (uint32_t)__shfl(incl, 31, 32);
        const uint32_t t = (uint32_t)(((unsigned long long)r * k) >> 32);
        const uint32_t excl = (uint32_t)(incl - rc);
        const bool mine = k != 0 && excl <= t && t < (uint32_t)incl;       // exactly one row when a candidate exists
        int a_loc = 0;
        {
            uint32_t v = cand;
            const uint32_t rank = t - excl;
#pragma unroll
            for (int x = 0; x < S - 1; x++) v &= ((uint32_t)x < rank && mine) ? (v - 1u) : ~0u;
            a_loc = y * S + (v ? __builtin_ctz(v) : 0);
        }
        const uint32_t who = rows::half_ballot(mine, half);
        return __shfl(a_loc, who ? (__ffs((int)who) - 1) : 0, 32);
    }
};

}  // namespace sgo
