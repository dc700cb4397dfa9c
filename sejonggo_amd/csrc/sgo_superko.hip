// sgo_superko.hip -- superko on the device (include/sgo.h "superko"): per listed record and per empty point whether one ply of the
// side to move there recreates a position the game has already held, and how many plies back.  The one analysis that reads a record
// AND the records before it.  A translation unit of its own, like sgo_moves.hip: tests/test_engine_isa.py pins the kernel set of
// sgo_engine.hip, and nothing here touches k_search or the legal set.
//
//   k_superko_keys<S>   stage 1: key_0 of every record [0, n_records) into the work array (z and the row walk of sgo_zkeys.hpp, the
//                       identity table only; the flag term under rule 1, not under rule 0)
//   k_superko<S>        stage 2: per listed row the three sets, back[N] and the eight counts
//
// Kernel form of stage 2: the form of k_moves.  One 32-lane HALF of a wavefront per listed row, one board row per lane (sgo_rows.hpp),
// one wavefront per workgroup.  The rules are rows::Board<S>::advance / legal: nothing is restated.
//   HISTORY KEYS of the row (records lo .. r, at most SGO_SUPERKO_MAX_HISTORY(S) of them) are staged in LDS, 8 bytes each: at 19x19
//     at most 1 445 * 8 B = 11.6 KB per half, 23.1 KB per workgroup.
//   QUIET points (empty, no stone among the four neighbours) take no advance: P' is the position with one more stone.
//   CONTACT points (empty, next to a stone) are walked in ascending order, one advance on a copy of the rows each.
//   Either way key' = key_r ^ XOR of z over the stones that differ between the record and P' (the new stone, the opponent's
//     captured stones, the mover's own on a suicide), folded over the half with the butterfly of the keys, ^ the flag term under
//     rule 1 (the side to move flips).
//   LOOKUP: every lane walks the history keys j = y (mod 32) from the top down to its first match; the largest match of the half is
//     a half-wide maximum; that ONE is confirmed on planes 0 / 1 of its record (and the flag under rule 1); a refuted match is
//     counted, its lane steps on, and the search continues with the next smaller match.  No verdict rests on a key.
//     The walk reads 8-byte words at j = y + 32 k: lane y of a half is on banks 2 y and 2 y + 1 whatever its k, so the 32 lanes of a
//     half never share a bank, and the two halves are separate lane groups of the read.
// LOCKSTEP: the floods of advance / legal, the ballots and the shuffles vote over the whole wave, so both halves run every loop in
// lockstep; trip counts are the wave's.  A half that is done, idle or invalid goes on with an EMPTY board and an EMPTY history and
// only its stores differ.  Nothing cross-lane sits under a per-half branch; the only per-lane loop is the key walk, which holds
// LDS reads and compares alone.  No scratch, no calls, no atomics.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_rows.hpp"
#include "sgo_zkeys.hpp"

namespace sgo {

template <int S>
__global__ __launch_bounds__(256) void k_superko_keys(int n_records, const uint32_t *records, int rule, uint64_t *keys) {
    using G = Geo<S>;
    const int hw = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long r = (long)blockIdx.x * 8 + hw;
    const bool ok = r < n_records;                                   // uniform over the half
    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    uint64_t key[1];
    stone_keys<S, true, 1>(rec, nullptr, y, key);                    // every half runs the shuffles
    if (ok && y == 0) keys[r] = key[0] ^ ((rule && (rec[G::META_WORD] & G::META_BIT)) ? zkey(S, 2, 0) : 0ull);
}

// maximum of a per-lane value over the 32 lanes of the half, delivered to every lane of it
SGO_DEV int half_max(int v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 32); v = w > v ? w : v; }
    return v;
}

// The largest j in [0, bound) whose history record lo + j holds the position (nb, nw) -- and, under rule 1, the flag `white_next`
// -- or -1.  hk: the half's history keys in LDS; only the bits of kmask are compared.  Every lane of the WAVE calls it (bound <= 0
// for a half with nothing to look up) and every lane of the half returns the same value.
// TRIPS: a lane's cursor only moves down, 32 at a time, so the inner walk takes at most ceil(bound / 32) steps per call in all;
// an outer trip either ends the half or retires one key match of it, so there are at most bound + 1 of them.
template <int S>
SGO_DEV int superko_lookup(const uint64_t *hk, int bound, uint64_t key, uint64_t kmask, uint32_t nb, uint32_t nw, bool white_next, int rule,
                           const uint32_t *records, int lo, int half, int y, int &refuted) {
    using G = Geo<S>;
    int cur = (y < bound) ? y + (((bound - 1 - y) >> 5) << 5) : -1;
    int res = -1;
    for (;;) {
        while (cur >= 0 && ((hk[cur] ^ key) & kmask) != 0ull) cur -= 32;
        const int best = half_max(cur);
        const bool found = best >= 0;                                // uniform over the half
        const uint32_t *h = found ? records + (size_t)(lo + best) * G::RW : nullptr;
        const uint32_t hb = h ? rows::load_row<S>(h, y) : 0u, hwt = h ? rows::load_row<S>(h + G::NW, y) : 0u;
        bool differ = rows::half_any(h ? ((hb ^ nb) | (hwt ^ nw)) : 0u, half);
        if (h && rule && (((h[G::META_WORD] & G::META_BIT) != 0) != white_next)) differ = true;
        if (found && differ) {
            refuted++;
            if (cur == best) cur -= 32;
        }
        if (found && !differ) res = best;
        if (!found || !differ) cur = -1;                             // this half is done: it idles while the other goes on
        if (!__any(cur >= 0)) break;
    }
    return res;
}

// TRIPS: two candidate loops (quiet, contact), each with one trip per candidate of the half with more of them, together at most N
// (every trip clears its point from `rest`; a half without candidates left plays a pass on an empty board against an empty
// history).  A trip makes at most one advance (at most four floods) and one lookup, whose trips are bounded by the history length
// (above); the history length is at most SGO_SUPERKO_MAX_HISTORY(S).  One more lookup for `seen`, and what Board::legal takes once.
// Termination does not depend on the data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_superko(int n, const uint32_t *records, int n_records, const int32_t *index, const int32_t *first,
                                                int rule, uint64_t kmask, const uint64_t *keys, uint32_t *sets, int16_t *back,
                                                int32_t *counts) {
    using G = Geo<S>;
    constexpr int MAXH = SGO_SUPERKO_MAX_HISTORY(S);
    __shared__ uint64_t hk_all[2][MAXH];
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long i = (long)blockIdx.x * 2 + half;
    const bool valid = i < n;
    const int r = valid ? (index ? index[i] : (int)i) : -1;
    const int f = valid ? first[i] : -1;
    const bool ok = r >= 0 && r < n_records && f >= 0 && f <= r;     // uniform over the half
    const int span = ok ? r - f + 1 : 0;
    const int nh = span < MAXH ? span : MAXH;                        // the records lo .. r are the history that is read
    const int lo = ok ? r - nh + 1 : 0;
    uint64_t *hk = hk_all[half];
    for (int j = y; j < nh; j += 32) hk[j] = keys[lo + j];
    __syncthreads();

    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    const rows::Board<S> bd(half, y);
    const uint32_t rb = rec ? rows::load_row<S>(rec, y) : 0u, rw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
    const bool mover_white = rec ? ((rec[G::META_WORD] & G::META_BIT) != 0) : false;
    const uint32_t own = mover_white ? rw : rb, opp = mover_white ? rb : rw;
    const uint32_t prev = rec ? rows::load_row<S>(rec + (mover_white ? 3 : 2) * G::NW, y) : own;
    const uint32_t emp = ok ? (~(own | opp) & bd.M) : 0u;
    const uint32_t lg_all = bd.legal(own, opp, prev);                // every half calls it: an invalid half has an empty board
    const uint32_t lg = ok ? lg_all : 0u;
    const uint32_t contact = emp & bd.nbr4(own | opp), quiet = emp & ~contact;
    const uint64_t key_r = ok ? hk[nh - 1] : 0ull;
    const uint64_t zflip = rule ? zkey(S, 2, 0) : 0ull;
    const int cm = mover_white ? 1 : 0;

    int16_t *bk = valid ? back + (size_t)i * G::N : nullptr;
    if (valid && y < S) {
#pragma unroll
        for (int x = 0; x < S; x++) bk[y * S + x] = (int16_t)-1;
    }

    int refuted = 0, n_rep = 0, n_ext = 0, max_back = 0, max_pt = -1;
    uint32_t rep = 0u;
    // the current position among the records before it: the game has already cycled
    const int js = superko_lookup<S>(hk, nh - 1, key_r, kmask, rb, rw, mover_white, rule, records, lo, half, y, refuted);
    const int seen = js >= 0 ? nh - 1 - js : 0;

    for (int phase = 0; phase < 2; phase++) {                        // 0: the quiet points, 1: the contact points
        uint32_t rest = phase ? contact : quiet;
        while (__any(rest != 0)) {
            const int a = lowest_point<S>(rest, half);               // -1: this half has no candidate left
            const bool live = a >= 0;
            const int ay = live ? a / S : -1, ax = live ? a - ay * S : 0;
            const uint32_t pb = (y == ay) ? (1u << ax) : 0u;
            rest &= ~pb;
            const uint32_t own0 = live ? own : 0u, opp0 = live ? opp : 0u;
            uint32_t o2 = own0, p2 = opp0;
            // advance returns early for an OCCUPIED point; never taken, every candidate comes from `emp` (k_moves has the same note)
            if (phase) (void)bd.advance(o2, p2, live ? a : G::N);    // a pass on an empty board for a finished half
            else o2 |= pb;
            // z over what differs: the new stone, the captured stones, the mover's own on a suicide (the new stone then cancels)
            uint64_t kx = 0ull;
            for (uint32_t d = o2 ^ own0; d; d &= d - 1u) kx ^= zkey(S, cm, y * S + __builtin_ctz(d));
            for (uint32_t d = p2 ^ opp0; d; d &= d - 1u) kx ^= zkey(S, 1 - cm, y * S + __builtin_ctz(d));
            const uint64_t key2 = key_r ^ half_xor(kx) ^ zflip;
            const int j = superko_lookup<S>(hk, live ? nh : 0, key2, kmask, mover_white ? p2 : o2, mover_white ? o2 : p2, !mover_white, rule,
                                            records, lo, half, y, refuted);
            const bool allowed = rows::half_any(lg & pb, half);
            if (live && j >= 0) {
                const int b = nh - 1 - j;
                rep |= pb;
                n_rep++;
                if (allowed) {
                    n_ext++;
                    if (max_pt < 0 || b > max_back || (b == max_back && a < max_pt)) { max_back = b; max_pt = a; }
                }
                if (valid && y == ay) bk[a] = (int16_t)b;
            }
        }
    }

    // every lane takes part in the gathers; only the stores are conditional
    const uint32_t w0 = rows::gather_word<S>(rep, half, y), w1 = rows::gather_word<S>(rep & lg, half, y);
    uint32_t w2 = rows::gather_word<S>(lg & ~rep, half, y);
    if (valid) {
        if (y < G::NW) {
            if (ok && y == (G::N >> 5)) w2 |= 1u << (G::N & 31);     // the pass
            uint32_t *so = sets + (size_t)i * 3 * G::NW;
            so[y] = w0;
            so[G::NW + y] = w1;
            so[2 * G::NW + y] = w2;
        }
        if (y == 0) {
            int32_t *co = counts + (size_t)i * 8;
            co[0] = n_rep; co[1] = n_ext; co[2] = max_back; co[3] = ok ? max_pt : 0;
            co[4] = seen; co[5] = nh; co[6] = refuted; co[7] = span > MAXH ? 1 : 0;
        }
    }
}

static int g_superko_mode = 0;    // 0: all 64 bits of a key are compared, 1: the low 6 only

int launch_superko(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_first, int rule,
                   uint64_t *d_keys, uint32_t *d_sets, int16_t *d_back, int32_t *d_counts, hipStream_t st) {
    const uint64_t kmask = g_superko_mode == 1 ? 63ull : ~0ull;
    if (n_records > 0) SGO_DISPATCH(S, k_superko_keys<kS><<<dim3(cdiv(n_records, 8)), dim3(256), 0, st>>>(n_records, d_records, rule, d_keys));
    SGO_HIP(hipGetLastError());
    SGO_DISPATCH(S, k_superko<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(n, d_records, n_records, d_index, d_first, rule, kmask, d_keys,
                                                                             d_sets, d_back, d_counts));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_superko_mode(int mode) {
    const int prev = g_superko_mode;
    if (mode == 0 || mode == 1) g_superko_mode = mode;
    return prev;
}

int sgo_superko_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_first, int rule,
                    uint64_t *d_keys, uint32_t *d_sets, int16_t *d_back, int32_t *d_counts, void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || (rule != 0 && rule != 1) || !d_records || !d_first || !d_keys || !d_sets || !d_back ||
        !d_counts) {
        set_error("sgo_superko_dev: bad argument (unsupported size, n < 0, n_records < 0, rule outside {0, 1}, a NULL record array, d_first, "
                  "d_keys or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_superko(S, n, d_records, n_records, d_index, d_first, rule, d_keys, d_sets, d_back, d_counts, (hipStream_t)stream);
}

int sgo_superko(int S, int n_records, const uint32_t *records, int n, const int32_t *index, const int32_t *first, int rule, uint32_t *sets,
                int16_t *back, int32_t *counts) {
    if (!size_ok(S) || n < 0 || n_records < 0 || (rule != 0 && rule != 1) || !records || !first || !sets || !back || !counts) {
        set_error("sgo_superko: bad argument (unsupported size, n < 0, n_records < 0, rule outside {0, 1}, a NULL record array, first or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const size_t ib = (size_t)n * sizeof(int32_t);
    // every row is written whole, so nothing of the caller's outputs goes in
    const HostArray a[] = {{(size_t)n * 3 * sgo_plane_words(S) * sizeof(uint32_t), nullptr, sets}, {(size_t)n * S * S * sizeof(int16_t), nullptr, back},
                           {(size_t)n * 8 * sizeof(int32_t), nullptr, counts}, {ib, index, nullptr}, {ib, first, nullptr},
                           {(size_t)n_records * sizeof(uint64_t), nullptr, nullptr}};
    return host_entry("sgo_superko", records, (size_t)n_records * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_superko(S, n, d_records, n_records, index ? reinterpret_cast<const int32_t *>(d[3]) : nullptr,
                              reinterpret_cast<const int32_t *>(d[4]), rule, reinterpret_cast<uint64_t *>(d[5]),
                              reinterpret_cast<uint32_t *>(d[0]), reinterpret_cast<int16_t *>(d[1]), reinterpret_cast<int32_t *>(d[2]), nullptr);
    });
}

}  // extern "C"
