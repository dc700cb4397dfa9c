// sgo_tactics.hip -- chains, liberties and ladders on the device (include/sgo.h "chains and ladders"): per packed record the
// liberty count of the chain on every point, the table of the chains with one or two liberties, and for each of them the verdict
// of a small exhaustive reader.  A translation unit of its own: tests/test_engine_isa.py pins the kernel set of sgo_engine.hip,
// and nothing here touches k_search.
//
//   k_tactics_chains<S>   per listed record: libs, n_chains, words 0..3 of the chain rows (words 4..7 preset to 0, -1, -1, 0)
//   k_tactics_read<S>     per (row, chain slot): queries A and D of the header's reader; words 4..7 of the chain row
//
// sgo_session_tactics runs the same two kernels over the context's records, with the root index k_session_roots
// (sgo_session.hpp) writes.
//
// Kernel form: one 32-lane HALF of a wavefront per item, one board row per lane (sgo_rows.hpp), one wavefront per workgroup.
// The rules are rows::Board<S>::advance / legal / flood: nothing is restated.  The floods vote over the whole wave, so both
// halves run every loop in lockstep: a half that is done, idle or out of range goes on with an EMPTY board (its floods end at
// once) and only its stores differ.  No flood, advance or shuffle sits under a per-item branch.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_rows.hpp"

namespace sgo {

template <int S>
__global__ __launch_bounds__(64) void k_tactics_chains(int n, const uint32_t *records, int n_records, const int32_t *index, int max_chains,
                                                       uint8_t *libs, int32_t *n_chains, int32_t *chains) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long i = (long)blockIdx.x * 2 + half;
    const bool valid = i < n;
    const int r = valid ? (index ? index[i] : (int)i) : -1;
    const bool ok = r >= 0 && r < n_records;                         // uniform over the half
    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    const rows::Board<S> bd(half, y);
    uint32_t rb = rec ? rows::load_row<S>(rec, y) : 0u, rw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
    const uint32_t emp = ~(rb | rw) & bd.M;
    uint32_t lb[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};               // bit k of the liberty count of the chain on each point of the row
    int count = 0;
    int32_t *rows_out = valid ? chains + (size_t)i * max_chains * 8 : nullptr;
    // the chain loop of Board::legal: the lowest remaining stone seeds a flood, the chain is removed.  At most N trips.
    while (__any((rb | rw) != 0)) {
        const uint32_t all = rb | rw;
        const int anchor = lowest_point<S>(all, half);
        const uint32_t seed = (anchor >= 0 && y == anchor / S) ? (1u << (anchor % S)) : 0u;
        const bool is_b = rows::half_any(seed & rb, half);
        const uint32_t g = bd.flood(seed, is_b ? rb : rw);
        const int size = half_sum(__popc(g)), L = half_sum(__popc(bd.nbr4(g) & emp));
        const int Ls = L < 255 ? L : 255;
#pragma unroll
        for (int k = 0; k < 8; k++) lb[k] |= ((Ls >> k) & 1) ? g : 0u;
        if (anchor >= 0 && L >= 1 && L <= 2) {
            if (y == 0 && count < max_chains) {
                int32_t *o = rows_out + (size_t)count * 8;
                o[0] = anchor; o[1] = is_b ? 1 : -1; o[2] = size; o[3] = L;
                o[4] = 0; o[5] = -1; o[6] = -1; o[7] = 0;
            }
            count++;
        }
        rb &= ~g;
        rw &= ~g;
    }
    if (valid) {
        if (y < S) {
            uint8_t *o = libs + (size_t)i * G::N + y * S;
#pragma unroll
            for (int x = 0; x < S; x++) {
                int v = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) v |= (int)((lb[k] >> x) & 1u) << k;
                o[x] = (uint8_t)v;
            }
        }
        if (y == 0) n_chains[i] = count;
    }
}

enum { R_NONE = 0, R_CAP = 1, R_ESC = 2, R_UNK = 3 };
constexpr int T_FRAMES = SGO_TACTICS_MAX_DEPTH + 1;                  // depths 0 .. MAX_DEPTH hold a frame

// One half-wavefront per (row, chain slot): an iterative depth-first search.  A frame is the position of a node BEFORE its move
// (own = the node's mover, opp), 256 bytes per half and frame, plus the candidate cursor (the last candidate tried; every lane
// of the half writes the same value): 2 * 81 * 260 bytes = 42 KB of LDS per workgroup.  The ko `prev` of a node is its parent
// frame's opp rows.  One trip of the loop is one node step: what the top frame's child returned is taken in; the frame's
// chain, liberties, candidates and legal set are recomputed; the next candidate above the cursor is played and judged; the frame
// returns, a child frame is pushed, or the cursor has moved on.
// TRIPS: every trip pushes a frame (at most MAX_NODES per query), pops one (no more pops than pushes, plus the root) or moves
// a cursor up (at most N times per frame), so a launch takes at most 2 * (MAX_NODES + 1) * (N + 2) trips -- 372 438 at 19x19; the
// golden records need a few dozen for most chains.  Termination does not depend on the data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_tactics_read(int n, const uint32_t *records, int n_records, const int32_t *index, int max_chains,
                                                     const int32_t *n_chains, int32_t *chains) {
    using G = Geo<S>;
    __shared__ uint32_t F[2][T_FRAMES][2][32];
    __shared__ int32_t Cs[2][T_FRAMES];
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const int j = blockIdx.x * 2 + half;                             // chain slot
    const rows::Board<S> bd(half, y);
    for (int i = blockIdx.y; i < n; i += gridDim.y) {                // the trip count is the workgroup's
        const int r = index ? index[i] : i;
        const bool ok = r >= 0 && r < n_records;
        const int cnt = ok ? n_chains[i] : 0;
        const bool item = j < max_chains && j < cnt;                 // uniform over the half
        if (!__any(item)) continue;
        int32_t *row = chains + ((size_t)i * max_chains + (item ? j : 0)) * 8;
        const uint32_t *rec = item ? records + (size_t)r * G::RW : nullptr;
        const uint32_t black = rec ? rows::load_row<S>(rec, y) : 0u, white = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
        const uint32_t pblack = rec ? rows::load_row<S>(rec + 2 * G::NW, y) : 0u, pwhite = rec ? rows::load_row<S>(rec + 3 * G::NW, y) : 0u;
        const bool stm_white = rec ? (rec[G::META_WORD] & G::META_BIT) != 0 : false;
        const int t = item ? row[0] : 0, L0 = item ? row[3] : 0;
        const bool def_white = item ? row[1] < 0 : false;
        const uint32_t tb = (item && y == t / S) ? (1u << (t % S)) : 0u;

        bool done = !item, root_atk = true;
        int q = 0;                                                   // 0: query A, 1: query D
        int d = 0, nodes = 1, ret = R_NONE;
        int resA = R_NONE, resD = R_NONE, mvA = -1, mvD = -1, nodes_sum = 0;
        uint32_t rootprev;
        {   // root of query A: the attacker moves
            const bool mw = !def_white;
            F[half][0][0][y] = mw ? white : black;
            F[half][0][1][y] = mw ? black : white;
            rootprev = (mw == stm_white) ? (mw ? pwhite : pblack) : (mw ? white : black);
            Cs[half][0] = -1;
        }
        do {
            const bool run = !done;
            const bool atk = ((d & 1) != 0) != root_atk;             // the top frame's mover is the attacker
            const int cur = Cs[half][d];
            bool popnow = false;
            if (run && ret != R_NONE) {                              // what the child of the last candidate returned
                if (atk ? ret == R_CAP : ret == R_ESC) popnow = true;
                else ret = R_NONE;
            }
            const bool work = run && !popnow;
            const uint32_t own = work ? F[half][d][0][y] : 0u, opp = work ? F[half][d][1][y] : 0u;
            const uint32_t prev = work ? (d > 0 ? F[half][d - 1][1][y] : rootprev) : 0u;
            const uint32_t dst = atk ? opp : own, ast = atk ? own : opp;
            const uint32_t emp = ~(own | opp) & bd.M;
            const uint32_t g = bd.flood(tb & dst, dst);
            const uint32_t lib = bd.nbr4(g) & emp;
            const int L = half_sum(__popc(lib));
            uint32_t cand = lib;
            // the defender may also capture an attacker chain that touches the target and has exactly one liberty
            uint32_t rr = atk ? 0u : bd.flood(bd.nbr4(g) & ast, ast);
            while (__any(rr != 0)) {
                const int lo = lowest_point<S>(rr, half);
                const uint32_t seed = (lo >= 0 && y == lo / S) ? (1u << (lo % S)) : 0u;
                const uint32_t c = bd.flood(seed, rr);
                const uint32_t cl = bd.nbr4(c) & emp;
                if (rows::half_one_bit(cl, half)) cand |= cl;
                rr &= ~c;
            }
            cand &= bd.legal(own, opp, prev);
            // the candidates above the cursor
            const int cy = cur < 0 ? -1 : cur / S, cx = cur < 0 ? 0 : cur % S;
            const uint32_t rem = (y > cy) ? cand : ((y == cy) ? (cand & ~((2u << cx) - 1u)) : 0u);
            const int next = lowest_point<S>(rem, half);
            const int only = lowest_point<S>(cand, half);
            int res = R_NONE, a = G::N;
            bool play = false;
            if (work) {
                if (atk && L >= 3) res = R_ESC;
                else if (atk && L == 1) { res = only >= 0 ? R_CAP : R_ESC; a = only; }
                else if (next < 0) res = atk ? R_ESC : R_CAP;
                else { a = next; play = true; }
            }
            if (work && (play || (res == R_CAP && atk && L == 1))) Cs[half][d] = a;
            // the ply (a pass where nothing is played: no stone, no flood)
            const int mv = play ? a : G::N;
            const uint32_t pb = (play && y == mv / S) ? (1u << (mv % S)) : 0u;
            uint32_t o2 = own, p2 = opp;
            (void)bd.advance(o2, p2, mv);
            const uint32_t d2 = atk ? p2 : o2;
            const bool tgone = !rows::half_any(d2 & tb, half);
            const bool sgone = !rows::half_any(o2 & pb, half);
            const uint32_t g2 = bd.flood(tb & d2, d2);
            const int L2 = half_sum(__popc(bd.nbr4(g2) & ~(o2 | p2) & bd.M));
            bool push = false;
            if (play) {
                if (atk) {
                    if (tgone) res = R_CAP;
                    else if (!sgone) push = true;
                } else {
                    if (tgone || L2 <= 1) {}
                    else if (L2 >= 3) res = R_ESC;
                    else push = true;
                }
            }
            bool finished = false;
            if (push) {
                nodes++;
                if (nodes > SGO_TACTICS_MAX_NODES || d + 1 > SGO_TACTICS_MAX_DEPTH) { ret = R_UNK; finished = true; }
                else {
                    d++;
                    F[half][d][0][y] = p2;
                    F[half][d][1][y] = o2;
                    Cs[half][d] = -1;
                    ret = R_NONE;
                }
            } else if (run && (popnow || res != R_NONE)) {           // the top frame returns
                if (!popnow) ret = res;
                if (d == 0) finished = true;
                else d--;
            }
            if (finished) {                                          // the query is over: ret, and the root's cursor
                const int m0 = Cs[half][0];
                nodes_sum += nodes;
                if (q == 0) {
                    resA = ret;
                    mvA = ret == R_CAP ? m0 : -1;
                    if (L0 == 1 || (L0 == 2 && ret == R_CAP)) {      // query D: the defender moves first
                        q = 1;
                        root_atk = false;
                        d = 0; nodes = 1; ret = R_NONE;
                        const bool mw = def_white;
                        F[half][0][0][y] = mw ? white : black;
                        F[half][0][1][y] = mw ? black : white;
                        rootprev = (mw == stm_white) ? (mw ? pwhite : pblack) : (mw ? white : black);
                        Cs[half][0] = -1;
                    } else done = true;
                } else {
                    resD = ret;
                    mvD = ret == R_ESC ? m0 : -1;
                    done = true;
                }
            }
        } while (__any(!done));
        if (item && y == 0) {
            int st = 0;
            if (resA == R_CAP) st |= SGO_TACTICS_A_CAPTURED;
            if (resA == R_UNK) st |= SGO_TACTICS_A_UNKNOWN;
            if (q == 1) st |= SGO_TACTICS_D_RAN;
            if (resD == R_CAP) st |= SGO_TACTICS_D_CAPTURED;
            if (resD == R_UNK) st |= SGO_TACTICS_D_UNKNOWN;
            row[4] = st; row[5] = mvA; row[6] = mvD; row[7] = nodes_sum;
        }
    }
}

static int g_tactics_stage = 0;   // 0: both kernels, 1: k_tactics_chains only, 2: k_tactics_read only (timing)

int launch_tactics(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int max_chains, uint8_t *d_libs,
                   int32_t *d_n_chains, int32_t *d_chains, hipStream_t st) {
    if (g_tactics_stage != 2) {
        SGO_DISPATCH(S, k_tactics_chains<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(n, d_records, n_records, d_index, max_chains, d_libs,
                                                                                      d_n_chains, d_chains));
        SGO_HIP(hipGetLastError());
    }
    if (g_tactics_stage != 1) {
        SGO_DISPATCH(S, k_tactics_read<kS><<<dim3(cdiv(max_chains, 2), n < 65535 ? n : 65535), dim3(64), 0, st>>>(
                            n, d_records, n_records, d_index, max_chains, d_n_chains, d_chains));
        SGO_HIP(hipGetLastError());
    }
    return SGO_OK;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_tactics_stage(int stage) {
    const int prev = g_tactics_stage;
    if (stage >= 0 && stage <= 2) g_tactics_stage = stage;
    return prev;
}

int sgo_tactics_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int max_chains, uint8_t *d_libs,
                    int32_t *d_n_chains, int32_t *d_chains, void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || max_chains < 1 || max_chains > SGO_TACTICS_MAX_CHAINS || !d_records || !d_libs ||
        !d_n_chains || !d_chains) {
        set_error("sgo_tactics_dev: bad argument (unsupported size, n < 0, max_chains outside [1, 128], a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_tactics(S, n, d_records, n_records, d_index, max_chains, d_libs, d_n_chains, d_chains, (hipStream_t)stream);
}

int sgo_tactics(int S, int n, const uint32_t *records, int max_chains, uint8_t *libs, int32_t *n_chains, int32_t *chains) {
    if (!size_ok(S) || n < 0 || max_chains < 1 || max_chains > SGO_TACTICS_MAX_CHAINS || !records || !libs || !n_chains || !chains) {
        set_error("sgo_tactics: bad argument (unsupported size, n < 0, max_chains outside [1, 128], a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    // the caller's chain rows go in, so that unwritten rows come back as they were
    const HostArray a[] = {{(size_t)n * max_chains * 8 * sizeof(int32_t), chains, chains}, {(size_t)n * sizeof(int32_t), nullptr, n_chains}, {(size_t)n * S * S, nullptr, libs}};
    return host_entry("sgo_tactics", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_tactics(S, n, d_records, n, nullptr, max_chains, d[2], reinterpret_cast<int32_t *>(d[1]), reinterpret_cast<int32_t *>(d[0]), nullptr);
    });
}

}  // extern "C"
