// sgo_race.hip -- a capturing-race reader on the device (include/sgo.h "capturing races"): per packed record the table of the pairs
// of a black and a white chain in contact and short of liberties (or the one pair asked for), the region M each pair is read in,
// and for EACH of the two chains the verdict of an exhaustive reader bounded by M in which both sides play -- the attacker first
// (query A) and, when that catches, the defender first (query D) -- and the defender may capture the attacker's chain back.  A
// translation unit of its own, like sgo_solve.hip: tests/test_engine_isa.py pins the kernel set of sgo_engine.hip, and nothing here
// touches k_search.
//
//   k_race_pairs<S>   per listed record: the black chains by lowest point, for each the white chains its stones or liberties touch
//                     by lowest point, liberties, M0 / M1 and the inner-chain rule; n_pairs, words 0..7 of the rows (words 8..15
//                     preset to -1 x 4, 0 x 4), the region sets
//   k_race_read<S>    per (row, pair slot): one wavefront, half 0 reads the black racer as the defender, half 1 the white one;
//                     queries A and D of the header's reader; status bits and words 8..15 of the row
//
// sgo_session_race runs the same two kernels over the context's records, with the root index k_session_roots (sgo_session.hpp)
// writes.
//
// No rule is restated: the ply is rows::Board<S>::advance, ALLOWED is Board::legal with the `prev` handling of k_solve_read, the
// "stone would stand" test of rules = 1 is the ply itself.  The frame walk of k_race_read is the TWIN of k_solve_read's
// (csrc/sgo_solve.hip): the same frames, cursor and trip; what differs is the terminal (one flood and a neighbour mask instead of
// life_core), the defender's capture of the other racer, and that the two halves of a wave read one pair.  The two are kept apart so
// that the solve kernel's code stays byte for byte what its tests pinned.
//
// Kernel form: one board row per lane (sgo_rows.hpp), one wavefront per workgroup.  The floods vote over the whole wave, so both
// halves run every loop in lockstep: a half that is done, idle or out of range goes on with an EMPTY board (its floods end at
// once) and only its stores differ.  No flood, advance or shuffle sits under a per-half branch; the branches around them (`rules`,
// "some half entered a node") are the wave's.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_rows.hpp"

namespace sgo {

// One 32-lane half per listed row.  The partners of a black chain B within the liberty bound are named by the white stones in
// nbr(B) | nbr(lib(B)): a white stone next to B touches it, a white stone next to a liberty of B shares that liberty, and there is no
// other contact.  The union of their chains is walked by lowest point, which is each chain's anchor, so the rows come out in
// ascending (anchor_b, anchor_w) order.
// TRIPS: three floods for an asked pair; the outer loop takes one trip per black chain of the half with more of them (every trip
// clears at least the seed from `rest_b`), the inner loop one per partner chain (the same for `rest_w`), with five floods a trip.
// Termination does not depend on the data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_race_pairs(int n, const uint32_t *records, int n_records, const int32_t *index, const int32_t *ask,
                                                   const uint32_t *region, int max_libs, int max_region, int max_pairs, int32_t *n_pairs,
                                                   int32_t *rows_out, uint32_t *regions) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long i = (long)blockIdx.x * 2 + half;
    const bool valid = i < n;
    const int r = valid ? (index ? index[i] : (int)i) : -1;
    const bool ok = r >= 0 && r < n_records;                         // uniform over the half
    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    const rows::Board<S> bd(half, y);
    const uint32_t rb = rec ? rows::load_row<S>(rec, y) : 0u, rw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
    const uint32_t emp = ok ? (~(rb | rw) & bd.M) : 0u;
    const int p = (ok && ask) ? ask[2 * i] : -1, q = (ok && ask) ? ask[2 * i + 1] : -1;
    const bool enumerate = p < 0;
    const bool given = !enumerate && region != nullptr;              // the caller's M, masked to the board by load_row
    const uint32_t given_m = given ? rows::load_row<S>(region + (size_t)i * G::NW, y) : 0u;

    // an asked row walks the one pair on the asked points, in either colour order
    const uint32_t pbit = (!enumerate && p < G::N && y == p / S) ? (1u << (p % S)) : 0u;
    const uint32_t qbit = (!enumerate && q >= 0 && q < G::N && y == q / S) ? (1u << (q % S)) : 0u;
    const bool p_b = rows::half_any(pbit & rb, half), p_w = rows::half_any(pbit & rw, half);
    const bool q_b = rows::half_any(qbit & rb, half), q_w = rows::half_any(qbit & rw, half);
    const bool pq = p_b && q_w, qp = !pq && p_w && q_b;
    const uint32_t ask_b = bd.flood((pq ? pbit : qp ? qbit : 0u) & rb, rb), ask_w = bd.flood((pq ? qbit : qp ? pbit : 0u) & rw, rw);
    uint32_t rest_b = enumerate ? rb : ask_b;

    int count = 0;
    int32_t *ro = valid ? rows_out + (size_t)i * max_pairs * 16 : nullptr;
    uint32_t *go = valid ? regions + (size_t)i * max_pairs * G::NW : nullptr;
    while (__any(rest_b != 0)) {
        const int ab = lowest_point<S>(rest_b, half);
        const uint32_t seed_b = (ab >= 0 && y == ab / S) ? (1u << (ab % S)) : 0u;
        const uint32_t B = bd.flood(seed_b, rb);
        const uint32_t nb_b = bd.nbr4(B), lib_b = nb_b & emp;
        const int n_b = half_sum(__popc(lib_b));
        const bool b_in = ab >= 0 && n_b >= 1 && n_b <= max_libs;
        const uint32_t named = enumerate ? (b_in ? rw & (nb_b | bd.nbr4(lib_b)) : 0u) : ask_w;
        uint32_t rest_w = bd.flood(ab >= 0 ? named : 0u, rw);        // a half whose chains are through names nothing
        while (__any(rest_w != 0)) {
            const int aw = lowest_point<S>(rest_w, half);
            const bool act = aw >= 0;
            const uint32_t seed_w = (act && y == aw / S) ? (1u << (aw % S)) : 0u;
            const uint32_t W = bd.flood(seed_w, rw);
            const uint32_t lib_w = bd.nbr4(W) & emp;
            const int n_w = half_sum(__popc(lib_w)), shared = half_sum(__popc(lib_b & lib_w));
            const uint32_t m0 = act ? (lib_b | lib_w) : 0u;
            const uint32_t m1 = m0 | (bd.nbr4(m0) & emp);
            // the other chains with a liberty, and every liberty in M1
            const uint32_t ob = act ? (rb & ~B) : 0u, ow = act ? (rw & ~W) : 0u;
            const uint32_t l_out = bd.nbr4(emp & ~m1), l_in = bd.nbr4(emp & m1);
            const uint32_t out_b = bd.flood(ob & l_out, ob), in_b = bd.flood(ob & l_in, ob);
            const uint32_t out_w = bd.flood(ow & l_out, ow), in_w = bd.flood(ow & l_in, ow);
            const uint32_t m = given ? given_m : (m1 | (in_b & ~out_b) | (in_w & ~out_w));
            const int re = half_sum(__popc(m & emp));
            const bool open = re < 1 || re > max_region;
            const uint32_t wm = rows::gather_word<S>(m, half, y);
            if (act && (enumerate ? (n_w >= 1 && n_w <= max_libs && !open) : true)) {
                if (count < max_pairs) {
                    if (y == 0) {
                        int32_t *o = ro + (size_t)count * 16;
                        o[0] = ab; o[1] = aw; o[2] = n_b; o[3] = n_w; o[4] = shared; o[5] = re; o[6] = open ? SGO_RACE_OPEN : 0; o[7] = 0;
                        o[8] = -1; o[9] = -1; o[10] = -1; o[11] = -1; o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 0;
                    }
                    if (y < G::NW) go[(size_t)count * G::NW + y] = wm;
                }
                count++;
            }
            rest_w &= ~W;
        }
        rest_b &= ~B;
    }
    if (ok && !enumerate && !pq && !qp) {                            // no pair on the asked points
        if (y == 0) {
            ro[0] = -1; ro[1] = -1; ro[2] = 0; ro[3] = 0; ro[4] = 0; ro[5] = 0; ro[6] = SGO_RACE_NO_PAIR; ro[7] = 0;
            ro[8] = -1; ro[9] = -1; ro[10] = -1; ro[11] = -1; ro[12] = 0; ro[13] = 0; ro[14] = 0; ro[15] = 0;
        }
        if (y < G::NW) go[y] = 0u;
        count = 1;
    }
    if (valid && y == 0) n_pairs[i] = count;
}

enum { R_NONE = 0, R_CAUGHT = 1, R_SAFE = 2, R_UNK = 3 };
constexpr int R_FRAMES = SGO_RACE_MAX_DEPTH + 1;                     // depths 0 .. MAX_DEPTH hold a frame
constexpr int R_ENTER = -2;                                          // a cursor: the node has not been entered (no terminal test yet)

// One wavefront per (row, pair slot): half 0 reads the black racer of the pair as the defender, half 1 the white one, on the same
// record in the same region, so the queries of a pair that can run at once do, and the tail of a pair is its longer racer.  The
// walk is k_solve_read's: a frame is the position of a node BEFORE its move (own = the node's mover, opp), 256 bytes per half and
// frame, plus the candidate cursor: 2 * 81 * 260 bytes = 42 KB of static LDS per workgroup.  The cursor is R_ENTER for a frame just
// pushed, then -1, then the last candidate tried, and N once the defender's pass (or the attacker's wait) has been tried.  The ko
// `prev` of a node is its parent frame's opp rows; after a pass or a wait those are the node's own rows, so nothing is forbidden.
// One trip of the loop is one node step: what the top frame's child returned is taken in; a frame entered in this trip gets its
// terminal test (one flood of the defender's racer, its liberties against M and max_libs; the wave skips the flood when neither
// half entered a node); the candidates above the cursor are found; the next one is played and judged; the frame returns, a child
// frame is pushed, or the cursor has moved on.
// CANDIDATES: as in k_solve_read: rules = 0 takes the empty points of M in Board::legal; rules = 1 the empty points of M that are
// not the ko point, and the ply shows whether the stone stands.
// TRIPS: every trip pushes a frame (at most max_nodes per query), pops one or moves a cursor up (at most N + 1 times per frame), so
// a launch takes at most 2 * (max_nodes + 1) * (N + 3) trips per query and two queries per half; a trip is at most three floods, one
// Board::legal and one advance, each bounded on its own.  Termination does not depend on the data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_race_read(int n, const uint32_t *records, int n_records, const int32_t *index, int rules, int max_libs,
                                                  int max_nodes, int max_pairs, const int32_t *n_pairs, int32_t *rows_out,
                                                  const uint32_t *regions) {
    using G = Geo<S>;
    __shared__ uint32_t F[2][R_FRAMES][2][32];
    __shared__ int32_t Cs[2][R_FRAMES];
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const int j = blockIdx.x;                                        // pair slot
    const rows::Board<S> bd(half, y);
    for (int i = blockIdx.y; i < n; i += gridDim.y) {                // the trip count is the workgroup's
        const int r = index ? index[i] : i;
        const bool ok = r >= 0 && r < n_records;
        const int cnt = ok ? n_pairs[i] : 0;
        const bool listed = j < max_pairs && j < cnt;
        int32_t *row = rows_out + ((size_t)i * max_pairs + (listed ? j : 0)) * 16;
        const bool item = listed && row[6] == 0;                     // uniform over the WAVE; open and pair-less rows are not read
        if (!item) continue;
        const uint32_t *rec = records + (size_t)r * G::RW;
        const uint32_t black = rows::load_row<S>(rec, y), white = rows::load_row<S>(rec + G::NW, y);
        const uint32_t pblack = rows::load_row<S>(rec + 2 * G::NW, y), pwhite = rows::load_row<S>(rec + 3 * G::NW, y);
        const bool stm_white = (rec[G::META_WORD] & G::META_BIT) != 0;
        const uint32_t m = rows::load_row<S>(regions + ((size_t)i * max_pairs + j) * G::NW, y);
        const bool def_white = half != 0;
        const int t = row[def_white ? 1 : 0], u = row[def_white ? 0 : 1];   // tD, tA
        const uint32_t tb = (y == t / S) ? (1u << (t % S)) : 0u, ub = (y == u / S) ? (1u << (u % S)) : 0u;

        bool done = false, root_atk = true;
        int q = 0;                                                   // 0: query A, 1: query D
        int d = 0, nodes = 1, ret = R_NONE;
        int resA = R_NONE, resD = R_NONE, mvA = -1, mvD = -1, nodesA = 0, nodesD = 0;
        uint32_t rootprev;
        {   // root of query A: the attacker moves
            const bool mw = !def_white;
            F[half][0][0][y] = mw ? white : black;
            F[half][0][1][y] = mw ? black : white;
            rootprev = (mw == stm_white) ? (mw ? pwhite : pblack) : (mw ? white : black);
            Cs[half][0] = R_ENTER;
        }
        do {
            const bool run = !done;
            const bool atk = ((d & 1) != 0) != root_atk;             // the top frame's mover is the attacker
            int cur = Cs[half][d];
            bool popnow = false;
            if (run && ret != R_NONE) {                              // what the child of the last candidate returned
                if (atk ? ret == R_CAUGHT : ret == R_SAFE) popnow = true;
                else ret = R_NONE;
            }
            const bool work = run && !popnow;
            const bool fresh = work && cur == R_ENTER;
            if (cur == R_ENTER) cur = -1;
            const uint32_t own = work ? F[half][d][0][y] : 0u, opp = work ? F[half][d][1][y] : 0u;
            const uint32_t prev = work ? (d > 0 ? F[half][d - 1][1][y] : rootprev) : 0u;
            const uint32_t dst = atk ? opp : own;
            const uint32_t emp = ~(own | opp) & bd.M;
            // the terminal test of a node entered in this trip: the racer's liberties leave M or pass max_libs
            uint32_t chain = 0u;
            if (__any(fresh)) chain = bd.flood(fresh ? (dst & tb) : 0u, fresh ? dst : 0u);
            const uint32_t L = bd.nbr4(chain) & emp;
            const int nL = half_sum(__popc(L));
            const bool escaped = fresh && (rows::half_any(L & ~m, half) || nL > max_libs);
            // the candidates, and those above the cursor
            const uint32_t gone = prev & ~own;
            const uint32_t ko = rows::half_one_bit(gone, half) ? gone : 0u;
            const bool banned = rows::half_any(ko & emp & m, half);  // the ko test forbids the mover an empty point of M
            uint32_t cand = rules ? (emp & ~ko) : bd.legal(own, opp, prev);
            cand &= m;
            const int cy = cur < 0 ? -1 : cur / S, cx = cur < 0 ? 0 : cur % S;
            const uint32_t rem = cur >= G::N ? 0u : ((y > cy) ? cand : ((y == cy) ? (cand & ~((2u << cx) - 1u)) : 0u));
            const int next = lowest_point<S>(rem, half);
            int res = R_NONE, a = G::N;
            bool play = false, pass = false;
            if (work) {
                if (escaped) res = R_SAFE;
                else if (next >= 0) { a = next; play = true; }
                else if (cur < G::N && (!atk || banned)) pass = true;   // the defender's pass, the attacker's wait: the last candidate
                else res = atk ? R_SAFE : R_CAUGHT;
            }
            if (play || pass) Cs[half][d] = a;
            // the ply (a pass where nothing is played: no stone, no flood).  Every candidate comes from `emp`, so advance never
            // takes its early return for an occupied point, which would be a per-half branch.
            const int mv = play ? a : G::N;
            const uint32_t pb = (play && y == mv / S) ? (1u << (mv % S)) : 0u;
            uint32_t o2 = own, p2 = opp;
            (void)bd.advance(o2, p2, mv);
            const bool tgone = !rows::half_any((atk ? p2 : o2) & tb, half);
            const bool ugone = !rows::half_any((atk ? o2 : p2) & ub, half);
            const bool sgone = !rows::half_any(o2 & pb, half);
            bool push = pass;
            if (play) {
                if (atk) {
                    if (tgone) res = R_CAUGHT;
                    else if (!sgone) push = true;                    // else: the next candidate
                } else if (!tgone && !sgone) {
                    if (ugone) res = R_SAFE;                         // the defender captured the attacker's racer
                    else push = true;
                }
            }
            bool finished = false;
            if (push) {
                nodes++;
                if (nodes > max_nodes || d + 1 > SGO_RACE_MAX_DEPTH) { ret = R_UNK; finished = true; }
                else {
                    d++;
                    F[half][d][0][y] = p2;
                    F[half][d][1][y] = o2;
                    Cs[half][d] = R_ENTER;
                    ret = R_NONE;
                }
            } else if (run && (popnow || res != R_NONE)) {           // the top frame returns
                if (!popnow) ret = res;
                if (d == 0) finished = true;
                else d--;
            }
            if (finished) {                                          // the query is over: ret, and the root's cursor
                const int c0 = Cs[half][0], m0 = c0 < 0 ? -1 : c0;
                if (q == 0) {
                    resA = ret;
                    mvA = ret == R_CAUGHT ? m0 : -1;
                    nodesA = nodes;
                    if (ret == R_CAUGHT) {                           // query D: the defender moves first
                        q = 1;
                        root_atk = false;
                        d = 0; nodes = 1; ret = R_NONE;
                        const bool mw = def_white;
                        F[half][0][0][y] = mw ? white : black;
                        F[half][0][1][y] = mw ? black : white;
                        rootprev = (mw == stm_white) ? (mw ? pwhite : pblack) : (mw ? white : black);
                        Cs[half][0] = R_ENTER;
                    } else done = true;
                } else {
                    resD = ret;
                    mvD = ret == R_SAFE ? m0 : -1;
                    nodesD = nodes;
                    done = true;
                }
            }
        } while (__any(!done));
        int st = 0;
        if (resA == R_CAUGHT) st |= SGO_RACE_A_CAUGHT;
        if (resA == R_UNK) st |= SGO_RACE_A_UNKNOWN;
        if (q == 1) st |= SGO_RACE_D_RAN;
        if (resD == R_CAUGHT) st |= SGO_RACE_D_CAUGHT;
        if (resD == R_UNK) st |= SGO_RACE_D_UNKNOWN;
        const int st_w = __shfl(st, 32, 64);                         // the white racer's bits, for the lane that writes the word
        if (y == 0) {
            int32_t *o = row + (def_white ? 10 : 8), *c = row + (def_white ? 14 : 12);
            o[0] = mvA; o[1] = mvD; c[0] = nodesA; c[1] = nodesD;
            if (!def_white) row[6] = st | (st_w << SGO_RACE_WHITE_SHIFT);
        }
    }
}

int launch_race(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask, const uint32_t *d_region,
                int rules, int max_libs, int max_region, int max_nodes, int max_pairs, int32_t *d_n_pairs, int32_t *d_rows, uint32_t *d_regions,
                hipStream_t st) {
    SGO_DISPATCH(S, k_race_pairs<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(n, d_records, n_records, d_index, d_ask, d_region, max_libs,
                                                                              max_region, max_pairs, d_n_pairs, d_rows, d_regions));
    SGO_HIP(hipGetLastError());
    SGO_DISPATCH(S, k_race_read<kS><<<dim3(max_pairs, n < 65535 ? n : 65535), dim3(64), 0, st>>>(
                        n, d_records, n_records, d_index, rules, max_libs, max_nodes, max_pairs, d_n_pairs, d_rows, d_regions));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

bool race_params_ok(int rules, int max_libs, int max_region, int max_nodes, int max_pairs) {
    return (rules == 0 || rules == 1) && max_libs >= 1 && max_libs <= SGO_RACE_MAX_LIBS && max_region >= 1 && max_region <= SGO_RACE_MAX_REGION &&
           max_nodes >= 1 && max_nodes <= SGO_RACE_MAX_NODES && max_pairs >= 1 && max_pairs <= SGO_RACE_MAX_PAIRS;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_race_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask, const uint32_t *d_region,
                 int rules, int max_libs, int max_region, int max_nodes, int max_pairs, int32_t *d_n_pairs, int32_t *d_rows, uint32_t *d_regions,
                 void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || !race_params_ok(rules, max_libs, max_region, max_nodes, max_pairs) || !d_records || !d_n_pairs ||
        !d_rows || !d_regions) {
        set_error("sgo_race_dev: bad argument (unsupported size, n < 0, n_records < 0, rules outside {0, 1}, max_libs outside [1, 8], "
                  "max_region outside [1, 32], max_nodes outside [1, 32768], max_pairs outside [1, 64], a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_race(S, n, d_records, n_records, d_index, d_ask, d_region, rules, max_libs, max_region, max_nodes, max_pairs, d_n_pairs, d_rows,
                       d_regions, (hipStream_t)stream);
}

int sgo_race(int S, int n, const uint32_t *records, const int32_t *ask, const uint32_t *region, int rules, int max_libs, int max_region,
             int max_nodes, int max_pairs, int32_t *n_pairs, int32_t *rows_out, uint32_t *regions) {
    if (!size_ok(S) || n < 0 || !race_params_ok(rules, max_libs, max_region, max_nodes, max_pairs) || !records || !n_pairs || !rows_out || !regions) {
        set_error("sgo_race: bad argument (unsupported size, n < 0, rules outside {0, 1}, max_libs outside [1, 8], max_region outside [1, 32], "
                  "max_nodes outside [1, 32768], max_pairs outside [1, 64], a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const size_t plane = sizeof(uint32_t) * sgo_plane_words(S);
    // the caller's rows and region sets go in, so that unwritten rows come back as they were
    const HostArray a[] = {{(size_t)n * max_pairs * 16 * sizeof(int32_t), rows_out, rows_out},
                           {(size_t)n * max_pairs * plane, regions, regions},
                           {(size_t)n * sizeof(int32_t), nullptr, n_pairs},
                           {ask ? (size_t)n * 2 * sizeof(int32_t) : 0, ask, nullptr},
                           {region ? (size_t)n * plane : 0, region, nullptr}};
    return host_entry("sgo_race", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_race(S, n, d_records, n, nullptr, ask ? reinterpret_cast<const int32_t *>(d[3]) : nullptr,
                           region ? reinterpret_cast<const uint32_t *>(d[4]) : nullptr, rules, max_libs, max_region, max_nodes, max_pairs,
                           reinterpret_cast<int32_t *>(d[2]), reinterpret_cast<int32_t *>(d[0]), reinterpret_cast<uint32_t *>(d[1]), nullptr);
    });
}

}  // extern "C"
