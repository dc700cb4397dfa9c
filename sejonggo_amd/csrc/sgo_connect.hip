// sgo_connect.hip -- a connection reader on the device (include/sgo.h "connections"): per packed record the table of the pairs of two
// chains of ONE colour that are near each other (or the one pair asked for), the region M each pair is read in, the verdict of an
// exhaustive reader bounded by M -- can the other colour keep the two from becoming one chain, moving first (query A) and, when it
// can, moving second (query D)? -- and, on top of the verdicts, the map of the GROUPS the `connected` pairs tie the chains into.  A
// translation unit of its own, like sgo_solve.hip and sgo_race.hip: tests/test_engine_isa.py pins the kernel set of sgo_engine.hip,
// and nothing here touches k_search.
//
//   k_connect_pairs<S>    per listed record: the chains of either colour by lowest point, for each the chains of its colour that its
//                         liberties, their empty neighbours or an opposing chain in contact lead to, by lowest point; link points,
//                         cutting chains, M1 and the inner-chain rule; n_pairs, words 0..7 of the rows (words 8..11 preset to -1 x 2,
//                         0 x 2), the region sets
//   k_connect_read<S>     per (row, two pair slots): one wavefront, half h reads pair slot 2k + h; queries A and D of the header's
//                         reader; status bits and words 8..11 of the row
//   k_connect_groups<S>   per listed record: labels over the written rows to a fixed point, then one flood per chain paints the map
//
// sgo_session_connect runs the same three kernels over the context's records, with the root index k_session_roots (sgo_session.hpp)
// writes.
//
// No rule is restated: the ply is rows::Board<S>::advance, ALLOWED is Board::legal with the `prev` handling of k_solve_read, the
// "stone would stand" test of rules = 1 is the ply itself.  The frame walk of k_connect_read is the third TWIN of k_solve_read's and
// k_race_read's (DESIGN.md "The two walks are twins"): the same frames, cursor and trip; what differs is the terminal (one flood from
// tx and a bit test), the attacker's pass that is always its last candidate, a defender that never passes, and that the two halves of
// a wave read two PAIRS.  The three are kept apart so that the other kernels' code stays byte for byte what their tests pinned.
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

constexpr int C_WORDS = 12;                                          // words of a table row

// One 32-lane half per listed row.  The chains of BOTH colours are walked by lowest point of black | white, which is each chain's
// anchor, so the rows come out in ascending (anchor_x, anchor_y) order with the colours interleaved.  The partners of a chain X are
// named by the stones of its colour in nbr(lib(X)) (a common liberty), in nbr(nbr(lib(X)) & empty) (a liberty next to a liberty of
// X) and next to an opposing chain that touches X (a cutting chain, whatever its liberties: the pair's own test decides); there is no
// other way for K to be non-empty.  Only chains not yet walked are partners: anchor_x < anchor_y.
// TRIPS: two floods for an asked pair; the outer loop takes one trip per chain of the half with more of them (every trip clears at
// least the seed from `rest`), the middle loop one per partner chain (the same for `rest_y`) with seven floods a trip, the inner
// loop one per opposing chain that touches both (the same for `rest_z`) with one flood a trip.  Termination does not depend on the
// data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_connect_pairs(int n, const uint32_t *records, int n_records, const int32_t *index, const int32_t *ask,
                                                      const uint32_t *region, int cut_libs, int max_region, int max_pairs, int32_t *n_pairs,
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

    // an asked row walks the one pair on the asked points: two stones of one colour in two chains
    const uint32_t pbit = (!enumerate && p < G::N && y == p / S) ? (1u << (p % S)) : 0u;
    const uint32_t qbit = (!enumerate && q >= 0 && q < G::N && y == q / S) ? (1u << (q % S)) : 0u;
    const bool p_b = rows::half_any(pbit & rb, half), p_w = rows::half_any(pbit & rw, half);
    const bool q_b = rows::half_any(qbit & rb, half), q_w = rows::half_any(qbit & rw, half);
    const bool same = (p_b && q_b) || (p_w && q_w);
    const uint32_t ask_s = same ? (p_b ? rb : rw) : 0u;
    const uint32_t ask_p = bd.flood(pbit & ask_s, ask_s), ask_q = bd.flood(qbit & ask_s, ask_s);
    const bool pair_ok = same && !rows::half_any(ask_p & qbit, half);
    const uint32_t ask_set = pair_ok ? (ask_p | ask_q) : 0u;
    uint32_t rest = enumerate ? (rb | rw) : ask_set;

    int count = 0;
    int32_t *ro = valid ? rows_out + (size_t)i * max_pairs * C_WORDS : nullptr;
    uint32_t *go = valid ? regions + (size_t)i * max_pairs * G::NW : nullptr;
    while (__any(rest != 0)) {
        const int ax = lowest_point<S>(rest, half);
        const uint32_t seed_x = (ax >= 0 && y == ax / S) ? (1u << (ax % S)) : 0u;
        const bool x_black = rows::half_any(seed_x & rb, half);
        const uint32_t own = ax >= 0 ? (x_black ? rb : rw) : 0u, opp = ax >= 0 ? (x_black ? rw : rb) : 0u;
        const uint32_t X = bd.flood(seed_x, own);
        rest &= ~X;
        const uint32_t nb_x = bd.nbr4(X), lib_x = nb_x & emp;
        const uint32_t ZX = bd.flood(opp & nb_x, opp);               // the opposing chains that touch X
        const uint32_t named = enumerate ? (own & (bd.nbr4(lib_x) | bd.nbr4(bd.nbr4(lib_x) & emp) | bd.nbr4(ZX))) : ask_set;
        uint32_t rest_y = bd.flood(named & own & ~X, own) & rest;    // whole chains, and only those not walked yet
        while (__any(rest_y != 0)) {
            const int ay = lowest_point<S>(rest_y, half);
            const bool act = ay >= 0;
            const uint32_t seed_y = (act && y == ay / S) ? (1u << (ay % S)) : 0u;
            const uint32_t Y = bd.flood(seed_y, own);
            rest_y &= ~Y;
            const uint32_t nb_y = bd.nbr4(Y), lib_y = nb_y & emp;
            const int shared = half_sum(__popc(lib_x & lib_y));
            uint32_t k = act ? ((lib_x & lib_y) | (lib_x & bd.nbr4(lib_y)) | (lib_y & bd.nbr4(lib_x))) : 0u;
            // the cutting chains: the opposing chains that touch both, short of liberties
            uint32_t rest_z = (act && cut_libs > 0) ? bd.flood(ZX & nb_y, ZX) : 0u;
            int n_cut = 0;
            while (__any(rest_z != 0)) {
                const int az = lowest_point<S>(rest_z, half);
                const uint32_t seed_z = (az >= 0 && y == az / S) ? (1u << (az % S)) : 0u;
                const uint32_t Z = bd.flood(seed_z, rest_z);
                rest_z &= ~Z;
                const uint32_t lib_z = bd.nbr4(Z) & emp;
                const int n_z = half_sum(__popc(lib_z));
                if (az >= 0 && n_z >= 1 && n_z <= cut_libs) { k |= lib_z; n_cut++; }
            }
            const int n_k = half_sum(__popc(k));
            const uint32_t m1 = k | (bd.nbr4(k) & emp);
            // the other chains with a liberty, and every liberty in M1; a cutting chain is one of them, its liberties lie in K
            const uint32_t oo = act ? (own & ~(X | Y)) : 0u, op = act ? opp : 0u;
            const uint32_t l_out = bd.nbr4(emp & ~m1), l_in = bd.nbr4(emp & m1);
            const uint32_t out_o = bd.flood(oo & l_out, oo), in_o = bd.flood(oo & l_in, oo);
            const uint32_t out_p = bd.flood(op & l_out, op), in_p = bd.flood(op & l_in, op);
            const uint32_t m = given ? given_m : (m1 | (in_o & ~out_o) | (in_p & ~out_p));
            const int re = half_sum(__popc(m & emp));
            const bool open = re < 1 || re > max_region;
            const uint32_t wm = rows::gather_word<S>(m, half, y);
            if (act && (enumerate ? (n_k >= 1 && !open) : true)) {
                if (count < max_pairs) {
                    if (y == 0) {
                        int32_t *o = ro + (size_t)count * C_WORDS;
                        o[0] = ax; o[1] = ay; o[2] = x_black ? 1 : -1; o[3] = shared; o[4] = n_k; o[5] = re;
                        o[6] = open ? SGO_CONNECT_OPEN : 0; o[7] = n_cut; o[8] = -1; o[9] = -1; o[10] = 0; o[11] = 0;
                    }
                    if (y < G::NW) go[(size_t)count * G::NW + y] = wm;
                }
                count++;
            }
        }
    }
    if (ok && !enumerate && !pair_ok) {                              // no pair on the asked points
        if (y == 0) {
            ro[0] = -1; ro[1] = -1; ro[2] = 0; ro[3] = 0; ro[4] = 0; ro[5] = 0; ro[6] = SGO_CONNECT_NO_PAIR; ro[7] = 0;
            ro[8] = -1; ro[9] = -1; ro[10] = 0; ro[11] = 0;
        }
        if (y < G::NW) go[y] = 0u;
        count = 1;
    }
    if (valid && y == 0) n_pairs[i] = count;
}

enum { C_NONE = 0, C_CUT = 1, C_JOINED = 2, C_UNK = 3 };
constexpr int C_FRAMES = SGO_CONNECT_MAX_DEPTH + 1;                  // depths 0 .. MAX_DEPTH hold a frame
constexpr int C_ENTER = -2;                                          // a cursor: the node has not been entered (no terminal test yet)

// One wavefront per (row, two pair slots): half h reads pair slot 2 * blockIdx.x + h of the row, so two pairs share every flood's
// vote, the way the two racers of a pair do in k_race_read.  The walk is k_solve_read's: a frame is the position of a node BEFORE its
// move (own = the node's mover, opp), 256 bytes per half and frame, plus the candidate cursor: 2 * 81 * 260 bytes = 42 120 bytes of
// static LDS per workgroup, three workgroups per CU.  The cursor is C_ENTER for a frame just pushed, then -1, then the last candidate
// tried, and N once the attacker's pass has been tried.  The ko `prev` of a node is its parent frame's opp rows; after a pass those
// are the node's own rows, so nothing is forbidden.
// One trip of the loop is one node step: what the top frame's child returned is taken in; a frame entered in this trip gets its
// terminal test (one flood of the defender's stones from tx and the bit of ty; the wave skips the flood when neither half entered a
// node); the candidates above the cursor are found; the next one is played and judged; the frame returns, a child frame is pushed,
// or the cursor has moved on.
// CANDIDATES: as in k_solve_read: rules = 0 takes the empty points of M in Board::legal; rules = 1 the empty points of M that are
// not the ko point, and the ply shows whether the stone stands.
// TRIPS: every trip pushes a frame (at most max_nodes per query), pops one or moves a cursor up (at most N + 1 times per frame), so
// a launch takes at most 2 * (max_nodes + 1) * (N + 3) trips per query and two queries per half; a trip is at most three floods, one
// Board::legal and one advance, each bounded on its own.  Termination does not depend on the data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_connect_read(int n, const uint32_t *records, int n_records, const int32_t *index, int rules, int max_nodes,
                                                     int max_pairs, const int32_t *n_pairs, int32_t *rows_out, const uint32_t *regions) {
    using G = Geo<S>;
    __shared__ uint32_t F[2][C_FRAMES][2][32];
    __shared__ int32_t Cs[2][C_FRAMES];
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const int j = blockIdx.x * 2 + half;                             // pair slot
    const rows::Board<S> bd(half, y);
    for (int i = blockIdx.y; i < n; i += gridDim.y) {                // the trip count is the workgroup's
        const int r = index ? index[i] : i;
        const bool ok = r >= 0 && r < n_records;
        const int cnt = ok ? n_pairs[i] : 0;
        const bool listed = j < max_pairs && j < cnt;
        int32_t *row = rows_out + ((size_t)i * max_pairs + (listed ? j : 0)) * C_WORDS;
        const bool item = listed && row[6] == 0;                     // uniform over the HALF; open and pair-less rows are not read
        if (!__any(item)) continue;
        const uint32_t *rec = records + (size_t)r * G::RW;           // some half has an item, so the record is in range
        const uint32_t black = item ? rows::load_row<S>(rec, y) : 0u, white = item ? rows::load_row<S>(rec + G::NW, y) : 0u;
        const uint32_t pblack = item ? rows::load_row<S>(rec + 2 * G::NW, y) : 0u, pwhite = item ? rows::load_row<S>(rec + 3 * G::NW, y) : 0u;
        const bool stm_white = item && (rec[G::META_WORD] & G::META_BIT) != 0;
        const uint32_t m = item ? rows::load_row<S>(regions + ((size_t)i * max_pairs + j) * G::NW, y) : 0u;
        const int tx = item ? row[0] : 0, ty = item ? row[1] : 0;
        const bool def_white = item && row[2] < 0;
        const uint32_t txb = (item && y == tx / S) ? (1u << (tx % S)) : 0u, tyb = (item && y == ty / S) ? (1u << (ty % S)) : 0u;

        bool done = !item, root_atk = true;
        int q = 0;                                                   // 0: query A, 1: query D
        int d = 0, nodes = 1, ret = C_NONE;
        int resA = C_NONE, resD = C_NONE, mvA = -1, mvD = -1, nodesA = 0, nodesD = 0;
        uint32_t rootprev;
        {   // root of query A: the attacker moves
            const bool mw = !def_white;
            F[half][0][0][y] = mw ? white : black;
            F[half][0][1][y] = mw ? black : white;
            rootprev = (mw == stm_white) ? (mw ? pwhite : pblack) : (mw ? white : black);
            Cs[half][0] = C_ENTER;
        }
        do {
            const bool run = !done;
            const bool atk = ((d & 1) != 0) != root_atk;             // the top frame's mover is the attacker
            int cur = Cs[half][d];
            bool popnow = false;
            if (run && ret != C_NONE) {                              // what the child of the last candidate returned
                if (atk ? ret == C_CUT : ret == C_JOINED) popnow = true;
                else ret = C_NONE;
            }
            const bool work = run && !popnow;
            const bool fresh = work && cur == C_ENTER;
            if (cur == C_ENTER) cur = -1;
            const uint32_t own = work ? F[half][d][0][y] : 0u, opp = work ? F[half][d][1][y] : 0u;
            const uint32_t prev = work ? (d > 0 ? F[half][d - 1][1][y] : rootprev) : 0u;
            const uint32_t dst = atk ? opp : own;
            const uint32_t emp = ~(own | opp) & bd.M;
            // the terminal test of a node entered in this trip: the chain on tx holds ty
            uint32_t chain = 0u;
            if (__any(fresh)) chain = bd.flood(fresh ? (dst & txb) : 0u, fresh ? dst : 0u);
            const bool joined = fresh && rows::half_any(chain & tyb, half);
            // the candidates, and those above the cursor
            const uint32_t gone = prev & ~own;
            const uint32_t ko = rows::half_one_bit(gone, half) ? gone : 0u;
            uint32_t cand = rules ? (emp & ~ko) : bd.legal(own, opp, prev);
            cand &= m;
            const int cy = cur < 0 ? -1 : cur / S, cx = cur < 0 ? 0 : cur % S;
            const uint32_t rem = cur >= G::N ? 0u : ((y > cy) ? cand : ((y == cy) ? (cand & ~((2u << cx) - 1u)) : 0u));
            const int next = lowest_point<S>(rem, half);
            int res = C_NONE, a = G::N;
            bool play = false, pass = false;
            if (work) {
                if (joined) res = C_JOINED;
                else if (next >= 0) { a = next; play = true; }
                else if (cur < G::N && atk) pass = true;             // the attacker's pass: always its last candidate
                else res = atk ? C_JOINED : C_CUT;                   // the defender never passes
            }
            if (play || pass) Cs[half][d] = a;
            // the ply (a pass where nothing is played: no stone, no flood).  Every candidate comes from `emp`, so advance never
            // takes its early return for an occupied point, which would be a per-half branch.
            const int mv = play ? a : G::N;
            const uint32_t pb = (play && y == mv / S) ? (1u << (mv % S)) : 0u;
            uint32_t o2 = own, p2 = opp;
            (void)bd.advance(o2, p2, mv);
            const uint32_t def2 = atk ? p2 : o2;
            const bool tgone = !rows::half_any(def2 & txb, half) || !rows::half_any(def2 & tyb, half);
            const bool sgone = !rows::half_any(o2 & pb, half);
            bool push = pass;
            if (play) {
                if (atk) {
                    if (tgone) res = C_CUT;
                    else if (!sgone) push = true;                    // else: the next candidate
                } else if (!tgone && !sgone) push = true;
            }
            bool finished = false;
            if (push) {
                nodes++;
                if (nodes > max_nodes || d + 1 > SGO_CONNECT_MAX_DEPTH) { ret = C_UNK; finished = true; }
                else {
                    d++;
                    F[half][d][0][y] = p2;
                    F[half][d][1][y] = o2;
                    Cs[half][d] = C_ENTER;
                    ret = C_NONE;
                }
            } else if (run && (popnow || res != C_NONE)) {           // the top frame returns
                if (!popnow) ret = res;
                if (d == 0) finished = true;
                else d--;
            }
            if (finished) {                                          // the query is over: ret, and the root's cursor
                const int c0 = Cs[half][0], m0 = c0 < 0 ? -1 : c0;
                if (q == 0) {
                    resA = ret;
                    mvA = ret == C_CUT ? m0 : -1;
                    nodesA = nodes;
                    if (ret == C_CUT) {                              // query D: the defender moves first
                        q = 1;
                        root_atk = false;
                        d = 0; nodes = 1; ret = C_NONE;
                        const bool mw = def_white;
                        F[half][0][0][y] = mw ? white : black;
                        F[half][0][1][y] = mw ? black : white;
                        rootprev = (mw == stm_white) ? (mw ? pwhite : pblack) : (mw ? white : black);
                        Cs[half][0] = C_ENTER;
                    } else done = true;
                } else {
                    resD = ret;
                    mvD = ret == C_JOINED ? m0 : -1;
                    nodesD = nodes;
                    done = true;
                }
            }
        } while (__any(!done));
        int st = 0;
        if (resA == C_CUT) st |= SGO_CONNECT_A_CUT;
        if (resA == C_UNK) st |= SGO_CONNECT_A_UNKNOWN;
        if (q == 1) st |= SGO_CONNECT_D_RAN;
        if (resD == C_CUT) st |= SGO_CONNECT_D_CUT;
        if (resD == C_UNK) st |= SGO_CONNECT_D_UNKNOWN;
        if (item && y == 0) { row[6] = st; row[8] = mvA; row[9] = mvD; row[10] = nodesA; row[11] = nodesD; }
    }
}

// One 32-lane half per listed row.  A chain's label lives on its anchor point in LDS; every lane of the half runs the same
// sequential sweep over the written rows and stores the same values, so no lane depends on another's store and nothing is atomic.
// A sweep takes the min over the two anchors' labels of every `connected` row; sweeps go on to a fixed point, max_pairs at the most
// (a label travels at least one tie per sweep).  Then the chains of either colour are walked by lowest point, one flood each: the
// stones get the label on the anchor, the empty points -1.
// TRIPS: at most max_pairs sweeps of at most max_pairs rows; one trip of the chain walk per chain of the half with more of them.
template <int S>
__global__ __launch_bounds__(64) void k_connect_groups(int n, const uint32_t *records, int n_records, const int32_t *index, int max_pairs,
                                                       const int32_t *n_pairs, const int32_t *rows_out, int16_t *groups, int32_t *group_counts) {
    using G = Geo<S>;
    __shared__ int16_t Lab[2][G::N];
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long i = (long)blockIdx.x * 2 + half;
    const bool valid = i < n;
    const int r = valid ? (index ? index[i] : (int)i) : -1;
    const bool ok = r >= 0 && r < n_records;                         // uniform over the half
    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    const rows::Board<S> bd(half, y);
    const uint32_t rb = rec ? rows::load_row<S>(rec, y) : 0u, rw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
    const int total = ok ? n_pairs[i] : 0, cnt = total < max_pairs ? total : max_pairs;
    const int32_t *ro = rows_out + (size_t)(valid ? i : 0) * max_pairs * C_WORDS;
    int16_t *lab = Lab[half];
    for (int a = y; a < G::N; a += 32) lab[a] = (int16_t)a;
    __syncthreads();
    int flags = total > max_pairs ? 1 : 0, tied = 0;
    for (int k = 0; k < cnt; k++) {
        const int st = ro[k * C_WORDS + 6];
        if (st & (SGO_CONNECT_OPEN | SGO_CONNECT_A_UNKNOWN | SGO_CONNECT_D_UNKNOWN)) flags |= 2;
        if ((st & ~SGO_CONNECT_D_RAN) == 0) tied++;
    }
    bool changed = tied > 0;
    for (int sweep = 0; sweep < max_pairs && __any(changed); sweep++) {
        changed = false;
        for (int k = 0; k < cnt; k++) {
            const int32_t *o = ro + k * C_WORDS;
            if ((o[6] & ~SGO_CONNECT_D_RAN) != 0) continue;          // connected: no bit but (never set here) D_RAN
            const int ax = o[0], ay = o[1];
            if ((unsigned)ax >= (unsigned)G::N || (unsigned)ay >= (unsigned)G::N) continue;
            const int16_t lx = lab[ax], ly = lab[ay], lo = lx < ly ? lx : ly;
            if (lx != lo || ly != lo) { lab[ax] = lo; lab[ay] = lo; changed = true; }
        }
    }
    __syncthreads();
    int16_t *go = groups + (size_t)(valid ? i : 0) * G::N;
    if (ok && y < S) {
        uint32_t e = ~(rb | rw) & bd.M;
        while (e) { const int x = __builtin_ctz(e); e &= e - 1; go[y * S + x] = -1; }
    }
    uint32_t rest = rb | rw;
    int chains = 0, n_groups = 0;
    while (__any(rest != 0)) {
        const int a = lowest_point<S>(rest, half);
        const uint32_t seed = (a >= 0 && y == a / S) ? (1u << (a % S)) : 0u;
        const bool is_b = rows::half_any(seed & rb, half);
        const uint32_t c = bd.flood(seed, a >= 0 ? (is_b ? rb : rw) : 0u);
        rest &= ~c;
        if (a >= 0) {
            const int16_t l = lab[a];
            chains++;
            if (l == a) n_groups++;
            uint32_t v = c;
            while (v) { const int x = __builtin_ctz(v); v &= v - 1; go[y * S + x] = l; }
        }
    }
    if (ok && y == 0) {
        int32_t *c = group_counts + (size_t)i * 4;
        c[0] = chains; c[1] = n_groups; c[2] = tied; c[3] = flags;
    }
}

int launch_connect(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask, const uint32_t *d_region,
                   int rules, int cut_libs, int max_region, int max_nodes, int max_pairs, int32_t *d_n_pairs, int32_t *d_rows, uint32_t *d_regions,
                   int16_t *d_groups, int32_t *d_group_counts, hipStream_t st) {
    SGO_DISPATCH(S, k_connect_pairs<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(n, d_records, n_records, d_index, d_ask, d_region, cut_libs,
                                                                                 max_region, max_pairs, d_n_pairs, d_rows, d_regions));
    SGO_HIP(hipGetLastError());
    SGO_DISPATCH(S, k_connect_read<kS><<<dim3(cdiv(max_pairs, 2), n < 65535 ? n : 65535), dim3(64), 0, st>>>(
                        n, d_records, n_records, d_index, rules, max_nodes, max_pairs, d_n_pairs, d_rows, d_regions));
    SGO_HIP(hipGetLastError());
    SGO_DISPATCH(S, k_connect_groups<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(n, d_records, n_records, d_index, max_pairs, d_n_pairs, d_rows,
                                                                                  d_groups, d_group_counts));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

bool connect_params_ok(int rules, int cut_libs, int max_region, int max_nodes, int max_pairs) {
    return (rules == 0 || rules == 1) && cut_libs >= 0 && cut_libs <= SGO_CONNECT_MAX_CUT_LIBS && max_region >= 1 &&
           max_region <= SGO_CONNECT_MAX_REGION && max_nodes >= 1 && max_nodes <= SGO_CONNECT_MAX_NODES && max_pairs >= 1 &&
           max_pairs <= SGO_CONNECT_MAX_PAIRS;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_connect_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask, const uint32_t *d_region,
                    int rules, int cut_libs, int max_region, int max_nodes, int max_pairs, int32_t *d_n_pairs, int32_t *d_rows,
                    uint32_t *d_regions, int16_t *d_groups, int32_t *d_group_counts, void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || !connect_params_ok(rules, cut_libs, max_region, max_nodes, max_pairs) || !d_records ||
        !d_n_pairs || !d_rows || !d_regions || !d_groups || !d_group_counts) {
        set_error("sgo_connect_dev: bad argument (unsupported size, n < 0, n_records < 0, rules outside {0, 1}, cut_libs outside [0, 4], "
                  "max_region outside [1, 32], max_nodes outside [1, 32768], max_pairs outside [1, 64], a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_connect(S, n, d_records, n_records, d_index, d_ask, d_region, rules, cut_libs, max_region, max_nodes, max_pairs, d_n_pairs,
                          d_rows, d_regions, d_groups, d_group_counts, (hipStream_t)stream);
}

int sgo_connect(int S, int n, const uint32_t *records, const int32_t *ask, const uint32_t *region, int rules, int cut_libs, int max_region,
                int max_nodes, int max_pairs, int32_t *n_pairs, int32_t *rows_out, uint32_t *regions, int16_t *groups, int32_t *group_counts) {
    if (!size_ok(S) || n < 0 || !connect_params_ok(rules, cut_libs, max_region, max_nodes, max_pairs) || !records || !n_pairs || !rows_out ||
        !regions || !groups || !group_counts) {
        set_error("sgo_connect: bad argument (unsupported size, n < 0, rules outside {0, 1}, cut_libs outside [0, 4], max_region outside [1, 32], "
                  "max_nodes outside [1, 32768], max_pairs outside [1, 64], a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const size_t plane = sizeof(uint32_t) * sgo_plane_words(S);
    // the caller's rows and region sets go in, so that unwritten rows come back as they were
    const HostArray a[] = {{(size_t)n * max_pairs * C_WORDS * sizeof(int32_t), rows_out, rows_out},
                           {(size_t)n * max_pairs * plane, regions, regions},
                           {(size_t)n * sizeof(int32_t), nullptr, n_pairs},
                           {ask ? (size_t)n * 2 * sizeof(int32_t) : 0, ask, nullptr},
                           {region ? (size_t)n * plane : 0, region, nullptr},
                           {(size_t)n * S * S * sizeof(int16_t), groups, groups},
                           {(size_t)n * 4 * sizeof(int32_t), group_counts, group_counts}};
    return host_entry("sgo_connect", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_connect(S, n, d_records, n, nullptr, ask ? reinterpret_cast<const int32_t *>(d[3]) : nullptr,
                              region ? reinterpret_cast<const uint32_t *>(d[4]) : nullptr, rules, cut_libs, max_region, max_nodes, max_pairs,
                              reinterpret_cast<int32_t *>(d[2]), reinterpret_cast<int32_t *>(d[0]), reinterpret_cast<uint32_t *>(d[1]),
                              reinterpret_cast<int16_t *>(d[5]), reinterpret_cast<int32_t *>(d[6]), nullptr);
    });
}

}  // extern "C"
