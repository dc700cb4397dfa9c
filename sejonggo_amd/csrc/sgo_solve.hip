// sgo_solve.hip -- a life-and-death reader on the device (include/sgo.h "life and death"): per packed record the table of the
// enclosed chains (or the one chain asked for), the region M each is read in, and for each the verdict of an exhaustive reader
// bounded by M in which BOTH sides play -- the attacker first (query A) and, when that kills, the defender first (query D) -- with
// unconditional life as the terminal for "lives".  A translation unit of its own, like sgo_tactics.hip and sgo_secure.hip:
// tests/test_engine_isa.py pins the kernel set of sgo_engine.hip, and nothing here touches k_search.
//
//   k_solve_targets<S>   per listed record: life_core for both colours, the chain walk by lowest point, the region flood and the
//                        inner-chain rule; n_targets, words 0..3 of the rows (words 4..7 preset to -1, -1, 0, 0), the region sets
//   k_solve_read<S>      per (row, target slot): queries A and D of the header's reader; status bits and words 4..7 of the row
//
// sgo_session_solve runs the same two kernels over the context's records, with the root index k_session_roots (sgo_session.hpp)
// writes.
//
// No rule is restated: the ply is rows::Board<S>::advance, ALLOWED is Board::legal with the `prev` handling of k_tactics_read, the
// "stone would stand" test of rules = 1 is the one of k_moves (play the ply, look for the stone), and the fixed point is life_core
// (sgo_life_core.hpp), which k_life and k_secure run too.
//
// Kernel form: one 32-lane HALF of a wavefront per item, one board row per lane (sgo_rows.hpp), one wavefront per workgroup.  The
// floods vote over the whole wave, so both halves run every loop in lockstep: a half that is done, idle or out of range goes on with
// an EMPTY board (its floods end at once) and only its stores differ.  No flood, advance, life_core call or shuffle sits under a
// per-item branch; the branches around them (`rules`, "some half entered a node") are the wave's.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_life_core.hpp"
#include "sgo_rows.hpp"

namespace sgo {

// TRIPS: two life_core calls (sgo_life_core.hpp has their bound), one flood for an asked chain, and the chain loop: one trip per
// chain of the half with more of them, at most N (every trip clears at least the seed from `rest`), with five floods a trip.
// Termination does not depend on the data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_solve_targets(int n, const uint32_t *records, int n_records, const int32_t *index, const int32_t *ask,
                                                      const uint32_t *region, int max_region, int max_targets, int32_t *n_targets,
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
    const int a = (ok && ask) ? ask[i] : -1;
    const bool enumerate = a < 0;
    const bool given = !enumerate && region != nullptr;              // the caller's M, masked to the board by load_row
    const uint32_t given_m = given ? rows::load_row<S>(region + (size_t)i * G::NW, y) : 0u;

    uint32_t alive_b, alive_w, terr;
    life_core<S>(bd, half, y, rb, rw, ok, alive_b, terr);
    life_core<S>(bd, half, y, rw, rb, ok, alive_w, terr);
    const uint32_t alive = alive_b | alive_w;

    // an asked row walks the one chain on the asked point; an enumerated row every chain
    const uint32_t askbit = (!enumerate && a < G::N && y == a / S) ? (1u << (a % S)) : 0u;
    const bool ask_b = rows::half_any(askbit & rb, half), ask_w = rows::half_any(askbit & rw, half);
    const uint32_t askchain = bd.flood(askbit & (ask_b ? rb : rw), ask_b ? rb : rw);
    uint32_t rest = enumerate ? (rb | rw) : askchain;

    int count = 0;
    int32_t *ro = valid ? rows_out + (size_t)i * max_targets * 8 : nullptr;
    uint32_t *go = valid ? regions + (size_t)i * max_targets * G::NW : nullptr;
    while (__any(rest != 0)) {
        const int anchor = lowest_point<S>(rest, half);
        const uint32_t seed = (anchor >= 0 && y == anchor / S) ? (1u << (anchor % S)) : 0u;
        const bool is_b = rows::half_any(seed & rb, half);
        const uint32_t X = is_b ? rb : rw, O = is_b ? rw : rb;
        const uint32_t g = bd.flood(seed, X);
        const uint32_t R = bd.flood(g, ~O & bd.M);                   // life's region of O around the chain
        // the O chains with a liberty, and every liberty in R
        const uint32_t out = bd.flood(O & bd.nbr4(emp & ~R), O), in = bd.flood(O & bd.nbr4(emp & R), O);
        const uint32_t m = given ? given_m : (R | (in & ~out));
        const int re = half_sum(__popc(m & emp));
        const bool is_alive = rows::half_any(g & alive, half);
        const bool open = re < 1 || re > max_region;
        const uint32_t wm = rows::gather_word<S>(m, half, y);
        if (anchor >= 0 && (enumerate ? (!is_alive && !open) : true)) {
            if (count < max_targets) {
                if (y == 0) {
                    int32_t *o = ro + (size_t)count * 8;
                    o[0] = anchor; o[1] = is_b ? 1 : -1; o[2] = re; o[3] = open ? SGO_SOLVE_OPEN : 0;
                    o[4] = -1; o[5] = -1; o[6] = 0; o[7] = 0;
                }
                if (y < G::NW) go[(size_t)count * G::NW + y] = wm;
            }
            count++;
        }
        rest &= ~g;
    }
    if (ok && !enumerate && !ask_b && !ask_w) {                      // an asked point without a stone
        if (y == 0) {
            ro[0] = -1; ro[1] = 0; ro[2] = 0; ro[3] = SGO_SOLVE_NO_STONE;
            ro[4] = -1; ro[5] = -1; ro[6] = 0; ro[7] = 0;
        }
        if (y < G::NW) go[y] = 0u;
        count = 1;
    }
    if (valid && y == 0) n_targets[i] = count;
}

enum { V_NONE = 0, V_DEAD = 1, V_ALIVE = 2, V_UNK = 3 };
constexpr int V_FRAMES = SGO_SOLVE_MAX_DEPTH + 1;                    // depths 0 .. MAX_DEPTH hold a frame
constexpr int V_ENTER = -2;                                          // a cursor: the node has not been entered (no life test yet)

// One half-wavefront per (row, target slot): the iterative depth-first search of k_tactics_read.  A frame is the position of a node
// BEFORE its move (own = the node's mover, opp), 256 bytes per half and frame, plus the candidate cursor (every lane of the half
// writes the same value): 2 * 81 * 260 bytes = 42 KB of static LDS per workgroup.  The cursor is V_ENTER for a frame just pushed,
// then -1, then the last candidate tried, and N once the defender's pass (or the attacker's wait, which exists only while the ko test
// forbids it an empty point of M) has been tried: that is how a frame knows that its cursor has reached the pass.  The ko `prev`
// of a node is its parent frame's opp rows; after a pass or a wait those are the node's own rows, so nothing is forbidden.  One trip of the loop is one node step: what the top frame's child returned is taken in; a frame entered in
// this trip gets its life test (life_core on the defender's colour, once per node; the wave skips the call when neither half
// entered a node); the candidates above the cursor are found; the next one is played and judged; the frame returns, a child frame
// is pushed, or the cursor has moved on.
// CANDIDATES: rules = 0 takes the empty points of M in Board::legal.  rules = 1 takes the empty points of M that are not the ko
// point and finds out by the ply whether the stone stands (a candidate whose stone is gone costs one trip and is passed over): the
// header's set, since every point of Board::legal is no ko point and keeps its stone.
// TRIPS: every trip pushes a frame (at most max_nodes per query), pops one (no more pops than pushes, plus the root) or moves a
// cursor up (at most N + 1 times per frame: N points and the pass), so a launch takes at most 2 * (max_nodes + 1) * (N + 3) trips
// per item; a trip is at most one life_core call, one Board::legal and one advance, each bounded on its own.  Termination does not
// depend on the data beyond that.
template <int S>
__global__ __launch_bounds__(64) void k_solve_read(int n, const uint32_t *records, int n_records, const int32_t *index, int rules, int max_nodes,
                                                   int max_targets, const int32_t *n_targets, int32_t *rows_out, const uint32_t *regions) {
    using G = Geo<S>;
    __shared__ uint32_t F[2][V_FRAMES][2][32];
    __shared__ int32_t Cs[2][V_FRAMES];
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const int j = blockIdx.x * 2 + half;                             // target slot
    const rows::Board<S> bd(half, y);
    for (int i = blockIdx.y; i < n; i += gridDim.y) {                // the trip count is the workgroup's
        const int r = index ? index[i] : i;
        const bool ok = r >= 0 && r < n_records;
        const int cnt = ok ? n_targets[i] : 0;
        const bool listed = j < max_targets && j < cnt;
        int32_t *row = rows_out + ((size_t)i * max_targets + (listed ? j : 0)) * 8;
        const bool item = listed && row[3] == 0;                     // uniform over the half; open and stone-less rows are not read
        if (!__any(item)) continue;
        const uint32_t *rec = item ? records + (size_t)r * G::RW : nullptr;
        const uint32_t black = rec ? rows::load_row<S>(rec, y) : 0u, white = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
        const uint32_t pblack = rec ? rows::load_row<S>(rec + 2 * G::NW, y) : 0u, pwhite = rec ? rows::load_row<S>(rec + 3 * G::NW, y) : 0u;
        const bool stm_white = rec ? (rec[G::META_WORD] & G::META_BIT) != 0 : false;
        const uint32_t m = item ? rows::load_row<S>(regions + ((size_t)i * max_targets + j) * G::NW, y) : 0u;
        const int t = item ? row[0] : 0;
        const bool def_white = item ? row[1] < 0 : false;
        const uint32_t tb = (item && y == t / S) ? (1u << (t % S)) : 0u;

        bool done = !item, root_atk = true;
        int q = 0;                                                   // 0: query A, 1: query D
        int d = 0, nodes = 1, ret = V_NONE;
        int resA = V_NONE, resD = V_NONE, mvA = -1, mvD = -1, nodesA = 0, nodesD = 0;
        uint32_t rootprev;
        {   // root of query A: the attacker moves
            const bool mw = !def_white;
            F[half][0][0][y] = mw ? white : black;
            F[half][0][1][y] = mw ? black : white;
            rootprev = (mw == stm_white) ? (mw ? pwhite : pblack) : (mw ? white : black);
            Cs[half][0] = V_ENTER;
        }
        do {
            const bool run = !done;
            const bool atk = ((d & 1) != 0) != root_atk;             // the top frame's mover is the attacker
            int cur = Cs[half][d];
            bool popnow = false;
            if (run && ret != V_NONE) {                              // what the child of the last candidate returned
                if (atk ? ret == V_DEAD : ret == V_ALIVE) popnow = true;
                else ret = V_NONE;
            }
            const bool work = run && !popnow;
            const bool fresh = work && cur == V_ENTER;
            if (cur == V_ENTER) cur = -1;
            const uint32_t own = work ? F[half][d][0][y] : 0u, opp = work ? F[half][d][1][y] : 0u;
            const uint32_t prev = work ? (d > 0 ? F[half][d - 1][1][y] : rootprev) : 0u;
            const uint32_t dst = atk ? opp : own, ast = atk ? own : opp;
            const uint32_t emp = ~(own | opp) & bd.M;
            // the life test of a node entered in this trip
            uint32_t alive = 0u, terr = 0u;
            if (__any(fresh)) life_core<S>(bd, half, y, fresh ? dst : 0u, fresh ? ast : 0u, fresh, alive, terr);
            const bool is_alive = fresh && rows::half_any(alive & tb, half);
            // the candidates, and those above the cursor
            const uint32_t gone = prev & ~own;
            const uint32_t ko = rows::half_one_bit(gone, half) ? gone : 0u;
            const bool banned = rows::half_any(ko & emp & m, half);  // the ko test forbids the mover an empty point of M
            uint32_t cand = rules ? (emp & ~ko) : bd.legal(own, opp, prev);
            cand &= m;
            const int cy = cur < 0 ? -1 : cur / S, cx = cur < 0 ? 0 : cur % S;
            const uint32_t rem = cur >= G::N ? 0u : ((y > cy) ? cand : ((y == cy) ? (cand & ~((2u << cx) - 1u)) : 0u));
            const int next = lowest_point<S>(rem, half);
            int res = V_NONE, a = G::N;
            bool play = false, pass = false;
            if (work) {
                if (is_alive) res = V_ALIVE;
                else if (next >= 0) { a = next; play = true; }
                else if (cur < G::N && (!atk || banned)) pass = true;   // the defender's pass, the attacker's wait: the last candidate
                else res = atk ? V_ALIVE : V_DEAD;
            }
            if (play || pass) Cs[half][d] = a;
            // the ply (a pass where nothing is played: no stone, no flood).  Every candidate comes from `emp`, so advance never
            // takes its early return for an occupied point, which would be a per-half branch.
            const int mv = play ? a : G::N;
            const uint32_t pb = (play && y == mv / S) ? (1u << (mv % S)) : 0u;
            uint32_t o2 = own, p2 = opp;
            (void)bd.advance(o2, p2, mv);
            const uint32_t d2 = atk ? p2 : o2;
            const bool tgone = !rows::half_any(d2 & tb, half);
            const bool sgone = !rows::half_any(o2 & pb, half);
            bool push = pass;
            if (play) {
                if (atk && tgone) res = V_DEAD;
                else if (!tgone && !sgone) push = true;              // else: the next candidate
            }
            bool finished = false;
            if (push) {
                nodes++;
                if (nodes > max_nodes || d + 1 > SGO_SOLVE_MAX_DEPTH) { ret = V_UNK; finished = true; }
                else {
                    d++;
                    F[half][d][0][y] = p2;
                    F[half][d][1][y] = o2;
                    Cs[half][d] = V_ENTER;
                    ret = V_NONE;
                }
            } else if (run && (popnow || res != V_NONE)) {           // the top frame returns
                if (!popnow) ret = res;
                if (d == 0) finished = true;
                else d--;
            }
            if (finished) {                                          // the query is over: ret, and the root's cursor
                const int c0 = Cs[half][0], m0 = c0 < 0 ? -1 : c0;
                if (q == 0) {
                    resA = ret;
                    mvA = ret == V_DEAD ? m0 : -1;
                    nodesA = nodes;
                    if (ret == V_DEAD) {                             // query D: the defender moves first
                        q = 1;
                        root_atk = false;
                        d = 0; nodes = 1; ret = V_NONE;
                        const bool mw = def_white;
                        F[half][0][0][y] = mw ? white : black;
                        F[half][0][1][y] = mw ? black : white;
                        rootprev = (mw == stm_white) ? (mw ? pwhite : pblack) : (mw ? white : black);
                        Cs[half][0] = V_ENTER;
                    } else done = true;
                } else {
                    resD = ret;
                    mvD = ret == V_ALIVE ? m0 : -1;
                    nodesD = nodes;
                    done = true;
                }
            }
        } while (__any(!done));
        if (item && y == 0) {
            int st = 0;
            if (resA == V_DEAD) st |= SGO_SOLVE_A_DEAD;
            if (resA == V_UNK) st |= SGO_SOLVE_A_UNKNOWN;
            if (q == 1) st |= SGO_SOLVE_D_RAN;
            if (resD == V_DEAD) st |= SGO_SOLVE_D_DEAD;
            if (resD == V_UNK) st |= SGO_SOLVE_D_UNKNOWN;
            row[3] = st; row[4] = mvA; row[5] = mvD; row[6] = nodesA; row[7] = nodesD;
        }
    }
}

int launch_solve(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask, const uint32_t *d_region,
                 int rules, int max_region, int max_nodes, int max_targets, int32_t *d_n_targets, int32_t *d_rows, uint32_t *d_regions,
                 hipStream_t st) {
    SGO_DISPATCH(S, k_solve_targets<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(n, d_records, n_records, d_index, d_ask, d_region, max_region,
                                                                                 max_targets, d_n_targets, d_rows, d_regions));
    SGO_HIP(hipGetLastError());
    SGO_DISPATCH(S, k_solve_read<kS><<<dim3(cdiv(max_targets, 2), n < 65535 ? n : 65535), dim3(64), 0, st>>>(
                        n, d_records, n_records, d_index, rules, max_nodes, max_targets, d_n_targets, d_rows, d_regions));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

bool solve_params_ok(int rules, int max_region, int max_nodes, int max_targets) {
    return (rules == 0 || rules == 1) && max_region >= 1 && max_region <= SGO_SOLVE_MAX_REGION && max_nodes >= 1 &&
           max_nodes <= SGO_SOLVE_MAX_NODES && max_targets >= 1 && max_targets <= SGO_SOLVE_MAX_TARGETS;
}

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_solve_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask, const uint32_t *d_region,
                  int rules, int max_region, int max_nodes, int max_targets, int32_t *d_n_targets, int32_t *d_rows, uint32_t *d_regions,
                  void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || !solve_params_ok(rules, max_region, max_nodes, max_targets) || !d_records || !d_n_targets ||
        !d_rows || !d_regions) {
        set_error("sgo_solve_dev: bad argument (unsupported size, n < 0, n_records < 0, rules outside {0, 1}, max_region outside [1, 32], "
                  "max_nodes outside [1, 65536], max_targets outside [1, 64], a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_solve(S, n, d_records, n_records, d_index, d_ask, d_region, rules, max_region, max_nodes, max_targets, d_n_targets, d_rows,
                        d_regions, (hipStream_t)stream);
}

int sgo_solve(int S, int n, const uint32_t *records, const int32_t *ask, const uint32_t *region, int rules, int max_region, int max_nodes,
              int max_targets, int32_t *n_targets, int32_t *rows_out, uint32_t *regions) {
    if (!size_ok(S) || n < 0 || !solve_params_ok(rules, max_region, max_nodes, max_targets) || !records || !n_targets || !rows_out || !regions) {
        set_error("sgo_solve: bad argument (unsupported size, n < 0, rules outside {0, 1}, max_region outside [1, 32], max_nodes outside "
                  "[1, 65536], max_targets outside [1, 64], a NULL record array or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const size_t plane = sizeof(uint32_t) * sgo_plane_words(S);
    // the caller's rows and region sets go in, so that unwritten rows come back as they were
    const HostArray a[] = {{(size_t)n * max_targets * 8 * sizeof(int32_t), rows_out, rows_out},
                           {(size_t)n * max_targets * plane, regions, regions},
                           {(size_t)n * sizeof(int32_t), nullptr, n_targets},
                           {ask ? (size_t)n * sizeof(int32_t) : 0, ask, nullptr},
                           {region ? (size_t)n * plane : 0, region, nullptr}};
    return host_entry("sgo_solve", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_solve(S, n, d_records, n, nullptr, ask ? reinterpret_cast<const int32_t *>(d[3]) : nullptr,
                            region ? reinterpret_cast<const uint32_t *>(d[4]) : nullptr, rules, max_region, max_nodes, max_targets,
                            reinterpret_cast<int32_t *>(d[2]), reinterpret_cast<int32_t *>(d[0]), reinterpret_cast<uint32_t *>(d[1]), nullptr);
    });
}

}  // extern "C"
