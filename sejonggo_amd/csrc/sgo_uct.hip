// sgo_uct.hip -- playout tree search on the device (include/sgo.h "playout tree search"): per listed record `trees` independent
// Monte-Carlo tree searches of `sims` simulations each -- selection by a RAVE-blended value, expansion, a light playout below the tree,
// back-propagation of the result and of the all-moves-as-first credit -- each search played from first to last inside ONE kernel, with
// no net and no host loop.  A translation unit of its own: tests/test_playout_isa.py pins the kernel set of sgo_playout.hip.
//
//   k_uct_zero          zeroes the outputs of the n rows (the searching kernel adds into them)
//   k_uct<S>            runs the trees and adds what they found, one round of integer atomics per tree
//   k_uct_best          writes info[3] = best of every row from the summed root tables
//
// Kernel form: the form of k_playout.  One 32-lane HALF of a wavefront per tree, one board row per lane (sgo_rows.hpp), one wavefront
// per workgroup, two trees side by side.  The game of the running simulation lives in registers: both colours' rows, the ko row
// `prev`, the two first-play sets Fb / Fw, the ply and pass counters; across the simulations of a tree the ownership counts and the
// eight sums accumulate in registers as well.  Nothing of the rules is restated: the candidates and the pick are those of the light
// playouts (sgo_playout_core.hpp), the ply Board::advance, the score area_owners, the draw draw32 (sgo_draw.hpp).
// LOCKSTEP: both halves run ONE ply loop.  A half is either in its tree or below it, and only how the ply's move is chosen differs:
// in the tree an argmax over the node's child tables (lane y evaluates the children of row y, lane S the pass; one 64-bit key
// v << 41 | h << 9 | (511 - a) per child, a max-reduction over the half), below it the playouts' pick; `cand` is computed once per
// ply for both.  The selection sits under a wave-uniform __any(in tree), the scoring and the back-propagation under a wave-uniform
// __any(ended); the back-propagation loop runs to the larger D of the two halves with a per-half predicate.  Nothing cross-lane sits
// under a per-half branch: such branches hold loads, stores and lane-local arithmetic only.
// MEMORY: the PATH (node and move of every tree ply, SGO_UCT_MAX_DEPTH entries per half) is in LDS; every lane of the half writes the
// same word and reads it back itself.  The NODE TABLES are in d_work, per tree max_nodes nodes of UctNode<S>::WORDS words:
// nw [N + 1] (n | w << 16), rr [N + 1] (rn | rw << 16), cs [S] (the child set, one row per lane), link [N + 1] (16 bits each, 0 =
// none).  16-bit counters fit because sims <= 4096.  Point a = y * S + x belongs to lane y and the pass (a = N) to lane S, and a lane
// reads and writes only what belongs to it, so the tables need no fence: a node is zeroed by its lanes when it is created, its child
// set is stored by the selection that visits it, and the back-propagation reads both back in the lane that wrote them.  The link of
// the chosen child and its n are read by the owning lane and handed to the half with one shuffle.
// TRIPS: one trip of the ply loop is one ply of every live half and a simulation ends at ply == max_plies at the latest, so a tree
// takes at most sims * max_plies trips; the selection visits at most S children per lane; the back-propagation at most
// SGO_UCT_MAX_DEPTH steps; the stride loop ceil(n * trees / (2 * grid)) trips.  Termination does not depend on the data beyond that.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_draw.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_playout_core.hpp"
#include "sgo_rows.hpp"

namespace sgo {

constexpr int UCT_MAX_BLOCKS = 1 << 15;         // two trees per workgroup and trip

template <int S>
struct UctNode {
    static constexpr int N1 = S * S + 1;
    static constexpr int NW = 0, RR = N1, CS = 2 * N1, LINK = 2 * N1 + S;      // word offsets; link holds 16-bit entries
    static constexpr int WORDS = 2 * N1 + S + (N1 + 1) / 2;
};
static size_t uct_node_words(int S) { return (size_t)(2 * (S * S + 1) + S + (S * S + 2) / 2); }

struct UctOut {
    int32_t *visits, *wins2, *rave, *own;
    unsigned long long *sums;
    int32_t *info, *trace;
};

__global__ __launch_bounds__(256) void k_uct_zero(long n, int N, long n_trace, UctOut o) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long n_tab = n * (N + 1), n_own = n * 2 * N, big = 2 * n_tab > n_trace ? 2 * n_tab : n_trace;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < big; t += stride) {
        if (t < n_tab) { o.visits[t] = 0; o.wins2[t] = 0; }
        if (o.rave && t < 2 * n_tab) o.rave[t] = 0;
        if (o.own && t < n_own) o.own[t] = 0;
        if (t < n * 8) o.sums[t] = 0ull;
        if (t < n * 4) o.info[t] = 0;
        if (o.trace && t < n_trace) o.trace[t] = 0;
    }
}

// the value of one child as the key the selection maximises: v, then the hash, then the lower point
SGO_DEV unsigned long long uct_key(uint32_t a, uint32_t nw, uint32_t rr, uint32_t P, uint32_t E, uint32_t rdraw) {
    const uint32_t n = nw & 0xffffu, w = nw >> 16;
    const uint32_t rn = (rr & 0xffffu) + P, rw = (rr >> 16) + P;
    const uint32_t rq = (E && rn) ? (rw << 16) / rn : 65536u;
    const uint32_t q = n ? (w << 16) / n : rq;
    const uint32_t beta = n == 0 ? 65536u : ((E && rn) ? (rn << 16) / (rn + n + rn * n / E) : 0u);
    const unsigned long long v = ((unsigned long long)beta * rq + (unsigned long long)(65536u - beta) * q) >> 16;
    return (v << 41) | ((unsigned long long)mix32(rdraw + a) << 9) | (unsigned long long)(511u - a);
}

template <int S>
__global__ __launch_bounds__(64) void k_uct(int n, const uint32_t *records, int n_records, const int32_t *index, int trees, int sims, uint32_t seed,
                                            int rules, int max_plies, int komi2, int expand_at, uint32_t E, uint32_t P, int max_nodes, UctOut o,
                                            uint32_t *work) {
    using G = Geo<S>;
    using ND = UctNode<S>;
    __shared__ uint32_t path[2][SGO_UCT_MAX_DEPTH];                  // node | a << 16 of every tree ply
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const rows::Board<S> bd(half, y);
    const PlayoutCore<S> core(bd);
    const long n_units = (long)n * trees;
    const int own_n = (y < S) ? S : (y == S ? 1 : 0);                // the table entries of this lane: row y, or the pass

    for (long u0 = (long)blockIdx.x * 2; u0 < n_units; u0 += (long)gridDim.x * 2) {    // the trip count is the workgroup's
        const long u = u0 + half;
        const bool valid = u < n_units;
        const int i = valid ? (int)(u / trees) : 0;
        const int r = valid ? (index ? index[i] : i) : -1;
        const bool ok = r >= 0 && r < n_records;                     // uniform over the half
        const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
        const uint32_t sb = rec ? rows::load_row<S>(rec, y) : 0u, sw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
        const bool start_white = rec ? ((rec[G::META_WORD] & G::META_BIT) != 0) : false;
        const uint32_t sprev = rec ? rows::load_row<S>(rec + (start_white ? 3 : 2) * G::NW, y) : 0u;
        const uint32_t gs0 = (uint32_t)u * (uint32_t)sims;
        const bool weird = playout_weird<S>(bd, sb, sw);
        uint32_t *tree = work + (size_t)(valid ? u : 0) * max_nodes * ND::WORDS;
        uint16_t *tlink = reinterpret_cast<uint16_t *>(tree + ND::LINK);   // of node 0; a node further on is ND::WORDS words further

        if (ok)                                                      // the root
            for (int x = 0; x < own_n; x++) { tree[ND::NW + y * S + x] = 0u; tree[ND::RR + y * S + x] = 0u; tlink[y * S + x] = 0; }

        int bacc[S], wacc[S];
#pragma unroll
        for (int x = 0; x < S; x++) { bacc[x] = 0; wacc[x] = 0; }
        int s_bw = 0, s_ww = 0, s_dr = 0, s_sc = 0, s_sq = 0, s_pl = 0, s_cap = 0, s_n = 0;
        int nodes = 1, deepest = 0, refused = 0;

        bool active = ok, mover_white = start_white, in_tree = true;
        uint32_t own = active ? (start_white ? sw : sb) : 0u, opp = active ? (start_white ? sb : sw) : 0u, prev = active ? sprev : 0u;
        uint32_t Fb = 0u, Fw = 0u;
        int s = 0, ply = 0, passes = 0, node = 0, D = 0, a0 = 0;

        for (int trip = 0; trip < sims * max_plies; trip++) {
            if (!__any(active)) break;
            const uint32_t cand = core.cand(own, opp, prev, rules, weird);
            const uint32_t rdraw = draw32(seed, gs0 + (uint32_t)s, (uint32_t)ply);
            uint32_t k;
            const int a_pick = core.pick(cand, rdraw, k);

            const bool tsel = active && in_tree;                     // uniform over the half
            uint32_t *nd = tree + (size_t)node * ND::WORDS;
            int a_tree = G::N;
            uint32_t child = 0u;                                     // of the chosen child: n | link << 16
            if (__any(tsel)) {                                       // uniform over the wave: the reduction and the shuffle vote over it
                uint32_t cset = (y < S) ? (k ? cand : 0u) : ((y == S && k == 0) ? 1u : 0u);
                unsigned long long key = 0ull;
                if (tsel) {
                    if (y < S) nd[ND::CS + y] = cset;
                    while (cset) {
                        const int x = __builtin_ctz(cset);
                        cset &= cset - 1u;
                        const unsigned long long kk = uct_key((uint32_t)(y * S + x), nd[ND::NW + y * S + x], nd[ND::RR + y * S + x], P, E, rdraw);
                        key = kk > key ? kk : key;
                    }
                }
#pragma unroll
                for (int ofs = 16; ofs > 0; ofs >>= 1) {
                    const unsigned long long other = __shfl_xor(key, ofs, 32);
                    key = other > key ? other : key;
                }
                a_tree = (tsel && key) ? 511 - (int)(key & 511ull) : G::N;   // a node always has a child: key != 0
                const int ow = a_tree / S;
                if (tsel && y == ow)
                    child = (nd[ND::NW + a_tree] & 0xffffu) | ((uint32_t)reinterpret_cast<uint16_t *>(nd + ND::LINK)[a_tree] << 16);
                child = (uint32_t)__shfl((int)child, ow, 32);
            }
            const int a = !active ? G::N : (in_tree ? a_tree : (k != 0 ? a_pick : G::N));

            const uint32_t before_opp = opp;
            (void)bd.advance(own, opp, a);                           // a candidate is never occupied: no early return
            const uint32_t pb = (a < G::N && y == a / S) ? (1u << (a % S)) : 0u;
            if (active && !in_tree) {                                // below the tree: who played the point first since ply D
                const uint32_t fresh = pb & ~(Fb | Fw);
                if (mover_white) Fw |= fresh; else Fb |= fresh;
            }
            {   // the other colour moves next; its stones one ply ago are its row before this ply
                const uint32_t t2 = own;
                own = opp; opp = t2; prev = before_opp;
                mover_white = !mover_white;
            }
            passes = (a == G::N) ? passes + 1 : 0;
            const bool ended = active && (passes >= 2 || ply + 1 >= max_plies);
            if (tsel) {
                path[half][ply] = (uint32_t)node | ((uint32_t)a << 16);    // ply < SGO_UCT_MAX_DEPTH: no node lies deeper
                if (ply == 0) a0 = a;
                const int link = (int)(child >> 16);
                if (link) {
                    node = link;
                } else {
                    D = ply + 1;
                    in_tree = false;
                    if ((int)(child & 0xffffu) >= expand_at && D < SGO_UCT_MAX_DEPTH && !ended) {
                        if (nodes < max_nodes) {
                            uint32_t *nn = tree + (size_t)nodes * ND::WORDS;
                            uint16_t *nl = reinterpret_cast<uint16_t *>(nn + ND::LINK);
                            for (int x = 0; x < own_n; x++) { nn[ND::NW + y * S + x] = 0u; nn[ND::RR + y * S + x] = 0u; nl[y * S + x] = 0; }
                            if (y == a / S) reinterpret_cast<uint16_t *>(nd + ND::LINK)[a] = (uint16_t)nodes;
                            nodes++;
                        } else {
                            refused = 1;
                        }
                    }
                }
            }
            ply++;

            if (__any(ended)) {                                      // uniform over the wave: the fills below vote over it
                const uint32_t nb = ended ? (mover_white ? opp : own) : 0u, nw = ended ? (mover_white ? own : opp) : 0u;
                uint32_t bo, wo;
                area_owners<S>(bd, nb, nw, bo, wo);
                const int diff = half_sum(__popc(bo)) - half_sum(__popc(wo));
                const int res2 = 2 * diff > komi2 ? 2 : (2 * diff == komi2 ? 1 : 0);     // from black's view
                const int Dmine = ended ? D : 0, Dother = __shfl(Dmine, (int)(threadIdx.x ^ 32u), 64);
                for (int d = (Dmine > Dother ? Dmine : Dother) - 1; d >= 0; d--) {
                    if (ended && d < D) {                            // per half: loads, stores and lane-local arithmetic only
                        const uint32_t e = path[half][d];
                        const int pa = (int)(e >> 16);
                        uint32_t *pn = tree + (size_t)(e & 0xffffu) * ND::WORDS;
                        const bool c_white = start_white != ((d & 1) != 0);
                        const uint32_t add = 1u | ((uint32_t)(c_white ? 2 - res2 : res2) << 16);
                        const uint32_t ppb = (pa < G::N && y == pa / S) ? (1u << (pa % S)) : 0u;
                        if (c_white) { Fw |= ppb; Fb &= ~ppb; } else { Fb |= ppb; Fw &= ~ppb; }
                        if (y == pa / S) pn[ND::NW + pa] += add;
                        uint32_t m = (y < S) ? ((c_white ? Fw : Fb) & pn[ND::CS + y]) : 0u;
                        while (m) {
                            const int x = __builtin_ctz(m);
                            m &= m - 1u;
                            pn[ND::RR + y * S + x] += add;
                        }
                    }
                }
                if (ended) {
#pragma unroll
                    for (int x = 0; x < S; x++) {
                        bacc[x] += (int)((bo >> x) & 1u);
                        wacc[x] += (int)((wo >> x) & 1u);
                    }
                    s_bw += diff > 0; s_ww += diff < 0; s_dr += diff == 0;
                    s_sc += diff; s_sq += diff * diff; s_pl += ply; s_cap += passes < 2; s_n++;
                    if (o.trace && y == 0)
                        o.trace[(size_t)u * sims + s] = a0 | (D << 9) | (res2 << 16) | ((passes < 2 ? 1 : 0) << 18);
                    deepest = D > deepest ? D : deepest;
                    s++;
                    active = s < sims;                               // the next simulation of the tree, or an empty board
                    mover_white = start_white; in_tree = true;
                    own = active ? (start_white ? sw : sb) : 0u;
                    opp = active ? (start_white ? sb : sw) : 0u;
                    prev = active ? sprev : 0u;
                    Fb = 0u; Fw = 0u; ply = 0; passes = 0; node = 0; D = 0;
                }
            }
        }

        if (ok) {
            const size_t t1 = (size_t)i * ND::N1;
            for (int x = 0; x < own_n; x++) {
                const int a = y * S + x;
                const uint32_t nw = tree[ND::NW + a], rr = tree[ND::RR + a];
                if (nw) { atomicAdd(o.visits + t1 + a, (int)(nw & 0xffffu)); atomicAdd(o.wins2 + t1 + a, (int)(nw >> 16)); }
                if (o.rave && rr) { atomicAdd(o.rave + 2 * t1 + a, (int)(rr & 0xffffu)); atomicAdd(o.rave + 2 * t1 + ND::N1 + a, (int)(rr >> 16)); }
            }
            if (o.own && y < S) {
                int32_t *ob = o.own + (size_t)i * 2 * G::N + y * S;
#pragma unroll
                for (int x = 0; x < S; x++) {
                    if (bacc[x]) atomicAdd(ob + x, bacc[x]);
                    if (wacc[x]) atomicAdd(ob + G::N + x, wacc[x]);
                }
            }
            if (y == 0) {
                unsigned long long *sm = o.sums + (size_t)i * 8;
                const int v[8] = {s_bw, s_ww, s_dr, s_sc, s_sq, s_pl, s_cap, s_n};
#pragma unroll
                for (int q = 0; q < 8; q++)
                    if (v[q]) atomicAdd(sm + q, (unsigned long long)(long long)v[q]);   // two's complement: read back as int64
                atomicAdd(o.info + (size_t)i * 4, nodes);
                atomicMax(o.info + (size_t)i * 4 + 1, deepest);
                if (refused) atomicAdd(o.info + (size_t)i * 4 + 2, 1);
            }
        }
    }
}

// best: the largest visits, then the larger wins2, then the lower point; -1 for a row without a visit (a record out of range)
__global__ __launch_bounds__(256) void k_uct_best(int n, int N, const int32_t *visits, const int32_t *wins2, int32_t *info) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t *v = visits + (size_t)i * (N + 1), *w = wins2 + (size_t)i * (N + 1);
    int best = -1, bv = 0, bw = 0;
    for (int a = 0; a <= N; a++)
        if (v[a] > bv || (v[a] == bv && bv > 0 && w[a] > bw)) { best = a; bv = v[a]; bw = w[a]; }
    info[(size_t)i * 4 + 3] = best;
}

bool uct_params_ok(int S, int n, int trees, int sims, int rules, int max_plies, int komi2, int expand_at, int rave_equiv, int prior, int max_nodes) {
    return size_ok(S) && n >= 0 && trees >= 1 && trees <= SGO_UCT_MAX_TREES && sims >= 1 && sims <= SGO_UCT_MAX_SIMS && (rules == 0 || rules == 1) &&
           max_plies <= 4 * S * S && komi2 >= -4 * S * S && komi2 <= 4 * S * S && expand_at >= 0 && expand_at <= sims && rave_equiv >= 0 &&
           rave_equiv <= (1 << 20) && prior >= 0 && prior <= 1024 && max_nodes >= 1 && max_nodes <= sims + 1 &&
           (long)n * trees * sims <= 0x7fffffffL;
}

size_t uct_work_bytes(int S, int n, int trees, int max_nodes) { return (size_t)n * trees * max_nodes * uct_node_words(S) * sizeof(uint32_t); }

int launch_uct(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int trees, int sims, uint32_t seed, int rules,
               int max_plies, int komi2, int expand_at, int rave_equiv, int prior, int max_nodes, int32_t *d_visits, int32_t *d_wins2, int32_t *d_rave,
               int32_t *d_own, int64_t *d_sums, int32_t *d_info, int32_t *d_trace, void *d_work, hipStream_t st) {
    const int N = S * S;
    const long n_units = (long)n * trees, wg = (n_units + 1) / 2, n_trace = d_trace ? n_units * sims : 0;
    const long big = 2L * n * (N + 1) > n_trace ? 2L * n * (N + 1) : n_trace;
    const UctOut o = {d_visits, d_wins2, d_rave, d_own, reinterpret_cast<unsigned long long *>(d_sums), d_info, d_trace};
    k_uct_zero<<<dim3(cdiv(big, 256) < 4096 ? cdiv(big, 256) : 4096), dim3(256), 0, st>>>((long)n, N, n_trace, o);
    SGO_HIP(hipGetLastError());
    const int blocks = wg < UCT_MAX_BLOCKS ? (int)wg : UCT_MAX_BLOCKS;
    const int plies = max_plies > 0 ? max_plies : 3 * N;
    SGO_DISPATCH(S, k_uct<kS><<<dim3(blocks), dim3(64), 0, st>>>(n, d_records, n_records, d_index, trees, sims, seed, rules, plies, komi2, expand_at,
                                                                   (uint32_t)rave_equiv, (uint32_t)prior, max_nodes, o,
                                                                   reinterpret_cast<uint32_t *>(d_work)));
    SGO_HIP(hipGetLastError());
    k_uct_best<<<dim3(cdiv(n, 256)), dim3(256), 0, st>>>(n, N, d_visits, d_wins2, d_info);
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

static const char *const UCT_BOUNDS =
    ": bad argument (unsupported size, n < 0, n_records < 0, trees outside [1, SGO_UCT_MAX_TREES], sims outside [1, SGO_UCT_MAX_SIMS], "
    "n * trees * sims beyond int32, rules outside {0, 1}, max_plies above 4 * S * S, |komi2| above 4 * S * S, expand_at outside [0, sims], "
    "rave_equiv outside [0, 1 << 20], prior outside [0, 1024], max_nodes outside [1, sims + 1], a NULL record array, visits, wins2, sums or "
    "info, a workspace that is NULL or too small)";

}  // namespace sgo

using namespace sgo;

extern "C" {

int64_t sgo_uct_workspace(int S, int n, int trees, int max_nodes) {
    if (!size_ok(S) || n < 0 || trees < 1 || trees > SGO_UCT_MAX_TREES || max_nodes < 1 || max_nodes > SGO_UCT_MAX_SIMS + 1) {
        set_error("sgo_uct_workspace: bad argument (unsupported size, n < 0, trees outside [1, SGO_UCT_MAX_TREES], max_nodes outside "
                  "[1, SGO_UCT_MAX_SIMS + 1])");
        return SGO_ERR_ARG;
    }
    return (int64_t)uct_work_bytes(S, n, trees, max_nodes);
}

int sgo_uct_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int trees, int sims, uint32_t seed, int rules,
                int max_plies, int komi2, int expand_at, int rave_equiv, int prior, int max_nodes, int32_t *d_visits, int32_t *d_wins2,
                int32_t *d_rave, int32_t *d_own, int64_t *d_sums, int32_t *d_info, int32_t *d_trace, void *d_work, int64_t work_bytes,
                void *stream) {
    if (!uct_params_ok(S, n, trees, sims, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes) || n_records < 0 || !d_records ||
        !d_visits || !d_wins2 || !d_sums || !d_info || (n && (!d_work || work_bytes < (int64_t)uct_work_bytes(S, n, trees, max_nodes)))) {
        set_error(std::string("sgo_uct_dev") + UCT_BOUNDS);
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_uct(S, n, d_records, n_records, d_index, trees, sims, seed, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes,
                      d_visits, d_wins2, d_rave, d_own, d_sums, d_info, d_trace, d_work, (hipStream_t)stream);
}

int sgo_uct(int S, int n_records, const uint32_t *records, int n, const int32_t *index, int trees, int sims, uint32_t seed, int rules, int max_plies,
            int komi2, int expand_at, int rave_equiv, int prior, int max_nodes, int32_t *visits, int32_t *wins2, int32_t *rave, int32_t *own,
            int64_t *sums, int32_t *info, int32_t *trace) {
    if (!uct_params_ok(S, n, trees, sims, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes) || n_records < 0 || !records || !visits ||
        !wins2 || !sums || !info) {
        set_error(std::string("sgo_uct") + UCT_BOUNDS);
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const size_t N = (size_t)S * S, tb = (size_t)n * (N + 1) * sizeof(int32_t);
    // every row is written whole, so nothing of the caller's outputs goes in; the last array is the workspace
    const HostArray a[] = {{tb, nullptr, visits},
                           {tb, nullptr, wins2},
                           {rave ? 2 * tb : 0, nullptr, rave},
                           {own ? (size_t)n * 2 * N * sizeof(int32_t) : 0, nullptr, own},
                           {(size_t)n * 8 * sizeof(int64_t), nullptr, sums},
                           {(size_t)n * 4 * sizeof(int32_t), nullptr, info},
                           {trace ? (size_t)n * trees * sims * sizeof(int32_t) : 0, nullptr, trace},
                           {index ? (size_t)n * sizeof(int32_t) : 0, index, nullptr},
                           {uct_work_bytes(S, n, trees, max_nodes), nullptr, nullptr}};
    return host_entry("sgo_uct", records, (size_t)n_records * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        const auto i32 = [&](int k, const void *have) { return have ? reinterpret_cast<int32_t *>(d[k]) : nullptr; };
        return launch_uct(S, n, d_records, n_records, i32(7, index), trees, sims, seed, rules, max_plies, komi2, expand_at, rave_equiv, prior,
                          max_nodes, i32(0, visits), i32(1, wins2), i32(2, rave), i32(3, own), reinterpret_cast<int64_t *>(d[4]), i32(5, info),
                          i32(6, trace), d[8], nullptr);
    });
}

}  // extern "C"
