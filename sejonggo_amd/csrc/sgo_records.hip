// sgo_records.hip -- game records as data (include/sgo.h "game records"): whole move lists replayed on the device into one
// packed record per ply, and a net's policy / value scored against the recorded moves.  A translation unit of its own:
// tests/test_engine_isa.py pins the kernel set of sgo_engine.hip, and nothing here touches an engine context.
//
//   k_records_replay<S>  every entry of every listed game: make_play, the legal set, one record and one legal bitset per ply
//   k_records_score<S>   per listed row: the rank of the recorded move in the net's policy, the best legal move, the counters
//
// k_records_replay: one 32-lane HALF of a wavefront per game, one board row per lane (sgo_rows.hpp), as k_board_advance_rows and
// k_rollout_step.  The two halves of a wave run in LOCKSTEP (the flood fills of sgo_rows.hpp vote over the whole wave): the loop
// runs to the longer of the two lists, and a half whose game has ended, was refused or does not exist plays passes on the
// position it holds and writes nothing outside its own LDS.  A recorded move is tested and its turn decided as sgo_session_play and
// sgo_session_setup do it (sgo_bits.hpp: external_move_status, moves_in_turn).
//
// The running record lives in LDS, two records per half (rows::advance_record_rows needs in != out), with a barrier between
// plies; every finished record and its legal words are copied out from there, coalesced.  Global memory is WRITE-ONLY for this
// kernel apart from the move lists: no lane ever loads a word another lane has stored to global memory.
//
// k_records_score: one half of a wavefront per row; integer arithmetic and float comparisons only, the one float it emits is a
// verbatim copy.  Results do not depend on the order of the rows.
#include <string.h>

#include "sgo_common.hpp"
#include "sgo_rows.hpp"

namespace sgo {

struct Recs {          // passed by value to the kernels
    int max_games, max_entries;
    long cap;          // records: max_entries + max_games
    uint32_t *rec;     // [cap][RW]
    uint32_t *legal;   // [cap][NW]
    int32_t *lut;      // [8][A] symmetry.py SWAP tables
    // staging, int32 each: n_entries[max_games], off[max_games], status[max_games], fail_at[max_games], actions[max_entries],
    // colors[max_entries]
    int32_t *stage;
};

template <int S>
__global__ __launch_bounds__(64) void k_records_replay(Recs d, int n_games, int n_total) {
    using G = Geo<S>;
    __shared__ __attribute__((aligned(16))) uint32_t rec[2][2][G::RW];
    __shared__ __attribute__((aligned(16))) uint32_t lg[2][G::NW];
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const int g0 = blockIdx.x * 2, g = g0 + half;
    const bool has = g < n_games;
    const int32_t *n_entries = d.stage, *offs = d.stage + d.max_games;
    int32_t *status = d.stage + 2 * (size_t)d.max_games, *fail_at = d.stage + 3 * (size_t)d.max_games;
    const int32_t *actions = d.stage + 4 * (size_t)d.max_games, *colors = actions + d.max_entries;
    // both lengths in every lane: the trip count is the wave's
    const int na = n_entries[g0], nb = (g0 + 1 < n_games) ? n_entries[g0 + 1] : 0;
    const int n = has ? (half ? nb : na) : 0, nmax = na > nb ? na : nb;
    const int off = has ? offs[g] : 0;
    const size_t base = (size_t)off + (size_t)(has ? g : 0);     // game g owns records base .. base + n

    // the empty board and its legal set (every point and the pass)
    {
        uint32_t *both = &rec[half][0][0];                       // the two records of the half are contiguous
        for (int i = y; i < 2 * G::RW; i += 32) both[i] = 0u;
    }
    if (y < G::NW) lg[half][y] = empty_legal_word<S>(y);
    __syncthreads();
    if (has) {
        uint32_t *o = d.rec + base * G::RW;
        for (int i = y; i < G::RW; i += 32) o[i] = rec[half][0][i];
        if (y < G::NW) d.legal[base * G::NW + y] = lg[half][y];
    }

    int rc = SGO_OK, fail = -1;
    for (int j = 0; j < nmax; j++) {
        const int cur = j & 1;
        const uint32_t *in = rec[half][cur];
        uint32_t *out = rec[half][cur ^ 1];
        bool live = has && rc == SGO_OK && j < n;                // uniform over the half
        int a = G::N, col = 0;
        if (live) {
            const int idx = off + j;
            if (idx < n_total) { a = actions[idx]; col = colors[idx]; }
            rc = external_move_status<S>(in, a);
            if (rc) { fail = j; live = false; a = G::N; col = 0; }
        }
        int to_play;
        const bool in_turn = moves_in_turn<S>(in, col, to_play);
        // an idle half passes on the position it holds: it takes part in every vote and touches its own LDS only
        (void)rows::advance_record_rows<S>(in, out, a, !in_turn, lg[half], half, y);
        __syncthreads();
        if (live) {
            const size_t r = base + (size_t)j + 1;
            uint32_t *o = d.rec + r * G::RW;
            for (int i = y; i < G::RW; i += 32) o[i] = out[i];
            if (y < G::NW) d.legal[r * G::NW + y] = lg[half][y];
        }
    }
    if (has && y == 0) { status[g] = rc; fail_at[g] = fail; }
}

// flags of a scored row
enum { RF_LEGAL = 1, RF_SKIPPED = 2 };

SGO_DEV float key_of(float p) { return (p != p) ? -__builtin_huge_valf() : p; }

template <int S>
__global__ __launch_bounds__(64) void k_records_score(Recs d, int n, const int32_t *index, const int32_t *target, const int32_t *zs,
                                                       const int32_t *bucket, int n_buckets, const float *policy, const float *value,
                                                       int sym_k, int32_t *rank_out, int32_t *best_out, float *p_target,
                                                       int32_t *flags_out, unsigned long long *counters) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const int i = blockIdx.x * 2 + half;
    if (i >= n) return;
    const int r = index[i], t = target[i], b = bucket[i];
    if (r < 0 || r >= d.cap || t < 0 || t >= G::A || b < 0 || b >= n_buckets) {      // uniform over the half
        if (y == 0) { rank_out[i] = -1; best_out[i] = -1; p_target[i] = 0.f; flags_out[i] = RF_SKIPPED; }
        return;
    }
    const uint32_t *lw = d.legal + (size_t)r * G::NW;
    const int32_t *lut = d.lut + (size_t)sym_k * G::A;
    const float *prow = policy + (size_t)i * G::A;
    const float pt = prow[lut[t]], kt = key_of(pt);
    const bool t_legal = (lw[t >> 5] >> (t & 31)) & 1u;
    int ahead = 0, ba = -1;
    float bk = 0.f;
    for (int a = y; a < G::A; a += 32) {
        const bool legal = (lw[a >> 5] >> (a & 31)) & 1u;
        if (!legal && a != t) continue;
        const float k = key_of(prow[lut[a]]);
        if (a != t && (k > kt || (k == kt && a < t))) ahead++;
        if (legal && (ba < 0 || k > bk)) { ba = a; bk = k; }     // ascending a: the lowest index of a tie stays
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        ahead += __shfl_xor(ahead, o, 32);
        const int oa = __shfl_xor(ba, o, 32);
        const float ok = __shfl_xor(bk, o, 32);
        if (oa >= 0 && (ba < 0 || ok > bk || (ok == bk && oa < ba))) { ba = oa; bk = ok; }
    }
    if (y == 0) {
        rank_out[i] = ahead;
        best_out[i] = ba;
        p_target[i] = pt;
        flags_out[i] = t_legal ? RF_LEGAL : 0;
        unsigned long long *c = counters + (size_t)b * 8;
        atomicAdd(c + 0, 1ull);
        if (ahead == 0) atomicAdd(c + 1, 1ull);
        if (ahead < 5) atomicAdd(c + 2, 1ull);
        if (!t_legal) atomicAdd(c + 3, 1ull);
        const int z = zs[i];
        if (z != 0) {
            atomicAdd(c + 4, 1ull);
            const float v = value[i];
            if ((v > 0.f && z > 0) || (v < 0.f && z < 0)) atomicAdd(c + 5, 1ull);
        }
    }
}

}  // namespace sgo

using namespace sgo;

struct sgo_records {
    Recs d;
    int S, N, A, RW, NW, device;
    int32_t *h_stage;      // pinned twin of Recs::stage
};

namespace {
size_t stage_words(const sgo_records *r) { return 4 * (size_t)r->d.max_games + 2 * (size_t)r->d.max_entries; }

void free_all(sgo_records *r) {
    void *dev[] = {r->d.rec, r->d.legal, r->d.lut, r->d.stage};
    for (void *p : dev) if (p) (void)hipFree(p);
    if (r->h_stage) (void)hipHostFree(r->h_stage);
    delete r;
}
}  // namespace

extern "C" {

sgo_records *sgo_records_create(int S, int max_games, int max_entries, int device_id) {
    if (!size_ok(S) || max_games < 1 || max_entries < 0 || (long)max_entries + max_games > (1l << 30)) {
        set_error("sgo_records_create: unsupported size, max_games < 1, max_entries < 0 or more than 2^30 records");
        return nullptr;
    }
    DeviceGuard guard(device_id);
    sgo_records *r = new sgo_records();
    memset(r, 0, sizeof *r);
    r->S = S; r->N = S * S; r->A = r->N + 1; r->RW = sgo_packed_words(S); r->NW = sgo_plane_words(S); r->device = device_id;
    Recs &d = r->d;
    d.max_games = max_games;
    d.max_entries = max_entries;
    d.cap = (long)max_entries + max_games;
    const size_t sw = stage_words(r) * sizeof(int32_t);
    bool ok = hipMalloc((void **)&d.rec, (size_t)d.cap * r->RW * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void **)&d.legal, (size_t)d.cap * r->NW * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void **)&d.lut, (size_t)8 * r->A * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.stage, sw) == hipSuccess &&
              hipHostMalloc((void **)&r->h_stage, sw, hipHostMallocDefault) == hipSuccess;
    ok = ok && upload_sym_luts(S, d.lut) == hipSuccess;
    if (!ok) {
        set_error("sgo_records_create: out of memory (device or pinned host)");
        free_all(r);
        return nullptr;
    }
    return r;
}

void sgo_records_destroy(sgo_records *r) {
    if (!r) return;
    DeviceGuard guard(r->device);
    (void)hipDeviceSynchronize();
    free_all(r);
}

int sgo_records_replay(sgo_records *r, int n_games, const int32_t *n_entries, const int32_t *off, const int32_t *actions,
                       const int32_t *colors, int32_t *status, int32_t *fail_at, void *stream) {
    if (!r || n_games < 0 || (n_games && (!n_entries || !off || !status || !fail_at))) {
        set_error("sgo_records_replay: bad argument");
        return SGO_ERR_ARG;
    }
    if (n_games == 0) return SGO_OK;
    const Recs &d = r->d;
    if (n_games > d.max_games) { set_error("sgo_records_replay: more games than the object was created for"); return SGO_ERR_ARG; }
    size_t total = 0;
    for (int g = 0; g < n_games; g++) {
        if (n_entries[g] < 0 || n_entries[g] > SGO_SETUP_MAX_MOVES(r->S)) {
            set_error("sgo_records_replay: a list is negative in length or longer than SGO_SETUP_MAX_MOVES");
            return SGO_ERR_ARG;
        }
        if (off[g] < 0 || (size_t)off[g] != total) {
            set_error("sgo_records_replay: the lists must lie back to back, off[g] = n_entries[0] + ... + n_entries[g-1]");
            return SGO_ERR_ARG;
        }
        total += (size_t)n_entries[g];
        if (total > (size_t)d.max_entries) { set_error("sgo_records_replay: more entries than the object was created for"); return SGO_ERR_ARG; }
    }
    if (total && !actions) { set_error("sgo_records_replay: bad argument"); return SGO_ERR_ARG; }
    DeviceGuard guard(r->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t mg = (size_t)d.max_games, me = (size_t)d.max_entries;
    int32_t *h = r->h_stage;
    memcpy(h, n_entries, sizeof(int32_t) * n_games);
    memcpy(h + mg, off, sizeof(int32_t) * n_games);
    memcpy(h + 4 * mg, actions, sizeof(int32_t) * total);
    if (colors) memcpy(h + 4 * mg + me, colors, sizeof(int32_t) * total);
    else memset(h + 4 * mg + me, 0, sizeof(int32_t) * total);
    // ONE copy takes lengths, offsets, (stale) verdicts and both lists over: everything up to the last colour used
    SGO_HIP(hipMemcpyAsync(d.stage, h, sizeof(int32_t) * (4 * mg + me + total), hipMemcpyHostToDevice, st));
    SGO_DISPATCH(r->S, k_records_replay<kS><<<dim3(cdiv(n_games, 2)), dim3(64), 0, st>>>(d, n_games, (int)total));
    SGO_HIP(hipGetLastError());
    SGO_HIP(hipMemcpyAsync(h + 2 * mg, d.stage + 2 * mg, sizeof(int32_t) * 2 * mg, hipMemcpyDeviceToHost, st));   // status, fail_at
    SGO_HIP(hipStreamSynchronize(st));
    memcpy(status, h + 2 * mg, sizeof(int32_t) * n_games);
    memcpy(fail_at, h + 3 * mg, sizeof(int32_t) * n_games);
    return SGO_OK;
}

int sgo_records_list(sgo_records *r, const uint32_t **d_records, const uint32_t **d_legal) {
    if (!r) { set_error("sgo_records_list: bad argument"); return SGO_ERR_ARG; }
    if (d_records) *d_records = r->d.rec;
    if (d_legal) *d_legal = r->d.legal;
    return (int)r->d.cap;
}

int sgo_records_score_dev(sgo_records *r, int n, const int32_t *d_index, const int32_t *d_target, const int32_t *d_z,
                          const int32_t *d_bucket, int n_buckets, const float *d_policy, const float *d_value, int sym_k,
                          int32_t *d_rank, int32_t *d_best, float *d_p_target, int32_t *d_flags, int64_t *d_counters, void *stream) {
    if (!r || n < 0 || sym_k < 0 || sym_k > 7 || n_buckets < 1 ||
        (n && (!d_index || !d_target || !d_z || !d_bucket || !d_policy || !d_value || !d_rank || !d_best || !d_p_target || !d_flags ||
               !d_counters))) {
        set_error("sgo_records_score_dev: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    DeviceGuard guard(r->device);
    SGO_DISPATCH(r->S, k_records_score<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, (hipStream_t)stream>>>(
                           r->d, n, d_index, d_target, d_z, d_bucket, n_buckets, d_policy, d_value, sym_k, d_rank, d_best, d_p_target,
                           d_flags, reinterpret_cast<unsigned long long *>(d_counters)));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

}  // extern "C"
