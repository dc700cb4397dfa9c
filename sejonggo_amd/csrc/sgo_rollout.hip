// sgo_rollout.hip -- policy rollouts on the device (include/sgo.h "policy rollouts"): thousands of tree-less games advance one
// policy-sampled move per net call; at their end every point is counted for the colour that holds it.  What final_score,
// final_status_list and the review's dead-stone count are made of.  A translation unit of its own: tests/test_engine_isa.py
// pins the kernel set of sgo_engine.hip, and nothing here touches k_search.
//
//   k_rollout_start     clones the source records into the rollout records, zeroes counters and accumulators; the sources are
//                       (records, index): host records staged once, device records, or the root records of holding session
//                       slots in the context's blocks, named by k_session_roots (sgo_session.hpp)
//   k_rollout_step<S>   one ply of every listed rollout: legal set, weights, pick, make_play, end test, score, accumulation,
//                       append of the survivors to the next list.  The ply is rows::load_ply / rows::store_ply, the two halves of
//                       rows::advance_record_rows, around its own legal -> draw -> advance
//
// Kernel form: one 32-lane HALF of a wavefront per listed rollout, one board row per lane (sgo_rows.hpp), as
// k_board_advance_rows.  A step's list is a few thousand rollouts at most, far too few for the lane-per-position form.
// The two halves of a wave run in LOCKSTEP (the flood fills of sgo_rows.hpp vote over the whole wave), so nothing below branches
// on a per-rollout condition around a rules call: a half without a rollout repeats the last one and writes nothing.
//
// Records PING-PONG: rollout i lives in record i or in record max_rollouts + i, a ply reads one and writes the other, so the
// history planes move with plain loads and stores and no lane ever reads a word another lane has already overwritten.  The
// index list names the record, which is all a consumer of sgo_rollout_list needs.
//
// Everything that decides a move is integer arithmetic (include/sgo.h states it in full): results are exact and do not depend
// on the order of the list, which the survivors' appends (one atomicAdd each) leave unspecified.
#include <string.h>

#include "sgo_draw.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_rows.hpp"

namespace sgo {

struct Roll {          // passed by value to the kernels
    int max_r, max_src;
    uint32_t *rec;     // [2 * max_r][RW]
    int32_t *list[2];  // [max_r] record indices of the live rollouts: the step reads one list and fills the other
    int32_t *ply, *passes;        // [max_r], by rollout id (= its global id g)
    int32_t *bown, *wown;         // [max_src][N]
    unsigned long long *sums;     // [max_src][8]
    int32_t *count;    // [0] entries of the list being filled
    int32_t *lut;      // [8][A] symmetry.py SWAP tables
    uint32_t *src;     // [max_src][RW] staging of the source records of sgo_rollout_start (host records)
    int32_t *slots, *sroot;       // sgo_rollout_start_sessions: slot ids in [max_src]; status and root record index out [2][max_src]
};

// floor(clamp(p) * 2^20) + 1: the scaling is exact in float32, the conversion truncates a non-negative value
__device__ __forceinline__ uint32_t weight_of(float p) {
    if (!(p > 0.f)) return 1u;                 // NaN, negatives, +-0
    if (p >= 1.f) return (1u << 20) + 1u;      // 1, above, +inf
    return (uint32_t)(p * 1048576.f) + 1u;
}
template <int S>
__global__ __launch_bounds__(256) void k_rollout_start(Roll d, int n_src, const uint32_t *srcrec, const int32_t *index, int per_src) {
    using G = Geo<S>;
    const long n_r = (long)n_src * per_src, words = n_r * G::RW;
    const long stride = (long)gridDim.x * blockDim.x;
    const long own_n = (long)n_src * G::N, top = words > own_n ? words : own_n;      // RW < N on the larger boards
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < top; t += stride) {
        if (t < words) {
            const long i = t / G::RW;
            const int w = (int)(t - i * G::RW), s = (int)(i / per_src);
            d.rec[t] = srcrec[(size_t)(index ? index[s] : s) * G::RW + w];
            if (w == 0) { d.list[0][i] = (int32_t)i; d.ply[i] = 0; d.passes[i] = 0; }
        }
        if (t < own_n) { d.bown[t] = 0; d.wown[t] = 0; }
        if (t < (long)n_src * 8) d.sums[t] = 0ull;
        if (t == 0) d.count[0] = 0;
    }
}

template <int S>
__global__ __launch_bounds__(64) void k_rollout_step(Roll d, int n, int cur, const float *policy, int sym_k, uint32_t seed,
                                                      int per_src, int max_plies) {
    using G = Geo<S>;
    __shared__ float sp[2][G::A + 1];
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const int iw = blockIdx.x * 2 + half;
    const bool valid = iw < n;
    const int i = valid ? iw : n - 1;                  // an idle half repeats the last rollout and writes nothing
    const int e = d.list[cur][i];
    const int rid = e >= d.max_r ? e - d.max_r : e;    // the rollout's id, also its global id g
    const int o = e >= d.max_r ? rid : rid + d.max_r;  // the record this ply writes
    const uint32_t *in = d.rec + (size_t)e * G::RW;
    uint32_t *out = d.rec + (size_t)o * G::RW;
    const int ply = d.ply[rid], passes = d.passes[rid];

    // the policy row, read coalesced; it arrives as the net produced it from the input transformed by sym_k
    const float *prow = policy + (size_t)i * G::A;
    for (int j = y; j < G::N; j += 32) sp[half][j] = prow[j];
    __syncthreads();

    const rows::Board<S> bd(half, y);
    rows::Ply p = rows::load_ply<S>(in, false, y);
    const uint32_t prev = rows::load_row<S>(in + (p.mover_white ? 3 : 2) * G::NW, y);
    const uint32_t lg = bd.legal(p.own, p.opp, prev);

    // weights of this row's points and their sum; an inclusive scan over the rows of the half
    const int32_t *lut = d.lut + (size_t)sym_k * G::A;
    uint32_t w[S];
    uint32_t rs = 0;
#pragma unroll
    for (int x = 0; x < S; x++) {
        const bool on = (lg >> x) & 1u;                // rows >= S have no legal bit
        const int a = on ? y * S + x : 0;
        const float p = sp[half][lut[a]];
        w[x] = on ? weight_of(p) : 0u;
        rs += w[x];
    }
    uint32_t incl = rs;
#pragma unroll
    for (int s = 1; s < 32; s <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, s, 32);
        if (y >= s) incl += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 31, 32);     // < 2^29
    const uint32_t r = draw32(seed, (uint32_t)rid, (uint32_t)ply);
    const uint32_t t = (uint32_t)(((unsigned long long)r * total) >> 32);
    const uint32_t excl = incl - rs;
    const bool mine = total != 0 && excl <= t && t < incl;          // exactly one row when a board move exists
    int a_loc = 0;
    {
        uint32_t c = excl;
        bool found = false;
#pragma unroll
        for (int x = 0; x < S; x++) {
            c += w[x];
            if (!found && c > t) { found = true; a_loc = y * S + x; }
        }
    }
    const uint32_t who = rows::half_ballot(mine, half);
    const int from = who ? (__ffs((int)who) - 1) : 0;
    const int a_pick = __shfl(a_loc, from, 32);
    const int a = total != 0 ? a_pick : G::N;                       // no legal board point: a pass

    (void)bd.advance(p.own, p.opp, a);                              // a legal point is never occupied
    const uint32_t nb = p.black(), nw = p.white();
    rows::store_ply<S>(in, out, p, 0u, nullptr, half, y, valid);    // an idle half writes nothing

    const int ply1 = ply + 1, passes1 = (a == G::N) ? passes + 1 : 0;
    const bool ended = passes1 >= 2 || ply1 >= max_plies;
    if (__any(ended)) {                                             // uniform over the wave: the fills below vote over it
        uint32_t bo, wo;
        area_owners<S>(bd, nb, nw, bo, wo);                         // play.py:244-292: reached by one colour only
        const int bp = half_sum(__popc(bo)), wp = half_sum(__popc(wo));
        if (ended && valid) {
            const int s = rid / per_src;
            int32_t *ob = d.bown + (size_t)s * G::N + y * S, *ow = d.wown + (size_t)s * G::N + y * S;
#pragma unroll
            for (int x = 0; x < S; x++) {
                if ((bo >> x) & 1u) atomicAdd(ob + x, 1);
                if ((wo >> x) & 1u) atomicAdd(ow + x, 1);
            }
            if (y == 0) {
                unsigned long long *sm = d.sums + (size_t)s * 8;
                const long long diff = bp - wp;
                atomicAdd(sm + (diff > 0 ? 0 : (diff < 0 ? 1 : 2)), 1ull);
                atomicAdd(sm + 3, (unsigned long long)diff);        // two's complement: the sum is read back as int64
                atomicAdd(sm + 4, (unsigned long long)(diff * diff));
                atomicAdd(sm + 5, (unsigned long long)ply1);
                if (passes1 < 2) atomicAdd(sm + 6, 1ull);
                atomicAdd(sm + 7, 1ull);
            }
        }
    }
    if (valid && y == 0) {
        d.ply[rid] = ply1;
        d.passes[rid] = passes1;
        if (!ended) d.list[cur ^ 1][atomicAdd(d.count, 1)] = o;
    }
}

}  // namespace sgo

using namespace sgo;

struct sgo_rollout {
    Roll d;
    int S, N, A, RW, device;
    int n_src, per_src, max_plies, n_live, n_total, steps, cur;
    uint32_t seed;
    bool started;
    int32_t *h_stat;       // pinned: the count of the next list
    uint32_t *h_src;       // pinned twin of Roll::src
    int32_t *h_slots;      // pinned [2][max_src]: slot ids out, status back
    hipEvent_t ev_src;     // the staged sources have left the pinned block
    bool src_busy;
};

namespace {
void free_all(sgo_rollout *r) {
    Roll &d = r->d;
    void *dev[] = {d.rec, d.list[0], d.list[1], d.ply, d.passes, d.bown, d.wown, d.sums, d.count, d.lut, d.src, d.slots, d.sroot};
    for (void *p : dev) if (p) (void)hipFree(p);
    if (r->h_stat) (void)hipHostFree(r->h_stat);
    if (r->h_src) (void)hipHostFree(r->h_src);
    if (r->h_slots) (void)hipHostFree(r->h_slots);
    if (r->ev_src) (void)hipEventDestroy(r->ev_src);
    delete r;
}

int check_start(const sgo_rollout *r, const char *what, int n_src, int per_src) {
    if (n_src < 1 || per_src < 1 || n_src > r->d.max_src || (long)n_src * per_src > r->d.max_r) {
        set_error(std::string(what) + ": n_src in [1, max_sources], per_src >= 1 and n_src * per_src <= max_rollouts are required");
        return SGO_ERR_ARG;
    }
    return SGO_OK;
}

// queues the start kernel on `st` and sets the host state of a fresh run
int launch_start(sgo_rollout *r, int n_src, const uint32_t *d_records, const int32_t *d_index, int per_src, uint32_t seed,
                 int max_plies, hipStream_t st) {
    const long words = (long)n_src * per_src * r->RW;
    const int blocks = cdiv(words, 256) < 4096 ? cdiv(words, 256) : 4096;
    SGO_DISPATCH(r->S, k_rollout_start<kS><<<dim3(blocks), dim3(256), 0, st>>>(r->d, n_src, d_records, d_index, per_src));
    SGO_HIP(hipGetLastError());
    r->n_src = n_src;
    r->per_src = per_src;
    r->seed = seed;
    r->max_plies = max_plies > 0 ? max_plies : 2 * r->N;
    r->n_total = r->n_live = n_src * per_src;
    r->steps = 0;
    r->cur = 0;
    r->started = true;
    return SGO_OK;
}
}  // namespace

extern "C" {

sgo_rollout *sgo_rollout_create(int S, int max_rollouts, int max_sources, int device_id) {
    if (!size_ok(S) || max_rollouts < 1 || max_sources < 1 || max_sources > max_rollouts) {
        set_error("sgo_rollout_create: unsupported size, or not 1 <= max_sources <= max_rollouts");
        return nullptr;
    }
    DeviceGuard guard(device_id);
    sgo_rollout *r = new sgo_rollout();
    memset(r, 0, sizeof *r);
    r->S = S; r->N = S * S; r->A = r->N + 1; r->RW = sgo_packed_words(S); r->device = device_id;
    Roll &d = r->d;
    d.max_r = max_rollouts;
    d.max_src = max_sources;
    const size_t mr = (size_t)max_rollouts, ms = (size_t)max_sources;
    bool ok = hipMalloc((void **)&d.rec, 2 * mr * r->RW * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void **)&d.list[0], mr * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.list[1], mr * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.ply, mr * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.passes, mr * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.bown, ms * r->N * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.wown, ms * r->N * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.sums, ms * 8 * sizeof(unsigned long long)) == hipSuccess &&
              hipMalloc((void **)&d.count, 4 * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.lut, (size_t)8 * r->A * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.src, ms * r->RW * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void **)&d.slots, ms * sizeof(int32_t)) == hipSuccess &&
              hipMalloc((void **)&d.sroot, 2 * ms * sizeof(int32_t)) == hipSuccess &&
              hipHostMalloc((void **)&r->h_stat, 4 * sizeof(int32_t), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&r->h_src, ms * r->RW * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&r->h_slots, 2 * ms * sizeof(int32_t), hipHostMallocDefault) == hipSuccess &&
              hipEventCreateWithFlags(&r->ev_src, hipEventDisableTiming) == hipSuccess;
    ok = ok && upload_sym_luts(S, d.lut) == hipSuccess;
    if (!ok) {
        set_error("sgo_rollout_create: out of memory (device or pinned host)");
        free_all(r);
        return nullptr;
    }
    return r;
}

void sgo_rollout_destroy(sgo_rollout *r) {
    if (!r) return;
    DeviceGuard guard(r->device);
    (void)hipDeviceSynchronize();
    free_all(r);
}

int sgo_rollout_start_dev(sgo_rollout *r, int n_src, const uint32_t *d_records, const int32_t *d_index, int per_src, uint32_t seed,
                          int max_plies, void *stream) {
    if (!r || !d_records) { set_error("sgo_rollout_start_dev: bad argument"); return SGO_ERR_ARG; }
    const int rc = check_start(r, "sgo_rollout_start_dev", n_src, per_src);
    if (rc) return rc;
    return launch_start(r, n_src, d_records, d_index, per_src, seed, max_plies, (hipStream_t)stream);
}

int sgo_rollout_start(sgo_rollout *r, int n_src, const uint32_t *records, int per_src, uint32_t seed, int max_plies, void *stream) {
    if (!r || !records) { set_error("sgo_rollout_start: bad argument"); return SGO_ERR_ARG; }
    const int rc = check_start(r, "sgo_rollout_start", n_src, per_src);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the pinned block is reused: wait (host side, this one copy only) until the previous batch has left it
    if (r->src_busy) { SGO_HIP(hipEventSynchronize(r->ev_src)); r->src_busy = false; }
    const size_t bytes = (size_t)n_src * r->RW * sizeof(uint32_t);
    memcpy(r->h_src, records, bytes);
    SGO_HIP(hipMemcpyAsync(r->d.src, r->h_src, bytes, hipMemcpyHostToDevice, st));
    SGO_HIP(hipEventRecord(r->ev_src, st));
    r->src_busy = true;
    return launch_start(r, n_src, r->d.src, nullptr, per_src, seed, max_plies, st);
}

int sgo_rollout_start_sessions(sgo_rollout *r, sgo_ctx *x, int n, const int32_t *slots, int per_src, uint32_t seed, int max_plies,
                               int32_t *status, void *stream) {
    if (!r || !x || !slots || !status || x->c.S != r->S) { set_error("sgo_rollout_start_sessions: bad argument (or board sizes differ)"); return SGO_ERR_ARG; }
    const int rc = check_start(r, "sgo_rollout_start_sessions", n, per_src);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (slots[i] < 0 || slots[i] >= x->c.G) { set_error("sgo_rollout_start_sessions: slot outside the context"); return SGO_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    // the root records are read in place: k_session_roots names them, k_rollout_start clones them from the context's blocks
    const size_t ms = (size_t)r->d.max_src;
    int32_t *h_status = r->h_slots + ms, *d_status = r->d.sroot, *d_index = r->d.sroot + ms;
    memcpy(r->h_slots, slots, sizeof(int32_t) * (size_t)n);
    SGO_HIP(hipMemcpyAsync(r->d.slots, r->h_slots, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    const int lrc = launch_session_roots(x->c, n, r->d.slots, d_status, d_index, st);
    if (lrc != SGO_OK) return lrc;
    SGO_HIP(hipMemcpyAsync(h_status, d_status, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    SGO_HIP(hipStreamSynchronize(st));           // the verdict decides whether anything starts
    bool bad = false;
    for (int i = 0; i < n; i++) { status[i] = h_status[i]; bad = bad || h_status[i] != SGO_OK; }
    if (bad) { set_error("sgo_rollout_start_sessions: a listed slot is not a holding session; nothing started"); return SGO_ERR_STATE; }
    return launch_start(r, n, x->c.pos, d_index, per_src, seed, max_plies, st);
}

int sgo_rollout_list(sgo_rollout *r, const uint32_t **d_records, const int32_t **d_index) {
    if (!r) { set_error("sgo_rollout_list: bad argument"); return SGO_ERR_ARG; }
    if (d_records) *d_records = r->d.rec;
    if (d_index) *d_index = r->d.list[r->cur];
    return r->d.max_r;
}

int sgo_rollout_step(sgo_rollout *r, const float *d_policy, int sym_k, void *stream, sgo_rollout_status *out) {
    if (!r || !d_policy || !out || sym_k < 0 || sym_k > 7) { set_error("sgo_rollout_step: bad argument"); return SGO_ERR_ARG; }
    if (!r->started || r->n_live == 0) { set_error("sgo_rollout_step: no live rollouts (start first)"); return SGO_ERR_STATE; }
    hipStream_t st = (hipStream_t)stream;
    const int n = r->n_live;
    SGO_HIP(hipMemsetAsync(r->d.count, 0, sizeof(int32_t), st));
    SGO_DISPATCH(r->S, k_rollout_step<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(r->d, n, r->cur, d_policy, sym_k, r->seed, r->per_src,
                                                                                     r->max_plies));
    SGO_HIP(hipGetLastError());
    SGO_HIP(hipMemcpyAsync(r->h_stat, r->d.count, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SGO_HIP(hipStreamSynchronize(st));
    r->n_live = r->h_stat[0];
    r->cur ^= 1;
    r->steps++;
    out->n_live = r->n_live;
    out->n_done = r->n_total - r->n_live;
    out->steps = r->steps;
    out->error = 0;
    return SGO_OK;
}

int sgo_rollout_result(sgo_rollout *r, int n_src, int32_t *black_own, int32_t *white_own, int64_t *sums) {
    if (!r || n_src < 0) { set_error("sgo_rollout_result: bad argument"); return SGO_ERR_ARG; }
    if (!r->started || r->n_live != 0) { set_error("sgo_rollout_result: rollouts are live, or none were started"); return SGO_ERR_STATE; }
    if (n_src > r->n_src) { set_error("sgo_rollout_result: more sources than were started"); return SGO_ERR_ARG; }
    // the last step synchronised its stream: the accumulators are final
    const size_t ob = sizeof(int32_t) * (size_t)n_src * r->N;
    if (black_own && ob) SGO_HIP(hipMemcpy(black_own, r->d.bown, ob, hipMemcpyDeviceToHost));
    if (white_own && ob) SGO_HIP(hipMemcpy(white_own, r->d.wown, ob, hipMemcpyDeviceToHost));
    if (sums && n_src) SGO_HIP(hipMemcpy(sums, r->d.sums, sizeof(int64_t) * (size_t)n_src * 8, hipMemcpyDeviceToHost));
    return SGO_OK;
}

}  // extern "C"
