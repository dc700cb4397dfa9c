// sgo_session.hip -- interactive (session) slots of the self-play engine: sgo_session_play, _genmove, _analyze, _setup, _report, the
// "interactive games" section of include/sgo.h, and the host side of sgo_session_keys ("position keys"; its kernel is in
// sgo_keys.hip), of sgo_session_tactics ("chains and ladders"; sgo_tactics.hip), of sgo_session_life ("unconditional life";
// sgo_life.hip), of sgo_session_shapes ("shape search"; sgo_shapes.hip), of sgo_session_moves ("move outcomes"; sgo_moves.hip), of
// sgo_session_influence ("influence"; sgo_influence.hip), of sgo_session_secure ("securing moves"; sgo_secure.hip), of
// sgo_session_solve ("life and death"; sgo_solve.hip) and of sgo_session_race ("capturing races"; sgo_race.hip) and of sgo_session_connect
// ("connections"; sgo_connect.hip) and of sgo_session_playout ("light playouts"; sgo_playout.hip).
// Those nine (session_rows below, over the launchers of sgo_analysis.hpp) and sgo_rollout_start_sessions (sgo_rollout.hip) find
// the root records of the listed slots with launch_session_roots below and run their ordinary record kernels over the context's
// blocks.  sgo_session_open is a restart and lives beside sgo_start_games in sgo_engine.hip; the
// kernels are in sgo_session.hpp.  What it replaces of the reference (drsagitn/sejonggo): sejonggo_nomodel.py:20-100, the
// SejongGoEngine a GTP front-end drives.
#include <string.h>
#include <functional>
#include <vector>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_session.hpp"

using namespace sgo;

namespace sgo {
int launch_session_roots(const Ctx &c, int n, const int32_t *d_slots, int32_t *d_status, int32_t *d_index, hipStream_t st) {
    k_session_roots<<<dim3(cdiv(n, 64)), dim3(64), 0, st>>>(c, n, d_slots, d_status, d_index);
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}
}

// Stage n slots (+ optional actions / colours) in the context's staging area, as sgo_start_games does: wait until the previous
// batch has left the pinned block, fill it, one host-to-device copy on the caller's stream.
static int stage_slots(sgo_ctx *x, const char *who, int n, const int32_t *slots, const int32_t *actions, const int32_t *colors,
                       StageLayout &L, hipStream_t st) {
    Ctx &c = x->c;
    if (n > c.G) { set_error(std::string(who) + ": more slots than the context has"); return SGO_ERR_ARG; }
    std::vector<char> seen((size_t)c.G, 0);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= c.G) { set_error(std::string(who) + ": slot out of range"); return SGO_ERR_ARG; }
        if (seen[slots[i]]) { set_error(std::string(who) + ": a slot is listed twice"); return SGO_ERR_ARG; }
        seen[slots[i]] = 1;
    }
    SGO_HIP(hipSetDevice(c.cfg.device_id));
    if (x->h.stage_busy) { SGO_HIP(hipEventSynchronize(x->h.ev_stage)); x->h.stage_busy = false; }
    L = stage_layout(n, c.APAD, 0, false);
    uint8_t *h = x->h.stage;
    memcpy(h + L.slots, slots, sizeof(int32_t) * n);
    if (actions) memcpy(h + L.resign, actions, sizeof(int32_t) * n);
    int32_t *hc = reinterpret_cast<int32_t *>(h + L.resign2);
    for (int i = 0; actions && i < n; i++) hc[i] = colors ? colors[i] : 0;
    SGO_HIP(hipMemcpyAsync(c.stage, h, L.total, hipMemcpyHostToDevice, st));
    return SGO_OK;
}

// The arming behind sgo_session_genmove and sgo_session_analyze: all listed slots or none.
static int arm_slots(sgo_ctx *x, const char *who, int n, const int32_t *slots, int analysis, int rounds, hipStream_t st) {
    Ctx &c = x->c;
    StageLayout L;
    const int rc = stage_slots(x, who, n, slots, nullptr, nullptr, L, st);
    if (rc != SGO_OK) return rc;
    k_session_arm<<<dim3(1), dim3(1024), 0, st>>>(c, n, L, analysis, rounds);
    SGO_HIP(hipGetLastError());
    int32_t *hs = reinterpret_cast<int32_t *>(x->h.stage + L.first);
    SGO_HIP(hipMemcpyAsync(hs, c.stage + L.first, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SGO_HIP(hipStreamSynchronize(st));
    if (hs[0] != SGO_OK) { set_error(std::string(who) + ": a listed slot is not a holding session; nothing was armed"); return hs[0]; }
    return SGO_OK;
}

// The session buffer (HostSide::sess_h / sess_d) holds at least `bytes`: it only grows, so a caller that repeats a call of one
// size allocates once.  Both users wait for their stream before they return, so nothing is in flight when it is replaced.
static int session_buffer(sgo_ctx *x, size_t bytes) {
    HostSide &h = x->h;
    if (bytes <= h.sess_cap) return SGO_OK;
    size_t cap = h.sess_cap ? h.sess_cap : 4096;
    while (cap < bytes) cap *= 2;
    if (h.sess_h) (void)hipHostFree(h.sess_h);
    if (h.sess_d) (void)hipFree(h.sess_d);
    h.sess_h = h.sess_d = nullptr;
    h.sess_cap = 0;
    SGO_HIP(hipHostMalloc((void **)&h.sess_h, cap, hipHostMallocDefault));
    SGO_HIP(hipMalloc((void **)&h.sess_d, cap));
    h.sess_cap = cap;
    return SGO_OK;
}

// The shared opening of sgo_session_report and of session_rows below (readers: a slot may be listed twice): the list is checked
// against the context, the device set, the session buffer grown to `bytes`, and the slots staged in its first al8(4 n) bytes.
static int stage_session_list(sgo_ctx *x, const char *who, int n, const int32_t *slots, size_t bytes, hipStream_t st) {
    const Ctx &c = x->c;
    if (n > c.G) { set_error(std::string(who) + ": more slots than the context has"); return SGO_ERR_ARG; }
    for (int i = 0; i < n; i++)
        if (slots[i] < 0 || slots[i] >= c.G) { set_error(std::string(who) + ": slot out of range"); return SGO_ERR_ARG; }
    SGO_HIP(hipSetDevice(c.cfg.device_id));
    const int rc = session_buffer(x, bytes);
    if (rc != SGO_OK) return rc;
    memcpy(x->h.sess_h, slots, sizeof(int32_t) * n);
    SGO_HIP(hipMemcpyAsync(x->h.sess_d, x->h.sess_h, al8(sizeof(int32_t) * (size_t)n), hipMemcpyHostToDevice, st));
    return SGO_OK;
}

// One output column of a session analysis: `row` bytes per listed slot in the caller's array `dst`, the device column on an
// `align`-byte boundary (8 at the least).  Where a kernel leaves the end of a row unwritten, `stored(i)` gives the bytes of row i
// to copy; it runs after the columns before it have their row i.
struct RowCol {
    void *dst;
    size_t row, align;
    std::function<size_t(int)> stored;
};

// The body of the eleven session analyses (keys, tactics, life, shapes, moves, influence, secure, solve, race, connect, playout).  The session buffer is laid out as
//     slots | input | record index | status | columns
// the slots (and `input`, where there is one: a shape table, the dead sets) go up, k_session_roots names the root records,
// launch(d_index, d_input, d_cols) runs the ordinary record launcher over the context's blocks, and everything behind the index
// comes back in ONE copy.  A refused slot keeps its status; its rows stay as the caller filled them.
template <size_t NC, class Launch>
static int session_rows(sgo_ctx *x, const char *who, int n, const int32_t *slots, const void *input, size_t input_bytes, int32_t *status,
                        const RowCol (&cols)[NC], hipStream_t st, Launch launch) {
    const size_t ib = al8(sizeof(int32_t) * (size_t)n), xo = ib + (input ? al8(input_bytes) : 0), so = xo + ib;
    size_t off[NC], end = so + ib;
    for (size_t k = 0; k < NC; k++) {
        const size_t a = cols[k].align < 8 ? 8 : cols[k].align;
        off[k] = (end + a - 1) & ~(a - 1);
        end = off[k] + cols[k].row * n;
    }
    int rc = stage_session_list(x, who, n, slots, end, st);
    if (rc != SGO_OK) return rc;
    uint8_t *h = x->h.sess_h, *d = x->h.sess_d, *dc[NC];
    for (size_t k = 0; k < NC; k++) dc[k] = d + off[k];
    if (input) {
        memcpy(h + ib, input, input_bytes);
        SGO_HIP(hipMemcpyAsync(d + ib, h + ib, input_bytes, hipMemcpyHostToDevice, st));
    }
    int32_t *d_index = reinterpret_cast<int32_t *>(d + xo);
    rc = launch_session_roots(x->c, n, reinterpret_cast<const int32_t *>(d), reinterpret_cast<int32_t *>(d + so), d_index, st);
    if (rc == SGO_OK) rc = launch(d_index, input ? d + ib : nullptr, dc);
    if (rc != SGO_OK) return rc;
    SGO_HIP(hipMemcpyAsync(h + so, d + so, end - so, hipMemcpyDeviceToHost, st));
    SGO_HIP(hipStreamSynchronize(st));
    const int32_t *hs = reinterpret_cast<const int32_t *>(h + so);
    for (int i = 0; i < n; i++) {
        status[i] = hs[i];
        if (hs[i] != SGO_OK) continue;
        for (size_t k = 0; k < NC; k++) {
            const RowCol &col = cols[k];
            memcpy(static_cast<uint8_t *>(col.dst) + col.row * i, h + off[k] + col.row * i, col.stored ? col.stored(i) : col.row);
        }
    }
    return SGO_OK;
}

extern "C" {

int sgo_session_play(sgo_ctx *x, int n, const int32_t *slots, const int32_t *actions, const int32_t *colors, int32_t *status,
                     void *stream) {
    if (!x || n < 0 || (n && (!slots || !actions || !status))) { set_error("sgo_session_play: bad argument"); return SGO_ERR_ARG; }
    if (n == 0) return SGO_OK;
    Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    StageLayout L;
    const int rc = stage_slots(x, "sgo_session_play", n, slots, actions, colors, L, st);
    if (rc != SGO_OK) return rc;
    SGO_DISPATCH(c.S, {
        const size_t lds = search_lds<kS>(c);
        if (lds > 64 * 1024 && !x->h.lds_attr_session) {
            SGO_HIP(hipFuncSetAttribute((const void *)k_session_play<kS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            x->h.lds_attr_session = true;
        }
        k_session_play<kS><<<dim3(n), dim3(64), lds, st>>>(c, n, L);
    });
    SGO_HIP(hipGetLastError());
    // the status words come back through the pinned block; the stream is waited for, so the block is free again on return
    int32_t *hs = reinterpret_cast<int32_t *>(x->h.stage + L.first);
    SGO_HIP(hipMemcpyAsync(hs, c.stage + L.first, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    SGO_HIP(hipStreamSynchronize(st));
    memcpy(status, hs, sizeof(int32_t) * n);
    return SGO_OK;
}

int sgo_session_genmove(sgo_ctx *x, int n, const int32_t *slots, void *stream) {
    if (!x || n < 0 || (n && !slots)) { set_error("sgo_session_genmove: bad argument"); return SGO_ERR_ARG; }
    if (n == 0) return SGO_OK;
    hipStream_t st = (hipStream_t)stream;
    return arm_slots(x, "sgo_session_genmove", n, slots, 0, 0, st);
}

int sgo_session_analyze(sgo_ctx *x, int n, const int32_t *slots, int sims, void *stream) {
    if (!x || n < 0 || (n && !slots)) { set_error("sgo_session_analyze: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    if (sims <= 0) sims = c.cfg.sims;
    if (sims < c.cfg.energy) { set_error("sgo_session_analyze: fewer simulations than one round (energy) holds"); return SGO_ERR_ARG; }
    if (n == 0) return SGO_OK;
    return arm_slots(x, "sgo_session_analyze", n, slots, 1, sims / c.cfg.energy, (hipStream_t)stream);
}

int sgo_session_setup(sgo_ctx *x, int n, const int32_t *slots, const int32_t *n_moves, const int32_t *moves_off,
                      const int32_t *actions, const int32_t *colors, int32_t *status, int32_t *fail_at, void *stream) {
    if (!x || n < 0 || (n && (!slots || !n_moves || !moves_off || !status || !fail_at))) {
        set_error("sgo_session_setup: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    if (n > c.G) { set_error("sgo_session_setup: more slots than the context has"); return SGO_ERR_ARG; }
    std::vector<char> seen((size_t)c.G, 0);
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= c.G) { set_error("sgo_session_setup: slot out of range"); return SGO_ERR_ARG; }
        if (seen[slots[i]]) { set_error("sgo_session_setup: a slot is listed twice"); return SGO_ERR_ARG; }
        seen[slots[i]] = 1;
        if (n_moves[i] < 0 || n_moves[i] > SGO_SETUP_MAX_MOVES(c.S) || moves_off[i] < 0 || (n_moves[i] && !actions)) {
            set_error("sgo_session_setup: a move list is negative in length or longer than SGO_SETUP_MAX_MOVES");
            return SGO_ERR_ARG;
        }
        total += (size_t)n_moves[i];
    }
    SGO_HIP(hipSetDevice(c.cfg.device_id));
    const SetupLayout L = setup_layout(n, total);
    const int rc = session_buffer(x, L.total);
    if (rc != SGO_OK) return rc;
    // the lists are packed back to back in the pinned block (the caller's offsets need not be), then ONE copy takes them over
    uint8_t *h = x->h.sess_h;
    memcpy(h + L.slots, slots, sizeof(int32_t) * n);
    memcpy(h + L.n_moves, n_moves, sizeof(int32_t) * n);
    int32_t *ho = reinterpret_cast<int32_t *>(h + L.off), *ha = reinterpret_cast<int32_t *>(h + L.actions),
            *hc = reinterpret_cast<int32_t *>(h + L.colors);
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        ho[i] = (int32_t)at;
        for (int j = 0; j < n_moves[i]; j++) {
            ha[at + j] = actions[(size_t)moves_off[i] + j];
            hc[at + j] = colors ? colors[(size_t)moves_off[i] + j] : 0;
        }
        at += (size_t)n_moves[i];
    }
    SGO_HIP(hipMemcpyAsync(x->h.sess_d + L.slots, h + L.slots, L.total - L.slots, hipMemcpyHostToDevice, st));
    SGO_DISPATCH(c.S, k_session_setup<kS><<<dim3(n), dim3(64), 0, st>>>(c, n, x->h.sess_d, L));
    SGO_HIP(hipGetLastError());
    SGO_HIP(hipMemcpyAsync(h, x->h.sess_d, L.slots, hipMemcpyDeviceToHost, st));      // status and fail_at, adjacent
    SGO_HIP(hipStreamSynchronize(st));
    memcpy(status, h + L.status, sizeof(int32_t) * n);
    memcpy(fail_at, h + L.fail_at, sizeof(int32_t) * n);
    return SGO_OK;
}

int sgo_session_report(sgo_ctx *x, int n, const int32_t *slots, int K, int D, int32_t *status, int32_t *to_play,
                       int32_t *root_count, float *root_value, float *root_mean, int32_t *n_children, int32_t *N, float *Q,
                       float *P, int32_t *top_action, int32_t *pv, void *stream) {
    if (!x || n < 0 || (n && (!slots || !status)) || K < 0 || K > SGO_REPORT_MAX_TOP || D < 0 || D > SGO_REPORT_MAX_DEPTH) {
        set_error("sgo_session_report: bad argument (K <= SGO_REPORT_MAX_TOP, D <= SGO_REPORT_MAX_DEPTH)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const size_t rw = report_words(c.A, K, D), head = al8(sizeof(int32_t) * (size_t)n), body = sizeof(int32_t) * rw * n;
    const int rc = stage_session_list(x, "sgo_session_report", n, slots, head + body, st);
    if (rc != SGO_OK) return rc;
    uint8_t *h = x->h.sess_h, *d = x->h.sess_d;
    SGO_DISPATCH(c.S, k_session_report<kS><<<dim3(n), dim3(64), 0, st>>>(c, n, reinterpret_cast<const int32_t *>(d),
                                                                            reinterpret_cast<int32_t *>(d + head), K, D));
    SGO_HIP(hipGetLastError());
    SGO_HIP(hipMemcpyAsync(h + head, d + head, body, hipMemcpyDeviceToHost, st));       // the one copy back
    SGO_HIP(hipStreamSynchronize(st));
    const size_t A = (size_t)c.A;
    for (int i = 0; i < n; i++) {
        const int32_t *o = reinterpret_cast<const int32_t *>(h + head) + rw * i;
        const float *of = reinterpret_cast<const float *>(o);
        status[i] = o[0];
        if (o[0] != SGO_OK) continue;                       // the rows of a refused slot stay as the caller filled them
        if (to_play) to_play[i] = o[1];
        if (root_count) root_count[i] = o[2];
        if (root_value) root_value[i] = of[3];
        if (root_mean) root_mean[i] = of[4];
        if (n_children) n_children[i] = o[5];
        if (N) memcpy(N + A * i, o + 8, sizeof(int32_t) * A);
        if (Q) memcpy(Q + A * i, o + 8 + A, sizeof(float) * A);
        if (P) memcpy(P + A * i, o + 8 + 2 * A, sizeof(float) * A);
        if (top_action && K) memcpy(top_action + (size_t)K * i, o + 8 + 3 * A, sizeof(int32_t) * K);
        if (pv && K && D) memcpy(pv + (size_t)K * D * i, o + 8 + 3 * A + K, sizeof(int32_t) * K * D);
    }
    return SGO_OK;
}

int sgo_session_keys(sgo_ctx *x, int n, const int32_t *slots, int32_t *status, uint64_t *key0, uint64_t *canon, int32_t *mask,
                     void *stream) {
    if (!x || n < 0 || (n && (!slots || !status || !key0 || !canon || !mask))) { set_error("sgo_session_keys: bad argument"); return SGO_ERR_ARG; }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const RowCol cols[] = {{mask, sizeof(int32_t), 4}, {key0, sizeof(uint64_t), 8}, {canon, sizeof(uint64_t), 8}};
    return session_rows(x, "sgo_session_keys", n, slots, nullptr, 0, status, cols, st, [&](const int32_t *d_index, const uint8_t *, uint8_t *const *d) {
        return launch_keys(c.S, n, c.pos, ctx_records(c), d_index, nullptr, reinterpret_cast<uint64_t *>(d[1]), reinterpret_cast<uint64_t *>(d[2]),
                           reinterpret_cast<int32_t *>(d[0]), nullptr, st);
    });
}

int sgo_session_tactics(sgo_ctx *x, int n, const int32_t *slots, int max_chains, int32_t *status, uint8_t *libs, int32_t *n_chains,
                        int32_t *chains, void *stream) {
    if (!x || n < 0 || max_chains < 1 || max_chains > SGO_TACTICS_MAX_CHAINS || (n && (!slots || !status || !libs || !n_chains || !chains))) {
        set_error("sgo_session_tactics: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const size_t chain = sizeof(int32_t) * 8;
    // the chain rows behind min(n_chains, max_chains) were not written; n_chains stands before them, so its row is scattered first
    const RowCol cols[] = {{n_chains, sizeof(int32_t), 4},
                           {chains, chain * max_chains, 4, [=](int i) { return chain * (n_chains[i] < max_chains ? n_chains[i] : max_chains); }},
                           {libs, (size_t)c.S * c.S, 1}};
    return session_rows(x, "sgo_session_tactics", n, slots, nullptr, 0, status, cols, st, [&](const int32_t *d_index, const uint8_t *, uint8_t *const *d) {
        return launch_tactics(c.S, n, c.pos, ctx_records(c), d_index, max_chains, d[2], reinterpret_cast<int32_t *>(d[0]),
                              reinterpret_cast<int32_t *>(d[1]), st);
    });
}

int sgo_session_life(sgo_ctx *x, int n, const int32_t *slots, int32_t *status, uint32_t *sets, int32_t *counts, void *stream) {
    if (!x || n < 0 || (n && (!slots || !status || !sets || !counts))) { set_error("sgo_session_life: bad argument"); return SGO_ERR_ARG; }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const RowCol cols[] = {{counts, sizeof(int32_t) * 8, 4}, {sets, sizeof(uint32_t) * 4 * sgo_plane_words(c.S), 4}};
    return session_rows(x, "sgo_session_life", n, slots, nullptr, 0, status, cols, st, [&](const int32_t *d_index, const uint8_t *, uint8_t *const *d) {
        return launch_life(c.S, n, c.pos, ctx_records(c), d_index, reinterpret_cast<uint32_t *>(d[1]), reinterpret_cast<int32_t *>(d[0]), st);
    });
}

int sgo_session_shapes(sgo_ctx *x, int n, const int32_t *slots, const sgo_shape *shape, int32_t *status, int32_t *hits, uint32_t *cover,
                       void *stream) {
    if (!x || n < 0 || !shape || (n && (!slots || !status || !hits || !cover))) { set_error("sgo_session_shapes: bad argument"); return SGO_ERR_ARG; }
    const Ctx &c = x->c;
    uint32_t table[SGO_SHAPE_TABLE_WORDS];
    const int crc = session_shape_table(c.S, shape, table);
    if (crc != SGO_OK) return crc;
    if ((int)table[0] != c.S) { set_error("sgo_session_shapes: the table was compiled for another size"); return SGO_ERR_ARG; }
    if (n == 0) return SGO_OK;
    hipStream_t st = (hipStream_t)stream;
    const RowCol cols[] = {{hits, sizeof(int32_t) * 4, 4}, {cover, sizeof(uint32_t) * sgo_plane_words(c.S), 4}};
    return session_rows(x, "sgo_session_shapes", n, slots, table, sizeof(table), status, cols, st,
                        [&](const int32_t *d_index, const uint8_t *d_table, uint8_t *const *d) {
        return launch_shapes(c.S, n, c.pos, ctx_records(c), d_index, reinterpret_cast<const uint32_t *>(d_table), reinterpret_cast<int32_t *>(d[0]),
                             reinterpret_cast<uint32_t *>(d[1]), st);
    });
}

int sgo_session_moves(sgo_ctx *x, int n, const int32_t *slots, int side, int32_t *status, int16_t *moves, int32_t *counts, void *stream) {
    if (!x || n < 0 || (side != 0 && side != 1) || (n && (!slots || !status || !moves || !counts))) {
        set_error("sgo_session_moves: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const RowCol cols[] = {{counts, sizeof(int32_t) * 8, 4}, {moves, sizeof(int16_t) * 8 * c.S * c.S, 16}};     // k_moves stores 16 bytes at a time
    return session_rows(x, "sgo_session_moves", n, slots, nullptr, 0, status, cols, st, [&](const int32_t *d_index, const uint8_t *, uint8_t *const *d) {
        return launch_moves(c.S, n, c.pos, ctx_records(c), d_index, side, reinterpret_cast<int16_t *>(d[1]), reinterpret_cast<int32_t *>(d[0]), st);
    });
}

int sgo_session_secure(sgo_ctx *x, int n, const int32_t *slots, int side, int32_t *status, int16_t *table, uint32_t *sets, int32_t *counts,
                       void *stream) {
    if (!x || n < 0 || (side != 0 && side != 1) || (n && (!slots || !status || !table || !sets || !counts))) {
        set_error("sgo_session_secure: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const RowCol cols[] = {{counts, sizeof(int32_t) * 8, 4}, {sets, sizeof(uint32_t) * 4 * sgo_plane_words(c.S), 4},
                           {table, sizeof(int16_t) * 4 * c.S * c.S, 8}};                                        // k_secure stores 8 bytes at a time
    return session_rows(x, "sgo_session_secure", n, slots, nullptr, 0, status, cols, st, [&](const int32_t *d_index, const uint8_t *, uint8_t *const *d) {
        return launch_secure(c.S, n, c.pos, ctx_records(c), d_index, side, reinterpret_cast<int16_t *>(d[2]), reinterpret_cast<uint32_t *>(d[1]),
                             reinterpret_cast<int32_t *>(d[0]), st);
    });
}

int sgo_session_influence(sgo_ctx *x, int n, const int32_t *slots, const uint32_t *dead, int dilate, int erode_moyo, int erode_terr,
                          int32_t *status, int16_t *values, uint32_t *sets, int32_t *counts, void *stream) {
    if (!x || n < 0 || !influence_params_ok(dilate, erode_moyo, erode_terr) || (n && (!slots || !status || !values || !sets || !counts))) {
        set_error("sgo_session_influence: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const size_t plane = sizeof(uint32_t) * sgo_plane_words(c.S);
    const RowCol cols[] = {{counts, sizeof(int32_t) * 8, 4}, {sets, 4 * plane, 4}, {values, sizeof(int16_t) * c.S * c.S, 2}};
    return session_rows(x, "sgo_session_influence", n, slots, dead, plane * n, status, cols, st,
                        [&](const int32_t *d_index, const uint8_t *d_dead, uint8_t *const *d) {
        return launch_influence(c.S, n, c.pos, ctx_records(c), d_index, reinterpret_cast<const uint32_t *>(d_dead), dilate, erode_moyo, erode_terr,
                                reinterpret_cast<int16_t *>(d[2]), reinterpret_cast<uint32_t *>(d[1]), reinterpret_cast<int32_t *>(d[0]), st);
    });
}

int sgo_session_solve(sgo_ctx *x, int n, const int32_t *slots, const int32_t *ask, const uint32_t *region, int rules, int max_region,
                      int max_nodes, int max_targets, int32_t *status, int32_t *n_targets, int32_t *rows, uint32_t *regions, void *stream) {
    if (!x || n < 0 || !solve_params_ok(rules, max_region, max_nodes, max_targets) || (n && (!slots || !status || !n_targets || !rows || !regions))) {
        set_error("sgo_session_solve: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const size_t row = sizeof(int32_t) * 8, plane = sizeof(uint32_t) * sgo_plane_words(c.S), ab = al8(sizeof(int32_t) * (size_t)n);
    // the optional input block: ask [n] (enumerate where the caller gave none), then region [n][NW]
    std::vector<uint8_t> in;
    if (ask || region) {
        in.assign(ab + (region ? plane * n : 0), 0);
        int32_t *ha = reinterpret_cast<int32_t *>(in.data());
        for (int i = 0; i < n; i++) ha[i] = ask ? ask[i] : -1;
        if (region) memcpy(in.data() + ab, region, plane * n);
    }
    // the table rows and region sets behind min(n_targets, max_targets) were not written; n_targets stands before them
    const auto listed = [=](int i) { return (size_t)(n_targets[i] < max_targets ? n_targets[i] : max_targets); };
    const RowCol cols[] = {{n_targets, sizeof(int32_t), 4},
                           {rows, row * max_targets, 4, [=](int i) { return row * listed(i); }},
                           {regions, plane * max_targets, 4, [=](int i) { return plane * listed(i); }}};
    return session_rows(x, "sgo_session_solve", n, slots, in.empty() ? nullptr : in.data(), in.size(), status, cols, st,
                        [&](const int32_t *d_index, const uint8_t *d_in, uint8_t *const *d) {
        return launch_solve(c.S, n, c.pos, ctx_records(c), d_index, d_in ? reinterpret_cast<const int32_t *>(d_in) : nullptr,
                            (d_in && region) ? reinterpret_cast<const uint32_t *>(d_in + ab) : nullptr, rules, max_region, max_nodes, max_targets,
                            reinterpret_cast<int32_t *>(d[0]), reinterpret_cast<int32_t *>(d[1]), reinterpret_cast<uint32_t *>(d[2]), st);
    });
}

int sgo_session_race(sgo_ctx *x, int n, const int32_t *slots, const int32_t *ask, const uint32_t *region, int rules, int max_libs, int max_region,
                     int max_nodes, int max_pairs, int32_t *status, int32_t *n_pairs, int32_t *rows, uint32_t *regions, void *stream) {
    if (!x || n < 0 || !race_params_ok(rules, max_libs, max_region, max_nodes, max_pairs) || (n && (!slots || !status || !n_pairs || !rows || !regions))) {
        set_error("sgo_session_race: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const size_t row = sizeof(int32_t) * 16, plane = sizeof(uint32_t) * sgo_plane_words(c.S), ab = al8(sizeof(int32_t) * 2 * (size_t)n);
    // the optional input block: ask [n][2] (enumerate where the caller gave none), then region [n][NW]
    std::vector<uint8_t> in;
    if (ask || region) {
        in.assign(ab + (region ? plane * n : 0), 0);
        int32_t *ha = reinterpret_cast<int32_t *>(in.data());
        for (int i = 0; i < 2 * n; i++) ha[i] = ask ? ask[i] : -1;
        if (region) memcpy(in.data() + ab, region, plane * n);
    }
    // the table rows and region sets behind min(n_pairs, max_pairs) were not written; n_pairs stands before them
    const auto listed = [=](int i) { return (size_t)(n_pairs[i] < max_pairs ? n_pairs[i] : max_pairs); };
    const RowCol cols[] = {{n_pairs, sizeof(int32_t), 4},
                           {rows, row * max_pairs, 4, [=](int i) { return row * listed(i); }},
                           {regions, plane * max_pairs, 4, [=](int i) { return plane * listed(i); }}};
    return session_rows(x, "sgo_session_race", n, slots, in.empty() ? nullptr : in.data(), in.size(), status, cols, st,
                        [&](const int32_t *d_index, const uint8_t *d_in, uint8_t *const *d) {
        return launch_race(c.S, n, c.pos, ctx_records(c), d_index, d_in ? reinterpret_cast<const int32_t *>(d_in) : nullptr,
                           (d_in && region) ? reinterpret_cast<const uint32_t *>(d_in + ab) : nullptr, rules, max_libs, max_region, max_nodes,
                           max_pairs, reinterpret_cast<int32_t *>(d[0]), reinterpret_cast<int32_t *>(d[1]), reinterpret_cast<uint32_t *>(d[2]), st);
    });
}

int sgo_session_connect(sgo_ctx *x, int n, const int32_t *slots, const int32_t *ask, const uint32_t *region, int rules, int cut_libs, int max_region,
                        int max_nodes, int max_pairs, int32_t *status, int32_t *n_pairs, int32_t *rows, uint32_t *regions, int16_t *groups,
                        int32_t *group_counts, void *stream) {
    if (!x || n < 0 || !connect_params_ok(rules, cut_libs, max_region, max_nodes, max_pairs) ||
        (n && (!slots || !status || !n_pairs || !rows || !regions || !groups || !group_counts))) {
        set_error("sgo_session_connect: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const size_t row = sizeof(int32_t) * 12, plane = sizeof(uint32_t) * sgo_plane_words(c.S), ab = al8(sizeof(int32_t) * 2 * (size_t)n);
    // the optional input block: ask [n][2] (enumerate where the caller gave none), then region [n][NW]
    std::vector<uint8_t> in;
    if (ask || region) {
        in.assign(ab + (region ? plane * n : 0), 0);
        int32_t *ha = reinterpret_cast<int32_t *>(in.data());
        for (int i = 0; i < 2 * n; i++) ha[i] = ask ? ask[i] : -1;
        if (region) memcpy(in.data() + ab, region, plane * n);
    }
    // the table rows and region sets behind min(n_pairs, max_pairs) were not written; n_pairs stands before them
    const auto listed = [=](int i) { return (size_t)(n_pairs[i] < max_pairs ? n_pairs[i] : max_pairs); };
    const RowCol cols[] = {{n_pairs, sizeof(int32_t), 4},
                           {rows, row * max_pairs, 4, [=](int i) { return row * listed(i); }},
                           {regions, plane * max_pairs, 4, [=](int i) { return plane * listed(i); }},
                           {group_counts, sizeof(int32_t) * 4, 4},
                           {groups, sizeof(int16_t) * c.S * c.S, 2}};
    return session_rows(x, "sgo_session_connect", n, slots, in.empty() ? nullptr : in.data(), in.size(), status, cols, st,
                        [&](const int32_t *d_index, const uint8_t *d_in, uint8_t *const *d) {
        return launch_connect(c.S, n, c.pos, ctx_records(c), d_index, d_in ? reinterpret_cast<const int32_t *>(d_in) : nullptr,
                              (d_in && region) ? reinterpret_cast<const uint32_t *>(d_in + ab) : nullptr, rules, cut_libs, max_region, max_nodes,
                              max_pairs, reinterpret_cast<int32_t *>(d[0]), reinterpret_cast<int32_t *>(d[1]), reinterpret_cast<uint32_t *>(d[2]),
                              reinterpret_cast<int16_t *>(d[4]), reinterpret_cast<int32_t *>(d[3]), st);
    });
}

int sgo_session_playout(sgo_ctx *x, int n, const int32_t *slots, int per_row, uint32_t seed, int rules, int max_plies, int32_t *status,
                        int32_t *own, int32_t *amaf, int64_t *sums, void *stream) {
    if (!x || !playout_params_ok(x->c.S, n, per_row, rules, max_plies) || (n && (!slots || !status || !own || !sums))) {
        set_error("sgo_session_playout: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const size_t tb = sizeof(int32_t) * 2 * c.S * c.S;
    // without amaf the third column has no bytes and the kernel gets no table
    const RowCol cols[] = {{sums, sizeof(int64_t) * 8, 8}, {own, tb, 4}, {amaf ? amaf : own, amaf ? tb : 0, 4}};
    return session_rows(x, "sgo_session_playout", n, slots, nullptr, 0, status, cols, st, [&](const int32_t *d_index, const uint8_t *, uint8_t *const *d) {
        return launch_playout(c.S, n, c.pos, ctx_records(c), d_index, per_row, seed, rules, max_plies, reinterpret_cast<int32_t *>(d[1]),
                              amaf ? reinterpret_cast<int32_t *>(d[2]) : nullptr, reinterpret_cast<int64_t *>(d[0]), st);
    });
}

int sgo_session_uct(sgo_ctx *x, int n, const int32_t *slots, int trees, int sims, uint32_t seed, int rules, int max_plies, int komi2, int expand_at,
                    int rave_equiv, int prior, int max_nodes, int32_t *status, int32_t *visits, int32_t *wins2, int32_t *rave, int32_t *own,
                    int64_t *sums, int32_t *info, void *stream) {
    if (!x || !uct_params_ok(x->c.S, n, trees, sims, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes) ||
        (n && (!slots || !status || !visits || !wins2 || !sums || !info))) {
        set_error("sgo_session_uct: bad argument");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    const Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)c.S * c.S, tb = sizeof(int32_t) * (N + 1);
    // the workspace is this call's own; an optional table that was not asked for is a column without bytes
    void *work = nullptr;
    SGO_HIP(hipMalloc(&work, uct_work_bytes(c.S, n, trees, max_nodes)));
    const RowCol cols[] = {{sums, sizeof(int64_t) * 8, 8}, {visits, tb, 4}, {wins2, tb, 4}, {info, sizeof(int32_t) * 4, 4},
                           {rave ? rave : visits, rave ? 2 * tb : 0, 4}, {own ? own : visits, own ? sizeof(int32_t) * 2 * N : 0, 4}};
    const int rc = session_rows(x, "sgo_session_uct", n, slots, nullptr, 0, status, cols, st, [&](const int32_t *d_index, const uint8_t *, uint8_t *const *d) {
        return launch_uct(c.S, n, c.pos, ctx_records(c), d_index, trees, sims, seed, rules, max_plies, komi2, expand_at, rave_equiv, prior, max_nodes,
                          reinterpret_cast<int32_t *>(d[1]), reinterpret_cast<int32_t *>(d[2]), rave ? reinterpret_cast<int32_t *>(d[4]) : nullptr,
                          own ? reinterpret_cast<int32_t *>(d[5]) : nullptr, reinterpret_cast<int64_t *>(d[0]), reinterpret_cast<int32_t *>(d[3]),
                          nullptr, work, st);
    });
    if (rc != SGO_OK) (void)hipStreamSynchronize(st);                // session_rows synchronised when it succeeded
    (void)hipFree(work);
    return rc;
}

}  // extern "C"
