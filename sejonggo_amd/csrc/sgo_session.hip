// sgo_session.hip -- interactive (session) slots of the self-play engine: sgo_session_play and sgo_session_genmove, the
// "interactive games" section of include/sgo.h.  sgo_session_open is a restart and lives beside sgo_start_games in sgo_engine.hip;
// the kernels are in sgo_session.hpp.  What it replaces of the reference (drsagitn/sejonggo): sejonggo_nomodel.py:20-100, the
// SejongGoEngine a GTP front-end drives.
#include <string.h>
#include <vector>

#include "sgo_engine_state.hpp"
#include "sgo_session.hpp"

using namespace sgo;

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
    Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    StageLayout L;
    const int rc = stage_slots(x, "sgo_session_genmove", n, slots, nullptr, nullptr, L, st);
    if (rc != SGO_OK) return rc;
    k_session_arm<<<dim3(1), dim3(1024), 0, st>>>(c, n, L);
    SGO_HIP(hipGetLastError());
    int32_t *hs = reinterpret_cast<int32_t *>(x->h.stage + L.first);
    SGO_HIP(hipMemcpyAsync(hs, c.stage + L.first, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SGO_HIP(hipStreamSynchronize(st));
    if (hs[0] != SGO_OK) { set_error("sgo_session_genmove: a listed slot is not a holding session; nothing was armed"); return hs[0]; }
    return SGO_OK;
}

}  // extern "C"
