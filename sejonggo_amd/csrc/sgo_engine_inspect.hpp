// sgo_engine_inspect.hpp -- HOST code used by tests and tools only; nothing here runs in a step.  Included at the end of
// sgo_engine.hip (it needs sgo_ctx and the kernels).  A snapshot of one game's blocks walked on the host (sgo_root_table,
// sgo_tree_serialize, sgo_tree_dump, sgo_game_board), the raw block-accounting dumps (sgo_debug_block_state,
// sgo_debug_pool_state) and the debug entry points (sgo_debug_counters, sgo_debug_top_one, sgo_advance_timing).
#pragma once

extern "C" {

struct Snap {
    GameState s;
    std::vector<float> P, W, Q;
    std::vector<int32_t> N, B;
    std::vector<uint8_t> busy;
    std::vector<uint32_t> legal;
    std::vector<double> p64;
    std::vector<int32_t> ovf;     // the game's row of the overflow map
};
// physical block behind local id `blk` of game g, given the game's row of the overflow map
static size_t host_phys(const Ctx &c, int g, int blk, const std::vector<int32_t> &ovf) {
    if (blk < c.cap) return (size_t)g * c.cap + blk;
    return (size_t)c.G * c.cap + (size_t)ovf[blk - c.cap];
}
static int ovf_row(Ctx &c, int g, std::vector<int32_t> &ovf) {
    ovf.assign((size_t)c.ovf_cap, -1);
    if (c.ovf_cap > 0)
        SGO_HIP(hipMemcpy(ovf.data(), c.ovfMap + (size_t)g * c.ovf_cap, sizeof(int32_t) * c.ovf_cap, hipMemcpyDeviceToHost));
    return SGO_OK;
}
static int snapshot(Ctx &c, int g, Snap &sn) {
    SGO_HIP(hipDeviceSynchronize());
    SGO_HIP(hipMemcpy(&sn.s, c.gs + g, sizeof(GameState), hipMemcpyDeviceToHost));
    if (sn.s.error) { set_error("this slot's game failed (its tree was abandoned and its shared blocks released)"); return SGO_ERR_STATE; }
    CK(ovf_row(c, g, sn.ovf));
    int hi = 0;                                            // local ids [0, cap + hi) may hold blocks
    for (int j = 0; j < c.ovf_cap; j++)
        if (sn.ovf[j] >= 0) hi = j + 1;
    const size_t nb = (size_t)c.cap + hi, ns = nb * c.APAD;
    sn.P.resize(ns); sn.W.resize(ns); sn.Q.resize(ns); sn.N.resize(ns); sn.B.resize(ns); sn.busy.resize(ns);
    sn.legal.resize(nb * c.NW); sn.p64.resize(c.APAD);
    // the private region in one piece, then every backed overflow block on its own
    auto pull = [&](size_t dst_blk, size_t src_blk, size_t n_blk) -> int {
        const size_t k = n_blk * c.APAD, d = dst_blk * c.APAD, o = src_blk * c.APAD;
        SGO_HIP(hipMemcpy(sn.P.data() + d, c.cP + o, sizeof(float) * k, hipMemcpyDeviceToHost));
        SGO_HIP(hipMemcpy(sn.W.data() + d, c.cW + o, sizeof(float) * k, hipMemcpyDeviceToHost));
        SGO_HIP(hipMemcpy(sn.Q.data() + d, c.cQ + o, sizeof(float) * k, hipMemcpyDeviceToHost));
        SGO_HIP(hipMemcpy(sn.N.data() + d, c.cN + o, sizeof(int32_t) * k, hipMemcpyDeviceToHost));
        SGO_HIP(hipMemcpy(sn.B.data() + d, c.cB + o, sizeof(int32_t) * k, hipMemcpyDeviceToHost));
        SGO_HIP(hipMemcpy(sn.busy.data() + d, c.cBusy + o, k, hipMemcpyDeviceToHost));
        SGO_HIP(hipMemcpy(sn.legal.data() + dst_blk * c.NW, c.legal + src_blk * c.NW, sizeof(uint32_t) * n_blk * c.NW, hipMemcpyDeviceToHost));
        return SGO_OK;
    };
    CK(pull(0, (size_t)g * c.cap, c.cap));
    for (int j = 0; j < hi; j++)
        if (sn.ovf[j] >= 0) CK(pull((size_t)c.cap + j, (size_t)c.G * c.cap + sn.ovf[j], 1));
    SGO_HIP(hipMemcpy(sn.p64.data(), c.rootP64 + (size_t)g * c.APAD, sizeof(double) * c.APAD, hipMemcpyDeviceToHost));
    return SGO_OK;
}
static bool snap_exists(const Ctx &c, const Snap &sn, int blk, int i) {
    return (sn.legal[(size_t)blk * c.NW + (i >> 5)] >> (i & 31)) & 1u;
}

/* Test hooks (tests/block_audit.py): the raw tree-block accounting of one slot and of the context, copied and not interpreted.
 * hdr[20] = {phase, error, root_blk, other_root, free_top, min_free, ovf_hi, fifo_head, fifo_tail, cap, L, ovf_cap, APAD, NW, E,
 * rows, A, 2 * MAXE, 0, 0}; rows = cap + hi block rows follow (hi as in snapshot(): 1 + the highest backed map index), 0 for a
 * failed slot, whose block arrays are left out.  Any array pointer may be NULL (a first call with hdr alone gives the sizes);
 * rows of overflow ids that are not backed are left as the caller filled them. */
int sgo_debug_block_state(sgo_ctx *x, int slot, int32_t *hdr, int32_t *free_list, int32_t *ovf_map, int32_t *b_parent,
                          int32_t *b_slot, int32_t *c_b, uint32_t *legal, int32_t *fifo) {
    if (!x || slot < 0 || slot >= x->c.G || !hdr) { set_error("sgo_debug_block_state: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    SGO_HIP(hipDeviceSynchronize());
    GameState s;
    SGO_HIP(hipMemcpy(&s, c.gs + slot, sizeof s, hipMemcpyDeviceToHost));
    std::vector<int32_t> ovf;
    CK(ovf_row(c, slot, ovf));
    int hi = 0;
    for (int j = 0; j < c.ovf_cap; j++)
        if (ovf[j] >= 0) hi = j + 1;
    const int rows = s.error ? 0 : c.cap + hi;
    auto backed = [&](int j) { return ovf[j] >= 0 && ovf[j] < c.pool_blocks; };   // a map entry beyond the pool has no row to copy
    const int32_t h[20] = {s.phase, s.error, s.root_blk, s.other_root, s.free_top, s.min_free, s.ovf_hi, s.fifo_head, s.fifo_tail,
                           c.cap, c.L, c.ovf_cap, c.APAD, c.NW, c.E, rows, c.A, 2 * MAXE, 0, 0};
    memcpy(hdr, h, sizeof h);
    if (ovf_map && c.ovf_cap > 0) memcpy(ovf_map, ovf.data(), sizeof(int32_t) * c.ovf_cap);
    if (s.error) return SGO_OK;
    if (free_list) SGO_HIP(hipMemcpy(free_list, c.freeList + (size_t)slot * c.L, sizeof(int32_t) * c.L, hipMemcpyDeviceToHost));
    auto pull = [&](size_t dst, size_t src, size_t n) -> int {
        if (b_parent) SGO_HIP(hipMemcpy(b_parent + dst, c.bParent + src, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        if (b_slot) SGO_HIP(hipMemcpy(b_slot + dst, c.bSlot + src, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        if (c_b) SGO_HIP(hipMemcpy(c_b + dst * c.APAD, c.cB + src * c.APAD, sizeof(int32_t) * n * c.APAD, hipMemcpyDeviceToHost));
        if (legal) SGO_HIP(hipMemcpy(legal + dst * c.NW, c.legal + src * c.NW, sizeof(uint32_t) * n * c.NW, hipMemcpyDeviceToHost));
        return SGO_OK;
    };
    const bool want_rows = b_parent || b_slot || c_b || legal;
    if (want_rows) CK(pull(0, (size_t)slot * c.cap, c.cap));
    // every backed overflow block on its own, as snapshot() does
    for (int j = 0; want_rows && j < hi; j++)
        if (backed(j)) CK(pull((size_t)c.cap + j, (size_t)c.G * c.cap + ovf[j], 1));
    if (fifo) {                                            // [4][2 * MAXE]: fParent, fSlot, fBlk, fEvaluated
        const int32_t *src[4] = {c.fParent, c.fSlot, c.fBlk, c.fEvaluated};
        for (int k = 0; k < 4; k++)
            SGO_HIP(hipMemcpy(fifo + (size_t)k * 2 * MAXE, src[k] + (size_t)slot * 2 * MAXE, sizeof(int32_t) * 2 * MAXE, hipMemcpyDeviceToHost));
    }
    return SGO_OK;
}

/* hdr[4] = {poolCtl[0], poolCtl[1], poolCtl[2], pool_blocks}; pool_free / pool_ret (pool_blocks entries each) may be NULL */
int sgo_debug_pool_state(sgo_ctx *x, int32_t *hdr, int32_t *pool_free, int32_t *pool_ret) {
    if (!x || !hdr) { set_error("sgo_debug_pool_state: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    SGO_HIP(hipDeviceSynchronize());
    SGO_HIP(hipMemcpy(hdr, c.poolCtl, sizeof(int32_t) * 3, hipMemcpyDeviceToHost));
    hdr[3] = (int32_t)c.pool_blocks;
    if (pool_free && c.pool_blocks > 0) SGO_HIP(hipMemcpy(pool_free, c.poolFree, sizeof(int32_t) * c.pool_blocks, hipMemcpyDeviceToHost));
    if (pool_ret && c.pool_blocks > 0) SGO_HIP(hipMemcpy(pool_ret, c.poolRet, sizeof(int32_t) * c.pool_blocks, hipMemcpyDeviceToHost));
    return SGO_OK;
}

int sgo_root_table(sgo_ctx *x, int slot, int32_t *N, float *W, float *Q, double *P, int8_t *EX, int32_t *root_count,
                   float *root_value) {
    if (!x || slot < 0 || slot >= x->c.G) { set_error("sgo_root_table: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    Snap sn;
    CK(snapshot(c, slot, sn));
    const int rb = sn.s.root_blk;
    std::vector<int32_t> bslot(1);
    SGO_HIP(hipMemcpy(bslot.data(), c.bSlot + host_phys(c, slot, rb, sn.ovf), sizeof(int32_t), hipMemcpyDeviceToHost));
    const bool expanded = bslot[0] != -2;
    for (int a = 0; a < c.A; a++) {
        const size_t o = (size_t)rb * c.APAD + a;
        bool ex = expanded && snap_exists(c, sn, rb, a);
        if (N) N[a] = ex ? sn.N[o] : 0;
        if (W) W[a] = ex ? sn.W[o] : 0;
        if (Q) Q[a] = ex ? sn.Q[o] : 0;
        if (P) P[a] = ex ? (sn.s.root_f64 ? sn.p64[a] : (double)sn.P[o]) : 0;
        if (EX) EX[a] = ex ? 1 : 0;
    }
    if (root_count) *root_count = sn.s.root_count;
    if (root_value) *root_value = sn.s.root_value;
    return SGO_OK;
}

static void ser_rec(const Ctx &c, const Snap &sn, int blk, bool f64, uint8_t *buf, int64_t cap, int64_t &off, int64_t &nn,
                    int64_t &ne, int depth = -1) {
    const int rec = depth >= 0 ? 40 : 32;   // depth >= 0: extended 40-byte records (+ i depth, i pad) for sgo_tree_dump
    for (int a = 0; a < c.A; a++) {
        if (!snap_exists(c, sn, blk, a)) continue;
        const size_t o = (size_t)blk * c.APAD + a;
        const int32_t cb = sn.B[o];
        if (buf && off + rec <= cap) {
            int32_t i32;
            double p = f64 ? sn.p64[a] : (double)sn.P[o];
            if (depth >= 0) { i32 = depth; memcpy(buf + off + 32, &i32, 4); i32 = 0; memcpy(buf + off + 36, &i32, 4); }
            i32 = a; memcpy(buf + off, &i32, 4);
            i32 = sn.N[o]; memcpy(buf + off + 4, &i32, 4);
            memcpy(buf + off + 8, &sn.W[o], 4);
            memcpy(buf + off + 12, &sn.Q[o], 4);
            memcpy(buf + off + 16, &p, 8);
            i32 = sn.busy[o]; memcpy(buf + off + 24, &i32, 4);
            i32 = cb >= 0 ? 1 : 0; memcpy(buf + off + 28, &i32, 4);
        }
        off += rec;
        nn++;
        if (cb >= 0) { ne++; ser_rec(c, sn, cb, false, buf, cap, off, nn, ne, depth >= 0 ? depth + 1 : -1); }
    }
}

int64_t sgo_tree_serialize(sgo_ctx *x, int slot, uint8_t *buf, int64_t cap, int64_t *n_nodes, int64_t *n_expanded) {
    if (!x || slot < 0 || slot >= x->c.G) { set_error("sgo_tree_serialize: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    Snap sn;
    CK(snapshot(c, slot, sn));
    int32_t bslot = 0;
    SGO_HIP(hipMemcpy(&bslot, c.bSlot + host_phys(c, slot, sn.s.root_blk, sn.ovf), sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t off = 0, nn = 0, ne = 0;
    if (bslot != -2) ser_rec(c, sn, sn.s.root_blk, sn.s.root_f64 != 0, buf, cap, off, nn, ne);
    if (n_nodes) *n_nodes = nn;
    if (n_expanded) *n_expanded = ne;
    return off;
}

int64_t sgo_tree_dump(sgo_ctx *x, int slot, uint8_t *buf, int64_t cap, int64_t *n_nodes) {
    if (!x || slot < 0 || slot >= x->c.G) { set_error("sgo_tree_dump: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    Snap sn;
    CK(snapshot(c, slot, sn));
    int32_t bslot = 0;
    SGO_HIP(hipMemcpy(&bslot, c.bSlot + host_phys(c, slot, sn.s.root_blk, sn.ovf), sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t off = 0, nn = 0, ne = 0;
    if (bslot != -2) ser_rec(c, sn, sn.s.root_blk, sn.s.root_f64 != 0, buf, cap, off, nn, ne, 0);
    if (n_nodes) *n_nodes = nn;
    return off;
}

int sgo_game_board(sgo_ctx *x, int slot, int32_t *board17) {
    if (!x || slot < 0 || slot >= x->c.G || !board17) { set_error("sgo_game_board: bad argument"); return SGO_ERR_ARG; }
    Ctx &c = x->c;
    SGO_HIP(hipDeviceSynchronize());
    GameState s;
    SGO_HIP(hipMemcpy(&s, c.gs + slot, sizeof s, hipMemcpyDeviceToHost));
    int32_t *d = nullptr;
    const size_t bsz = sizeof(int32_t) * (size_t)c.S * c.S * 17;
    SGO_HIP(hipMalloc((void **)&d, bsz));
    std::vector<int32_t> ovf;
    CK(ovf_row(c, slot, ovf));
    int r = sgo_unpack_dev(c.S, 1, c.pos + host_phys(c, slot, s.root_blk, ovf) * c.RW, d, nullptr);
    if (r == SGO_OK) {
        hipError_t e = hipMemcpy(board17, d, bsz, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = hip_fail(e, "hipMemcpy", __FILE__, __LINE__);
    }
    (void)hipFree(d);
    return r;
}

/* Diagnostic: cycles per phase of k_search summed over games and calls (zeros unless built with -DSGO_KSEARCH_PROFILE):
 * [0] consuming evaluations (expand), [1] round set-up, [2] selection, [7] the round's back-propagation, [3] the move step,
 * [4] wave-calls. */
int sgo_debug_counters(sgo_ctx *x, unsigned long long *out, int n) {
    if (!x || !out || n < 0) return SGO_ERR_ARG;
    Counters h;
    SGO_HIP(hipMemcpy(&h, x->c.counters, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < n && i < 8; i++) out[i] = h.dbg[i];
    return SGO_OK;
}

/* Test hook (tests/test_gpu_selector.py): Eng<S>::top_one on caller-supplied child tables.  Flat [n_cases][A] DEVICE arrays;
 * the cases run in chunks of the context's game count, case k of a chunk in the root block of slot k, whose contents it
 * replaces -- so the context must have no game in flight, and trees of finished games are gone afterwards. */
int sgo_debug_top_one(sgo_ctx *x, int n_cases, const float *P32, const double *P64, const int32_t *N, const float *Q,
                      const int8_t *busy, const uint8_t *legal, int f64, int32_t *out, void *stream) {
    if (!x || n_cases < 0 || !P32 || !N || !Q || !busy || !legal || !out || (f64 && !P64)) {
        set_error("sgo_debug_top_one: bad argument");
        return SGO_ERR_ARG;
    }
    Ctx &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    SGO_HIP(hipSetDevice(c.cfg.device_id));
    SGO_HIP(hipDeviceSynchronize());
    std::vector<GameState> all(c.G);
    SGO_HIP(hipMemcpy(all.data(), c.gs, sizeof(GameState) * c.G, hipMemcpyDeviceToHost));
    for (int g = 0; g < c.G; g++)
        if (all[g].phase == PH_WAIT_ROOT || all[g].phase == PH_SEARCH) {
            set_error("sgo_debug_top_one: the context has games in flight (the hook overwrites the root block of every slot)");
            return SGO_ERR_STATE;
        }
    for (int c0 = 0; c0 < n_cases; c0 += c.G) {
        const int n = std::min(c.G, n_cases - c0);
        const size_t o = (size_t)c0 * c.A;
        SGO_DISPATCH(c.S, k_debug_top_one<kS><<<dim3(n), dim3(64), 0, st>>>(c, n, P32 + o, f64 ? P64 + o : nullptr, N + o, Q + o,
                                                                            busy + o, legal + o, f64, out + c0));
        SGO_HIP(hipGetLastError());
    }
    return SGO_OK;
}

int sgo_advance_timing(sgo_ctx *x, double *total_ms, int64_t *launches, int64_t *positions) {
    if (!x) { set_error("sgo_advance_timing: bad argument"); return SGO_ERR_ARG; }
    if (total_ms) *total_ms = x->h.adv_ms;
    if (launches) *launches = x->h.adv_launches;
    if (positions) *positions = x->h.adv_positions;
    x->h.adv_ms = 0; x->h.adv_launches = 0; x->h.adv_positions = 0;
    return SGO_OK;
}

}  // extern "C"
