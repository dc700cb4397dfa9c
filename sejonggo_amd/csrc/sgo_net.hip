// sgo_net.hip -- the heads of the resident net as one kernel (sgo_heads.hpp: sgo_heads_dev) and the whole-net forward behind the
// C ABI (sgo_net_*): the stem from packed records, 2 * n_blocks tower launches and k_heads, queued on the caller's stream through
// the library's own entry points, so that a caller of include/sgo.h evaluates positions without a framework or a BLAS library.
#include <vector>

#include "sgo_common.hpp"
#include "sgo_heads.hpp"

extern "C" long sgo_heads_packed_bytes(int S) {
    long b = -1;
    SGO_DISPATCH(S, b = sgo_heads::bank_bytes<kS>());
    return b;
}

extern "C" int sgo_heads_prepack_dev(int S, const void *d_p_fc_w, const void *d_v_fc1_w, void *d_bank, void *stream) {
    using namespace sgo;
    if (!size_ok(S) || !d_p_fc_w || !d_v_fc1_w || !d_bank || ((uintptr_t)d_bank & 15) || (((uintptr_t)d_p_fc_w | (uintptr_t)d_v_fc1_w) & 1)) {
        set_error("sgo_heads_prepack_dev: S in {5, 7, 9, 13, 19}, p_fc_w [S*S+1][2 t t] and v_fc1_w [256][2 t t] fp16, bank "
                  "(sgo_heads_packed_bytes(S)) 16-byte aligned");
        return SGO_ERR_ARG;
    }
    SGO_DISPATCH(S, sgo_heads::prepack<kS>(d_p_fc_w, d_v_fc1_w, d_bank, (hipStream_t)stream));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

extern "C" int sgo_heads_dev(int S, int n, const void *d_y, const void *d_head_w, const void *d_head_b, const void *d_bank,
                             const void *d_p_fc_b, const void *d_v_fc1_b, const void *d_v_fc2_w, const void *d_v_fc2_b,
                             float *d_policy, float *d_value, void *stream) {
    using namespace sgo;
    if (!size_ok(S) || n < 0 || !d_y || !d_head_w || !d_head_b || !d_bank || !d_p_fc_b || !d_v_fc1_b || !d_v_fc2_w || !d_v_fc2_b ||
        !d_policy || !d_value) {
        set_error("sgo_heads_dev: bad argument (S in {5, 7, 9, 13, 19}, n >= 0, no null pointer)");
        return SGO_ERR_ARG;
    }
    if ((((uintptr_t)d_y | (uintptr_t)d_head_w | (uintptr_t)d_bank) & 15) || (((uintptr_t)d_policy | (uintptr_t)d_value) & 3) ||
        (((uintptr_t)d_head_b | (uintptr_t)d_p_fc_b | (uintptr_t)d_v_fc1_b | (uintptr_t)d_v_fc2_w | (uintptr_t)d_v_fc2_b) & 1)) {
        set_error("sgo_heads_dev: y, head_w and the bank must be 16-byte aligned (the kernel moves 16 B per lane)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    SGO_DISPATCH(S, sgo_heads::launch<kS>(n, d_y, d_head_w, d_head_b, d_bank, d_p_fc_b, d_v_fc1_b, d_v_fc2_w, d_v_fc2_b, d_policy,
                                          d_value, (hipStream_t)stream));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

// ---- the resident net ---------------------------------------------------------------------------------------------------------
namespace {
constexpr long CH = 256;
constexpr long CONV_W_BYTES = CH * 9 * CH * 2, BIAS_BYTES = CH * 2;

// Makes `device` current for a scope and puts the caller's device back: allocations and copies of a net happen on ITS device, and
// the calling thread (a multi-GPU framework process, say) keeps the one it had.
struct device_scope {
    int prev = -1;
    bool ok = false;
    explicit device_scope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~device_scope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
}

struct sgo_net {
    int S = 0, t = 0, A = 0, n_blocks = 0, max_batch = 0, device = 0;
    bool packed = false, have_weights = false;
    void *stem_w10 = nullptr, *stem_b = nullptr, *stem_wcol = nullptr;
    std::vector<void *> w1, b1, w2, b2, bank1, bank2;
    void *head_w = nullptr, *head_b = nullptr, *p_fc_w = nullptr, *p_fc_b = nullptr, *v_fc1_w = nullptr, *v_fc1_b = nullptr,
         *v_fc2_w = nullptr, *v_fc2_b = nullptr, *heads_bank = nullptr;
    void *act[3] = {nullptr, nullptr, nullptr};
    std::vector<void *> owned;

    long stem_w10_bytes() const { return CH * 10 * 16 * 2; }
    long p_fc_w_bytes() const { return (long)A * 2 * t * t * 2; }
    long v_fc1_w_bytes() const { return 256L * 2 * t * t * 2; }
    bool alloc(void **p, long bytes) {
        if (hipMalloc(p, (size_t)bytes) != hipSuccess) { *p = nullptr; return false; }
        owned.push_back(*p);
        return true;
    }
};

extern "C" void sgo_net_destroy(sgo_net *net) {
    if (!net) return;
    device_scope dev(net->device);
    for (void *p : net->owned) (void)hipFree(p);
    delete net;
}

extern "C" sgo_net *sgo_net_create(int S, int n_blocks, int max_batch, int device_id) {
    using namespace sgo;
    if (!size_ok(S) || n_blocks < 1 || max_batch < 1) {
        set_error("sgo_net_create: S in {5, 7, 9, 13, 19}, n_blocks >= 1, max_batch >= 1 (256 channels, 'valid' stem)");
        return nullptr;
    }
    device_scope dev(device_id);
    if (!dev.ok) { set_error("sgo_net_create: hipSetDevice failed (no HIP device?)"); return nullptr; }
    sgo_net *x = new sgo_net();
    x->S = S; x->t = S - 2; x->A = S * S + 1; x->n_blocks = n_blocks; x->max_batch = max_batch; x->device = device_id;
    x->w1.resize(n_blocks); x->b1.resize(n_blocks); x->w2.resize(n_blocks); x->b2.resize(n_blocks);
    const long act_bytes = (long)max_batch * x->t * x->t * CH * 2;
    bool ok = x->alloc(&x->stem_w10, x->stem_w10_bytes()) && x->alloc(&x->stem_b, BIAS_BYTES) && x->alloc(&x->stem_wcol, CH * 4);
    for (int i = 0; ok && i < n_blocks; i++)
        ok = x->alloc(&x->w1[i], CONV_W_BYTES) && x->alloc(&x->b1[i], BIAS_BYTES) && x->alloc(&x->w2[i], CONV_W_BYTES) && x->alloc(&x->b2[i], BIAS_BYTES);
    ok = ok && x->alloc(&x->head_w, 4 * CH * 2) && x->alloc(&x->head_b, 4 * 2) && x->alloc(&x->p_fc_w, x->p_fc_w_bytes()) &&
         x->alloc(&x->p_fc_b, x->A * 2) && x->alloc(&x->v_fc1_w, x->v_fc1_w_bytes()) && x->alloc(&x->v_fc1_b, 256 * 2) &&
         x->alloc(&x->v_fc2_w, 256 * 2) && x->alloc(&x->v_fc2_b, 2) && x->alloc(&x->heads_bank, sgo_heads_packed_bytes(S));
    for (int i = 0; ok && i < 3; i++) ok = x->alloc(&x->act[i], act_bytes);
    if (!ok) {
        set_error("sgo_net_create: out of device memory");
        sgo_net_destroy(x);
        return nullptr;
    }
    return x;
}

namespace {
int prepack_tower(sgo_net *net, void *stream) {
    for (int i = 0; i < net->n_blocks; i++) {
        int rc = sgo_conv3x3_tower_prepack_dev(net->w1[i], net->bank1[i], stream);
        if (rc == SGO_OK) rc = sgo_conv3x3_tower_prepack_dev(net->w2[i], net->bank2[i], stream);
        if (rc != SGO_OK) return rc;
    }
    return SGO_OK;
}
}  // namespace

extern "C" int sgo_net_packed_tower(sgo_net *net, int on, void *stream) {
    using namespace sgo;
    if (!net || (on != 0 && on != 1)) { set_error("sgo_net_packed_tower: null net, or `on` is neither 0 nor 1"); return SGO_ERR_ARG; }
    if (on) {
        device_scope dev(net->device);
        if (!dev.ok) { set_error("sgo_net_packed_tower: hipSetDevice failed"); return SGO_ERR_HIP; }
        // banks that a failed earlier call did allocate are kept and used: only the missing ones are allocated
        net->bank1.resize(net->n_blocks, nullptr);
        net->bank2.resize(net->n_blocks, nullptr);
        for (int i = 0; i < net->n_blocks; i++)
            if ((!net->bank1[i] && !net->alloc(&net->bank1[i], sgo_conv3x3_tower_packed_bytes())) ||
                (!net->bank2[i] && !net->alloc(&net->bank2[i], sgo_conv3x3_tower_packed_bytes()))) {
                set_error("sgo_net_packed_tower: out of device memory");
                return SGO_ERR_HIP;
            }
        if (net->have_weights) {
            const int rc = prepack_tower(net, stream);
            if (rc != SGO_OK) return rc;
        }
    }
    net->packed = on != 0;
    return SGO_OK;
}

extern "C" int sgo_net_set_weights(sgo_net *net, const sgo_net_weights *w, void *stream) {
    using namespace sgo;
    if (!net || !w || !w->stem_w10 || !w->stem_b || !w->stem_wcol || !w->block_w1 || !w->block_b1 || !w->block_w2 || !w->block_b2 ||
        !w->head_w || !w->head_b || !w->p_fc_w || !w->p_fc_b || !w->v_fc1_w || !w->v_fc1_b || !w->v_fc2_w || !w->v_fc2_b) {
        set_error("sgo_net_set_weights: null net, weights or field");
        return SGO_ERR_ARG;
    }
    for (int i = 0; i < net->n_blocks; i++)
        if (!w->block_w1[i] || !w->block_b1[i] || !w->block_w2[i] || !w->block_b2[i]) {
            set_error("sgo_net_set_weights: null block tensor");
            return SGO_ERR_ARG;
        }
    device_scope dev(net->device);
    if (!dev.ok) { set_error("sgo_net_set_weights: hipSetDevice failed"); return SGO_ERR_HIP; }
    hipStream_t st = (hipStream_t)stream;
#define NET_COPY(dst, src, bytes) SGO_HIP(hipMemcpyAsync(dst, src, (size_t)(bytes), hipMemcpyDefault, st))
    NET_COPY(net->stem_w10, w->stem_w10, net->stem_w10_bytes());
    NET_COPY(net->stem_b, w->stem_b, BIAS_BYTES);
    NET_COPY(net->stem_wcol, w->stem_wcol, CH * 4);
    for (int i = 0; i < net->n_blocks; i++) {
        NET_COPY(net->w1[i], w->block_w1[i], CONV_W_BYTES);
        NET_COPY(net->b1[i], w->block_b1[i], BIAS_BYTES);
        NET_COPY(net->w2[i], w->block_w2[i], CONV_W_BYTES);
        NET_COPY(net->b2[i], w->block_b2[i], BIAS_BYTES);
    }
    NET_COPY(net->head_w, w->head_w, 4 * CH * 2);
    NET_COPY(net->head_b, w->head_b, 4 * 2);
    NET_COPY(net->p_fc_w, w->p_fc_w, net->p_fc_w_bytes());
    NET_COPY(net->p_fc_b, w->p_fc_b, net->A * 2);
    NET_COPY(net->v_fc1_w, w->v_fc1_w, net->v_fc1_w_bytes());
    NET_COPY(net->v_fc1_b, w->v_fc1_b, 256 * 2);
    NET_COPY(net->v_fc2_w, w->v_fc2_w, 256 * 2);
    NET_COPY(net->v_fc2_b, w->v_fc2_b, 2);
#undef NET_COPY
    int rc = sgo_heads_prepack_dev(net->S, net->p_fc_w, net->v_fc1_w, net->heads_bank, stream);
    if (rc != SGO_OK) return rc;
    net->have_weights = true;
    if (net->packed) rc = prepack_tower(net, stream);
    return rc;
}

extern "C" int sgo_net_predict_packed_dev(sgo_net *net, int n, const uint32_t *d_records, const int32_t *d_index, int sym_k,
                                          const int32_t *d_sym_k, float *d_policy, float *d_value, void *stream) {
    using namespace sgo;
    if (!net || n < 0 || !d_records || !d_policy || !d_value || sym_k < 0 || sym_k > 7) {
        set_error("sgo_net_predict_packed_dev: bad argument");
        return SGO_ERR_ARG;
    }
    if (!net->have_weights) { set_error("sgo_net_predict_packed_dev: sgo_net_set_weights has not been called"); return SGO_ERR_STATE; }
    const int S = net->S, t = net->t, words = sgo_packed_words(S);
    for (int n0 = 0; n0 < n; n0 += net->max_batch) {
        const int nn = (n - n0 < net->max_batch) ? n - n0 : net->max_batch;
        // without an index list the rows are records 0..n-1: a slice starts at its own record
        const uint32_t *rec = d_index ? d_records : d_records + (size_t)n0 * words;
        const int32_t *idx = d_index ? d_index + n0 : nullptr;
        void *y = net->act[0], *z = net->act[1], *y2 = net->act[2];
        int rc = sgo_stem_packed_dev(S, nn, rec, idx, sym_k, d_sym_k, net->stem_w10, net->stem_b, (const float *)net->stem_wcol, y, stream);
        for (int i = 0; rc == SGO_OK && i < net->n_blocks; i++) {
            if (net->packed) {
                rc = sgo_conv3x3_tower_packed_dev(nn, t, t, y, net->bank1[i], net->b1[i], nullptr, z, stream);
                if (rc == SGO_OK) rc = sgo_conv3x3_tower_packed_dev(nn, t, t, z, net->bank2[i], net->b2[i], y, y2, stream);
            } else {
                rc = sgo_conv3x3_tower_dev(nn, t, t, y, net->w1[i], net->b1[i], nullptr, z, stream);
                if (rc == SGO_OK) rc = sgo_conv3x3_tower_dev(nn, t, t, z, net->w2[i], net->b2[i], y, y2, stream);
            }
            void *tmp = y; y = y2; y2 = tmp;
        }
        if (rc == SGO_OK)
            rc = sgo_heads_dev(S, nn, y, net->head_w, net->head_b, net->heads_bank, net->p_fc_b, net->v_fc1_b, net->v_fc2_w,
                               net->v_fc2_b, d_policy + (size_t)n0 * net->A, d_value + n0, stream);
        if (rc != SGO_OK) return rc;
    }
    return SGO_OK;
}
