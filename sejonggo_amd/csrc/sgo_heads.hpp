// sgo_heads.hpp -- k_heads: the policy and value heads of the resident net (model.py:62-95 of the reference) as ONE hand-written
// gfx950 kernel.  Input: the tower's output y [n][t][t][256] fp16 NHWC (t = S - 2); output: policy [n][S*S+1] f32 (softmax) and
// value [n] f32 (tanh).  It replaces the eight framework launches of net.FusedInferenceNet._tower_and_heads (a GEMM for the two
// 1x1 convolutions, reshapes, three F.linear, softmax, tanh) behind sgo_heads_dev.
//
// ARITHMETIC CONTRACT (tests/test_gpu_heads.py and tests/test_heads_rounding_model.py rest on it):
//   * every accumulation is fp32;
//   * h = relu(conv1x1(y) + bias) is rounded to fp16 ONCE (it is an MFMA operand);
//   * the logits, v1 = relu(v_fc1 . h + b), the pre-tanh value, the softmax and the tanh stay fp32;
//   * the softmax subtracts the row maximum;
//   * the library's flags apply (-ffp-contract=off, no fast-math); the 1x1 convolutions use explicit fmaf.
//
// One 256-thread workgroup owns a tile of 16 positions (the N of v_mfma_f32_16x16x32_f16 here: positions sit on the MFMA's
// columns, FC outputs on its rows).
//   phase 1  streams the tile's t*t*256 fp16 activations from HBM exactly once: the tile is one contiguous range, a wave-load is
//            1 KB = 2 pixels (16 B per lane, lane = 8 channels), four to eight loads in flight per wave.  Each lane forms its share of the
//            four dot products (p0 p1 v0 v1) with fmaf, a 6-shuffle reduce-scatter sums the 32 lanes of a pixel, and the lane
//            that ends up with output o writes h (fp16) into LDS in Keras' flatten order k = pixel * 2 + channel.  The LDS rows
//            are zeroed first, so the K padding (and the rows of a partial tile) are zeros, not stale bits.
//   phase 2  runs both wide FC layers on MFMA: B = h from LDS (ds_read_b128, row pitch (KP + 8) halves: the 16 rows of a
//            fragment read fall on 16 distinct 4-bank groups), A = the bank in FRAGMENT ORDER [n-tile][k-step][lane][8 halves],
//            so every weight fragment is one contiguous 1-KB global load (the pattern of sgo_conv3x3_tower_prepack_dev).  K is
//            zero-padded to a multiple of 32 and each layer's N to a multiple of 16.  N-tiles are dealt round-robin to the 4 waves;
//            the accumulators stay in registers.
//   phase 3  (VALU) adds the biases; the logits go to LDS (over the dead h rows) and each wave soft-maxes 4 positions with wave
//            reductions; v1 is folded into v_fc2 (256 -> 1) in registers, summed over lanes, then over the waves in a fixed
//            order (no atomics: the bits do not depend on timing), and tanh'd.
// Rows >= n of a partial last tile are neither read nor written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgo_heads {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 16;      // positions per workgroup
constexpr int C = 256;        // tower channels
constexpr int THREADS = 256;
constexpr int V1 = 256;       // width of v_fc1

template <int S>
struct geom {
    static constexpr int T = S - 2, T2 = T * T, K = 2 * T2, KP = (K + 31) / 32 * 32, KS = KP / 32, A = S * S + 1;
    static constexpr int NPT = (A + 15) / 16, NVT = V1 / 16, NT = NPT + NVT;      // n-tiles: policy first, then value
    static constexpr int NI = (NT + 3) / 4;                                       // n-tiles per wave
    static constexpr int ROWH = KP + 8;                                           // halves per LDS row of h
    static constexpr int H_BYTES = TILE * ROWH * 2;                               // one of the two h arrays (policy / value)
    static constexpr int LGW = NPT * 16;                                          // floats per LDS row of logits
    static constexpr int LG_BYTES = TILE * LGW * 4;
    static constexpr int LDS_BYTES = 2 * H_BYTES > LG_BYTES ? 2 * H_BYTES : LG_BYTES;
    static constexpr long BANK_BYTES = (long)NT * KS * 1024;
};

// fragment (nt, ks), lane l, element j  =  W[out = 16 * nt' + (l & 15)][k = 32 * ks + 8 * (l >> 4) + j], zero outside the layer
template <int S>
__global__ void k_heads_prepack(const _Float16 *__restrict__ pw, const _Float16 *__restrict__ vw, char *__restrict__ bank) {
    using G = geom<S>;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G::NT * G::KS * 64) return;
    const int lane = i & 63, f = i >> 6, ks = f % G::KS, nt = f / G::KS;
    const bool pol = nt < G::NPT;
    const _Float16 *src = pol ? pw : vw;
    const int out = (pol ? nt : nt - G::NPT) * 16 + (lane & 15), nout = pol ? G::A : V1;
    half8 v;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int k = ks * 32 + (lane >> 4) * 8 + j;
        v[j] = (out < nout && k < G::K) ? src[(size_t)out * G::K + k] : (_Float16)0;
    }
    reinterpret_cast<half8 *>(bank)[i] = v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <int S>
__global__ __launch_bounds__(THREADS) void k_heads(const char *__restrict__ y, const _Float16 *__restrict__ head_w,
                                                   const _Float16 *__restrict__ head_b, const char *__restrict__ bank,
                                                   const _Float16 *__restrict__ p_fc_b, const _Float16 *__restrict__ v_fc1_b,
                                                   const _Float16 *__restrict__ v_fc2_w, const _Float16 *__restrict__ v_fc2_b,
                                                   float *__restrict__ policy, float *__restrict__ value, int n) {
    using G = geom<S>;
    __shared__ __attribute__((aligned(16))) char smem[G::LDS_BYTES];
    __shared__ float vpart[4][TILE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * TILE;
    const int R = (n - row0 < TILE) ? n - row0 : TILE;       // rows of this tile that exist

    // ---- phase 0: h = 0 (K padding and absent rows must be zeros: zero weights do not neutralise stale NaN / Inf bits)
    for (int i = tid; i < 2 * G::H_BYTES / 16; i += THREADS) reinterpret_cast<intx4 *>(smem)[i] = intx4{0, 0, 0, 0};

    // this lane's 8 channels of the four 1x1 filters, and the bias of the output it will own after the reduce-scatter
    const int c0 = (lane & 31) * 8;
    float w[4][8];
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const half8 hw = *reinterpret_cast<const half8 *>(head_w + o * C + c0);
#pragma unroll
        for (int j = 0; j < 8; j++) w[o][j] = (float)hw[j];
    }
    const bool b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
    const int o_lane = (b4 ? 2 : 0) + (b3 ? 1 : 0);
    const float hb = (float)head_b[o_lane];
    __syncthreads();

    // ---- phase 1: the 1x1 convolutions, y read once
    const int P = R * G::T2;                                  // pixels of this tile: one contiguous range of y
    const char *yt = y + (size_t)row0 * G::T2 * (C * 2) + c0 * 2;
    // four 1-KB loads per wave and step, the next step's issued before this step's arithmetic
    auto load4 = [&](half8(&d)[4], int base) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int pix = base + 2 * u + (lane >> 5);
            d[u] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (pix < P) d[u] = __builtin_nontemporal_load(reinterpret_cast<const half8 *>(yt + (size_t)pix * (C * 2)));
        }
    };
    half8 x[4], xn[4];
    load4(x, wid * 8);
    for (int base = wid * 8; base < P; base += 32) {
        load4(xn, base + 32);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int pix = base + 2 * u + (lane >> 5);
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float xv = (float)x[u][j];
#pragma unroll
                for (int o = 0; o < 4; o++) s[o] = __builtin_fmaf(xv, w[o][j], s[o]);
            }
            // reduce-scatter over the 32 lanes of the pixel: lane bits 4, 3 select the output a lane keeps, bits 2..0 are summed
            float a = b4 ? s[2] : s[0], b = b4 ? s[3] : s[1];
            a += __shfl_xor(b4 ? s[0] : s[2], 16);
            b += __shfl_xor(b4 ? s[1] : s[3], 16);
            float c = (b3 ? b : a) + __shfl_xor(b3 ? a : b, 8);
            c += __shfl_xor(c, 4);
            c += __shfl_xor(c, 2);
            c += __shfl_xor(c, 1);
            if ((lane & 7) == 0 && pix < P) {
                const int pos = pix / G::T2, px = pix - pos * G::T2;
                const float hs = c + hb;
                const float h = __builtin_elementwise_maximum(hs, 0.f);   // IEEE maximum: passes NaN on (fmaxf would return the 0)
                // flatten order k = pixel * 2 + channel; outputs 0, 1 -> policy rows, 2, 3 -> value rows
                *reinterpret_cast<_Float16 *>(smem + (o_lane >> 1) * G::H_BYTES + (pos * G::ROWH + px * 2 + (o_lane & 1)) * 2) = (_Float16)h;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = xn[u];
    }
    __syncthreads();

    // ---- phase 2: logits^T [A x 16] and v1^T [256 x 16] on MFMA; wave `wid` takes n-tiles wid, wid + 4, ...
    floatx4 acc[G::NI];
#pragma unroll
    for (int i = 0; i < G::NI; i++) {
        const int nt = wid + 4 * i;
        acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (i < G::NI - 1 || nt < G::NT) {                    // only a wave's last n-tile can be absent
            const char *hrow = smem + (nt < G::NPT ? 0 : G::H_BYTES) + ((lane & 15) * G::ROWH + (lane >> 4) * 8) * 2;
            const char *bp = bank + ((size_t)nt * G::KS * 64 + lane) * 16;
#pragma unroll
            for (int ks = 0; ks < G::KS; ks++) {
                const half8 wf = *reinterpret_cast<const half8 *>(bp + ks * 1024);
                const half8 hf = *reinterpret_cast<const half8 *>(hrow + ks * 64);
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, hf, acc[i], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                          // every wave has read h for the last time: the LDS becomes the logits

    // ---- phase 3: biases, v_fc2, softmax, tanh.  Lane l holds outputs 16 * nt' + 4 * (l >> 4) + r of position l & 15.
    float *lg = reinterpret_cast<float *>(smem);
    const int pos_l = lane & 15, q = lane >> 4;
    float vp = 0.f;
#pragma unroll
    for (int i = 0; i < G::NI; i++) {
        const int nt = wid + 4 * i;
        if (nt >= G::NT) continue;
        if (nt < G::NPT) {
            const int out0 = nt * 16 + q * 4;
            floatx4 v;
#pragma unroll
            for (int r = 0; r < 4; r++) v[r] = acc[i][r] + ((out0 + r < G::A) ? (float)p_fc_b[out0 + r] : 0.f);
            *reinterpret_cast<floatx4 *>(lg + pos_l * G::LGW + out0) = v;
        } else {
            const int out0 = (nt - G::NPT) * 16 + q * 4;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float vs = acc[i][r] + (float)v_fc1_b[out0 + r];
                const float v1 = __builtin_elementwise_maximum(vs, 0.f);  // NaN passes, as above
                vp += v1 * (float)v_fc2_w[out0 + r];
            }
        }
    }
    vp += __shfl_xor(vp, 16);
    vp += __shfl_xor(vp, 32);
    if (lane < TILE) vpart[wid][lane] = vp;
    __syncthreads();

    if (tid < R) {
        const float v = ((vpart[0][tid] + vpart[1][tid]) + vpart[2][tid]) + vpart[3][tid] + (float)v_fc2_b[0];
        value[row0 + tid] = tanhf(v);
    }
    constexpr int NV = (G::A + 63) / 64;
#pragma unroll
    for (int pi = 0; pi < TILE / 4; pi++) {
        const int pos = wid * (TILE / 4) + pi;
        if (pos >= R) break;
        float v[NV], m = -INFINITY;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int a = lane + 64 * j;
            v[j] = (a < G::A) ? lg[pos * G::LGW + a] : -INFINITY;
            m = fmaxf(m, v[j]);
        }
        m = wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            v[j] = (lane + 64 * j < G::A) ? expf(v[j] - m) : 0.f;
            sum += v[j];
        }
        sum = wave_sum(sum);
        float *prow = policy + (size_t)(row0 + pos) * G::A;
#pragma unroll
        for (int j = 0; j < NV; j++)
            if (lane + 64 * j < G::A) prow[lane + 64 * j] = v[j] / sum;
    }
}

template <int S>
static inline long bank_bytes() { return geom<S>::BANK_BYTES; }

template <int S>
static inline void prepack(const void *pw, const void *vw, void *bank, hipStream_t st) {
    const int pieces = geom<S>::NT * geom<S>::KS * 64;
    hipLaunchKernelGGL(k_heads_prepack<S>, dim3((pieces + 255) / 256), dim3(256), 0, st, (const _Float16 *)pw, (const _Float16 *)vw,
                       (char *)bank);
}

template <int S>
static inline void launch(int n, const void *y, const void *head_w, const void *head_b, const void *bank, const void *p_fc_b,
                          const void *v_fc1_b, const void *v_fc2_w, const void *v_fc2_b, float *policy, float *value, hipStream_t st) {
    hipLaunchKernelGGL(k_heads<S>, dim3((n + TILE - 1) / TILE), dim3(THREADS), 0, st, (const char *)y, (const _Float16 *)head_w,
                       (const _Float16 *)head_b, (const char *)bank, (const _Float16 *)p_fc_b, (const _Float16 *)v_fc1_b,
                       (const _Float16 *)v_fc2_w, (const _Float16 *)v_fc2_b, policy, value, n);
}

}  // namespace sgo_heads
