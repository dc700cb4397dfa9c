// sgo_conv4r.hpp -- third hand-written kernel for the residual tower's 3x3 / 256 -> 256 'same' convolution with bias (+ skip) +
// ReLU fused (model.py:37-46).  Same math, workgroup tile (256 pixels x 128 channels, 4 waves, two workgroups per CU), pixel
// window, masks and epilogue as sgo_conv4w.hpp; different OPERAND ROUTE for the weights:
//
//   k_conv4w: weights L2 -> LDS (DMA, double-buffered per K-tile) -> registers (ds_read_b128), two barriers per K-tile.  Per
//             K-tile a wave issues 24 fragment reads (16 pixel, 8 weight) and 4 DMA pieces; the CU's LDS is busy ~89 % of the
//             MFMA time (8 waves x 24 x 8 cycles + 36 KB of DMA writes per 2 048 cycles), and the ablations of round 3
//             (profiles/r03_conv4w_ablations.json) show the MFMA bursts waiting for exactly that.
//   k_conv4r: weights L2 / L1 -> REGISTERS, one global_load_dwordx4 per fragment, from a copy of the filter bank laid out in
//             fragment order (sgo_conv3x3_tower_prepack_dev: every load of a wave is 1 KB contiguous), three rotating 16-register
//             sets: in use / next / next-next.  The LDS carries the pixel window only (-1/3 of the fragment reads, no DMA writes
//             of weights: ~53 % busy), and the K loop has NO barrier except at the three chunk boundaries where the single-
//             buffered window is restaged (as in k_conv4w), so the four waves of a workgroup drift freely in between.
//
// Per K-tile t (tap T of 64-channel chunk cc), weights lo(t) / hi(t) = filters [0, 64) / [64, 128) of this wave's channel group,
// loads numbered L(2t) = lo(t), L(2t+1) = hi(t), load j into set j % 3:
//   phase A: issue L(2t+2) (set of hi(t-1), dead) | read pixel-lo fragments | vmcnt: L(2t) landed | 16 MFMA lo | vmcnt: L(2t+1)
//            landed | 16 MFMA hi
//   phase B: read pixel-hi fragments | 16 MFMA lo | issue L(2t+3) (set of lo(t), dead from here) | 16 MFMA hi
// A wave issues exactly eight weight loads per K-tile, so the counted waits are vmcnt(8) / vmcnt(4); chunk boundaries add the
// window pieces (see R4_TILE).  The last K-tile's two look-ahead loads read the 8 KB of padding behind the packed bank.
//
// RESULT (round 3, profiles/r03_conv4r_experiment.json): identical bits, and the same speed as k_conv4w within 1 % on every box
// (2.10-2.20 ms per 8 192 x 17 x 17 launch, 0.52 of the fp16 MFMA peak), wherever the loads are issued.  The route saves cycles
// (LDS instruction cycles -29 %, kernel cycles -0.8 %) and pays them back in clock: the chip is power-limited under this kernel,
// and 64 KB per K-tile pair through the vector-memory path costs frequency even though the duplicates hit in L1
// (profiles/r03_pmc_conv4r_ablate.json: the weight loads are 5 % of the cycles and 16 % of the time; the pixel reads 13 % / 16 %).
// It is kept as a selectable route (sgo_conv3x3_tower_packed_dev), not as the default.
//
// Tile decode, window staging, pixel fragment reads, masks and the epilogue are sgo_conv_tile.hpp's (shared with k_conv4w).
#pragma once
#include "sgo_conv_tile.hpp"

namespace sgo_conv4r {
using namespace sgo_conv_tile;   // vector types, CIN, COUT, ROWB, MAXW, LZ_BYTES, launch_geometry

constexpr int CT = 128;   // output channels per workgroup
// packed filter bank: [channel half 2][wave channel group 2][K-tile 36 = chunk-major, tap][lo / hi 2][nt 2][ks 2][lane 64][8 halves]
constexpr int WAVE_BANK = 36 * 8192, PACKED_BYTES = 4 * WAVE_BANK + 8192;
// LDS map: window (320 rows x 128 B), zero area; the epilogue reuses [0, 64 KiB)
constexpr int LW = 0, LZ = 40960, LDS_BYTES = 65536;

#define R4_VMWAITW(n) SGT_VMWAIT(n)   /* a wait for WEIGHT loads */

// VAR bit 0: s_setprio(1) around the MFMA bursts; bit 1: the look-ahead load of hi(t+1) is issued at the END of phase B instead
// of between its two MFMA groups; bit 4 (16): the loads spread inside the bursts (R4_TILE_S).  -DSGO_CONV4W_VARIANTS builds select
// 0, 3 and 17 (sgo_conv_packed_variant); 1 = default.  Every variant computes the same bits, and tests/test_conv_schedule.py
// models both tile forms.
// Retired variant bits (commit dbd02d8 is the last tree that contains their code), all timing-only ablations with wrong results:
// 4 no weight loads, 64 no pixel fragment reads (variants 5, 65, 69: profiles/r03_pmc_conv4r_ablate.json); 32 no window DMA in
// the prologue, 128 no restage and no barrier at the chunk boundaries (variants 33, 129, 197: profiles/r03_conv4r_experiment.json).
// Measured and dropped (round 3): a DOUBLE-BUFFERED window for board widths <= 17 (two 292-row buffers + the zero area = 81 152 B,
// two workgroups per CU still fit; the next chunk's pieces staged two per tap at the start of taps 0..4 with the lanes beyond the
// window masked off, ONE barrier per chunk boundary, no drain): bit-identical, 252 VGPRs, and 3.2 % SLOWER (2.180 vs 2.112 ms in
// one process, gpurun_out/r03bi_ab.log) although the boundaries' restage + barriers are worth 5.9 % when ablated away together
// (variant 129): what costs at the boundaries is the window DMA itself, not the synchronisation around it.
// (There is no "loads without waits" ablation: a load that lands after the compiler has given its registers to something else --
// an address, say -- corrupts it; the one run of such a variant ended in a memory access fault.)
template <bool HAS_SKIP, int VAR>
__global__ __launch_bounds__(256, 2) void k_conv4r(const char *__restrict__ xb, const char *__restrict__ wpk,
                                                    const _Float16 *__restrict__ bias, const char *__restrict__ skipb,
                                                    char *__restrict__ yb, int M, int H, int W, unsigned magicHW, unsigned magicW,
                                                    int pairs_q, int pairs_r) {
    __shared__ __attribute__((aligned(1024))) char smem[LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    SGT_TILE_DECODE();
    const int HW = H * W, HALO = W + 1, NROWS = 256 + 2 * HALO;

    SGT_ZERO_FILL();

    const int rowA = HALO + wr * 64 + (lane & 15);
    // this wave's slice of the packed bank: a scalar pointer that walks 4 KB per load group, plus lane * 16
    const char *wptr = wpk + (size_t)((chalf * 2 + wc) * WAVE_BANK);
    const int wlane = lane * 16;

    SGT_ACC_INIT();
    half8 pa[4][2];
    half8 ws[3][2][2];                                   // [set][nt][ks]

// one load group (4 KB: fragments [nt][ks] of 64 filters x 64 K) into set S; the scalar pointer moves on
#define R4_LOADW(S)                                                                                                     \
    do {                                                                                                                \
        asm volatile("global_load_dwordx4 %0, %4, %5\n\tglobal_load_dwordx4 %1, %4, %5 offset:1024\n\t"                 \
                     "global_load_dwordx4 %2, %4, %5 offset:2048\n\tglobal_load_dwordx4 %3, %4, %5 offset:3072"         \
                     : "=&v"(ws[S][0][0]), "=&v"(ws[S][0][1]), "=&v"(ws[S][1][0]), "=&v"(ws[S][1][1])                   \
                     : "v"(wlane), "s"(wptr)                                                                            \
                     : "memory");                                                                                       \
        wptr += 4096;                                                                                                   \
    } while (0)
// behind the counted wait after which set S holds its fragments: the set is tied there, so that nothing that uses it (and no
// copy of it) is placed above the wait
#define R4_TIEW(S) asm volatile("" : "+v"(ws[S][0][0]), "+v"(ws[S][0][1]), "+v"(ws[S][1][0]), "+v"(ws[S][1][1])::"memory")
#define R4_MFMA(QM, QN, S)                                                                             \
    _Pragma("unroll") for (int ks_ = 0; ks_ < 2; ks_++) _Pragma("unroll") for (int mt_ = 0; mt_ < 4; mt_++) \
        _Pragma("unroll") for (int nt_ = 0; nt_ < 2; nt_++) acc[QM][QN][mt_][nt_] =                    \
            __builtin_amdgcn_mfma_f32_16x16x32_f16(ws[S][nt_][ks_], pa[mt_][ks_], acc[QM][QN][mt_][nt_], 0, 0, 0)
// vmcnt(base + nlate): the late window pieces of a chunk boundary (3..6 per wave) are among the younger loads
#define R4_VMWAIT_LATE(base)                                                      \
    do {                                                                          \
        if (nlate == 6) { R4_VMWAIT_SUM(base, 6); }                               \
        else if (nlate == 5) { R4_VMWAIT_SUM(base, 5); }                          \
        else if (nlate == 4) { R4_VMWAIT_SUM(base, 4); }                          \
        else { R4_VMWAIT_SUM(base, 0); }                                          \
    } while (0)
#define R4_VMWAIT_SUM(a, b) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((a) + (b)) : "memory")

// One K-tile, tap T of chunk cc (runtime); the set indices depend on T only (9 cc = 0 mod 3).
#define R4_TILE(T)                                                                                        \
    do {                                                                                                  \
        constexpr int SLO_ = (2 * (T)) % 3, SHI_ = (2 * (T) + 1) % 3, SNX_ = (2 * (T) + 2) % 3;           \
        int swid = wid;                                                                                   \
        asm volatile("" : "+s"(swid));                                                                    \
        const bool boundary_ = (T) == 8 && cc < 3;  /* last tap of a chunk that has a successor */        \
        const bool restaged_ = (T) == 0 && cc > 0;  /* first tap on a restaged window */                  \
        /* ---- phase A */                                                                                \
        R4_LOADW(SNX_);                           /* L(2t+2) = lo(t+1) */                                  \
        SGT_READ_A(0, T);                                                                                 \
        SGT_LGKM0();                                                                                      \
        /* L(2t) has landed; younger: L(2t+1), L(2t+2) -- and, on a restaged window, the boundary's late pieces, which are */ \
        /* older than L(2t+1) and get until the next wait to land */                                      \
        if (restaged_) R4_VMWAIT_LATE(8);                                                                 \
        else R4_VMWAITW(8);                                                                               \
        R4_TIEW(SLO_);                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if (boundary_) {                                                                                  \
            /* every wave has read window rows [0, 128) for the last time (phase B of the last tap, shift +W+1, reads rows */ \
            /* >= 128 + 2 (W + 1) only): pieces 0..15 take the next chunk's window one phase early, 4 DMAs per wave */ \
            SGT_BARRIER();                                                                                \
            SGT_STAGE_WP((cc + 1) * 128, 0, 4);                                                           \
        }                                                                                                 \
        SGT_PRIO(VAR & 1);                                                                                \
        R4_MFMA(0, 0, SLO_);                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        /* L(2t+1) has landed; younger: L(2t+2) and a boundary tap's four early pieces */                 \
        if (boundary_) SGT_VMWAIT(8);                                                                     \
        else R4_VMWAITW(4);                                                                               \
        R4_TIEW(SHI_);                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        R4_MFMA(0, 1, SHI_);                                                                              \
        SGT_PRIO(0);                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if (restaged_) {                                                                                  \
            /* phase A read the early rows [0, 128) only; every wave's late pieces were retired by its vmcnt(4) above */ \
            SGT_BARRIER();                                                                                \
        }                                                                                                 \
        /* ---- phase B */                                                                                \
        SGT_READ_A(1, T);                                                                                 \
        SGT_LGKM0();                                                                                      \
        if (boundary_) {                                                                                  \
            SGT_BARRIER();                         /* this chunk's window reads are retired in every wave */ \
            SGT_STAGE_WP((cc + 1) * 128, 4, 10);                                                          \
        }                                                                                                 \
        SGT_PRIO(VAR & 1);                                                                                \
        R4_MFMA(1, 0, SLO_);                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if (!(VAR & 2)) R4_LOADW(SLO_);           /* L(2t+3) = hi(t+1) into the set lo(t) has just left */ \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        R4_MFMA(1, 1, SHI_);                                                                              \
        SGT_PRIO(0);                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if (VAR & 2) R4_LOADW(SLO_);                                                                      \
        if (boundary_) {                                                                                  \
            /* the next tap's phase A reads window rows [0, 128) = the EARLY pieces; younger: the late pieces and L(2t+3) */ \
            R4_VMWAIT_LATE(4);                                                                            \
            SGT_BARRIER();                                                                                \
        }                                                                                                 \
    } while (0)

// ---- VAR bit 4 (16): the weight loads are issued BETWEEN the MFMAs of a burst, one 1-KB piece behind every 8th (phase A:
// L(2t+2)) or 4th (second half of phase B: L(2t+3)) MFMA, instead of in groups of four at a phase start / in mid-burst: a VMEM
// instruction costs its wave tens of issue cycles, which beside a running MFMA (16 cycles, 8 of them holding the issue port) are
// hidden, and in the read interval between two bursts are not.
#define R4_LOADP(S, P)                                                                                                  \
    do {                                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3"                                         \
                                     : "=&v"(ws[S][(P) >> 1][(P) & 1]) : "v"(wlane), "s"(wptr), "n"((P) * 1024) : "memory"); \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
    } while (0)
#define R4_M1(QM, QN, S, I)                                                                                             \
    acc[QM][QN][((I) >> 1) & 3][(I) & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(                                      \
        ws[S][(I) & 1][(I) >> 3], pa[((I) >> 1) & 3][(I) >> 3], acc[QM][QN][((I) >> 1) & 3][(I) & 1], 0, 0, 0)
#define R4_M2(QM, QN, S, I) R4_M1(QM, QN, S, I); R4_M1(QM, QN, S, (I) + 1)
#define R4_M4(QM, QN, S, I) R4_M2(QM, QN, S, I); R4_M2(QM, QN, S, (I) + 2)
// 16 MFMAs with pieces P0, P0 + 1 of set LS behind the 4th and the 12th
#define R4_G2(QM, QN, S, LS, P0)                                                                                        \
    do {                                                                                                                \
        R4_M4(QM, QN, S, 0); R4_LOADP(LS, P0); R4_M4(QM, QN, S, 4); R4_M4(QM, QN, S, 8); R4_LOADP(LS, (P0) + 1);        \
        R4_M4(QM, QN, S, 12);                                                                                           \
    } while (0)
// 16 MFMAs with all four pieces of set LS behind the 2nd, 6th, 10th and 14th
#define R4_G4(QM, QN, S, LS)                                                                                            \
    do {                                                                                                                \
        R4_M2(QM, QN, S, 0); R4_LOADP(LS, 0); R4_M4(QM, QN, S, 2); R4_LOADP(LS, 1); R4_M4(QM, QN, S, 6); R4_LOADP(LS, 2); \
        R4_M4(QM, QN, S, 10); R4_LOADP(LS, 3); R4_M2(QM, QN, S, 14);                                                    \
    } while (0)
#define R4_TILE_S(T)                                                                                      \
    do {                                                                                                  \
        constexpr int SLO_ = (2 * (T)) % 3, SHI_ = (2 * (T) + 1) % 3, SNX_ = (2 * (T) + 2) % 3;           \
        int swid = wid;                                                                                   \
        asm volatile("" : "+s"(swid));                                                                    \
        const bool boundary_ = (T) == 8 && cc < 3;                                                        \
        const bool restaged_ = (T) == 0 && cc > 0;                                                        \
        /* ---- phase A */                                                                                \
        SGT_READ_A(0, T);                                                                                 \
        SGT_LGKM0();                                                                                      \
        /* L(2t) has landed; younger: L(2t+1) -- and, on a restaged window, the boundary's late pieces before it */ \
        if (restaged_) R4_VMWAIT_LATE(4);                                                                 \
        else R4_VMWAITW(4);                                                                               \
        R4_TIEW(SLO_);                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if (boundary_) {                                                                                  \
            SGT_BARRIER();                                                                                \
            SGT_STAGE_WP((cc + 1) * 128, 0, 4);                                                           \
        }                                                                                                 \
        SGT_PRIO(VAR & 1);                                                                                \
        R4_G2(0, 0, SLO_, SNX_, 0);               /* + L(2t+2) pieces 0, 1 */                              \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        /* L(2t+1) has landed; younger: two pieces of L(2t+2), before them a boundary tap's four early window pieces */ \
        if (boundary_) SGT_VMWAIT(6);                                                                     \
        else R4_VMWAITW(2);                                                                               \
        R4_TIEW(SHI_);                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        R4_G2(0, 1, SHI_, SNX_, 2);               /* + L(2t+2) pieces 2, 3 */                              \
        wptr += 4096;                                                                                     \
        SGT_PRIO(0);                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if (restaged_) {                                                                                  \
            SGT_BARRIER();                         /* every wave's late pieces were retired by its vmcnt(2) above */ \
        }                                                                                                 \
        /* ---- phase B */                                                                                \
        SGT_READ_A(1, T);                                                                                 \
        SGT_LGKM0();                                                                                      \
        if (boundary_) {                                                                                  \
            SGT_BARRIER();                                                                                \
            SGT_STAGE_WP((cc + 1) * 128, 4, 10);                                                          \
        }                                                                                                 \
        SGT_PRIO(VAR & 1);                                                                                \
        R4_MFMA(1, 0, SLO_);                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        R4_G4(1, 1, SHI_, SLO_);                  /* + L(2t+3) = hi(t+1) into the set lo(t) has just left */ \
        wptr += 4096;                                                                                     \
        SGT_PRIO(0);                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if (boundary_) {                                                                                  \
            /* the early pieces have landed; younger: L(2t+2), the late pieces, L(2t+3) */                \
            R4_VMWAIT_LATE(8);                                                                            \
            SGT_BARRIER();                                                                                \
        }                                                                                                 \
    } while (0)

    SGT_NLATE();

    // ---- prologue: window of chunk 0, weights of K-tile 0
    {
        int swid = wid;
        SGT_STAGE_WP(0, 0, 10);
        R4_LOADW(0);
        R4_LOADW(1);
    }
    SGT_MASKS();
    SGT_VMWAIT(8);                                       // the window has landed; in flight: L(0), L(1)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the zero area
    SGT_BARRIER();

#pragma nounroll
    for (int cc = 0; cc < 4; cc++) {
        if constexpr ((VAR & 16) != 0) {
            R4_TILE_S(0); R4_TILE_S(1); R4_TILE_S(2); R4_TILE_S(3); R4_TILE_S(4);
            R4_TILE_S(5); R4_TILE_S(6); R4_TILE_S(7); R4_TILE_S(8);
        } else {
            R4_TILE(0); R4_TILE(1); R4_TILE(2); R4_TILE(3); R4_TILE(4);
            R4_TILE(5); R4_TILE(6); R4_TILE(7); R4_TILE(8);
        }
    }
    // the last K-tile's look-ahead loads (padding bytes) must not land in registers the epilogue has taken over
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(ws[0][0][0]), "+v"(ws[0][0][1]), "+v"(ws[0][1][0]), "+v"(ws[0][1][1]), "+v"(ws[1][0][0]), "+v"(ws[1][0][1]),
                   "+v"(ws[1][1][0]), "+v"(ws[1][1][1]), "+v"(ws[2][0][0]), "+v"(ws[2][0][1]), "+v"(ws[2][1][0]), "+v"(ws[2][1][1])::"memory");
    SGT_BARRIER();   // every wave is done with the window: the LDS becomes the output stage

    SGT_EPILOGUE();
}

// filter bank OHWI [256][3][3][256] fp16 -> fragment order (see PACKED_BYTES): one thread per 16-byte piece
__global__ void k_prepack(const char *__restrict__ w, char *__restrict__ wp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // piece index in the packed bank
    if (i >= 4 * WAVE_BANK / 16) {
        if (i < PACKED_BYTES / 16) reinterpret_cast<intx4 *>(wp)[i] = intx4{0, 0, 0, 0};
        return;
    }
    const int lane = i & 63, ks = (i >> 6) & 1, nt = (i >> 7) & 1, qn = (i >> 8) & 1;
    const int t = (i >> 9) % 36, g = (i >> 9) / 36;               // g = chalf * 2 + wc
    const int cc = t / 9, T = t % 9;
    const int filter = (g >> 1) * 128 + qn * 64 + (g & 1) * 32 + nt * 16 + (lane & 15);
    const int ci = cc * 64 + ks * 32 + (lane >> 4) * 8;
    reinterpret_cast<intx4 *>(wp)[i] = *reinterpret_cast<const intx4 *>(w + ((size_t)(filter * 9 + T) * CIN + ci) * 2);
}

static inline int prepack(const void *w, void *wp, hipStream_t st) {
    const int pieces = PACKED_BYTES / 16;
    hipLaunchKernelGGL(k_prepack, dim3((pieces + 255) / 256), dim3(256), 0, st, (const char *)w, (char *)wp);
    return 0;
}

template <int VAR>
static inline int launch_var(int n, int h, int w, const void *x, const void *wpk, const void *bias, const void *skip, void *y,
                             hipStream_t st) {
    launch_geom g;
    if (!launch_geometry(n, h, w, g)) return -1;
#define R4_ARGS (const char *)x, (const char *)wpk, (const _Float16 *)bias, (const char *)skip, (char *)y, g.M, h, w, g.magic_hw, g.magic_w, g.xcd_q, g.xcd_r
    if (skip) hipLaunchKernelGGL((k_conv4r<true, VAR>), grid_pairs(g), dim3(256), 0, st, R4_ARGS);
    else hipLaunchKernelGGL((k_conv4r<false, VAR>), grid_pairs(g), dim3(256), 0, st, R4_ARGS);
#undef R4_ARGS
    return 0;
}

static inline int launch(int n, int h, int w, const void *x, const void *wpk, const void *bias, const void *skip, void *y,
                         hipStream_t st, int var = 1) {
    switch (var) {
#ifdef SGO_CONV4W_VARIANTS
    case 0: return launch_var<0>(n, h, w, x, wpk, bias, skip, y, st);
    case 3: return launch_var<3>(n, h, w, x, wpk, bias, skip, y, st);
    case 17: return launch_var<17>(n, h, w, x, wpk, bias, skip, y, st);      // loads spread inside the bursts
#endif
    default: return launch_var<1>(n, h, w, x, wpk, bias, skip, y, st);
    }
}

}  // namespace sgo_conv4r

#undef R4_MFMA
#undef R4_TILE
#undef R4_VMWAITW
#undef R4_VMWAIT_LATE
#undef R4_VMWAIT_SUM
#undef R4_LOADW
#undef R4_TIEW
#undef R4_LOADP
#undef R4_M1
#undef R4_M2
#undef R4_M4
#undef R4_G2
#undef R4_G4
#undef R4_TILE_S
#include "sgo_conv_tile_undef.hpp"
