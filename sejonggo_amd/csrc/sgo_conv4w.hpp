// sgo_conv4w.hpp -- second hand-written kernel for the residual tower's 3x3 / 256 -> 256 'same' convolution with bias
// (+ skip) + ReLU fused (model.py:37-46).  Same math, layouts and per-wave MFMA tile as sgo_conv8w.hpp; different
// OCCUPANCY model:
//
//   k_conv8w: one 512-thread workgroup per CU (256 pixels x 256 channels, 150 KiB of LDS).  Its prologue (7.4k cycles) and
//             epilogue (11.5k) run with the CU's MFMA pipes idle -- 17 % of a tile's 109k cycles -- because nothing else
//             fits on the CU beside it.
//   k_conv4w: 256-thread workgroups of 256 pixels x 128 channels (4 waves = 2 pixel groups x 2 channel groups, one wave per
//             SIMD) in 78 KiB of LDS, so TWO workgroups share a CU: while one is in its prologue / epilogue / a staging
//             bubble, the other one's waves issue MFMAs on the same SIMDs.  The price: the pixel window is single-buffered
//             (restaged at the three chunk boundaries behind the last tap's MFMAs) and staged once per channel half
//             (L2 -> LDS bytes per MAC +12 %).
//
// Per K-tile (tap T of 64-channel chunk cc; weights buffer BUF = K-tile parity), all four waves in step:
//   phase A: read chan-lo, chan-hi fragments (weights[t]) and pixel-lo fragments | barrier (buffer of weights[t] is free)
//            | 32 MFMA
//   phase B: read pixel-hi fragments | stage weights[t+2] into the freed buffer | vmcnt(4): weights[t+1] have landed
//            | barrier (they are visible) | [last tap of a chunk: stage the next chunk's window] | 32 MFMA
//            | [last tap of a chunk: vmcnt(0), barrier]
// A wave issues exactly four weight DMAs per K-tile, so the counted wait is always vmcnt(4); chunk boundaries drain.
//
// Tile decode, window staging, pixel fragment reads, masks and the epilogue are sgo_conv_tile.hpp's (shared with k_conv4r).
#pragma once
#include "sgo_conv_tile.hpp"

namespace sgo_conv4w {
using namespace sgo_conv_tile;   // vector types, CIN, COUT, ROWB, MAXW, LZ_BYTES, launch_geometry

#define S4_MFMA_PRIO (VAR & 1)

constexpr int CT = 128;              // output channels per workgroup
constexpr int WROWB = 9 * CIN * 2;   // bytes per output channel of the weights
// LDS map: two weight buffers (128 rows x 128 B; first, so that every weight fragment address is one base register + a 16-bit
// immediate: 6 VGPRs less), window (320 rows x 128 B), zero area
constexpr int LB0 = 0, LB1 = 16384, LW = 32768, LZ = 73728, LDS_BYTES = LZ + LZ_BYTES;

// VAR: schedule variants kept selectable for A/B runs in one process (sgo_conv_tower_kernel(16 + VAR), -DSGO_CONV4W_VARIANTS
//   builds: 0, 4, 5, 6); 7 = all on = default.  Every variant computes the same bits, and tests/test_conv_schedule.py models each.
//   bit 0: s_setprio(1) around the MFMA bursts; bit 1: split wait at chunk boundaries (early pieces now, late pieces one phase
//   later); bit 2: early restage of the dead window rows [0, 128) during the last tap's phase A.
//   Same-process A/B at 8192 x 17 x 17 (TFLOP/s): 0 -> 1312, 4 -> 1305, 5 -> 1314, 6 -> 1324, 7 -> 1342 (k_conv8w: 1310).
//   Retired variant bits (commit dbd02d8 is the last tree that contains their code):
//   bit 3 (variant 15), the weights global -> registers -> LDS instead of by LDS-DMA: bit-identical, -6.3 %, 254 VGPRs
//   (profiles/r03_conv4w_register_route_ab.json).  Bits 4, 5, 6, 7 and 11, timing-only ablations with wrong results (no MFMAs /
//   no fragment reads / no weight staging / no K-loop barriers / no weight fragment reads): profiles/r03_conv4w_ablations.json.
//   Bit 8 (variant 263), chan-hi read last and waited for behind the first 16 MFMAs, barrier 1 behind them too: -3.4 %
//   (DESIGN.md section 8).  Bits 9 and 10 (variants 519 / 1543), the CU's second workgroup held back by half / a quarter of a tile
//   by s_sleep so that the MFMA-free prologues / epilogues do not coincide: -2.2 % / -3.2 %.
//   Measured and dropped: refilling the weight buffer after barrier 2 so that barrier 1 disappears (-4 %: the weights get less
//   time to land), prefetching bias + skip rows into dead LDS behind the last K-tile's MFMAs (-2 %), staging weights[t+2] right after
//   barrier 1 instead of behind phase A's MFMAs (-7 %: whatever sits between a barrier and the MFMA burst is exposed, what
//   follows the burst runs in its shadow), a fifth early window piece for W >= 15 (-1.3 %), s_setprio 3 (-1.9 %), the
//   priorities the other way round (read intervals at 2 or 3 above the bursts: -2.4 .. -3 %), window
//   staging unrolled with v_med3 clamps, 8 instead of ~20 instructions per piece (+-0), the next phase's fragment addresses
//   computed inside the MFMA burst, one VALU instruction behind each MFMA (sched_group_barrier; -1.5 %), refilling fragment
//   registers that die inside a burst right there (chan-hi of the next K-tile + K-half 0 of the next phase's pixels: -6 %; the
//   same with the burst's last quadrant pixel-tile-outer so that whole rows are refilled, 6 / 2 instead of 16 / 8 exposed reads
//   per phase: -5.6 %, and hipcc renames the accumulators and spills at the chunk boundaries).
//   A leaner instruction stream (v_bfe / v_bfi mask select, phase B reusing phase A's row address, scalar weight-staging
//   addresses: 37 instead of 60 VALU per K-tile) ran 3.5 % SLOWER: differences of this size are inside the band that code
//   placement alone moves a hipcc-built kernel by (guide rule 27), so nothing below ~3 % is claimed as a schedule effect.
//   Priorities by hardware wave slot (round 3; the two waves of a SIMD belong to two workgroups and sit in slots 0 / 1, HW_ID bit 0):
//   one static priority per wave for the whole kernel, no flips (-3.3 %), or flips to 2 instead of 1 in odd slots so that two
//   colliding bursts are not a tie (-4.9 %); gpurun_out/r03ax_prio.log.
//   What DOES matter is the ORDER of the fragment reads: the two K-halves of a row (addresses a, a ^ 64: complementary LDS
//   banks) back to back, as SGT_READ_A issues them, is 5 % faster than all K-half-0 reads followed by all K-half-1 reads.
template <bool HAS_SKIP, int VAR>
__global__ __launch_bounds__(256, 2) void k_conv4w(const char *__restrict__ xb, const char *__restrict__ wb,
                                                    const _Float16 *__restrict__ bias, const char *__restrict__ skipb,
                                                    char *__restrict__ yb, int M, int H, int W, unsigned magicHW, unsigned magicW,
                                                    int pairs_q, int pairs_r) {
    __shared__ __attribute__((aligned(1024))) char smem[LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    SGT_TILE_DECODE();
    const int HW = H * W, HALO = W + 1, NROWS = 256 + 2 * HALO;
    const char *wbh = wb + (size_t)chalf * CT * WROWB;     // this half's 128 filters

    SGT_ZERO_FILL();

    // weight staging: instruction i of this wave fills rows (wid*2+i)*8 + (lane>>3) of a 64-row granule; 16-B chunk (lane&7)
    // of row r holds logical chunk (lane&7) ^ ((r>>1)&7)
    const int boff00 = (wid * 16 + (lane >> 3)) * WROWB + (((lane & 7) ^ (lane >> 4)) << 4);
    const int fragB = (((lane >> 4) ^ ((lane >> 1) & 7)) << 4);
    const int rdB0 = (wc * 32 + (lane & 15)) * 128 + fragB, rdB1 = rdB0 ^ 64;
    const int rowA = HALO + wr * 64 + (lane & 15);

    SGT_ACC_INIT();
    half8 pa[4][2], wlo[2][2], whi[2][2];

// weights of the K-tile whose bytes start at koff_ of a filter row, granule G (64 filters) into buffer BUF
#define S4_STAGE_BK(BUF, G, koff_)                                                                    \
    do {                                                                                              \
        int bo_ = boff00;                                                                             \
        asm volatile("" : "+v"(bo_));                                                                 \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; i_++) {                                            \
            const char *src_ = wbh + (unsigned)((bo_ ^ (i_ * 64)) + (i_ * 8 + (G) * 64) * WROWB + (koff_)); \
            SGT_GLDS(src_, ((BUF) ? LB1 : LB0) + (G) * 8192 + (swid * 2 + i_) * 1024);                 \
        }                                                                                             \
    } while (0)
#define S4_READ_B(BUF, G, dst)                                                                        \
    _Pragma("unroll") for (int nt_ = 0; nt_ < 2; nt_++) {                                             \
        dst[nt_][0] = SGT_LDS16(((BUF) ? LB1 : LB0) + (G) * 8192 + nt_ * 2048 + rdB0);                \
        dst[nt_][1] = SGT_LDS16(((BUF) ? LB1 : LB0) + (G) * 8192 + nt_ * 2048 + rdB1);                \
    }
#define S4_MFMA(QM, QN, wfrag)                                                                         \
    _Pragma("unroll") for (int ks_ = 0; ks_ < 2; ks_++) _Pragma("unroll") for (int mt_ = 0; mt_ < 4; mt_++) \
        _Pragma("unroll") for (int nt_ = 0; nt_ < 2; nt_++) acc[QM][QN][mt_][nt_] =                    \
            __builtin_amdgcn_mfma_f32_16x16x32_f16(wfrag[nt_][ks_], pa[mt_][ks_], acc[QM][QN][mt_][nt_], 0, 0, 0)

// One K-tile, tap T of chunk cc (runtime), K-tile index t = 9 cc + T; buffer parity = t & 1 = (cc + T) & 1 -> the caller
// instantiates both parities (CP = cc & 1).
#define S4_TILE(T, CP)                                                                                    \
    do {                                                                                                  \
        constexpr int BUF_ = ((T) + (CP)) & 1, T2_ = ((T) + 2) % 9, CARRY_ = ((T) + 2) / 9;               \
        int swid = wid;                                                                                   \
        asm volatile("" : "+s"(swid));                                                                    \
        const bool last2_ = cc == 3 && (T) >= 7;    /* K-tiles 34, 35: nothing left to stage */           \
        const bool boundary_ = (T) == 8 && cc < 3;  /* last tap of a chunk that has a successor */        \
        S4_READ_B(BUF_, 0, wlo);                                                                          \
        S4_READ_B(BUF_, 1, whi);                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        SGT_READ_A(0, T);                                                                                 \
        SGT_LGKM0();                                                                                      \
        /* barrier 1: every wave has read weights[t] (its buffer may be refilled) and, in the last tap, the window rows */ \
        /* [0, 128) for the last time */                                                                  \
        SGT_BARRIER();                                                                                    \
        /* last tap (shift +W+1): phase B reads window rows >= 128 + 2 (W + 1) only, so rows [0, 128) = pieces 0..15 are */ \
        /* dead from here on (whatever W) and take the next chunk's window one phase early: 4 DMAs per wave */ \
        if ((VAR & 4) && boundary_) SGT_STAGE_WP((cc + 1) * 128, 0, 4);                                   \
        SGT_PRIO(S4_MFMA_PRIO);                                                                           \
        S4_MFMA(0, 0, wlo);                                                                               \
        S4_MFMA(0, 1, whi);                                                                               \
        SGT_PRIO(0);                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if ((VAR & 6) == 6 && (T) == 0 && cc > 0) {   /* first tap of a restaged chunk: phase A read rows [0, 128) only (the */ \
            SGT_VMWAIT(0);                       /* early pieces); the late pieces, issued a whole phase ago, are needed from here */ \
            SGT_BARRIER();                                                                                \
        }                                                                                                 \
        SGT_READ_A(1, T);                                                                                 \
        if (!last2_) {                                                                                    \
            const int koff_ = T2_ * (CIN * 2) + (cc + CARRY_) * 128;                                      \
            S4_STAGE_BK(BUF_, 0, koff_);                                                                  \
            S4_STAGE_BK(BUF_, 1, koff_);                                                                  \
            /* weights[t+1] (issued one K-tile ago) have landed; younger: weights[t+2] and this tap's early window pieces */ \
            if ((VAR & 4) && boundary_) SGT_VMWAIT(8);                                                    \
            else SGT_VMWAIT(4);                                                                           \
        } else if ((T) == 7) {                                                                            \
            SGT_VMWAIT(0);                       /* K-tile 34: K-tile 35's weights */                       \
        }                                                                                                 \
        SGT_LGKM0();                                                                                      \
        SGT_BARRIER();                            /* barrier 2: weights[t+1] visible to all; this tap's window reads retired */ \
        if (boundary_) SGT_STAGE_WP((cc + 1) * 128, (VAR & 4) ? 4 : 0, 10);                               \
        SGT_PRIO(S4_MFMA_PRIO);                                                                           \
        S4_MFMA(1, 1, whi);                                                                               \
        S4_MFMA(1, 0, wlo);                                                                               \
        SGT_PRIO(0);                                                                                      \
        __builtin_amdgcn_sched_barrier(0);       /* the next K-tile's fragment reads stay below these MFMAs (registers) */ \
        if (boundary_) {                                                                                  \
            /* the next tap's phase A reads window rows [0, 128) = the EARLY pieces: the oldest of this wave's outstanding */ \
            /* DMAs ([early x 4][weights x 4][late x nlate]); the late pieces get one more phase to land */ \
            if ((VAR & 6) != 6) SGT_VMWAIT(0);                                                            \
            else if (nlate == 6) SGT_VMWAIT(10);                                                          \
            else if (nlate == 5) SGT_VMWAIT(9);                                                           \
            else if (nlate == 4) SGT_VMWAIT(8);                                                           \
            else SGT_VMWAIT(0);                                                                           \
            SGT_BARRIER();                        /* rows [0, 128) of the next chunk's window are in place */ \
        }                                                                                                 \
    } while (0)

    SGT_NLATE();

    // ---- prologue: window of chunk 0, weights of K-tiles 0 and 1
    {
        int swid = wid;
        SGT_STAGE_WP(0, 0, 10);
        S4_STAGE_BK(0, 0, 0);
        S4_STAGE_BK(0, 1, 0);
        S4_STAGE_BK(1, 0, CIN * 2);
        S4_STAGE_BK(1, 1, CIN * 2);
    }
    SGT_MASKS();
    // window + weights[0] have landed; in flight: weights[1]
    SGT_VMWAIT(4);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the zero area
    SGT_BARRIER();

    for (int kk = 0; kk < 2; kk++) {
        {
            const int cc = 2 * kk;
            S4_TILE(0, 0); S4_TILE(1, 0); S4_TILE(2, 0); S4_TILE(3, 0); S4_TILE(4, 0);
            S4_TILE(5, 0); S4_TILE(6, 0); S4_TILE(7, 0); S4_TILE(8, 0);
        }
        {
            const int cc = 2 * kk + 1;
            S4_TILE(0, 1); S4_TILE(1, 1); S4_TILE(2, 1); S4_TILE(3, 1); S4_TILE(4, 1);
            S4_TILE(5, 1); S4_TILE(6, 1); S4_TILE(7, 1); S4_TILE(8, 1);
        }
    }
    SGT_BARRIER();   // every wave is done with the window and the weights: the LDS becomes the output stage

    SGT_EPILOGUE();
}

template <int VAR>
static inline int launch_var(int n, int h, int w, const void *x, const void *wgt, const void *bias, const void *skip, void *y,
                             hipStream_t st) {
    launch_geom g;
    if (!launch_geometry(n, h, w, g)) return -1;
#define S4_ARGS (const char *)x, (const char *)wgt, (const _Float16 *)bias, (const char *)skip, (char *)y, g.M, h, w, g.magic_hw, g.magic_w, g.xcd_q, g.xcd_r
    if (skip) hipLaunchKernelGGL((k_conv4w<true, VAR>), grid_pairs(g), dim3(256), 0, st, S4_ARGS);
    else hipLaunchKernelGGL((k_conv4w<false, VAR>), grid_pairs(g), dim3(256), 0, st, S4_ARGS);
#undef S4_ARGS
    return 0;
}

static inline int launch(int n, int h, int w, const void *x, const void *wgt, const void *bias, const void *skip, void *y,
                         hipStream_t st, int var = 7) {
    switch (var) {
#ifdef SGO_CONV4W_VARIANTS
    case 0: return launch_var<0>(n, h, w, x, wgt, bias, skip, y, st);
    case 4: return launch_var<4>(n, h, w, x, wgt, bias, skip, y, st);
    case 5: return launch_var<5>(n, h, w, x, wgt, bias, skip, y, st);
    case 6: return launch_var<6>(n, h, w, x, wgt, bias, skip, y, st);
#endif
    default: return launch_var<7>(n, h, w, x, wgt, bias, skip, y, st);
    }
}

}  // namespace sgo_conv4w

#undef S4_MFMA
#undef S4_MFMA_PRIO
#undef S4_READ_B
#undef S4_STAGE_BK
#undef S4_TILE
#include "sgo_conv_tile_undef.hpp"
