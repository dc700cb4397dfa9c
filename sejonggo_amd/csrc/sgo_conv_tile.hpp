// sgo_conv_tile.hpp -- what the three tower kernels (sgo_conv8w.hpp, sgo_conv4w.hpp, sgo_conv4r.hpp) have in common, once.
//
// Device code is shared AT TOKEN LEVEL: macros that a kernel expands inside its own body and that pick up the kernel's locals
// (smem, lane, wid, wr, wc, tile, M, H, W, ...) and its namespace's constants (LW, LZ, CT) by name.  Moving such a piece into a
// __forceinline__ function instead changes the register allocation of these kernels (k_conv4w: 236 -> 240 VGPRs with the epilogue
// as a function) and with it their speed by up to the ~3 % that code placement alone is worth; a macro leaves the
// machine code byte for byte what it was, which tools/isa_diff.py proves without a GPU.  Host code is ordinary functions.
//
// Every kernel header includes this file at its top and sgo_conv_tile_undef.hpp at its bottom: the declarations below are
// guarded, the macros are defined afresh by each include and leave nothing behind.
#ifndef SGO_CONV_TILE_HPP
#define SGO_CONV_TILE_HPP
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgo_conv_tile {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef int intx2 __attribute__((ext_vector_type(2)));
typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr int CIN = 256, COUT = 256;
constexpr int ROWB = CIN * 2;               // bytes per pixel row of x / y
constexpr int MAXW = 19;                    // board width limit (window = 256 + 2 (w + 1) <= 296 of 320 rows)
constexpr int LZ_BYTES = 3 * 2048 + 256;    // the zero area off-board taps read from (SGT_READ_A)

// What a launch of n x h x w pixels x 256 channels needs besides its pointers.  x: [n][h][w][256] fp16, skip (may be null) / y
// alike, bias: fp16[256].  Requires w <= 19 and n*h*w*512 < 2^31 (the caller slices larger batches).
struct launch_geom {
    int M, tiles;              // pixels, 256-pixel tiles
    unsigned magic_hw, magic_w;   // ceil(2^32 / d) for d = h*w, w: x / d = umulhi(x, magic) while x * d < 2^32
    int xcd_q, xcd_r;          // tiles = 8 xcd_q + xcd_r: XCD c walks xcd_q (+ 1 for c < xcd_r) consecutive tiles
};

// false: the shape is outside what the kernels' 32-bit arithmetic covers
static inline bool launch_geometry(int n, int h, int w, launch_geom &g) {
    const long M = (long)n * h * w;
    if (M <= 0 || M * ROWB >= (1L << 31) || w > MAXW || w < 1 || h < 1) return false;   // 32-bit byte offsets into x / y
    // the pixel -> (sample, y, x) split uses magic-number division, exact only while p * (h*w) < 2^32 for every pixel
    // index the kernel forms (p < M + 256)
    if ((unsigned long long)(M + 256) * (unsigned long long)(h * w) >= (1ULL << 32)) return false;
    g.M = (int)M;
    g.tiles = (int)((M + 255) / 256);
    g.magic_hw = (unsigned)(((1ULL << 32) + (unsigned)(h * w) - 1) / (unsigned)(h * w));
    g.magic_w = (unsigned)(((1ULL << 32) + (unsigned)w - 1) / (unsigned)w);
    g.xcd_q = g.tiles / 8;
    g.xcd_r = g.tiles % 8;
    return true;
}

// grid of the 256-thread kernels (k_conv4w, k_conv4r; SGT_TILE_DECODE): 8 XCDs x (tile, channel half) pairs of the fullest XCD
static inline dim3 grid_pairs(const launch_geom &g) { return dim3(8 * 2 * (g.xcd_q + (g.xcd_r ? 1 : 0))); }

}  // namespace sgo_conv_tile
#endif

// ------------------------------------------------------------------------------------------------ all three kernels
#define SGT_AS1 __attribute__((address_space(1)))
#define SGT_AS3 __attribute__((address_space(3)))
// LDS accesses the compiler must not order against in-flight LDS-DMA (it would drain vmcnt to 0 before each of its own
// ds_read once a DMA is pending): issued as asm, waited for by hand (SGT_LGKM0 = lgkmcnt(0) + a scheduling fence).
#define SGT_DS_READ64(dst, addr, OFF) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory")
#define SGT_DS_READ128(dst, addr, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory")
#define SGT_DS_WRITE64(addr, val, OFF) asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(val), "n"(OFF) : "memory")
#define SGT_LGKM0()                                    \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    __builtin_amdgcn_sched_barrier(0)
#define SGT_VMWAIT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define SGT_BARRIER()                  \
    __builtin_amdgcn_sched_barrier(0); \
    __builtin_amdgcn_s_barrier();      \
    __builtin_amdgcn_sched_barrier(0)
#define SGT_PRIO(x) __builtin_amdgcn_s_setprio(x)
// LDS-DMA: 16 bytes per lane from global memory straight into smem + ldsoff + lane * 16
#define SGT_GLDS(src, ldsoff) \
    __builtin_amdgcn_global_load_lds((const SGT_AS1 void *)(src), (SGT_AS3 void *)((SGT_AS3 char *)smem + (ldsoff)), 16, 0, 0)
#define SGT_LDS16(off) (*reinterpret_cast<const half8 *>(smem + (off)))
// window row shift of tap T (compile time): (dy - 1) * W + (dx - 1)
#define SGT_SHIFT(T) (((T) / 3 == 0 ? -W : (T) / 3 == 2 ? W : 0) + (T) % 3 - 1)

// floatx4 acc[pixel half][channel half][mt][nt] = 0: the wave's 128 x 64 (k_conv8w) / 128 x 32 x 2 (k_conv4w, k_conv4r) outputs
#define SGT_ACC_INIT()                                                                                \
    floatx4 acc[2][2][4][2];                                                                          \
    _Pragma("unroll") for (int a = 0; a < 2; a++) _Pragma("unroll") for (int b = 0; b < 2; b++)       \
        _Pragma("unroll") for (int c = 0; c < 4; c++) _Pragma("unroll") for (int d = 0; d < 2; d++)   \
            acc[a][b][c][d] = floatx4{0.f, 0.f, 0.f, 0.f}

// int mk[2][2]: tap-validity masks of the lane's 8 fragment rows: row (G, mt) = G*128 + wr*64 + mt*16 + (lane&15);
// mk[G][mt>>1] holds 9 bits per row (bit T: tap T lies on the board) at bit (mt&1)*9.  Divisions by h*w and w through the
// host's magic numbers (launch_geometry).  A divisor of 1 has no 32-bit magic number -- ceil(2^32 / 1) wraps to 0 -- so x / 1 is
// added back by hand.
#define SGT_MASKS()                                                                                                   \
    int mk[2][2];                                                                                                     \
    _Pragma("unroll") for (int g = 0; g < 2; g++) _Pragma("unroll") for (int h2 = 0; h2 < 2; h2++) {                  \
        int v = 0;                                                                                                    \
        _Pragma("unroll") for (int e = 0; e < 2; e++) {                                                               \
            const int p = tile * 256 + g * 128 + wr * 64 + (h2 * 2 + e) * 16 + (lane & 15);                           \
            const int q = p - (int)(__umulhi((unsigned)p, magicHW) + (HW == 1 ? (unsigned)p : 0u)) * HW;              \
            const int yy = (int)(__umulhi((unsigned)q, magicW) + (W == 1 ? (unsigned)q : 0u)), xx = q - yy * W;       \
            const int cm = (xx >= 1 ? 1 : 0) | 2 | (xx <= W - 2 ? 4 : 0);                                             \
            int m = (yy >= 1 ? cm : 0) | (cm << 3) | (yy <= H - 2 ? cm << 6 : 0);                                     \
            m = p < M ? m : 0;                                                                                        \
            v |= m << (9 * e);                                                                                        \
        }                                                                                                             \
        mk[g][h2] = v;                                                                                                \
    }

// ------------------------------------------------------------------------------------------------ k_conv4w and k_conv4r
// (256 threads = 2 pixel groups wr x 2 channel groups wc; 256 pixels x CT = 128 channels per workgroup; window at LW, zero area
// at LZ of the kernel's own LDS map)

// int tile, chalf.  Workgroup b runs on XCD b % 8.  Within an XCD the sequence i = b / 8 walks (tile, channel half) pairs: both
// halves of a pixel tile are neighbours in launch order on the SAME XCD (they share the window rows in its L2), and the XCD's
// tiles are a contiguous range (halo rows shared with the neighbouring tile).  tiles = 8 pairs_q + pairs_r; the grid is padded to
// 8 x 2 x (pairs_q + 1) (grid_pairs), the workgroups beyond an XCD's share leave at once.
#define SGT_TILE_DECODE()                                                                                             \
    int tile, chalf;                                                                                                  \
    {                                                                                                                 \
        const int c = blockIdx.x & 7, i = blockIdx.x >> 3;                                                            \
        chalf = i & 1;                                                                                                \
        const int ti = i >> 1;                                                                                        \
        tile = (c < pairs_r) ? c * (pairs_q + 1) + ti : pairs_r * (pairs_q + 1) + (c - pairs_r) * pairs_q + ti;       \
        const int mine = (c < pairs_r) ? pairs_q + 1 : pairs_q;                                                       \
        if (ti >= mine) return;                                                                                       \
    }

#define SGT_ZERO_FILL()                                                                                               \
    if (tid < LZ_BYTES / 16) *reinterpret_cast<intx4 *>(smem + LZ + tid * 16) = intx4{0, 0, 0, 0};                    \
    if (tid + 256 < LZ_BYTES / 16) *reinterpret_cast<intx4 *>(smem + LZ + (tid + 256) * 16) = intx4{0, 0, 0, 0}

// int nlate: late window pieces (pc 4..9) this wave issues at a chunk boundary: the counted waits there depend on it
#define SGT_NLATE()                                                                                                   \
    int nlate = 0;                                                                                                    \
    _Pragma("unroll") for (int pc = 4; pc < 10; pc++) nlate += ((pc * 4 + wid) * 8 < NROWS) ? 1 : 0

// window pieces (8 rows each) pc*4 + wid for pc in [PC0, PC1) of the channel chunk at byte offset ccoff_ of a pixel row: piece id
// fills window rows id*8 + (lane>>3), pixel = tile*256 - HALO + row (clamped into the tensor: the masks keep such rows out of
// the sums); 16-B chunk c of row r sits at c ^ (r & 7)
#define SGT_STAGE_WP(ccoff_, PC0, PC1)                                                                \
    do {                                                                                              \
        _Pragma("nounroll") for (int pc_ = (PC0); pc_ < (PC1); pc_++) {                               \
            const int id_ = pc_ * 4 + swid;                                                           \
            if (id_ * 8 < NROWS) {                                                                    \
                int la_ = lane;                                                                       \
                asm volatile("" : "+v"(la_));                                                         \
                int q_ = tile * 256 - HALO + id_ * 8 + (la_ >> 3);                                    \
                q_ = q_ < 0 ? 0 : (q_ < M ? q_ : M - 1);                                              \
                const int wsrc_ = ((la_ & 7) ^ ((la_ >> 3) & 7)) << 4;   /* recomputed: not worth a register across the loop */ \
                const char *src_ = xb + (unsigned)(q_ * ROWB + (ccoff_) + wsrc_);                     \
                SGT_GLDS(src_, LW + id_ * 1024);                                                      \
            }                                                                                         \
        }                                                                                             \
    } while (0)

// pixel fragments of half G for tap T (compile time): window row = rowA + G*128 + mt*16 + shift(T), zeros where the tap is off the
// board -- from the SAME bank slot its window address has (row parity, chunk), so the redirect adds no bank conflict.  The two
// K-halves of a row (addresses a, a ^ 64: complementary LDS banks) are read back to back: 5 % faster than all K-half-0 reads
// followed by all K-half-1 reads.  ra_, mka_, mkb_ are opaque copies: 36 phases of address arithmetic are neither hoisted nor kept
// live, and the loop-invariant lane masks do not move into SGPR pairs.
#define SGT_READ_A(G, T)                                                                              \
    do {                                                                                              \
        int ra_ = rowA;                                                                               \
        asm volatile("" : "+v"(ra_));                                                                 \
        const int rl_ = ra_ + SGT_SHIFT(T);                                                           \
        const int c0_ = (((lane >> 4) ^ rl_) & 7) << 4;                                               \
        const int b0_ = LW + (G) * 16384 + (rl_ << 7) + c0_, b1_ = b0_ ^ 64;                          \
        const int z0_ = LZ + ((rl_ & 1) << 7) + c0_, z1_ = z0_ ^ 64;                                  \
        int mka_ = mk[G][0], mkb_ = mk[G][1];                                                         \
        asm volatile("" : "+v"(mka_), "+v"(mkb_));                                                    \
        _Pragma("unroll") for (int mt_ = 0; mt_ < 4; mt_++) {                                         \
            const bool ok_ = (((mt_ >> 1) ? mkb_ : mka_) & (1 << ((mt_ & 1) * 9 + (T)))) != 0;        \
            pa[mt_][0] = SGT_LDS16((ok_ ? b0_ : z0_) + mt_ * 2048);                                   \
            pa[mt_][1] = SGT_LDS16((ok_ ? b1_ : z1_) + mt_ * 2048);                                   \
        }                                                                                             \
    } while (0)

// ---- epilogue through LDS, after the barrier behind the K loop (the LDS is the output stage from there on): half hf (128 pixels
//      x 128 channels) lives at [hf*32 KiB, +32 KiB), rows of 256 B, 16-B chunk c of row r at chunk c ^ (r & 15).  The bias is
//      loaded by asm so that the compiler does not see an ordinary load beside the pending DMAs (it would wait vmcnt(0) for it,
//      draining the skip prefetch); the skip rows arrive by DMA, every lane adds bias / skip, applies ReLU and writes its 8-byte
//      pieces back in place, and whole 256-B rows leave as 16 B per lane.
#define SGT_EPILOGUE()                                                                                                \
    int elane = lane;                                                                                                 \
    asm volatile("" : "+v"(elane));                                                                                   \
    intx2 bvi[2][2];                                                                                                  \
    {                                                                                                                 \
        const _Float16 *bp = bias + chalf * CT + wc * 32 + (elane >> 4) * 4;                                          \
        _Pragma("unroll") for (int qn = 0; qn < 2; qn++) _Pragma("unroll") for (int nt = 0; nt < 2; nt++)             \
            asm volatile("global_load_dwordx2 %0, %1, off offset:%2" : "=v"(bvi[qn][nt]) : "v"(bp), "n"((qn * 64 + nt * 16) * 2) : "memory"); \
    }                                                                                                                 \
    if constexpr (HAS_SKIP) {                                                                                         \
        /* instruction j of this wave fills rows (wid*8+j)*4 + (lane>>4) of the half */                               \
        _Pragma("nounroll") for (int hf = 0; hf < 2; hf++) _Pragma("nounroll") for (int j = 0; j < 8; j++) {          \
            const int r_ = (wid * 8 + j) * 4 + (elane >> 4);                                                          \
            int p_ = tile * 256 + hf * 128 + r_;                                                                      \
            p_ = p_ < M ? p_ : M - 1;                                                                                 \
            SGT_GLDS(skipb + (unsigned)(p_ * ROWB + chalf * (CT * 2) + (((elane & 15) ^ (r_ & 15)) << 4)), hf * 32768 + (wid * 8 + j) * 1024); \
        }                                                                                                             \
    }                                                                                                                 \
    const int epx = (wr * 64 + (elane & 15)) * 256 + ((elane >> 4) & 1) * 8;                                          \
    const int epc = ((wc * 4 + (elane >> 5)) ^ (elane & 15)) << 4;       /* chunk of (qn = 0, nt = 0); qn toggles bit 3, nt bit 1 */ \
    _Pragma("unroll") for (int hf = 0; hf < 2; hf++) {                                                                \
        const int a00 = hf * 32768 + epx + epc, a01 = hf * 32768 + epx + (epc ^ 32);                                  \
        const int a10 = hf * 32768 + epx + (epc ^ 128), a11 = hf * 32768 + epx + (epc ^ 128 ^ 32);                    \
        intx2 sk[4][2][2];                                                                                            \
        if (hf == 0) {                                                                                                \
            if constexpr (HAS_SKIP) {                                                                                 \
                asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   /* bias + the lo half's rows (the hi half's 8 DMAs may fly) */ \
            } else {                                                                                                  \
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   /* the bias */                                     \
            }                                                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                                        \
        } else if constexpr (HAS_SKIP) {                                                                              \
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");       /* the hi half's rows (younger: the 8 row stores of half 0) */ \
            __builtin_amdgcn_sched_barrier(0);                                                                        \
        }                                                                                                             \
        if constexpr (HAS_SKIP) {                                                                                     \
            SGT_BARRIER();                                         /* everybody's skip rows of this half are in LDS */ \
            _Pragma("unroll") for (int mt = 0; mt < 4; mt++) {                                                        \
                SGT_DS_READ64(sk[mt][0][0], a00, mt * 4096);                                                          \
                SGT_DS_READ64(sk[mt][0][1], a01, mt * 4096);                                                          \
                SGT_DS_READ64(sk[mt][1][0], a10, mt * 4096);                                                          \
                SGT_DS_READ64(sk[mt][1][1], a11, mt * 4096);                                                          \
            }                                                                                                         \
            SGT_LGKM0();                                                                                              \
        }                                                                                                             \
        _Pragma("unroll") for (int mt = 0; mt < 4; mt++) _Pragma("unroll") for (int qn = 0; qn < 2; qn++)             \
            _Pragma("unroll") for (int nt = 0; nt < 2; nt++) {                                                        \
                floatx4 v = acc[hf][qn][mt][nt];                                                                      \
                if constexpr (HAS_SKIP) {                                                                             \
                    const half4 s4 = __builtin_bit_cast(half4, sk[mt][qn][nt]);                                       \
                    _Pragma("unroll") for (int j = 0; j < 4; j++) v[j] += (float)s4[j];                               \
                }                                                                                                     \
                half4 o;                                                                                              \
                _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                       \
                    const float f = v[j] + (float)__builtin_bit_cast(half4, bvi[qn][nt])[j];                          \
                    o[j] = (_Float16)__builtin_elementwise_maximum(f, 0.f);  /* v_maximum3_f32: NaN passes */ \
                }                                                                                                     \
                const intx2 oi = __builtin_bit_cast(intx2, o);                                                        \
                if (qn == 0 && nt == 0) SGT_DS_WRITE64(a00, oi, mt * 4096);                                           \
                else if (qn == 0) SGT_DS_WRITE64(a01, oi, mt * 4096);                                                 \
                else if (nt == 0) SGT_DS_WRITE64(a10, oi, mt * 4096);                                                 \
                else SGT_DS_WRITE64(a11, oi, mt * 4096);                                                              \
            }                                                                                                         \
        SGT_LGKM0();                                                                                                  \
        SGT_BARRIER();                                                                                                \
        /* copy-out: wave wid, instruction j, lane -> LDS bytes hf*32 KiB + wid*8192 + j*1024 + lane*16 = row wid*32 + j*4 + */ \
        /* (lane>>4), physical chunk lane&15 = logical chunk (lane&15) ^ (row & 15) */                                \
        intx4 ov[8];                                                                                                  \
        const int a2 = hf * 32768 + wid * 8192 + elane * 16;                                                          \
        _Pragma("unroll") for (int j = 0; j < 8; j++) SGT_DS_READ128(ov[j], a2, j * 1024);                            \
        const int r0 = wid * 32 + (elane >> 4);                                                                       \
        const int p0 = tile * 256 + hf * 128 + r0;                                                                    \
        char *dst = yb + (size_t)p0 * ROWB + chalf * (CT * 2);                                                        \
        SGT_LGKM0();                                                                                                  \
        _Pragma("unroll") for (int j = 0; j < 8; j++)                                                                 \
            if (p0 + j * 4 < M)                                                                                       \
                *reinterpret_cast<intx4 *>(dst + j * 4 * ROWB + (((elane & 15) ^ ((r0 + j * 4) & 15)) << 4)) = ov[j]; \
    }
