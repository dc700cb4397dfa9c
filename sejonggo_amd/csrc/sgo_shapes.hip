// sgo_shapes.hip -- shape search on the device (include/sgo.h "shape search"): per packed record, where does a local pattern of
// black / white / empty / don't-care cells occur, in any of its sixteen variants (eight symmetries of the grid, colours as drawn
// or exchanged), anchored to the board edges it names.  A translation unit of its own, like sgo_life.hip and sgo_keys.hip:
// tests/test_engine_isa.py pins the kernel set of sgo_engine.hip.
//
//   k_shapes<S>   per listed record: hits = {n_hits, first, vmask, n_cover} and the cover set
//
// sgo_shape_compile is host arithmetic (no device): it writes the kept variants of a shape as row masks into a table of
// SGO_SHAPE_TABLE_WORDS words.  sgo_session_shapes runs the same kernel over the context's records, with the root index
// k_session_roots (sgo_session.hpp) writes.
//
// Kernel form: one 32-lane HALF of a wavefront per listed row, one board row per lane (sgo_rows.hpp), two rows per 64-thread
// workgroup, as k_keys.  Lane y holds the rows rb, rw and emp of the record.  The table is the same for every lane: it is read
// with wave-uniform addresses (scalar loads), and the loops over variants, shape rows and set bits of a row mask are uniform
// over the wave: no per-lane branch anywhere.  A half whose row is out of range or does not exist (odd n) goes through the same
// code on an empty board with its matches masked off; only its stores differ.  Everything lives in registers: no LDS, no scratch.
#include <string.h>

#include "sgo_analysis.hpp"
#include "sgo_engine_state.hpp"
#include "sgo_half.hpp"
#include "sgo_rows.hpp"

namespace sgo {

// offsets inside a variant slot of the table (include/sgo.h)
constexpr int SH_HEAD = 16, SH_SLOT = 64, SH_X = 4, SH_O = 23, SH_E = 42;

template <int S>
__global__ __launch_bounds__(64) void k_shapes(int n, const uint32_t *__restrict__ records, int n_records, const int32_t *__restrict__ index,
                                               const uint32_t *__restrict__ table, int32_t *__restrict__ hits, uint32_t *__restrict__ cover) {
    using G = Geo<S>;
    const int half = threadIdx.x >> 5, y = threadIdx.x & 31;
    const long i = (long)blockIdx.x * 2 + half;
    const bool valid = i < n;
    const int r = valid ? (index ? index[i] : (int)i) : -1;
    const bool ok = r >= 0 && r < n_records;                         // uniform over the half
    const uint32_t *rec = ok ? records + (size_t)r * G::RW : nullptr;
    const rows::Board<S> bd(half, y);
    const uint32_t rb = rec ? rows::load_row<S>(rec, y) : 0u, rw = rec ? rows::load_row<S>(rec + G::NW, y) : 0u;
    const uint32_t emp = ~(rb | rw) & bd.M;                          // on the board only: an empty cell never matches beyond an edge
    const uint32_t live = ok ? ~0u : 0u;

    // a table that sgo_shape_compile did not write must not lead a read outside the table or a shift outside the word
    const int n_kept = min((int)table[1], 16);
    uint32_t cov = 0u;
    int cnt = 0, first = -1, vmask = 0;
    for (int t = 0; t < n_kept; t++) {
        const uint32_t *slot = table + SH_HEAD + SH_SLOT * t;
        const int v = (int)(slot[0] & 15u), w = min(max((int)slot[1], 1), S), h = min(max((int)slot[2], 1), S), edges = (int)slot[3];
        // acc: bit x0 of lane y0 = "rows y0 .. y0 + h - 1 agree with the variant from column x0 on", by Horner from the bottom row
        uint32_t acc = ~0u;
        for (int j = h - 1; j >= 0; j--) {
            uint32_t mx = slot[SH_X + j], mo = slot[SH_O + j], me = slot[SH_E + j];
            // all three masks in scalar registers HERE: the loads are issued together and waited for once, not one per loop
            asm volatile("" : "+s"(mx), "+s"(mo), "+s"(me));
            uint32_t R = ~0u;
            for (uint32_t m = mx; m; m &= m - 1u) R &= rb >> __builtin_ctz(m);
            for (uint32_t m = mo; m; m &= m - 1u) R &= rw >> __builtin_ctz(m);
            for (uint32_t m = me; m; m &= m - 1u) R &= emp >> __builtin_ctz(m);
            acc = R & (j == h - 1 ? ~0u : rows::row_below(acc));
        }
        // The placement mask: the window lies on the board (x0 <= S - w, y0 <= S - h) and touches the edges it names.  It is what
        // keeps don't-care cells -- whose R is all ones -- from matching off the board, and what keeps rows of the OTHER half from
        // leaking in: row_below crosses from lane 31 into lane 32, but a lane y0 <= S - h only ever reads rows y0 .. S - 1 of its
        // own half, and every other lane is cleared here.
        uint32_t xm = (2u << (S - w)) - 1u;
        if (edges & 1) xm &= 1u;
        if (edges & 4) xm &= 1u << (S - w);
        bool ym = y <= S - h;
        if (edges & 2) ym = ym && y == 0;
        if (edges & 8) ym = ym && y == S - h;
        acc &= (ym ? xm : 0u) & live;
        if (__any(acc != 0)) {                                       // the whole wave, both halves: most variants hit nowhere
            const int lo = lowest_point<S>(acc, half);               // -1 in a half without a hit
            if (lo >= 0) vmask |= 1 << v;
            if (lo >= 0 && first < 0) first = v * G::N + lo;         // variants come in ascending v
            cnt += __popc(acc);
            // the cover: the reverse dilation, row by row downwards.  D = the matches j rows up; lane 32 receives lane 31 of the
            // other half, which the placement mask has cleared.
            uint32_t D = acc;
            for (int j = 0; j < h; j++) {
                for (uint32_t m = slot[SH_X + j] | slot[SH_O + j] | slot[SH_E + j]; m; m &= m - 1u) cov |= D << __builtin_ctz(m);
                D = rows::row_above(D);
            }
        }
    }

    // every lane takes part in the gather and the sums; only the stores are conditional
    const uint32_t wc = rows::gather_word<S>(cov, half, y);
    const int n_hits = half_sum(cnt), n_cover = half_sum(__popc(cov));
    if (valid) {
        if (y < G::NW) cover[(size_t)i * G::NW + y] = wc;
        if (y == 0) {
            int32_t *ho = hits + (size_t)i * 4;
            ho[0] = n_hits;
            ho[1] = first;
            ho[2] = vmask;
            ho[3] = n_cover;
        }
    }
}

int launch_shapes(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const uint32_t *d_table,
                  int32_t *d_hits, uint32_t *d_cover, hipStream_t st) {
    SGO_DISPATCH(S, k_shapes<kS><<<dim3(cdiv(n, 2)), dim3(64), 0, st>>>(n, d_records, n_records, d_index, d_table, d_hits, d_cover));
    SGO_HIP(hipGetLastError());
    return SGO_OK;
}

// ---- the host side: the sixteen variants of a shape as row masks ---------------------------------------------------------------
namespace {

struct Grid {
    int w, h, edges;
    uint8_t c[19][19];             // [row][column]: 0 don't-care, 1 X, 2 O, 3 empty
};

// new L, T, R, B = old ... (bit numbers 0..3) per g, the table of include/sgo.h
const int EDGE_FROM[8][4] = {{0, 1, 2, 3}, {1, 0, 3, 2}, {2, 1, 0, 3}, {0, 3, 2, 1}, {3, 0, 1, 2}, {2, 3, 0, 1}, {1, 2, 3, 0}, {3, 2, 1, 0}};

Grid variant_of(const Grid &b, int v) {
    const int g = v & 7, w = b.w, h = b.h;
    const bool swap = v >= 8, turn = g == 1 || g == 4 || g == 6 || g == 7;
    Grid o;
    memset(&o, 0, sizeof(o));
    o.w = turn ? h : w;
    o.h = turn ? w : h;
    for (int j = 0; j < o.h; j++)
        for (int i = 0; i < o.w; i++) {
            int sj, si;
            switch (g) {
            case 0: sj = j; si = i; break;
            case 1: sj = i; si = j; break;
            case 2: sj = j; si = w - 1 - i; break;
            case 3: sj = h - 1 - j; si = i; break;
            case 4: sj = h - 1 - i; si = j; break;
            case 5: sj = h - 1 - j; si = w - 1 - i; break;
            case 6: sj = i; si = w - 1 - j; break;
            default: sj = h - 1 - i; si = w - 1 - j; break;
            }
            const uint8_t k = b.c[sj][si];
            o.c[j][i] = (swap && (k == 1 || k == 2)) ? (uint8_t)(3 - k) : k;
        }
    for (int s = 0; s < 4; s++)
        if ((b.edges >> EDGE_FROM[g][s]) & 1) o.edges |= 1 << s;
    return o;
}

bool same_grid(const Grid &a, const Grid &b) { return a.w == b.w && a.h == b.h && a.edges == b.edges && !memcmp(a.c, b.c, sizeof(a.c)); }

// the header's refusals; on success the base grid
bool read_shape(int S, const sgo_shape *s, Grid &b) {
    if (!size_ok(S) || !s || s->w < 1 || s->w > S || s->h < 1 || s->h > S || s->edges < 0 || s->edges > 15 || s->reserved != 0) return false;
    memset(&b, 0, sizeof(b));
    b.w = s->w; b.h = s->h; b.edges = s->edges;
    const uint32_t cols = (2u << (s->w - 1)) - 1u;
    for (int j = 0; j < 19; j++) {
        const uint32_t x = s->x[j], o = s->o[j], e = s->e[j];
        if (j >= s->h ? (x | o | e) != 0 : ((x | o | e) & ~cols) != 0) return false;
        if ((x & o) | (x & e) | (o & e)) return false;
        for (int i = 0; i < s->w && j < s->h; i++) b.c[j][i] = (uint8_t)(((x >> i) & 1) ? 1 : ((o >> i) & 1) ? 2 : ((e >> i) & 1) ? 3 : 0);
    }
    return true;
}

int compile_shape(const char *who, int S, const sgo_shape *shape, uint32_t *table) {
    Grid base;
    if (!table || !read_shape(S, shape, base)) {
        set_error(std::string(who) + ": bad shape (unsupported size, w or h outside [1, S], a bit outside the grid, a cell in two sets, "
                  "edges outside [0, 15], reserved != 0, or a NULL argument)");
        return SGO_ERR_ARG;
    }
    memset(table, 0, sizeof(uint32_t) * SGO_SHAPE_TABLE_WORDS);
    Grid kept[16];
    int n_kept = 0;
    uint32_t kept_mask = 0;
    for (int v = 0; v < 16; v++) {
        const Grid g = variant_of(base, v);
        bool dup = false;
        for (int k = 0; k < n_kept && !dup; k++) dup = same_grid(kept[k], g);
        if (dup) continue;
        uint32_t *slot = table + SH_HEAD + SH_SLOT * n_kept;
        slot[0] = (uint32_t)v; slot[1] = (uint32_t)g.w; slot[2] = (uint32_t)g.h; slot[3] = (uint32_t)g.edges;
        for (int j = 0; j < g.h; j++)
            for (int i = 0; i < g.w; i++)
                if (g.c[j][i]) slot[(g.c[j][i] == 1 ? SH_X : g.c[j][i] == 2 ? SH_O : SH_E) + j] |= 1u << i;
        kept[n_kept++] = g;
        kept_mask |= 1u << v;
    }
    table[0] = (uint32_t)S; table[1] = (uint32_t)n_kept; table[2] = kept_mask;
    table[3] = (uint32_t)base.w; table[4] = (uint32_t)base.h; table[5] = (uint32_t)base.edges;
    return SGO_OK;
}

}  // namespace

// for csrc/sgo_session.hip: the table of `shape` at the context's size, checked, into HOST memory
int session_shape_table(int S, const sgo_shape *shape, uint32_t *table) { return compile_shape("sgo_session_shapes", S, shape, table); }

}  // namespace sgo

using namespace sgo;

extern "C" {

int sgo_shape_compile(int S, const sgo_shape *shape, uint32_t *table) { return compile_shape("sgo_shape_compile", S, shape, table); }

int sgo_shapes_dev(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const uint32_t *d_table, int32_t *d_hits,
                   uint32_t *d_cover, void *stream) {
    if (!size_ok(S) || n < 0 || n_records < 0 || !d_records || !d_table || !d_hits || !d_cover) {
        set_error("sgo_shapes_dev: bad argument (unsupported size, n < 0, n_records < 0, a NULL record array, table or output)");
        return SGO_ERR_ARG;
    }
    if (n == 0) return SGO_OK;
    return launch_shapes(S, n, d_records, n_records, d_index, d_table, d_hits, d_cover, (hipStream_t)stream);
}

int sgo_shapes(int S, int n, const uint32_t *records, const sgo_shape *shape, int32_t *hits, uint32_t *cover) {
    if (!size_ok(S) || n < 0 || !records || !shape || !hits || !cover) {
        set_error("sgo_shapes: bad argument (unsupported size, n < 0, a NULL record array, shape or output)");
        return SGO_ERR_ARG;
    }
    uint32_t table[SGO_SHAPE_TABLE_WORDS];
    const int crc = compile_shape("sgo_shapes", S, shape, table);
    if (crc != SGO_OK) return crc;
    if ((int)table[0] != S) { set_error("sgo_shapes: the table was compiled for another size"); return SGO_ERR_ARG; }
    if (n == 0) return SGO_OK;
    // every row is written whole, so nothing of the caller's goes in
    const HostArray a[] = {{sizeof(table), table, nullptr}, {(size_t)n * 4 * sizeof(int32_t), nullptr, hits}, {(size_t)n * sgo_plane_words(S) * sizeof(uint32_t), nullptr, cover}};
    return host_entry("sgo_shapes", records, (size_t)n * sgo_packed_words(S) * sizeof(uint32_t), a, [&](const uint32_t *d_records, uint8_t *const *d) {
        return launch_shapes(S, n, d_records, n, nullptr, reinterpret_cast<const uint32_t *>(d[0]), reinterpret_cast<int32_t *>(d[1]), reinterpret_cast<uint32_t *>(d[2]), nullptr);
    });
}

}  // extern "C"
