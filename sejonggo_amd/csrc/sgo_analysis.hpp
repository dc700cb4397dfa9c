// sgo_analysis.hpp -- what the position analyses (keys, tactics, life, shapes, moves, influence, secure, solve, race, connect, playout) share on the host: the record
// launchers of their translation units, which sgo_session.hip runs over the context's root records, and the one body of their
// host entries sgo_X.  Host code only; every kernel stays in its own file.
#pragma once
#include "sgo_common.hpp"

namespace sgo {

// The record launchers: n listed records (d_index == nullptr: record i) of d_records; every pointer is device memory.
int launch_keys(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_target,
                uint64_t *d_key0, uint64_t *d_canon, int32_t *d_mask, int32_t *d_action, hipStream_t st);
int launch_tactics(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int max_chains, uint8_t *d_libs,
                   int32_t *d_n_chains, int32_t *d_chains, hipStream_t st);
int launch_life(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, uint32_t *d_sets, int32_t *d_counts,
                hipStream_t st);
int launch_shapes(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const uint32_t *d_table,
                  int32_t *d_hits, uint32_t *d_cover, hipStream_t st);
int launch_moves(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int side, int16_t *d_moves,
                 int32_t *d_counts, hipStream_t st);
int launch_influence(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const uint32_t *d_dead, int dilate,
                     int erode_moyo, int erode_terr, int16_t *d_values, uint32_t *d_sets, int32_t *d_counts, hipStream_t st);
int launch_secure(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int side, int16_t *d_table,
                  uint32_t *d_sets, int32_t *d_counts, hipStream_t st);
int launch_solve(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask, const uint32_t *d_region,
                 int rules, int max_region, int max_nodes, int max_targets, int32_t *d_n_targets, int32_t *d_rows, uint32_t *d_regions,
                 hipStream_t st);
int launch_race(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask, const uint32_t *d_region,
                int rules, int max_libs, int max_region, int max_nodes, int max_pairs, int32_t *d_n_pairs, int32_t *d_rows, uint32_t *d_regions,
                hipStream_t st);
int launch_connect(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_ask, const uint32_t *d_region,
                   int rules, int cut_libs, int max_region, int max_nodes, int max_pairs, int32_t *d_n_pairs, int32_t *d_rows, uint32_t *d_regions,
                   int16_t *d_groups, int32_t *d_group_counts, hipStream_t st);
// superko reads a record and the records of its game before it (d_first), through the work array d_keys [n_records]: two launches
int launch_superko(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, const int32_t *d_first, int rule,
                   uint64_t *d_keys, uint32_t *d_sets, int16_t *d_back, int32_t *d_counts, hipStream_t st);
// light playouts: per row per_row random games played to their end; d_amaf may be nullptr; two launches (zero, play)
int launch_playout(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int per_row, uint32_t seed, int rules,
                   int max_plies, int32_t *d_own, int32_t *d_amaf, int64_t *d_sums, hipStream_t st);
// playout tree search: per row `trees` searches of `sims` simulations; d_rave, d_own, d_trace may be nullptr; d_work holds
// uct_work_bytes; three launches (zero, search, best)
int launch_uct(int S, int n, const uint32_t *d_records, int n_records, const int32_t *d_index, int trees, int sims, uint32_t seed, int rules,
               int max_plies, int komi2, int expand_at, int rave_equiv, int prior, int max_nodes, int32_t *d_visits, int32_t *d_wins2, int32_t *d_rave,
               int32_t *d_own, int64_t *d_sums, int32_t *d_info, int32_t *d_trace, void *d_work, hipStream_t st);

// The host-side checks sgo_session.hip needs: the table of `shape` at the context's size, checked, into HOST memory
// (csrc/sgo_shapes.hip), and the bounds of the influence parameters (csrc/sgo_influence.hip) and of the solve parameters (csrc/sgo_solve.hip)
// and the race parameters (csrc/sgo_race.hip) and the connect parameters (csrc/sgo_connect.hip).
int session_shape_table(int S, const sgo_shape *shape, uint32_t *table);
bool influence_params_ok(int dilate, int erode_moyo, int erode_terr);
bool solve_params_ok(int rules, int max_region, int max_nodes, int max_targets);
bool race_params_ok(int rules, int max_libs, int max_region, int max_nodes, int max_pairs);
bool connect_params_ok(int rules, int cut_libs, int max_region, int max_nodes, int max_pairs);
bool playout_params_ok(int S, int n, int per_row, int rules, int max_plies);   // csrc/sgo_playout.hip
bool uct_params_ok(int S, int n, int trees, int sims, int rules, int max_plies, int komi2, int expand_at, int rave_equiv, int prior,
                   int max_nodes);                                             // csrc/sgo_uct.hip
size_t uct_work_bytes(int S, int n, int trees, int max_nodes);

// One array of a host entry's device block.  `up` (or nullptr) is copied in before the launch, `down` (or nullptr) is filled
// from it afterwards; an array with neither is only room.
struct HostArray {
    size_t bytes;
    const void *up;
    void *down;
};

// The body of a host entry sgo_X: one hipMalloc holds the arrays (each on a 16-byte boundary) and the records behind them,
// launch(d_records, d) runs on the null stream with d[k] the device address of a[k], the outputs come down, hipFree.
template <size_t NA, class Launch>
int host_entry(const char *who, const uint32_t *records, size_t record_bytes, const HostArray (&a)[NA], Launch launch) {
    size_t off[NA], at = 0;
    for (size_t k = 0; k < NA; k++) { off[k] = at; at += (a[k].bytes + 15) & ~(size_t)15; }
    uint8_t *d = nullptr, *p[NA];
    SGO_HIP(hipMalloc((void **)&d, at + record_bytes));
    for (size_t k = 0; k < NA; k++) p[k] = d + off[k];
    int rc = SGO_OK;
    hipError_t e = hipMemcpy(d + at, records, record_bytes, hipMemcpyHostToDevice);
    for (size_t k = 0; k < NA; k++)
        if (e == hipSuccess && a[k].up) e = hipMemcpy(p[k], a[k].up, a[k].bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) rc = launch(reinterpret_cast<const uint32_t *>(d + at), p);
    for (size_t k = 0; k < NA; k++)
        if (e == hipSuccess && rc == SGO_OK && a[k].down) e = hipMemcpy(a[k].down, p[k], a[k].bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, who, __FILE__, __LINE__);
    return rc;
}

}  // namespace sgo
