// dlp_addcols.hip — variables (columns) added to a live session (dlp_session_add_cols).
//
// The session's LP gains k variables with constraint columns P (m x k) and costs d.  The stored
// tableau is widened by k columns (the full layout's slack block and RHS move right by k, the
// condensed layout's RHS slot moves from n to n + k; either may change the row stride), and the new
// columns are expressed in the current basis by the column rule of dlp_batch_add_cols:
//   for new variable t and every stored row r (the objective row included):
//   acc = +0.0;  for l = 0 .. m-1 ascending:  acc = acc + (Tfull[r][n+l] * p_l),
//   product rounded, then the sum rounded (no fma);  constraint rows store acc, the objective row
//   acc - d_t.
// acc starts at +0.0 and is never -0.0, so a term whose coefficient or p_l is +-0 changes no bit of
// it: such terms may be skipped or folded alike (no select, unlike the row rule).
//
//   widen_copy_kernel  old tableau -> new tableau, values only, every row at its own index:
//                      destination column j < n from source j, n + k <= j < n + k + tail from
//                      source j - k (tail = m: the full layout's slack block; 0: condensed), the RHS
//                      from rhs_s to rhs_d, everything else +0.0 (the padding, and the new columns,
//                      which the fold overwrites).  Tiled by the DESTINATION as grow_copy_kernel:
//                      512-column tiles, one 16-B store per lane and row, a band of kWidenRows rows
//                      per workgroup, all of a lane's loads requested before its stores.  The
//                      shifted source is only 8-B aligned when k is odd: 8-B loads, 16-B stores.
//   col_fold_kernel    the k new columns.  The host hands it the ascending list of the R
//                      contributing slacks l (some p_{l,t} != 0.0), each as a SOURCE: a stored
//                      column (full layout: n + l; condensed: slot_of[n + l]) or -(row + 1) for a
//                      slack that is basic in `row` of a condensed session (its column is that
//                      row's unit vector, objective entry +0.0: nothing is loaded), and the
//                      CT-padded coefficients coef[t][entry] (wave-uniform: scalar loads).  The data
//                      movement is rhs_rebuild_kernel's (dlp_dual.hip): one wave owns a band of
//                      kColTile stored rows; a tile of (band rows x kColTile list entries) is
//                      fetched with lane = list entry (full layout, contiguous list: one coalesced
//                      512-B segment per row; condensed: a gather inside one row), staged
//                      transposed in LDS with a padded stride, and folded with lane = row, entries
//                      ascending, while the next tile's loads are in flight.  A lane carries CT
//                      accumulators, so one read of the slack block serves CT new columns;
//                      blockIdx.y is the column group.  The band stays at 64 rows although that
//                      gives few workgroups on a mid-size tableau: a narrower band idles the fold's
//                      lanes (lane = row) for the same loads, and the chain over l cannot be split
//                      across waves without a tree, which the rule excludes.
//                      It reads the OLD tableau, which nothing writes during the call, and writes
//                      only the new columns of the new one, after widen_copy_kernel in stream order.
//
// One ascending chain per entry; the k columns do not see each other; nothing depends on the grid,
// K, the layout or tuning.  64-bit indexing throughout (a C3 full layout is 17 GB); vector stores
// only; no atomics.
#include <hip/hip_runtime.h>

#include "dlp_internal.h"

namespace dlp {
namespace {

constexpr int kWidenThreads = kUpdThreads;   // 256 lanes x 2 doubles = one 512-column tile
constexpr int kWidenRows = 8;                // rows per workgroup band
constexpr int kColTile = 64;                 // band rows = lanes = list entries per staged tile
constexpr int kColStride = kColTile + 1;     // padded LDS row stride (doubles): lane r reads r * 65 + e,
                                             // a different bank pair per lane
constexpr int kColCT = 4;                    // new columns folded per read of the slack block
constexpr int64_t kColGridY = 65535;         // groups per launch (gridDim.y); more columns take further launches

__global__ __launch_bounds__(kWidenThreads) void widen_copy_kernel(
    const double* __restrict__ src, int64_t ld_s, double* __restrict__ dst, int64_t ld_d, int64_t rows_total,
    int64_t n, int64_t k, int64_t tail, int64_t rhs_s, int64_t rhs_d, int64_t ntiles) {
    const int64_t band = (int64_t)blockIdx.x / ntiles, tile = (int64_t)blockIdx.x % ntiles;
    const int64_t j = tile * kUpdTile + (int64_t)threadIdx.x * kUpdVec;
    if (j >= ld_d) return;   // (ld_d is even: the lane's pair is inside the stride or outside it)
    // the source column of each destination column, or none (-1: +0.0)
    int64_t sc[kUpdVec];
#pragma unroll
    for (int c = 0; c < kUpdVec; ++c) {
        const int64_t v = j + c;
        sc[c] = v < n ? v : ((v >= n + k && v < n + k + tail) ? v - k : (v == rhs_d ? rhs_s : -1));
    }
    const int64_t k0 = band * kWidenRows;
    double out[kWidenRows][kUpdVec];
#pragma unroll
    for (int u = 0; u < kWidenRows; ++u) {
        const int64_t r = k0 + u < rows_total ? k0 + u : rows_total - 1;   // rows past the end clamped (loaded, not stored)
        const double* row = src + r * ld_s;
#pragma unroll
        for (int c = 0; c < kUpdVec; ++c) out[u][c] = sc[c] >= 0 ? row[sc[c]] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kWidenRows; ++u) {
        const int64_t r = k0 + u;
        if (r < rows_total) *reinterpret_cast<double2*>(dst + r * ld_d + j) = make_double2(out[u][0], out[u][1]);
    }
}

// acc = acc + (t * p): two roundings, never contracted (whatever -ffp-contract says)
__device__ __forceinline__ double col_step(double acc, double t, double p) {
#pragma clang fp contract(off)
    const double prod = t * p;
    return acc + prod;
}

// list: R sources, ascending in l.  coef: (groups * CT) x R row-major, the rows past k zero.  d: k
// costs (device).  rows: the constraint rows (the objective row is stored row `rows`).  col0: the
// destination column of new variable 0.
template <int CT>
__global__ __launch_bounds__(kColTile) void col_fold_kernel(
    const double* __restrict__ src, int64_t ld_s, double* __restrict__ dst, int64_t ld_d, int64_t rows,
    int64_t k, int64_t col0, const int32_t* __restrict__ list, const double* __restrict__ coef, int64_t R,
    const double* __restrict__ d, int64_t group0) {
    __shared__ double tile[kColTile * kColStride];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kColTile;
    const int64_t t0 = (group0 + (int64_t)blockIdx.y) * CT;   // (a launch holds up to kColGridY groups)
    const int64_t ntile = (R + kColTile - 1) / kColTile;
    double acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0.0;
    double cur[kColTile];
    // entry e of the list in lane e of the tile: a stored column down the band's rows (a pointer
    // walked down, stopping at the objective row: rows past it are clamped, never folded into a
    // stored value), or the unit vector of a basic slack, which loads nothing
    auto load_tile = [&](int64_t t) {
        int64_t e = t * kColTile + lane;
        e = e < R ? e : R - 1;
        const int32_t sc = list[e];
        if (sc >= 0) {
            const double* p = src + r0 * ld_s + sc;
#pragma unroll
            for (int rr = 0; rr < kColTile; ++rr) {
                cur[rr] = *p;
                p += (r0 + rr < rows) ? ld_s : 0;
            }
        } else {
            const int64_t ur = -(int64_t)sc - 1;
#pragma unroll
            for (int rr = 0; rr < kColTile; ++rr) cur[rr] = (r0 + rr == ur) ? 1.0 : 0.0;
        }
    };
    if (ntile > 0) load_tile(0);
    for (int64_t t = 0; t < ntile; ++t) {
#pragma unroll
        for (int rr = 0; rr < kColTile; ++rr) tile[rr * kColStride + lane] = cur[rr];
        __syncthreads();
        // the next tile's loads are in flight during the fold (the last iteration requests its own
        // tile again: the same code path every time)
        load_tile(t + 1 < ntile ? t + 1 : t);
        const int64_t l0 = t * kColTile;
        const int emax = (int)(R - l0 < kColTile ? R - l0 : kColTile);
        const double* mine = tile + lane * kColStride;
        const double* cf = coef + t0 * R + l0;   // cf[c * R + e]: wave-uniform
        if (emax == kColTile) {
#pragma unroll 16
            for (int e = 0; e < kColTile; ++e) {
                const double v = mine[e];
#pragma unroll
                for (int c = 0; c < CT; ++c) acc[c] = col_step(acc[c], v, cf[c * R + e]);
            }
        } else {
            for (int e = 0; e < emax; ++e) {
                const double v = mine[e];
#pragma unroll
                for (int c = 0; c < CT; ++c) acc[c] = col_step(acc[c], v, cf[c * R + e]);
            }
        }
        __syncthreads();
    }
    const int64_t r = r0 + lane;
    if (r <= rows) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int64_t t = t0 + c;
            if (t < k) dst[r * ld_d + col0 + t] = r == rows ? acc[c] - d[t] : acc[c];
        }
    }
}

}  // namespace

int add_cols_fold_group() { return kColCT; }

// Whether the two launches below accept the geometry (nothing here depends on the values): the host
// asks before it changes anything, so a refusal cannot leave a half-widened session.
bool add_cols_launchable(int64_t ld_s, int64_t ld_d, int64_t m, int64_t n, int64_t k, int64_t tail,
                         int64_t rhs_s, int64_t rhs_d) {
    const int64_t ntiles = (ld_d + kUpdTile - 1) / kUpdTile;
    const int64_t bands = (m + 1 + kWidenRows - 1) / kWidenRows;
    const int64_t fold_bands = (m + 1 + kColTile - 1) / kColTile;
    return m >= 0 && n >= 0 && k > 0 && (tail == 0 || tail == m) && ld_d > 0 && ld_d % 2 == 0 &&
           bands * ntiles < ((int64_t)1 << 31) && fold_bands < ((int64_t)1 << 31) && rhs_s == n + tail &&
           rhs_d == n + k + tail && rhs_s + 1 <= ld_s && rhs_d + 1 <= ld_d;
}

hipError_t launch_widen_copy(const double* src, int64_t ld_s, double* dst, int64_t ld_d, int64_t m, int64_t n,
                             int64_t k, int64_t tail, int64_t rhs_s, int64_t rhs_d, hipStream_t s) {
    const int64_t ntiles = (ld_d + kUpdTile - 1) / kUpdTile;
    const int64_t bands = (m + 1 + kWidenRows - 1) / kWidenRows;
    if (!add_cols_launchable(ld_s, ld_d, m, n, k, tail, rhs_s, rhs_d)) return hipErrorInvalidValue;
    widen_copy_kernel<<<(unsigned)(bands * ntiles), kWidenThreads, 0, s>>>(src, ld_s, dst, ld_d, m + 1, n, k, tail,
                                                                         rhs_s, rhs_d, ntiles);
    return hipGetLastError();
}

hipError_t launch_col_fold(const double* src, int64_t ld_s, double* dst, int64_t ld_d, int64_t m, int64_t n,
                           int64_t k, int64_t tail, int64_t rhs_s, int64_t rhs_d, const int32_t* list,
                           const double* coef, int64_t R, const double* d, hipStream_t s) {
    const int64_t bands = (m + 1 + kColTile - 1) / kColTile;
    const int64_t groups = (k + kColCT - 1) / kColCT;
    if (!add_cols_launchable(ld_s, ld_d, m, n, k, tail, rhs_s, rhs_d) || R < 0 || R > m)
        return hipErrorInvalidValue;
    // the groups go on gridDim.y, kColGridY of them per launch (k > 262,140 takes a second one)
    for (int64_t g0 = 0; g0 < groups; g0 += kColGridY) {
        const int64_t gy = groups - g0 < kColGridY ? groups - g0 : kColGridY;
        col_fold_kernel<kColCT><<<dim3((unsigned)bands, (unsigned)gy), kColTile, 0, s>>>(
            src, ld_s, dst, ld_d, m, k, n, list, coef, R, d, g0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dlp
