// dlp_addrows.hip — constraint rows added to a live session (dlp_session_add_rows).
//
// The session's LP gains r rows G x <= h.  The stored tableau grows by r rows (the full layout
// also by r slack columns, which moves the RHS column and may change the row stride), and the new
// rows are expressed in the current basis by the row rule of dlp_batch_add_rows:
//   acc = g_v (structural v), +0.0 (slack), h_t (RHS);
//   for the old rows i ascending with gB_i = g[basis[i]] != 0.0:  acc = acc - (gB_i * T[i][v]),
//   product rounded, then the difference rounded (no fma);
//   the column of a basic variable is exact +0.0, the row's own slack 1.0.
//
//   grow_copy_kernel   old tableau -> new tableau, values only: the m constraint rows keep their
//                      index, the objective row moves to row m + r; columns [0, ncopy) keep their
//                      place, the RHS moves from column rhs_s to rhs_d, everything else (the new
//                      slack columns, the padding) is +0.0.  Tiled by the DESTINATION as
//                      dlp_relayout.hip: 512-column tiles, one 16-B store per lane and row, a
//                      band of kGrowRows rows per workgroup.
//   row_fold_kernel    rows m .. m+r-1 of the new tableau.  A lane owns one stored column
//                      (consecutive lanes, consecutive columns: every old-row load is one
//                      coalesced 512-B wave access).  The host hands it the ascending list of the R
//                      contributing old rows (some new row has gB_i != 0) and the coefficient
//                      matrix coef[t][k] = gB of new row t at list entry k; both are wave-uniform
//                      (scalar loads).  Each old row is read ONCE for a group of RT new rows (RT
//                      accumulators per lane; blockIdx.y is the group); a coefficient of exactly
//                      0.0 leaves its accumulator untouched (a select: acc - (0 * t) could flip the
//                      sign of a zero, and the rule skips the row).  kFoldRows row loads are
//                      requested ahead of the kFoldRows being folded, as in reopt_kernel, so the
//                      only dependent chain is the subtract.  It reads the OLD tableau, which
//                      nothing writes during the call.
//
// One ascending chain per entry; nothing depends on the grid, K, the layout or tuning.  64-bit
// indexing throughout (a C3 full layout is 17 GB); vector stores only; no atomics.
#include <hip/hip_runtime.h>

#include "dlp_internal.h"

namespace dlp {
namespace {

constexpr int kGrowThreads = kUpdThreads;   // 256 lanes x 2 doubles = one 512-column tile
constexpr int kGrowRows = 8;                // rows per workgroup band
constexpr int kFoldThreads = 64;            // one wave: a 64-column tile per workgroup
constexpr int kFoldRows = 16;               // old rows per batch; two batches in flight
constexpr int kFoldRT = 4;                  // new rows folded per read of an old row
constexpr int64_t kFoldGridY = 65535;       // groups per launch (gridDim.y); more rows take further launches

// k-th copied row (k in [0, m]): the constraint rows keep their index, the objective row (k = m) goes
// to row m + r.
__global__ __launch_bounds__(kGrowThreads) void grow_copy_kernel(
    const double* __restrict__ src, int64_t ld_s, double* __restrict__ dst, int64_t ld_d, int64_t m,
    int64_t r, int64_t ncopy, int64_t rhs_s, int64_t rhs_d, int64_t ntiles) {
    const int64_t band = (int64_t)blockIdx.x / ntiles, tile = (int64_t)blockIdx.x % ntiles;
    const int64_t j = tile * kUpdTile + (int64_t)threadIdx.x * kUpdVec;
    if (j >= ld_d) return;   // (ld_d is even: the lane's pair is inside the stride or outside it)
    // the source column of each destination column, or none (-1: +0.0)
    int64_t sc[kUpdVec];
#pragma unroll
    for (int k = 0; k < kUpdVec; ++k) {
        const int64_t v = j + k;
        sc[k] = v < ncopy ? v : (v == rhs_d ? rhs_s : -1);
    }
    const int64_t k0 = band * kGrowRows;
    double out[kGrowRows][kUpdVec];
#pragma unroll
    for (int u = 0; u < kGrowRows; ++u) {
        const int64_t k = k0 + u <= m ? k0 + u : m;   // rows past the end clamped (loaded, not stored)
        const double* row = src + k * ld_s;
#pragma unroll
        for (int c = 0; c < kUpdVec; ++c) out[u][c] = sc[c] >= 0 ? row[sc[c]] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kGrowRows; ++u) {
        const int64_t k = k0 + u;
        if (k <= m) {
            const int64_t rd = k < m ? k : m + r;
            *reinterpret_cast<double2*>(dst + rd * ld_d + j) = make_double2(out[u][0], out[u][1]);
        }
    }
}

// acc = acc - (g * t) where g != 0.0, else acc: two roundings, never contracted (whatever
// -ffp-contract says)
__device__ __forceinline__ double fold_sub(double acc, double g, double t) {
#pragma clang fp contract(off)
    const double prod = g * t;
    const double next = acc - prod;
    return g != 0.0 ? next : acc;
}

// coef: (groups * RT) x R row-major, the rows past r zero.  G: r x n, h: r (device).  var_of: the
// condensed layout's slot map (NULL: the full layout, column = variable).  basic (full layout
// only, else NULL): [ncopy] nonzero at the columns of basic variables.  slack0 (full layout, else
// -1): the column of new row 0's own slack (the old N).
template <int RT>
__global__ __launch_bounds__(kFoldThreads) void row_fold_kernel(
    const double* __restrict__ src, int64_t ld_s, double* __restrict__ dst, int64_t ld_d, int64_t m,
    int64_t r, int64_t n, int64_t ncopy, int64_t rhs_s, int64_t rhs_d, int64_t slack0,
    const int32_t* __restrict__ rlist, const double* __restrict__ coef, int64_t R,
    const double* __restrict__ G, const double* __restrict__ h, const int32_t* __restrict__ var_of,
    const int32_t* __restrict__ basic, int64_t group0) {
    const int64_t j = (int64_t)blockIdx.x * kFoldThreads + threadIdx.x;
    const int64_t t0 = (group0 + (int64_t)blockIdx.y) * RT;   // (a launch holds up to kFoldGridY groups)
    const int64_t jj = j < ld_d ? j : ld_d - 1;   // the tail lanes load a valid column, store nothing
    // the source column (none: the new slack columns and the padding, which load column 0 and keep
    // nothing of it) and the variable of this stored column (-1: RHS / none)
    const bool is_var = jj < ncopy, is_rhs = jj == rhs_d;
    const int64_t sc = is_var ? jj : (is_rhs ? rhs_s : 0);
    int64_t v = -1;
    if (is_var) v = var_of ? (int64_t)var_of[jj] : jj;
    double acc[RT];
#pragma unroll
    for (int k = 0; k < RT; ++k) {
        const int64_t t = t0 + k < r ? t0 + k : r - 1;
        acc[k] = (v >= 0 && v < n) ? G[t * n + v] : (is_rhs ? h[t] : 0.0);
    }
    const double* col = src + sc;
    const double* cf = coef + t0 * R;   // cf[k * R + i]: wave-uniform

    const int64_t nfull = R / kFoldRows * kFoldRows;
    if (nfull > 0) {
        double cur[kFoldRows];
#pragma unroll
        for (int u = 0; u < kFoldRows; ++u) cur[u] = col[(int64_t)rlist[u] * ld_s];
        for (int64_t i = 0; i < nfull; i += kFoldRows) {
            // the next batch (the last iteration requests its own batch again: no branch between
            // the loads and the fold, so the waits stay counted)
            const int64_t in = i + kFoldRows < nfull ? i + kFoldRows : i;
            double nxt[kFoldRows];
#pragma unroll
            for (int u = 0; u < kFoldRows; ++u) nxt[u] = col[(int64_t)rlist[in + u] * ld_s];
#pragma unroll
            for (int u = 0; u < kFoldRows; ++u)
#pragma unroll
                for (int k = 0; k < RT; ++k) acc[k] = fold_sub(acc[k], cf[k * R + i + u], cur[u]);
#pragma unroll
            for (int u = 0; u < kFoldRows; ++u) cur[u] = nxt[u];
        }
    }
    if (nfull < R) {   // the last, partial batch: every load requested (clamped), then the fold
        double cur[kFoldRows];
#pragma unroll
        for (int u = 0; u < kFoldRows; ++u) {
            const int64_t i = nfull + u < R ? nfull + u : R - 1;
            cur[u] = col[(int64_t)rlist[i] * ld_s];
        }
#pragma unroll
        for (int u = 0; u < kFoldRows; ++u)
            if (nfull + u < R) {
#pragma unroll
                for (int k = 0; k < RT; ++k) acc[k] = fold_sub(acc[k], cf[k * R + nfull + u], cur[u]);
            }
    }
    const bool zero = (!is_var && !is_rhs) || (basic && is_var && basic[jj]);
    if (j < ld_d) {
#pragma unroll
        for (int k = 0; k < RT; ++k) {
            const int64_t t = t0 + k;
            if (t < r) {
                double out = zero ? 0.0 : acc[k];
                if (slack0 >= 0 && j == slack0 + t) out = 1.0;
                dst[(m + t) * ld_d + j] = out;
            }
        }
    }
}

}  // namespace

int add_rows_fold_group() { return kFoldRT; }

// Whether the two launches below accept the geometry (nothing here depends on the values): the host
// asks before it changes anything, so a refusal cannot leave a half-grown session.
bool add_rows_launchable(int64_t ld_s, int64_t ld_d, int64_t m, int64_t r, int64_t ncopy, int64_t rhs_s,
                         int64_t rhs_d, int64_t slack0) {
    const int64_t ntiles = (ld_d + kUpdTile - 1) / kUpdTile;
    const int64_t bands = (m + 1 + kGrowRows - 1) / kGrowRows;
    const int64_t fold_blocks = (ld_d + kFoldThreads - 1) / kFoldThreads;
    return m >= 0 && r > 0 && ld_d > 0 && ld_d % 2 == 0 && bands * ntiles < ((int64_t)1 << 31) &&
           fold_blocks < ((int64_t)1 << 31) && ncopy <= rhs_s && ncopy <= rhs_d && rhs_s + 1 <= ld_s &&
           rhs_d + 1 <= ld_d && (slack0 < 0 || slack0 + r <= rhs_d);
}

hipError_t launch_grow_copy(const double* src, int64_t ld_s, double* dst, int64_t ld_d, int64_t m, int64_t r,
                            int64_t ncopy, int64_t rhs_s, int64_t rhs_d, hipStream_t s) {
    const int64_t ntiles = (ld_d + kUpdTile - 1) / kUpdTile;
    const int64_t bands = (m + 1 + kGrowRows - 1) / kGrowRows;
    const int64_t blocks = bands * ntiles;
    if (!add_rows_launchable(ld_s, ld_d, m, r, ncopy, rhs_s, rhs_d, -1)) return hipErrorInvalidValue;
    grow_copy_kernel<<<(unsigned)blocks, kGrowThreads, 0, s>>>(src, ld_s, dst, ld_d, m, r, ncopy, rhs_s, rhs_d,
                                                             ntiles);
    return hipGetLastError();
}

hipError_t launch_row_fold(const double* src, int64_t ld_s, double* dst, int64_t ld_d, int64_t m, int64_t r,
                           int64_t n, int64_t ncopy, int64_t rhs_s, int64_t rhs_d, int64_t slack0,
                           const int32_t* rlist, const double* coef, int64_t R, const double* G, const double* h,
                           const int32_t* var_of, const int32_t* basic, hipStream_t s) {
    const int64_t blocks = (ld_d + kFoldThreads - 1) / kFoldThreads;
    const int64_t groups = (r + kFoldRT - 1) / kFoldRT;
    if (!add_rows_launchable(ld_s, ld_d, m, r, ncopy, rhs_s, rhs_d, slack0) || R < 0 || R > m)
        return hipErrorInvalidValue;
    // the groups go on gridDim.y, kFoldGridY of them per launch (r > 262,140 takes a second one)
    for (int64_t g0 = 0; g0 < groups; g0 += kFoldGridY) {
        const int64_t gy = groups - g0 < kFoldGridY ? groups - g0 : kFoldGridY;
        row_fold_kernel<kFoldRT><<<dim3((unsigned)blocks, (unsigned)gy), kFoldThreads, 0, s>>>(
            src, ld_s, dst, ld_d, m, r, n, ncopy, rhs_s, rhs_d, slack0, rlist, coef, R, G, h, var_of, basic, g0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dlp
