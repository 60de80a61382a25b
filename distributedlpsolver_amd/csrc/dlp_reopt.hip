// dlp_reopt.hip — objective-row rebuild of a live session (dlp_session_set_objective).
//
// The tableau in HBM is a basic feasible tableau for any objective, so a new c only needs a
// new objective row: z_j = c_B^T T[:, j] - c_j, folded in one fixed order:
//   acc = -c_j (structural j) or +0.0 (slack, RHS);
//   for the rows i ascending whose basic variable costs cB_i != 0:  acc = acc + (cB_i * T[i][j]),
//   product rounded, then the sum rounded (no fma);
//   z_j = acc, and +0.0 for a basic variable's column.
// The host hands the kernel the ascending (row, cB) list of the contributing rows; the kernel is
// one read-only stream over those rows of the stored tableau.  A lane owns one stored column
// (consecutive lanes, consecutive columns: every row load is one coalesced 512-B wave access),
// the row index and cB are wave-uniform (scalar loads), and the only dependent chain is the add:
// kReoptRows row loads are requested ahead of the kReoptRows being folded, so 2 * kReoptRows
// loads per lane are in flight.  One wave per workgroup spreads the columns over as many CUs as
// there are 64-column tiles.  The fold order never depends on the grid: a column is one lane.
//
// Condensed sessions store slots: var_of[slot] names the variable whose cost
// starts the fold, and no basic column is stored.  Full-layout sessions pass basic[j] != 0 for
// the columns of basic variables, which get +0.0.
#include <hip/hip_runtime.h>

#include "dlp_internal.h"

namespace dlp {
namespace {

constexpr int kReoptThreads = 64;   // one wave: a 64-column tile per workgroup
constexpr int kReoptRows = 16;      // rows per batch; two batches in flight

// acc = acc + (cb * t): two roundings, never contracted (whatever -ffp-contract says)
__device__ __forceinline__ double fold_step(double acc, double cb, double t) {
#pragma clang fp contract(off)
    const double prod = cb * t;
    return acc + prod;
}

__global__ __launch_bounds__(kReoptThreads) void reopt_kernel(
    double* __restrict__ T, int64_t ld, int64_t rows, int64_t width, int64_t n, int64_t N,
    const int32_t* __restrict__ rlist, const double* __restrict__ cblist, int64_t R,
    const double* __restrict__ c, const int32_t* __restrict__ var_of,
    const int32_t* __restrict__ basic, DevState* st, int pricing) {
    const int64_t j = (int64_t)blockIdx.x * kReoptThreads + threadIdx.x;
    const int64_t jj = j < width ? j : width - 1;   // the tail lanes load a valid column, store nothing
    // the variable of this stored column (-1: RHS / padding)
    int64_t v;
    if (var_of)
        v = var_of[jj];
    else
        v = jj < N ? jj : -1;
    double acc = (v >= 0 && v < n) ? -c[v] : 0.0;
    const double* col = T + jj;

    const int64_t nfull = R / kReoptRows * kReoptRows;
    if (nfull > 0) {
        double cur[kReoptRows];
#pragma unroll
        for (int u = 0; u < kReoptRows; ++u) cur[u] = col[(int64_t)rlist[u] * ld];
        for (int64_t r = 0; r < nfull; r += kReoptRows) {
            // the next batch (the last iteration requests its own batch again: no branch between
            // the loads and the fold, so the waits stay counted)
            const int64_t rn = r + kReoptRows < nfull ? r + kReoptRows : r;
            double nxt[kReoptRows];
#pragma unroll
            for (int u = 0; u < kReoptRows; ++u) nxt[u] = col[(int64_t)rlist[rn + u] * ld];
#pragma unroll
            for (int u = 0; u < kReoptRows; ++u) acc = fold_step(acc, cblist[r + u], cur[u]);
#pragma unroll
            for (int u = 0; u < kReoptRows; ++u) cur[u] = nxt[u];
        }
    }
    if (nfull < R) {   // the last, partial batch: every load requested (clamped), then the fold
        double cur[kReoptRows];
#pragma unroll
        for (int u = 0; u < kReoptRows; ++u) {
            const int64_t r = nfull + u < R ? nfull + u : R - 1;
            cur[u] = col[(int64_t)rlist[r] * ld];
        }
#pragma unroll
        for (int u = 0; u < kReoptRows; ++u)
            if (nfull + u < R) acc = fold_step(acc, cblist[nfull + u], cur[u]);
    }
    if (basic && basic[jj]) acc = 0.0;
    if (j < width) T[rows * ld + j] = acc;
    if (j == 0) {   // runnable again, Bland state as at the Phase II switch (carry_in_kernel)
        st->status = DLP_RUNNING;
        st->q = -1;
        st->bland = pricing == DLP_PRICING_BLAND ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_reopt(const Geometry& g, int64_t n, int64_t N, const int32_t* rlist,
                        const double* cblist, int64_t R, const double* c, const int32_t* basic,
                        DevState* st, int pricing, hipStream_t s) {
    const int64_t blocks = (g.width + kReoptThreads - 1) / kReoptThreads;
    reopt_kernel<<<(unsigned)blocks, kReoptThreads, 0, s>>>(g.T, g.ld, g.rows, g.width, n, N, rlist, cblist, R, c,
                                                           g.cd.on ? g.cd.var_of : nullptr, basic, st, pricing);
    return hipGetLastError();
}

}  // namespace dlp
