// dlp_relayout.hip — the stored tableau of a live session moved between the full layout and the
// condensed one (dlp_session_set_defer).
//
//   cond_expand_kernel   condensed -> full: the rule of the host read-out (cond_read_rows), on the
//                        device: a nonbasic variable's entry from its slot, a basic variable's unit
//                        entry (1.0 in its row, +0.0 elsewhere and in the objective row), the RHS at
//                        column N, +0.0 in the padding up to the stride;
//   cond_pack_kernel     full -> condensed: slot s takes column var_of[s], slot n column N, +0.0 in
//                        the padding.
//
// Both copy values and compute nothing, so the result cannot depend on the grid.  One workgroup
// writes a band of kRelayoutRows rows of one 512-column tile of the DESTINATION (256 lanes x 2
// doubles, one 16-B vector store per lane and row: a wave writes 1 KiB of consecutive bytes).  The
// lane's two source columns (slot_of / var_of) are read once and serve every row of the band; the
// band's basic variables are wave-uniform scalar loads, one per row.  The reads are 8-B gathers
// inside one source row, served by L2 and the Infinity Cache behind it; they are not staged through
// LDS: with this tiling every tile's workgroup would have to stage the whole source row to use a
// seventeenth of it (C2), and a C3 row (262 KB) does not fit.  The price is measured in DESIGN.md
// §22: with the slots in solve order every 8-B gather pulls its own 128-B line into L1, and the
// expand runs at about 0.5 TB/s at C2 (7-9x a device copy's time, 0.8 ms); with the slots nearly in
// order (C3 after 256 pivots) both kernels run at a device copy's rate.
// 64-bit indexing throughout (a C3 full layout is 17 GB); vector stores only; no atomics.
#include <hip/hip_runtime.h>

#include "dlp_internal.h"

namespace dlp {
namespace {

constexpr int kRelayoutThreads = kUpdThreads;   // 256 lanes x 2 doubles = one 512-column tile
constexpr int kRelayoutRows = 8;                // rows per workgroup band

// dst (full layout: N variables, RHS at N, stride ld_d) from src (condensed: n slots, RHS at slot
// n, stride ld_s).  rows_total = constraint rows + the objective row; basis[r]: the basic variable
// of constraint row r.
__global__ __launch_bounds__(kRelayoutThreads) void cond_expand_kernel(
    const double* __restrict__ src, int64_t ld_s, int64_t n, double* __restrict__ dst, int64_t ld_d,
    int64_t N, int64_t rows_total, const int32_t* __restrict__ slot_of,
    const int32_t* __restrict__ basis, int64_t ntiles) {
    const int64_t band = (int64_t)blockIdx.x / ntiles, tile = (int64_t)blockIdx.x % ntiles;
    const int64_t j = tile * kUpdTile + (int64_t)threadIdx.x * kUpdVec;
    if (j >= ld_d) return;   // (ld_d is even: the lane's pair is inside the stride or outside it)
    // the source column of each destination column: a slot, the RHS slot, or none (-1)
    int64_t sc[kUpdVec];
#pragma unroll
    for (int k = 0; k < kUpdVec; ++k) {
        const int64_t v = j + k;
        int64_t s = -1;
        if (v < N)
            s = slot_of[v];
        else if (v == N)
            s = n;
        sc[k] = (s >= 0 && s <= n) ? s : -1;
    }
    // every load of the band is requested (rows past the end clamped), then the stores: 16 gathers
    // in flight per lane
    const int64_t r0 = band * kRelayoutRows;
    double out[kRelayoutRows][kUpdVec];
#pragma unroll
    for (int u = 0; u < kRelayoutRows; ++u) {
        const int64_t r = r0 + u < rows_total ? r0 + u : rows_total - 1;
        const int64_t bv = r < rows_total - 1 ? (int64_t)basis[r] : -1;   // wave-uniform
        const double* row = src + r * ld_s;
#pragma unroll
        for (int k = 0; k < kUpdVec; ++k) {
            const int64_t v = j + k;
            out[u][k] = sc[k] >= 0 ? row[sc[k]] : ((v < N && v == bv) ? 1.0 : 0.0);
        }
    }
#pragma unroll
    for (int u = 0; u < kRelayoutRows; ++u)
        if (r0 + u < rows_total)
            *reinterpret_cast<double2*>(dst + (r0 + u) * ld_d + j) = make_double2(out[u][0], out[u][1]);
}

// dst (condensed: n slots, RHS at slot n, stride ld_d) from src (full layout, RHS at column N,
// stride ld_s).  var_of[s] (s < ld_d): the variable of slot s, -1 for the RHS slot and the padding.
__global__ __launch_bounds__(kRelayoutThreads) void cond_pack_kernel(
    const double* __restrict__ src, int64_t ld_s, int64_t N, double* __restrict__ dst, int64_t ld_d,
    int64_t n, int64_t rows_total, const int32_t* __restrict__ var_of, int64_t ntiles) {
    const int64_t band = (int64_t)blockIdx.x / ntiles, tile = (int64_t)blockIdx.x % ntiles;
    const int64_t j = tile * kUpdTile + (int64_t)threadIdx.x * kUpdVec;
    if (j >= ld_d) return;
    int64_t sc[kUpdVec];
#pragma unroll
    for (int k = 0; k < kUpdVec; ++k) {
        const int64_t s = j + k;
        int64_t v = -1;
        if (s < n)
            v = var_of[s];
        else if (s == n)
            v = N;
        sc[k] = (v >= 0 && v <= N) ? v : -1;
    }
    const int64_t r0 = band * kRelayoutRows;
    double out[kRelayoutRows][kUpdVec];
#pragma unroll
    for (int u = 0; u < kRelayoutRows; ++u) {
        const int64_t r = r0 + u < rows_total ? r0 + u : rows_total - 1;
        const double* row = src + r * ld_s;
#pragma unroll
        for (int k = 0; k < kUpdVec; ++k) out[u][k] = sc[k] >= 0 ? row[sc[k]] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kRelayoutRows; ++u)
        if (r0 + u < rows_total)
            *reinterpret_cast<double2*>(dst + (r0 + u) * ld_d + j) = make_double2(out[u][0], out[u][1]);
}

// blocks = row bands x destination tiles, in one grid dimension (C3: 4,097 x 129)
bool relayout_grid(int64_t rows_total, int64_t ld_d, int64_t* ntiles, int64_t* blocks) {
    *ntiles = (ld_d + kUpdTile - 1) / kUpdTile;
    const int64_t bands = (rows_total + kRelayoutRows - 1) / kRelayoutRows;
    *blocks = bands * *ntiles;
    return rows_total > 0 && ld_d > 0 && ld_d % 2 == 0 && *blocks < ((int64_t)1 << 31);
}

}  // namespace

hipError_t launch_cond_expand(const double* src, int64_t ld_s, int64_t n, double* dst, int64_t ld_d,
                              int64_t N, int64_t rows_total, const int32_t* slot_of, const int32_t* basis,
                              hipStream_t s) {
    int64_t ntiles = 0, blocks = 0;
    if (!relayout_grid(rows_total, ld_d, &ntiles, &blocks) || n + 1 > ld_s || N + 1 > ld_d)
        return hipErrorInvalidValue;
    cond_expand_kernel<<<(unsigned)blocks, kRelayoutThreads, 0, s>>>(src, ld_s, n, dst, ld_d, N, rows_total,
                                                                   slot_of, basis, ntiles);
    return hipGetLastError();
}

hipError_t launch_cond_pack(const double* src, int64_t ld_s, int64_t N, double* dst, int64_t ld_d, int64_t n,
                            int64_t rows_total, const int32_t* var_of, hipStream_t s) {
    int64_t ntiles = 0, blocks = 0;
    if (!relayout_grid(rows_total, ld_d, &ntiles, &blocks) || N + 1 > ld_s || n + 1 > ld_d)
        return hipErrorInvalidValue;
    cond_pack_kernel<<<(unsigned)blocks, kRelayoutThreads, 0, s>>>(src, ld_s, N, dst, ld_d, n, rows_total, var_of,
                                                                 ntiles);
    return hipGetLastError();
}

}  // namespace dlp
