// dlp_dual.hip — dual simplex of a live session after new right-hand sides
// (dlp_session_set_rhs; the rule is dlp_batch_resolve_rhs's).
//
// After a primal solve the resident full-layout tableau is dual feasible for every b and its
// slack columns are B^-1.  A new b therefore needs a new RHS column,
//   T[r][N] = fold over l ascending of (T[r][n+l] * b_l), from +0.0, product rounded, then the sum,
// and dual pivots from the basis as it stands.  Three kernels live here; the rest of a dual pivot
// is the eager primal's (gather_q_kernel, prow_kernel, update_kernel) with a negative pivot:
//   rhs_rebuild_kernel  the fold, one lane per stored row, the slack block staged through LDS
//   dual_row_kernel     leaving row: argmin of T[i][N] < -tol_feas (ties: smallest basis[i];
//                       Bland: smallest basis[i] among the eligible); none -> DLP_OK
//   dual_col_kernel     entering column: argmin of max(z_j, +0) / -T[p][j] over T[p][j] < -tol_piv
//                       (ties: smallest j); none -> DLP_INFEASIBLE; else the selection
//                       (do_select: q, piv, leaving, basis[p], ratio, Bland flag, npivots, log)
// Both selections use the candidate order of the primal ratio test (valid, value, index), which is
// total, so any reduction tree picks the same winner; the per-workgroup partials are handed to the
// last workgroup exactly as ratio_kernel does (sc1 stores, vmcnt(0), ticket, sc1 loads).
// Built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "dlp_internal.h"

namespace dlp {
namespace {

#include "dlp_device.h"

constexpr int kFoldTile = 64;            // rows per workgroup = lanes; columns per staged tile
constexpr int kFoldStride = kFoldTile + 1;   // padded LDS row stride (doubles): lane r reads
                                             // r * 65 + k, a different bank pair per lane
constexpr int kDualThreads = 256;
constexpr int kDualColVec = 2;
constexpr int kDualColTile = kDualThreads * kDualColVec;

// acc = acc + (t * b): two roundings, never contracted (whatever -ffp-contract says)
__device__ __forceinline__ double fold_step(double acc, double t, double b) {
#pragma clang fp contract(off)
    const double prod = t * b;
    return acc + prod;
}

// One wave per workgroup owns 64 stored rows (the objective row included).  The 64 x 64 tile of
// the slack block is loaded as 64 coalesced 512-B row segments (lane = column) into registers
// while the previous tile, staged in LDS, is folded (lane = row, columns ascending); b_l is
// wave-uniform.  Rows past the objective row and columns past slack m-1 are clamped to a valid
// address and never folded / stored.
__global__ __launch_bounds__(kFoldTile) void rhs_rebuild_kernel(
    double* __restrict__ T, int64_t ld, int64_t rows, int64_t n, int64_t N,
    const double* __restrict__ b, DevState* st, int pricing) {
    __shared__ double tile[kFoldTile * kFoldStride];
    const int lane = threadIdx.x;
    const int64_t m = N - n;
    const int64_t r0 = (int64_t)blockIdx.x * kFoldTile;
    const int64_t ntile = (m + kFoldTile - 1) / kFoldTile;
    double acc = 0.0;
    double cur[kFoldTile];
    auto load_tile = [&](int64_t t) {
        int64_t l = t * kFoldTile + lane;
        l = l < m ? l : m - 1;
        // (a pointer walked down the rows, stopping at the objective row: one running uniform
        // offset instead of 64 hoisted ones)
        const double* src = T + r0 * ld + n + l;
#pragma unroll
        for (int rr = 0; rr < kFoldTile; ++rr) {
            cur[rr] = *src;
            src += (r0 + rr < rows) ? ld : 0;
        }
    };
    if (ntile > 0) load_tile(0);
    for (int64_t t = 0; t < ntile; ++t) {
#pragma unroll
        for (int rr = 0; rr < kFoldTile; ++rr) tile[rr * kFoldStride + lane] = cur[rr];
        __syncthreads();
        // the next tile's loads are in flight during the fold (the last iteration requests its own
        // tile again: no branch between the loads and the fold)
        load_tile(t + 1 < ntile ? t + 1 : t);
        const int64_t l0 = t * kFoldTile;
        const int kmax = (int)(m - l0 < kFoldTile ? m - l0 : kFoldTile);
        const double* mine = tile + lane * kFoldStride;
        if (kmax == kFoldTile) {
#pragma unroll 16
            for (int k = 0; k < kFoldTile; ++k) acc = fold_step(acc, mine[k], b[l0 + k]);
        } else {
            for (int k = 0; k < kmax; ++k) acc = fold_step(acc, mine[k], b[l0 + k]);
        }
        __syncthreads();
    }
    const int64_t r = r0 + lane;
    if (r <= rows) T[r * ld + N] = acc;
    if (blockIdx.x == gridDim.x - 1 && lane == kFoldTile - 1) {
        // a dual phase starts: running, Bland state of the options, no entering column yet
        st->status = DLP_RUNNING;
        st->q = -1;
        st->bland = pricing == DLP_PRICING_BLAND ? 1 : 0;
    }
}

// The last workgroup to arrive reduces the per-workgroup partials (ratio_kernel's hand-off: sc1
// stores drained by vmcnt(0) before the ticket add, sc1 loads after it).  Returns the winner in
// lane 0 of the last workgroup (*last = 1 there), the ticket re-armed.
__device__ inline Cand last_block_reduce(Cand c, Cand* partials, DevState* st, Cand* lds_c, int* s_last) {
    typedef unsigned int u4v __attribute__((ext_vector_type(4)));
    constexpr int kAuxSc1 = 16;
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)partials, (short)0, (int)(gridDim.x * sizeof(Cand)), 0x00020000);
    if (threadIdx.x == 0) {
        const u4v* cv = (const u4v*)&c;
        __builtin_amdgcn_raw_buffer_store_b128(cv[0], prs, (int)(blockIdx.x * sizeof(Cand)), 0, kAuxSc1);
        __builtin_amdgcn_raw_buffer_store_b128(cv[1], prs, (int)(blockIdx.x * sizeof(Cand)) + 16, 0,
                                               kAuxSc1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned prev =
            __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_last = (prev == gridDim.x - 1);
    }
    __syncthreads();
    if (!*s_last) return cand_empty();
    Cand best = cand_empty();
    for (int k = threadIdx.x; k < (int)gridDim.x; k += blockDim.x) {
        Cand o;
        u4v* ov = (u4v*)&o;
        ov[0] = __builtin_amdgcn_raw_buffer_load_b128(prs, (int)(k * sizeof(Cand)), 0, kAuxSc1);
        ov[1] = __builtin_amdgcn_raw_buffer_load_b128(prs, (int)(k * sizeof(Cand)) + 16, 0, kAuxSc1);
        if (cand_better(o, best)) best = o;
    }
    best = block_cand(best, lds_c);
    if (threadIdx.x == 0) st->ticket = 0;
    return best;
}

// Leaving row.  One lane per constraint row; the candidate's "ratio" is the RHS entry (+0.0 for
// every eligible row in Bland mode, so that the order falls through to basis[i] alone), its
// index basis[i].  The winner's row goes to st->p / p_local / leaving for dual_col_kernel.
__global__ __launch_bounds__(kDualThreads) void dual_row_kernel(
    const double* __restrict__ T, int64_t ld, int64_t rows, int64_t ncols,
    const int32_t* __restrict__ basis, DevState* st, Cand* partials, double tol_feas) {
    __shared__ Cand lds_c[4];
    __shared__ int s_last;
    if (st->status != DLP_RUNNING) return;
    const int bland = st->bland;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    Cand c = cand_empty();
    if (i < rows) {
        const double rhs = T[i * ld + ncols];
        if (rhs < -tol_feas) {
            c.ratio = bland ? 0.0 : rhs;
            c.row = (int32_t)i;
            c.basis_var = basis[i];
            c.valid = 1;
            c.pivot = rhs;
        }
    }
    c = block_cand(c, lds_c);
    const Cand best = last_block_reduce(c, partials, st, lds_c, &s_last);
    if (!s_last || threadIdx.x != 0) return;
    if (!best.valid) {   // primal and dual feasible
        st->q = -1;
        st->status = DLP_OK;
        return;
    }
    st->p = best.row;
    st->p_local = best.row;
    st->leaving = best.basis_var;
}

// Entering column.  Row p and the objective row are contiguous: 2 columns per lane, 512 per
// workgroup.  Candidate: ratio r_j, index j (ties to the smallest j), pivot T[p][j].
__global__ __launch_bounds__(kDualThreads) void dual_col_kernel(
    const double* __restrict__ T, int64_t ld, int64_t rows, int64_t ncols, int32_t* basis,
    DevState* st, Cand* partials, double tol_piv, int pricing, dlp_pivot* log, int64_t log_cap) {
    __shared__ Cand lds_c[4];
    __shared__ int s_last;
    if (st->status != DLP_RUNNING) return;
    const int32_t p = st->p_local;
    const double* __restrict__ prow = T + (int64_t)p * ld;
    const double* __restrict__ zrow = T + rows * ld;
    const int64_t j0 = (int64_t)blockIdx.x * kDualColTile + threadIdx.x * kDualColVec;
    Cand c = cand_empty();
    if (j0 < ncols) {   // ld is even and j0 is: the pair is inside the row
        const d2 a2 = *(const d2*)(prow + j0);
        const d2 z2 = *(const d2*)(zrow + j0);
        const double a[2] = {a2.x, a2.y}, z[2] = {z2.x, z2.y};
#pragma unroll
        for (int v = 0; v < kDualColVec; ++v) {
            if (j0 + v < ncols && a[v] < -tol_piv) {
                const double zc = z[v] > 0.0 ? z[v] : 0.0;
                const double r = zc / (-a[v]);
                if (!c.valid || r < c.ratio) {   // ascending j: a tie keeps the smaller j
                    c.ratio = r;
                    c.basis_var = (int32_t)(j0 + v);
                    c.row = (int32_t)(j0 + v);
                    c.valid = 1;
                    c.pivot = a[v];
                }
            }
        }
    }
    c = block_cand(c, lds_c);
    const Cand best = last_block_reduce(c, partials, st, lds_c, &s_last);
    if (!s_last || threadIdx.x != 0) return;
    if (!best.valid) {   // row p cannot be repaired: the new b is infeasible
        st->q = -1;
        st->status = DLP_INFEASIBLE;
        return;
    }
    // the selection in the primal's terms: row p, its basic variable leaving, ratio r_q, pivot a
    Cand sel;
    sel.ratio = best.ratio;
    sel.basis_var = st->leaving;
    sel.row = p;
    sel.valid = 1;
    sel.pad0 = 0;
    sel.pivot = best.pivot;
    do_select(st, sel, best.row, basis, 0, rows, pricing, log, log_cap);
}

}  // namespace

// (at least one workgroup: the last one decides, also on an LP without rows or columns)
int dual_col_blocks(const Geometry& g) {
    const int64_t nb = (g.ncols + kDualColTile - 1) / kDualColTile;
    return (int)(nb > 0 ? nb : 1);
}
int dual_row_blocks(const Geometry& g) {
    const int64_t nb = (g.rows + kDualThreads - 1) / kDualThreads;
    return (int)(nb > 0 ? nb : 1);
}

hipError_t launch_rhs_rebuild(const Geometry& g, int64_t n, const double* b, DevState* st, int pricing,
                              hipStream_t s) {
    const int64_t blocks = (g.rows + 1 + kFoldTile - 1) / kFoldTile;
    rhs_rebuild_kernel<<<(unsigned)blocks, kFoldTile, 0, s>>>(g.T, g.ld, g.rows, n, g.ncols, b, st, pricing);
    return hipGetLastError();
}

hipError_t launch_dual_row(const Geometry& g, const int32_t* basis, DevState* st, Cand* partials,
                           double tol_feas, hipStream_t s) {
    dual_row_kernel<<<dual_row_blocks(g), kDualThreads, 0, s>>>(g.T, g.ld, g.rows, g.ncols, basis, st, partials,
                                                               tol_feas);
    return hipGetLastError();
}

hipError_t launch_dual_col(const Geometry& g, int32_t* basis, DevState* st, Cand* partials, double tol_piv,
                           int pricing, dlp_pivot* log, int64_t log_cap, hipStream_t s) {
    dual_col_kernel<<<dual_col_blocks(g), kDualThreads, 0, s>>>(g.T, g.ld, g.rows, g.ncols, basis, st, partials,
                                                               tol_piv, pricing, log, log_cap);
    return hipGetLastError();
}

}  // namespace dlp
