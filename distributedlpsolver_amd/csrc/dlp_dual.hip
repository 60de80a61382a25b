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
// A deferred session (dlp_session_set_rhs_in_place) runs the same rule in blocks
// of K on replayed views: rhs_rebuild_cond_kernel (the fold on the condensed layout) and the four
// dual_*_defer kernels in the second half of this file.
// Built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "dlp_internal.h"

namespace dlp {
namespace {

#include "dlp_device.h"
#include "dlp_defer_device.h"

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

// ---- the dual phase on the deferred rank-K path (dlp_session_set_rhs_in_place) ----
// A dual pivot needs the same three slices of the current tableau as a deferred primal one (the RHS
// column, row p, column q), each re-derived from the stale tableau T0 by replaying the block's
// earlier steps with the per-element operations of dlp_chain.hip; only the order of the decisions
// differs: p first, then q from row p and the objective row.  Step j of a block is four launches,
// each a no-op once the status is not running, none waiting on another workgroup:
//   dual_row_defer_kernel     the RHS cache advanced by step j-1, the leaving row on it
//   dual_rowp_defer_kernel    row p replayed (raw, into `raw`), the entering slot, the selection
//   dual_colq_defer_kernel    column q replayed into C / Cc / nzc (before the commit, which
//                             overwrites rst[sq] and P[l < j][sq] and reads z_q from C[rows][j])
//   dual_commit_defer_kernel  raw / pivot, then commit_row (P[j], rst, objective row, pricing, log)
// The block is applied by the primal's pass (launch_flush_defer), unchanged.
constexpr int kDualChunk = 8;   // replay loads issued per round trip

// The RHS rebuild on the condensed layout (§20's fold on stored slots), one lane per stored row,
// l ascending, product rounded, then the sum; no atomics, no tree over l.  Row r's coefficient of slack
// n + l is its slot's entry when the slack is nonbasic, 1.0 in the row where it is basic, else +0
// (a +-0 coefficient adds +-0 to a sum that started from +0.0: no bit changes, the term is skipped).
__global__ __launch_bounds__(kDualThreads) void rhs_rebuild_cond_kernel(
    double* __restrict__ T, int64_t ld, int64_t rows, int64_t n, int64_t m,
    const int32_t* __restrict__ slot_of, const int32_t* __restrict__ basis, const double* __restrict__ b,
    DevState* st, int pricing) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= rows) {
        const double* __restrict__ row = T + r * ld;
        const int64_t bv = r < rows ? (int64_t)basis[r] : -1;
        double acc = 0.0;
        for (int64_t l = 0; l < m; ++l) {
            const int32_t sl = slot_of[n + l];   // (uniform)
            if (sl >= 0)
                acc = fold_step(acc, row[sl], b[l]);
            else if (bv == n + l)
                acc = fold_step(acc, 1.0, b[l]);
        }
        T[r * ld + n] = acc;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == blockDim.x - 1) {
        st->status = DLP_RUNNING;
        st->q = -1;
        st->bland = pricing == DLP_PRICING_BLAND ? 1 : 0;
    }
}

__global__ __launch_bounds__(kDualThreads) void dual_row_defer_kernel(
    const double* __restrict__ T, int64_t ld, int64_t rows, int64_t ncols,
    const int32_t* __restrict__ basis, DevState* st, const double* __restrict__ Cc, int64_t ldcc,
    const double* __restrict__ P, double* __restrict__ rhs, int K, Cand* partials, double tol_feas) {
    __shared__ Cand lds_c[4];
    __shared__ int s_last;
    if (st->status != DLP_RUNNING) return;
    const int bland = st->bland;
    const int j = st->blk;
    if (j < 0 || j >= K) {   // (an invariant: the host applies a block of K steps) — never index past C
        if (blockIdx.x == 0 && threadIdx.x == 0) st->status = DLP_ERR_STATE;
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    Cand c = cand_empty();
    if (i < rows) {
        // the RHS cache, as ratio_defer_body advances it: from T0 on an empty block, else by step j-1
        double r = j == 0 ? T[i * ld + ncols] : rhs[i];
        if (j > 0) {
            const int l = j - 1;
            const double pn = P[(int64_t)l * ld + ncols];
            const double f = Cc[(int64_t)l * ldcc + i];
            if ((int32_t)i == st->pl[l])
                r = pn;
            else if (f != 0.0)
                r = __builtin_fma(-f, pn, r);
        }
        rhs[i] = r;
        if (r < -tol_feas) {
            c.ratio = bland ? 0.0 : r;
            c.row = (int32_t)i;
            c.basis_var = basis[i];
            c.valid = 1;
            c.pivot = r;
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

// Row p of the current tableau: prow_defer_body's replay of T0[p] through steps 0..S-1 (the
// condensed restarts Rx / Ry included), without its division.  The candidate of a stored column is
// dual_col_kernel's; on a condensed tableau its index is the slot's variable (ties to the smaller
// variable), the RHS slot and the padding hold none.  Cand::row carries the slot.
__global__ __launch_bounds__(kDualThreads) void dual_rowp_defer_kernel(
    const double* __restrict__ T, int64_t ld, int64_t rows, int64_t ncols, int32_t* basis, DevState* st,
    const double* __restrict__ C, int64_t ldc, const double* __restrict__ P, double* __restrict__ raw,
    Cand* partials, double tol_piv, int pricing, dlp_pivot* log, int64_t log_cap, Cond cd) {
    __shared__ Cand lds_c[4];
    __shared__ int s_last;
    __shared__ double s_cp[kMaxDefer];
    __shared__ int32_t s_pl[kMaxDefer];
    if (st->status != DLP_RUNNING) return;
    const int32_t p = st->p_local;
    const int S = st->blk;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    const bool in = j < ld && p >= 0 && p < rows;   // (ld is even: the pair is inside the row)
    d2 t = d2{0.0, 0.0}, z = d2{0.0, 0.0};
    int32_t Rx = -1, Ry = -1, vx = -1, vy = -1;
    if (in) {
        t = *(const d2*)(T + (int64_t)p * ld + j);
        z = *(const d2*)(T + rows * ld + j);   // the objective row is current in place
        if (cd.on) {
            const int bs = st->bser;
            auto rof = [&](int32_t rv) -> int32_t { return rv >= 0 && (rv >> 7) == bs ? (rv & 127) : -1; };
            Rx = rof(cd.rst[j]);
            Ry = rof(cd.rst[j + 1]);
            vx = j < ncols ? cd.var_of[j] : -1;
            vy = j + 1 < ncols ? cd.var_of[j + 1] : -1;
        } else {
            vx = j < ncols ? (int32_t)j : -1;
            vy = j + 1 < ncols ? (int32_t)(j + 1) : -1;
        }
    }
    if (p >= 0 && p < rows)
        for (int l = threadIdx.x; l < S; l += blockDim.x) {
            s_cp[l] = C[(int64_t)p * ldc + l];
            s_pl[l] = st->pl[l];
        }
    __syncthreads();
    if (in) {
        for (int l0 = 0; l0 < S; l0 += kDualChunk) {
            d2 pv[kDualChunk];
#pragma unroll
            for (int u = 0; u < kDualChunk; ++u) {
                const int l = min(l0 + u, S - 1);
                pv[u] = *(const d2*)(P + (int64_t)l * ld + j);
            }
#pragma unroll
            for (int u = 0; u < kDualChunk; ++u) {
                const int l = l0 + u;
                if (l < S) {
                    if (l == Rx) t.x = 0.0;
                    if (l == Ry) t.y = 0.0;
                    if (p == s_pl[l]) {
                        t = pv[u];
                    } else if (s_cp[l] != 0.0) {
                        t.x = __builtin_fma(-s_cp[l], pv[u].x, t.x);
                        t.y = __builtin_fma(-s_cp[l], pv[u].y, t.y);
                    }
                }
            }
        }
        *(d2*)(raw + j) = t;
    }
    Cand c = cand_empty();
    auto take = [&](double a, double zz, int32_t v, int64_t slot) {
        if (v >= 0 && a < -tol_piv) {
            const double zc = zz > 0.0 ? zz : 0.0;
            const double r = zc / (-a);
            if (!c.valid || r < c.ratio || (r == c.ratio && v < c.basis_var)) {
                c.ratio = r;
                c.basis_var = v;
                c.row = (int32_t)slot;
                c.valid = 1;
                c.pivot = a;
            }
        }
    };
    take(t.x, z.x, vx, j);
    take(t.y, z.y, vy, j + 1);
    c = block_cand(c, lds_c);
    const Cand best = last_block_reduce(c, partials, st, lds_c, &s_last);
    if (!s_last || threadIdx.x != 0) return;
    if (!best.valid) {   // row p cannot be repaired: the new b is infeasible (the block keeps its S steps)
        st->q = -1;
        st->status = DLP_INFEASIBLE;
        return;
    }
    Cand sel;
    sel.ratio = best.ratio;
    sel.basis_var = st->leaving;
    sel.row = p;
    sel.valid = 1;
    sel.pad0 = 0;
    sel.pivot = best.pivot;
    st->sq = best.row;
    do_select(st, sel, best.basis_var, basis, 0, rows, pricing, log, log_cap, true, true, cd);
}

// Column q of the current tableau: ratio_defer_body's replay of slot sq through steps 0..j-1 (restart
// R), one lane per row; the objective row's lane takes z_q, current in place.  Writes step j's
// coefficients (C, its column-major copy Cc, the row classes nzc) and, at a block's first step, the
// zeroed tail of C the pass relies on.
__global__ __launch_bounds__(kDualThreads) void dual_colq_defer_kernel(
    const double* __restrict__ T, int64_t ld, int64_t rows, const DevState* st, double* __restrict__ C,
    int64_t ldc, double* __restrict__ Cc, int64_t ldcc, const double* __restrict__ P,
    int32_t* __restrict__ nzc, Cond cd) {
    __shared__ double s_pq[kMaxDefer];
    __shared__ int32_t s_pl[kMaxDefer];
    if (st->status != DLP_RUNNING) return;
    const int j = st->blk - 1;   // the step just selected
    if (j < 0 || j >= ldc) return;
    const int32_t sq = cd.on ? st->sq : st->q;
    int R = -1;
    if (cd.on) {
        const int32_t rv = cd.rst[sq];
        if (rv >= 0 && (rv >> 7) == st->bser) R = rv & 127;
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double a = i <= rows ? T[i * ld + sq] : 0.0;
    const int32_t nz_in = (i < rows && j > 0) ? nzc[i] : 0;
    for (int l = threadIdx.x; l < j; l += blockDim.x) {
        s_pq[l] = P[(int64_t)l * ld + sq];
        s_pl[l] = st->pl[l];
    }
    __syncthreads();
    if (i > rows) return;
    if (i < rows) {
        for (int l0 = 0; l0 < j; l0 += kDualChunk) {
            double f[kDualChunk];
#pragma unroll
            for (int u = 0; u < kDualChunk; ++u) f[u] = Cc[(int64_t)min(l0 + u, j - 1) * ldcc + i];
#pragma unroll
            for (int u = 0; u < kDualChunk; ++u) {
                const int l = l0 + u;
                if (l < j) {
                    if (l == R) a = 0.0;
                    if ((int32_t)i == s_pl[l])
                        a = s_pq[l];
                    else if (f[u] != 0.0)
                        a = __builtin_fma(-f[u], s_pq[l], a);
                }
            }
        }
    }
    C[i * ldc + j] = a;
    if (j == 0)
        for (int64_t l = 1; l < ldc; ++l) C[i * ldc + l] = 0.0;
    Cc[(int64_t)j * ldcc + i] = a;
    if (i < rows) nzc[i] = nz_in + (a != 0.0 ? 1 : 0);
}

// The commit: the raw row p over the pivot (IEEE division; on a condensed tableau the entering
// slot holds the leaving variable's unit 1 first, prow_defer_body's cond_fix), then commit_row.
__global__ __launch_bounds__(kDualThreads) void dual_commit_defer_kernel(
    double* __restrict__ T, int64_t ld, int64_t rows, int64_t ncols, int64_t nprice, const DevState* st,
    const double* __restrict__ C, int64_t ldc, double* __restrict__ P, const double* __restrict__ raw,
    PricePart* pp, double tol_dj, dlp_pivot* log, int64_t log_cap, Cond cd) {
    __shared__ PricePart lds_pp[4];
    if (st->status != DLP_RUNNING) return;
    const int s = st->blk - 1;
    if (s < 0 || s >= ldc) return;
    const int32_t sq = cd.on ? st->sq : -1;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    d2 pr = d2{0.0, 0.0};
    if (j < ld) {
        d2 t = *(const d2*)(raw + j);
        if (cd.on) {
            if (j == sq) t.x = 1.0;
            if (j + 1 == sq) t.y = 1.0;
        }
        const double piv = st->piv;
        pr.x = t.x / piv;
        pr.y = t.y / piv;
    }
    commit_row(T, ld, rows, ncols, nprice, st->npivots - 1, C, ldc, P, s, j, pr, pp, (int)blockIdx.x, tol_dj, log,
               log_cap, lds_pp, d2{0.0, 0.0}, 0.0, cd, sq, cd.on ? st->bser : 0);
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

// ---- the deferred dual chain's launchers
int dual_defer_parts(const Geometry& g) {
    const int64_t nr = (g.rows + 1 + kDualThreads - 1) / kDualThreads;
    const int64_t nc = (g.ld + kDualColTile - 1) / kDualColTile;
    return (int)(nr > nc ? nr : nc);
}

hipError_t launch_rhs_rebuild_cond(const Geometry& g, int64_t n, int64_t m, const int32_t* basis,
                                   const double* b, DevState* st, int pricing, hipStream_t s) {
    if (!g.cd.on || g.ncols != n) return hipErrorInvalidValue;
    const int64_t blocks = (g.rows + 1 + kDualThreads - 1) / kDualThreads;
    rhs_rebuild_cond_kernel<<<(unsigned)blocks, kDualThreads, 0, s>>>(g.T, g.ld, g.rows, n, m, g.cd.slot_of, basis,
                                                                     b, st, pricing);
    return hipGetLastError();
}

hipError_t launch_dual_row_defer(const Geometry& g, const Defer& d, const int32_t* basis, DevState* st,
                                 Cand* partials, double tol_feas, hipStream_t s) {
    if (d.K < 2 || d.K > kMaxDefer) return hipErrorInvalidValue;
    dual_row_defer_kernel<<<dual_row_blocks(g), kDualThreads, 0, s>>>(g.T, g.ld, g.rows, g.ncols, basis, st, d.Cc,
                                                                     d.ldcc, d.P, d.rhs, d.K, partials, tol_feas);
    return hipGetLastError();
}

hipError_t launch_dual_rowp_defer(const Geometry& g, const Defer& d, int32_t* basis, DevState* st, double* raw,
                                  Cand* partials, double tol_piv, int pricing, dlp_pivot* log, int64_t log_cap,
                                  hipStream_t s) {
    const int blocks = (int)((g.ld + kDualColTile - 1) / kDualColTile);
    dual_rowp_defer_kernel<<<blocks, kDualThreads, 0, s>>>(g.T, g.ld, g.rows, g.ncols, basis, st, d.C, d.ldc, d.P,
                                                          raw, partials, tol_piv, pricing, log, log_cap, g.cd);
    return hipGetLastError();
}

hipError_t launch_dual_colq_defer(const Geometry& g, const Defer& d, const DevState* st, hipStream_t s) {
    const int blocks = (int)((g.rows + 1 + kDualThreads - 1) / kDualThreads);
    dual_colq_defer_kernel<<<blocks, kDualThreads, 0, s>>>(g.T, g.ld, g.rows, st, d.C, d.ldc, d.Cc, d.ldcc, d.P,
                                                          d.nzc, g.cd);
    return hipGetLastError();
}

hipError_t launch_dual_commit_defer(const Geometry& g, const Defer& d, const DevState* st, const double* raw,
                                    PricePart* pp, double tol_dj, dlp_pivot* log, int64_t log_cap, hipStream_t s) {
    const int blocks = (int)((g.ld + kDualColTile - 1) / kDualColTile);
    dual_commit_defer_kernel<<<blocks, kDualThreads, 0, s>>>(g.T, g.ld, g.rows, g.ncols, g.nprice, st, d.C, d.ldc,
                                                            d.P, raw, pp, tol_dj, log, log_cap, g.cd);
    return hipGetLastError();
}

}  // namespace dlp
