// dlp_pass.hip — the tableau pass of the deferred rank-k pivot (the selection chain that
// chooses a block's pivots is dlp_chain.hip): forms 0-23, the block bookkeeping kernels (reset,
// restarted columns, failed step, seal) and their launchers.
//
// Deferred rank-k form of the pivot,
// gfx950.  Up to K pivots are chosen against the stale HBM tableau T0, then
// one pass applies them all: the tableau is streamed once per K pivots instead
// of once per pivot, and every value stays bit-identical to K eager rank-1
// updates (dlp_kernels.hip), because each element sees the same operations in
// the same order:
//   step l on row i:  i == p_l       -> T[i][c] := P[l][c]          (row p := prow)
//                     C[l][i] != 0   -> T[i][c] := fma(-C[l][i], P[l][c], T[i][c])
//                     C[l][i] == 0   -> untouched
// where C[l][i] = T_l[i][q_l] (row i's entry in the entering column just
// before step l) and P[l] = T_l[p_l] / T_l[p_l][q_l].  Per pivot only three
// things are needed from the current tableau, each re-derived by replaying
// the block's earlier steps on T0: column q (ratio_defer_kernel, one lane per
// row), the pivot row p (prow_defer_kernel) and the RHS column (kept current
// in `rhs`, one step per pivot).  The objective row is kept current in place
// (updated by the pivot-row kernel, which also emits the next pricing
// partials), and the pass (pass_kernel) skips it.
//
// Nearest reference analogs as for the eager kernels: the tight-set test
// R/global_problem.cpp:372-380 (ratio), first-wins scans :335-361 (pricing),
// the 2x2 basis solve :393-405 (elimination).  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <type_traits>
#include <utility>

#include "dlp_host.h"
#include "dlp_internal.h"

namespace dlp {
namespace {

#include "dlp_device.h"
#include "dlp_defer_device.h"

// The tableau pass.  Workgroup (tile, band): 512 columns (2 doubles per lane,
// one 16-B access) of rb constraint rows.  Each lane holds P[0..kb)[its two
// columns] in registers for the whole band.  The band's coefficients C[i][l]
// (row-major, one contiguous rb*K block) are staged in LDS, negated, and one
// lane per row classifies its row once:
//   kUntouched  every C[i][l] == 0 and never a pivot row -> no load, no store
//   kDense      every step touches it                   -> branch-free fma chain
//   kSparse     some steps skip it                      -> fma + select per step
//   >= 0        last step at which it was the pivot row  -> start from P[that step]
// Per element the operations are exactly the eager sequence.
constexpr int kUntouched = -3, kDense = -2, kSparse = -1;

template <int K>
__device__ inline d2 chain_dense(d2 t, const d2* pr, const double* nf) {
#pragma unroll
    for (int l = 0; l < K; ++l) {
        t.x = __builtin_fma(nf[l], pr[l].x, t.x);
        t.y = __builtin_fma(nf[l], pr[l].y, t.y);
    }
    return t;
}

template <bool NT, int K>
__global__ __launch_bounds__(256) void pass_kernel(double* __restrict__ T, int64_t ld, int64_t rows,
                                                   int64_t width, const DevState* st,
                                                   const double* __restrict__ C, int64_t ldc,
                                                   const double* __restrict__ P, int rb) {
    extern __shared__ double lds[];   // nf[rb][K] (negated C), then int32 cls[rb]
    __shared__ int32_t s_pl[K];
    const int kb = st->blk;
    if (kb == 0) return;
    const int64_t j = (int64_t)blockIdx.x * kDeferTile + threadIdx.x * 2;
    const bool colok = j < width;
    const int64_t jc = colok ? j : width - 2;
    d2 pr[K];
#pragma unroll
    for (int l = 0; l < K; ++l) {
        pr[l].x = 0.0;
        pr[l].y = 0.0;
        if (l < kb) pr[l] = *(const d2*)(P + (int64_t)l * ld + jc);
    }
    const int64_t i0 = (int64_t)blockIdx.y * rb;
    const int64_t iend = (i0 + rb < rows) ? i0 + rb : rows;
    const int nr = (int)(iend - i0);
    double* nf = lds;
    int32_t* cls = (int32_t*)(lds + (size_t)rb * K);
    const double* Cb = C + i0 * ldc;   // the band's rows: one contiguous block when ldc == K
    for (int idx = threadIdx.x; idx < nr * K; idx += blockDim.x) {
        const int r = idx / K, l = idx - r * K;
        nf[idx] = l < kb ? -Cb[(int64_t)r * ldc + l] : 0.0;
    }
    if (threadIdx.x < K) s_pl[threadIdx.x] = threadIdx.x < kb ? st->pl[threadIdx.x] : -1;
    __syncthreads();
    for (int r = threadIdx.x; r < nr; r += blockDim.x) {
        int last = -1, nz = 0;
        for (int l = 0; l < kb; ++l) {
            if (s_pl[l] == (int32_t)(i0 + r)) last = l;
            nz += nf[r * K + l] != 0.0;
        }
        cls[r] = last >= 0 ? last : (nz == kb ? kDense : (nz == 0 ? kUntouched : kSparse));
    }
    __syncthreads();
    const bool full = kb == K;
    for (int r = 0; r < nr; ++r) {
        const int c = cls[r];   // wave-uniform
        if (c == kUntouched) continue;
        double* row = T + (i0 + r) * ld;
        const double* f = nf + r * K;
        d2 t;
        if (c == kDense && full) {
            t = chain_dense<K>(ldv<NT>(row + jc), pr, f);
        } else {
            if (c >= 0) {
                t.x = 0.0;
                t.y = 0.0;
            } else {
                t = ldv<NT>(row + jc);
            }
#pragma unroll
            for (int l = 0; l < K; ++l) {
                if (l < kb && l >= c) {   // c < 0: every step; c >= 0: from the last pivot step on
                    if (l == c) {
                        t = pr[l];
                    } else {
                        d2 u;
                        u.x = __builtin_fma(f[l], pr[l].x, t.x);
                        u.y = __builtin_fma(f[l], pr[l].y, t.y);
                        const bool skip = f[l] == 0.0;
                        t.x = skip ? t.x : u.x;
                        t.y = skip ? t.y : u.y;
                    }
                }
            }
        }
        if (colok) stv<NT>(row + j, t);
    }
}

// Narrow form of the pass: one double per lane (256 columns per workgroup),
// so P[0..K) needs half the registers, and U rows per iteration, so each lane
// runs U independent fma chains (the chain, not HBM, limits the wide form at
// large K).  Dense groups (all U rows touched by every step, full block) take
// the branch-free path; everything else goes row by row through the generic
// replay.  Same per-element operations as pass_kernel.
template <bool NT, int K, int U>
__global__ __launch_bounds__(256) void pass1_kernel(double* __restrict__ T, int64_t ld, int64_t rows,
                                                    int64_t width, const DevState* st,
                                                    const double* __restrict__ C, int64_t ldc,
                                                    const double* __restrict__ P, int rb) {
    extern __shared__ double lds[];   // nf[rb][K] (negated C), then int32 cls[rb]
    __shared__ int32_t s_pl[K];
    const int kb = st->blk;
    if (kb == 0) return;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool colok = j < width;
    const int64_t jc = colok ? j : width - 1;
    double pr[K];
#pragma unroll
    for (int l = 0; l < K; ++l) pr[l] = (l < kb) ? P[(int64_t)l * ld + jc] : 0.0;
    const int64_t i0 = (int64_t)blockIdx.y * rb;
    const int64_t iend = (i0 + rb < rows) ? i0 + rb : rows;
    const int nr = (int)(iend - i0);
    double* nf = lds;
    int32_t* cls = (int32_t*)(lds + (size_t)rb * K);
    const double* Cb = C + i0 * ldc;
    for (int idx = threadIdx.x; idx < nr * K; idx += blockDim.x) {
        const int r = idx / K, l = idx - r * K;
        nf[idx] = l < kb ? -Cb[(int64_t)r * ldc + l] : 0.0;
    }
    if (threadIdx.x < K) s_pl[threadIdx.x] = threadIdx.x < kb ? st->pl[threadIdx.x] : -1;
    __syncthreads();
    for (int r = threadIdx.x; r < nr; r += blockDim.x) {
        int last = -1, nz = 0;
        for (int l = 0; l < kb; ++l) {
            if (s_pl[l] == (int32_t)(i0 + r)) last = l;
            nz += nf[r * K + l] != 0.0;
        }
        cls[r] = last >= 0 ? last : (nz == kb ? kDense : (nz == 0 ? kUntouched : kSparse));
    }
    __syncthreads();
    const bool full = kb == K;
    int r = 0;
    if (full)
        for (; r + U <= nr; r += U) {
            bool dense = true;
#pragma unroll
            for (int u = 0; u < U; ++u) dense = dense && cls[r + u] == kDense;
            if (!dense) break;
            double t[U];
#pragma unroll
            for (int u = 0; u < U; ++u) t[u] = ldv1<NT>(T + (i0 + r + u) * ld + jc);
            const double* f = nf + r * K;
#pragma unroll
            for (int l = 0; l < K; l += 2) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const d2 c = *(const d2*)(f + u * K + l);   // one 16-B LDS broadcast
                    t[u] = __builtin_fma(c.x, pr[l], t[u]);
                    t[u] = __builtin_fma(c.y, pr[l + 1], t[u]);
                }
            }
            if (colok)
#pragma unroll
                for (int u = 0; u < U; ++u) stv1<NT>(T + (i0 + r + u) * ld + j, t[u]);
        }
    for (; r < nr; ++r) {   // generic replay, one row at a time
        const int c = cls[r];
        if (c == kUntouched) continue;
        double* row = T + (i0 + r) * ld;
        const double* f = nf + r * K;
        double t = c >= 0 ? 0.0 : ldv1<NT>(row + jc);
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (l < kb && l >= c) {
                if (l == c) {
                    t = pr[l];
                } else {
                    const double u = __builtin_fma(f[l], pr[l], t);
                    t = f[l] == 0.0 ? t : u;
                }
            }
        }
        if (colok) stv1<NT>(row + j, t);
    }
}

// Scalar-coefficient form of the pass (forms 3-5).  The coefficients C[i][l]
// of a row are the same for every lane, so they are read with scalar loads
// straight from the C block (uniform address, read-only in this kernel) and
// enter v_fma_f64 as an SGPR operand with the negate modifier: no LDS traffic
// per fma, which bounds the LDS-staged forms at large K (one LDS broadcast
// per one or two fmas).  V doubles per lane (256 V columns per workgroup), U
// rows per group, P[0..K) in VGPRs.  Row class: nzc[i] = number of nonzero
// C[i][l] in the block (kept by ratio_defer_kernel), and the block's last
// pivot step on the row.  Same per-element operations as pass_kernel.
template <bool NT, int V>
__device__ inline void ldrow(double (&t)[V], const double* p) {
    if constexpr (V == 2) {
        const d2 v = ldv<NT>(p);
        t[0] = v.x;
        t[1] = v.y;
    } else {
        t[0] = ldv1<NT>(p);
    }
}
template <bool NT, int V>
__device__ inline void strow(double* p, const double (&t)[V]) {
    if constexpr (V == 2) {
        d2 v;
        v.x = t[0];
        v.y = t[1];
        stv<NT>(p, v);
    } else {
        stv1<NT>(p, t[0]);
    }
}

// The block's coefficients are read-only during the pass: through the constant
// address space, wave-uniform loads of them are always scalar loads.
typedef __attribute__((address_space(4))) const double* cdptr;

// T: the tableau read; Tout: where the rows go (== T in place; lookahead: the other
// buffer, so untouched rows are copied and an empty block copies everything); bd: the
// block (DevState::blk / pl, or a sealed copy).
template <bool NT, int K, int V, int U, bool PART, bool DEEP = false>
__device__ __forceinline__ void pass_s_body(const double* __restrict__ T, double* __restrict__ Tout,
                                            int64_t ld, int64_t rows, int64_t width,
                                            const BlockDesc* __restrict__ bd,
                                            const double* __restrict__ C, int64_t ldc,
                                            const double* __restrict__ P,
                                            const int32_t* __restrict__ nzc, int rb, int tails) {
    __shared__ int32_t cls[1024];
    const int kb = bd->blk;
    const bool outplace = Tout != T;
    // tails (the session's K is this instance's K): the block's unused steps were zeroed at
    // its start (C and P tails: ratio kernel, commit_row), so the full-block instance runs
    // partial blocks too, as one launch.  Otherwise two launches per pass: the full-block
    // instance (kb == K) and the partial one (0 < kb < K: a window's last block, or one cut
    // short by termination; kb == 0 out of place: a copy), so that neither carries the
    // other's register pressure; exactly one of them runs
    if ((kb == 0 && !outplace) || (PART ? kb == K : (kb != K && !tails))) return;
    const int64_t j = (int64_t)blockIdx.x * (256 * V) + threadIdx.x * V;
    const bool colok = j < width;
    const int64_t jc = colok ? j : width - V;
    double pr[K][V];
#pragma unroll
    for (int l = 0; l < K; ++l) {
        double v[V];
        // rows l >= kb are not used (and need not exist: P holds d.K <= K rows)
        ldrow<false, V>(v, P + (int64_t)(l < kb ? l : 0) * ld + jc);
#pragma unroll
        for (int e = 0; e < V; ++e) pr[l][e] = l < kb ? v[e] : 0.0;
    }
    const int64_t i0 = (int64_t)blockIdx.y * rb;
    const int64_t iend = (i0 + rb < rows) ? i0 + rb : rows;
    const int nr = (int)(iend - i0);
    for (int r = threadIdx.x; r < nr; r += blockDim.x) {
        const int nz = nzc[i0 + r];
        int last = -1;
        for (int l = 0; l < kb; ++l)
            if (bd->pl[l] == (int32_t)(i0 + r)) last = l;
        // (an empty block out of place is a copy: C and nzc are the previous block's, and
        // fma(-c, +0, t) would turn a t = -0 into +0 where c < 0 or c = -0)
        cls[r] = last >= 0 ? last : (kb == 0 || nz == 0 ? kUntouched : (nz == kb ? kDense : kSparse));
    }
    __syncthreads();
    // dense groups: U rows, every step of the block touches every row.  The next dense
    // group's rows are loaded before this group's fma chains, so every wave keeps two
    // groups of HBM loads in flight (vector loads retire in order: vmcnt covers them,
    // while the coefficients' scalar loads wait on lgkmcnt only).
    auto dense_at = [&](int r0) {
        if (r0 + U > nr) return false;
        bool d = true;
#pragma unroll
        for (int u = 0; u < U; ++u) d = d && cls[r0 + u] == kDense;
        return d;
    };
    const double* cbase = C + i0 * ldc;
    // one dense group: t = rows r0..r0+U-1 (already loaded), all K steps, store.
    // Coefficients in chunks of LC steps x U rows (16 doubles = 32 SGPRs), double
    // buffered: scalar loads return out of order, so a chunk is waited for (lgkmcnt(0))
    // BEFORE the next chunk's loads are issued, and those then land while the current
    // chunk's fmas run.  sched_barriers keep the compiler from re-merging the two.
    constexpr int LC = (16 / U) < K ? (16 / U) : K;
    auto fetch = [&](double (&f)[U][LC], cdptr cb, int l0) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int l = 0; l < LC; ++l) f[u][l] = cb[u * ldc + l0 + l];
    };
    auto chain = [&](double (&t)[U][V], const double (&f)[U][LC], int l0) {
#pragma unroll
        for (int l = 0; l < LC; ++l)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < V; ++e)
                    t[u][e] = __builtin_fma(-f[u][l], pr[l0 + l][e], t[u][e]);
    };
    // a partial block runs the full-block code: chunks past step kb-1 are skipped, and in
    // the chunk holding it the coefficients of steps >= kb are zeroed (scalar selects).
    // With P[l] = +0 for l >= kb (above) such a step is fma(-(+0), +0, t) = t + (-0) = t
    // for every t, so the result is exactly that of the kb real steps.
    auto mask = [&](double (&f)[U][LC], int l0) {
        if constexpr (PART) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int l = 0; l < LC; ++l) f[u][l] = (l0 + l < kb) ? f[u][l] : 0.0;
        }
    };
    auto group = [&](double (&t)[U][V], int r0) {
        const cdptr cb = (cdptr)(cbase + (int64_t)r0 * ldc);
        {
            double fa[U][LC], fb[U][LC];
            fetch(fa, cb, 0);
#pragma unroll
            for (int l0 = 0; l0 < K; l0 += 2 * LC) {
                if (PART && l0 >= kb) break;
                __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): chunk fa has landed
                const bool nb = l0 + LC < K && (!PART || l0 + LC < kb);
                if (nb) fetch(fb, cb, l0 + LC);
                mask(fa, l0);
                __builtin_amdgcn_sched_barrier(0);
                chain(t, fa, l0);
                __builtin_amdgcn_sched_barrier(0);
                if (nb) {
                    __builtin_amdgcn_s_waitcnt(0xC07F);   // chunk fb has landed
                    if (l0 + 2 * LC < K && (!PART || l0 + 2 * LC < kb)) fetch(fa, cb, l0 + 2 * LC);
                    mask(fb, l0 + LC);
                    __builtin_amdgcn_sched_barrier(0);
                    chain(t, fb, l0 + LC);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (colok)
#pragma unroll
            for (int u = 0; u < U; ++u) strow<NT, V>(Tout + (i0 + r0 + u) * ld + j, t[u]);
    };
    auto load = [&](double (&t)[U][V], int r0) {
#pragma unroll
        for (int u = 0; u < U; ++u) ldrow<NT, V>(t[u], T + (i0 + r0 + u) * ld + jc);
    };
    double ta[U][V], tb[U][V];
    int r = 0;
    while (r < nr) {
        if (DEEP && dense_at(r)) {
            // form 20: three register buffers, so the rows of the next TWO dense groups
            // are in flight while one group's chains run
            double tc[U][V];
            load(ta, r);
            bool nb = dense_at(r + U);
            load(tb, nb ? r + U : r);
            while (true) {
                const bool nc = nb && dense_at(r + 2 * U);
                load(tc, nc ? r + 2 * U : r);
                __builtin_amdgcn_sched_barrier(0);
                group(ta, r);
                r += U;
                if (!nb) break;
                const bool nd = nc && dense_at(r + 2 * U);
                load(ta, nd ? r + 2 * U : r);
                __builtin_amdgcn_sched_barrier(0);
                group(tb, r);
                r += U;
                if (!nc) break;
                const bool ne = nd && dense_at(r + 2 * U);
                load(tb, ne ? r + 2 * U : r);
                __builtin_amdgcn_sched_barrier(0);
                group(tc, r);
                r += U;
                if (!nd) break;
                nb = ne;
            }
            continue;
        }
        if (dense_at(r)) {
            // a run of dense groups, ping-ponging two register buffers
            load(ta, r);
            // The prefetch is unconditional (at the end of a run it re-reads the current
            // group's rows, an L2 hit), so the in-order vmcnt wait for the group being
            // computed is the same on every path and leaves the prefetch in flight.
            while (true) {
                const bool nb = dense_at(r + U);
                load(tb, nb ? r + U : r);
                __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ahead of the chains
                group(ta, r);
                r += U;
                if (!nb) break;
                const bool na = dense_at(r + U);
                load(ta, na ? r + U : r);
                __builtin_amdgcn_sched_barrier(0);
                group(tb, r);
                r += U;
                if (!na) break;
            }
            continue;
        }
        // generic replay, one row (sparse rows, the block's pivot rows, partial blocks): a
        // runtime loop over the steps with P[l] re-read from L2, so that the unrolled
        // register copy serves only the dense path
        const int c = cls[r];
        if (c == kUntouched && outplace) {
            double t[V];
            ldrow<NT, V>(t, T + (i0 + r) * ld + jc);
            if (colok) strow<NT, V>(Tout + (i0 + r) * ld + j, t);
        } else if (c != kUntouched) {
            const double* row = T + (i0 + r) * ld;
            const double* cr = C + (i0 + r) * ldc;
            double t[V];
            int l = 0;
            if (c >= 0) {
                ldrow<false, V>(t, P + (int64_t)c * ld + jc);
                l = c + 1;
            } else {
                ldrow<NT, V>(t, row + jc);
            }
            for (; l < kb; ++l) {
                const double f = cr[l];
                if (f != 0.0) {
                    double pv[V];
                    ldrow<false, V>(pv, P + (int64_t)l * ld + jc);
#pragma unroll
                    for (int e = 0; e < V; ++e) t[e] = __builtin_fma(-f, pv[e], t[e]);
                }
            }
            if (colok) strow<NT, V>(Tout + (i0 + r) * ld + j, t);
        }
        r += 1;
    }
}

template <bool NT, int K, int V, int U, bool PART, bool DEEP = false>
__global__ __launch_bounds__(256) void pass_s_kernel(const double* __restrict__ T, double* __restrict__ Tout,
                                                     int64_t ld, int64_t rows, int64_t width,
                                                     const BlockDesc* __restrict__ bd,
                                                     const double* __restrict__ C, int64_t ldc,
                                                     const double* __restrict__ P,
                                                     const int32_t* __restrict__ nzc, int rb, int tails) {
    pass_s_body<NT, K, V, U, PART, DEEP>(T, Tout, ld, rows, width, bd, C, ldc, P, nzc, rb, tails);
}

// The same body held to 3 waves per SIMD (<= 168 VGPRs; form 4 alone takes 170, which
// allocates 176 and leaves 2 waves per SIMD).
template <bool NT, int K, int V, int U, bool PART>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void pass_s3_kernel(
    const double* __restrict__ T, double* __restrict__ Tout, int64_t ld, int64_t rows, int64_t width,
    const BlockDesc* __restrict__ bd, const double* __restrict__ C, int64_t ldc,
    const double* __restrict__ P, const int32_t* __restrict__ nzc, int rb, int tails) {
    pass_s_body<NT, K, V, U, PART>(T, Tout, ld, rows, width, bd, C, ldc, P, nzc, rb, tails);
}

// Streamed form of the pass (forms 6-9): pass_s_body's per-element operations,
// with three changes aimed at the HBM stream.
//  * Work order.  A 1-D grid; workgroup b works on position q of a list of
//    (tile, band) pairs ordered by groups of kPassBands bands, tile-major inside
//    a group, and the list is cut into 8 equal contiguous pieces, piece b % 8
//    going to the workgroups that share b's XCD (blocks are dealt round-robin
//    over the 8 XCDs: MI355X_MICROARCH.md, workgroup dispatch).  So the
//    workgroups resident on one XCD at a time share a few tiles' P slices and a
//    few bands' coefficients in that XCD's L2, instead of every workgroup
//    fetching both again from the Infinity Cache.  Placement only moves speed.
//  * Dense groups first.  The band's dense groups (U rows, every step of the
//    block touches every row) are compacted into a list in LDS and streamed
//    through a ring of D register buffers: the rows of D-1 groups are in flight
//    while one group's fma chains run.  Everything else (sparse rows, the
//    block's pivot rows, rows of partly dense groups) follows, row by row,
//    through the generic replay.  Rows are independent, so order is free.
//  * Coefficients.  Scalar loads in chunks of LC steps x U rows, double
//    buffered, and the next dense group's first chunk is fetched during the
//    current group's last chunk (full blocks: K / LC is even).
constexpr int kPassBands = 16;   // bands per group of the work order

// Buffer access to one band of the tableau: the descriptor is built once from
// wave-uniform values, every lane keeps ONE 32-bit column offset, and the row
// offset is a scalar (soffset).  aux 2 = nt.
template <bool NT, int V>
__device__ inline void bld(double (&t)[V], __amdgpu_buffer_rsrc_t rs, int voff, int soff) {
    if constexpr (V == 2) {
        const u4v x = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, NT ? 2 : 0);
        const d2 v = __builtin_bit_cast(d2, x);
        t[0] = v.x;
        t[1] = v.y;
    } else {
        const u2v x = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, NT ? 2 : 0);
        t[0] = __builtin_bit_cast(double, x);
    }
}
template <bool NT, int V>
__device__ inline void bst(const double (&t)[V], __amdgpu_buffer_rsrc_t rs, int voff, int soff) {
    if constexpr (V == 2) {
        d2 v;
        v.x = t[0];
        v.y = t[1];
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, v), rs, voff, soff, NT ? 2 : 0);
    } else {
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, t[0]), rs, voff, soff, NT ? 2 : 0);
    }
}

template <int K, int V, int U>
struct PassGeo {
    static constexpr int LC = (16 / U) < K ? (16 / U) : K;   // steps per coefficient chunk
    static constexpr int NCH = K / LC;                       // chunks per group
};

template <bool NT, int K, int V, int U, int D, bool PART>
__global__ __launch_bounds__(256) void pass_r_kernel(double* __restrict__ T, int64_t ld,
                                                     int64_t rows, int64_t width,
                                                     const DevState* __restrict__ st,
                                                     const double* __restrict__ C, int64_t ldc,
                                                     const double* __restrict__ P,
                                                     const int32_t* __restrict__ nzc, int rb,
                                                     int ntiles, int nbands, int order) {
    static_assert(PassGeo<K, V, U>::NCH % 2 == 0, "the cross-group prefetch needs an even chunk count");
    __shared__ int32_t cls[1024];
    __shared__ int16_t dgl[512];
    __shared__ int32_t s_wtot[4];
    const int kb = st->blk;
    if (kb == 0 || (PART ? kb == K : kb != K)) return;
    // (tile, band) of this workgroup: order 1 = the XCD work order above; order 0 =
    // tile-fastest over the whole grid (consecutive workgroups stream one row range)
    const int64_t total = (int64_t)ntiles * nbands;
    int tile, band;
    if (order) {
        const int64_t per = (total + 7) >> 3;
        const int64_t q = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
        if ((int64_t)(blockIdx.x >> 3) >= per || q >= total) return;
        const int bgrp = (int)(q / ((int64_t)kPassBands * ntiles));
        const int rr = (int)(q - (int64_t)bgrp * kPassBands * ntiles);
        const int nbg = min(kPassBands, nbands - bgrp * kPassBands);
        tile = rr / nbg;
        band = bgrp * kPassBands + rr % nbg;
    } else if (order == 2) {
        // XCD b % 8 owns a range of ceil(ntiles / 8) column tiles and walks it band by
        // band: its resident workgroups share those tiles' P slices in its L2, and the
        // 8 XCDs together sweep whole rows, as the eager update does
        const int t8 = (ntiles + 7) >> 3;
        const int x = blockIdx.x & 7, k = blockIdx.x >> 3;
        const int tx0 = x * t8, ntx = min(t8, ntiles - tx0);
        if (ntx <= 0 || k >= ntx * nbands) return;
        band = k / ntx;
        tile = tx0 + k % ntx;
    } else {
        if ((int64_t)blockIdx.x >= total) return;
        band = (int)(blockIdx.x / ntiles);
        tile = (int)(blockIdx.x - (int64_t)band * ntiles);
    }

    const int64_t j = (int64_t)tile * (256 * V) + threadIdx.x * V;
    const int64_t jc = j < width ? j : width - V;
    double pr[K][V];
#pragma unroll
    for (int l = 0; l < K; ++l) {
        double v[V];
        ldrow<false, V>(v, P + (int64_t)(l < kb ? l : 0) * ld + jc);
#pragma unroll
        for (int e = 0; e < V; ++e) pr[l][e] = l < kb ? v[e] : 0.0;
    }
    const int64_t i0 = (int64_t)band * rb;
    const int64_t iend = (i0 + rb < rows) ? i0 + rb : rows;
    const int nr = (int)(iend - i0);
    for (int r = threadIdx.x; r < nr; r += blockDim.x) {
        const int nz = nzc[i0 + r];
        int last = -1;
        for (int l = 0; l < kb; ++l)
            if (st->pl[l] == (int32_t)(i0 + r)) last = l;
        cls[r] = last >= 0 ? last : (nz == kb ? kDense : (nz == 0 ? kUntouched : kSparse));
    }
    __syncthreads();
    // compact the dense groups into dgl[0..ndg); their rows leave the generic loop
    const int ng = nr / U;
    int ndg = 0;
    for (int base = 0; base < ng; base += 256) {
        const int g = base + (int)threadIdx.x;
        bool d = g < ng;
        if (d)
#pragma unroll
            for (int u = 0; u < U; ++u) d = d && cls[g * U + u] == kDense;
        const uint64_t m = __ballot(d);
        const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
        const int pre = __popcll(m & ((1ull << ln) - 1ull));
        if (ln == 0) s_wtot[wv] = __popcll(m);
        __syncthreads();
        int off = ndg;
        for (int w = 0; w < wv; ++w) off += s_wtot[w];
        if (d) {
            dgl[off + pre] = (int16_t)g;
#pragma unroll
            for (int u = 0; u < U; ++u) cls[g * U + u] = kUntouched;
        }
        ndg += s_wtot[0] + s_wtot[1] + s_wtot[2] + s_wtot[3];
        __syncthreads();
    }

    constexpr int LC = PassGeo<K, V, U>::LC;
    constexpr int NCH = PassGeo<K, V, U>::NCH;
    const double* cbase = C + i0 * ldc;
    auto fetch = [&](double (&f)[U][LC], cdptr cb, int l0) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int l = 0; l < LC; ++l) f[u][l] = cb[u * ldc + l0 + l];
    };
    auto chain = [&](double (&t)[U][V], const double (&f)[U][LC], int l0) {
#pragma unroll
        for (int l = 0; l < LC; ++l)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < V; ++e)
                    t[u][e] = __builtin_fma(-f[u][l], pr[l0 + l][e], t[u][e]);
    };
    // the chunk holding step kb-1: a uniform branch per step (no per-element selects)
    auto chain_part = [&](double (&t)[U][V], const double (&f)[U][LC], int l0) {
#pragma unroll
        for (int l = 0; l < LC; ++l)
            if (l0 + l < kb)
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int e = 0; e < V; ++e)
                        t[u][e] = __builtin_fma(-f[u][l], pr[l0 + l][e], t[u][e]);
    };
    auto grow = [&](int g) { return (int)__builtin_amdgcn_readfirstlane(dgl[g]) * U; };
    // the band through one buffer descriptor (the launcher keeps rb * ld * 8 < 2^31).
    // Lanes past the last column work on (and store) the last column group: the
    // same operations on the same inputs give the same bits as its owner lane, so
    // every store is unconditional (no exec-masked stores for vmcnt to second-guess)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(T + i0 * ld), (short)0, (int)((int64_t)nr * ld * 8), 0x00020000);
    const int voff = (int)(jc * 8);
    const int ld8 = (int)(ld * 8);
    auto load = [&](double (&t)[U][V], int r0) {
#pragma unroll
        for (int u = 0; u < U; ++u) bld<NT, V>(t[u], rs, voff, (r0 + u) * ld8);
    };
    auto store = [&](const double (&t)[U][V], int r0) {
#pragma unroll
        for (int u = 0; u < U; ++u) bst<NT, V>(t[u], rs, voff, (r0 + u) * ld8);
    };
    double fa[U][LC], fb[U][LC];
    // full block: fa holds chunk 0 of this group on entry and chunk 0 of group rn on exit
    auto group_full = [&](double (&t)[U][V], int r0, int rn) {
        const cdptr cb = (cdptr)(cbase + (int64_t)r0 * ldc);
        const cdptr cn = (cdptr)(cbase + (int64_t)rn * ldc);
#pragma unroll
        for (int c = 0; c < NCH; c += 2) {
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): fa has landed
            fetch(fb, cb, (c + 1) * LC);
            __builtin_amdgcn_sched_barrier(0);
            chain(t, fa, c * LC);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);   // fb has landed
            if (c + 2 < NCH)
                fetch(fa, cb, (c + 2) * LC);
            else
                fetch(fa, cn, 0);
            __builtin_amdgcn_sched_barrier(0);
            chain(t, fb, (c + 1) * LC);
            __builtin_amdgcn_sched_barrier(0);
        }
        store(t, r0);
    };
    // partial block: chunks up to step kb-1, the last one masked
    auto group_part = [&](double (&t)[U][V], int r0) {
        const cdptr cb = (cdptr)(cbase + (int64_t)r0 * ldc);
        fetch(fa, cb, 0);
#pragma unroll
        for (int c = 0; c < NCH; c += 2) {
            if (c * LC < kb) {
                __builtin_amdgcn_s_waitcnt(0xC07F);
                if ((c + 1) * LC < kb) fetch(fb, cb, (c + 1) * LC);
                __builtin_amdgcn_sched_barrier(0);
                if ((c + 1) * LC <= kb)
                    chain(t, fa, c * LC);
                else
                    chain_part(t, fa, c * LC);
                __builtin_amdgcn_sched_barrier(0);
                if ((c + 1) * LC < kb) {
                    __builtin_amdgcn_s_waitcnt(0xC07F);
                    if ((c + 2) * LC < kb && c + 2 < NCH) fetch(fa, cb, (c + 2) * LC);
                    __builtin_amdgcn_sched_barrier(0);
                    if ((c + 2) * LC <= kb)
                        chain(t, fb, (c + 1) * LC);
                    else
                        chain_part(t, fb, (c + 1) * LC);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        store(t, r0);
    };

    if (ndg > 0) {
        double buf[D][U][V];
#pragma unroll
        for (int b = 0; b < D - 1; ++b) load(buf[b], grow(b < ndg ? b : ndg - 1));
        if constexpr (!PART) fetch(fa, (cdptr)(cbase + (int64_t)grow(0) * ldc), 0);
        for (int g0 = 0; g0 < ndg; g0 += D) {
#pragma unroll
            for (int b = 0; b < D; ++b) {
                const int gi = g0 + b;
                if (gi < ndg) {
                    // the ring's next group: rows D-1 groups ahead (clamped: an L2 hit)
                    const int ga = gi + D - 1 < ndg ? gi + D - 1 : ndg - 1;
                    load(buf[(b + D - 1) % D], grow(ga));
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (!PART)
                        group_full(buf[b], grow(gi), grow(gi + 1 < ndg ? gi + 1 : gi));
                    else
                        group_part(buf[b], grow(gi));
                }
            }
        }
    }
    // everything else, row by row (as pass_s_body's generic replay)
    for (int r = 0; r < nr; ++r) {
        const int c = cls[r];
        if (c == kUntouched) continue;
        const double* cr = C + (i0 + r) * ldc;
        double t[V];
        int l = 0;
        if (c >= 0) {
            ldrow<false, V>(t, P + (int64_t)c * ld + jc);
            l = c + 1;
        } else {
            bld<NT, V>(t, rs, voff, r * ld8);
        }
        for (; l < kb; ++l) {
            const double f = cr[l];
            if (f != 0.0) {
                double pv[V];
                ldrow<false, V>(pv, P + (int64_t)l * ld + jc);
#pragma unroll
                for (int e = 0; e < V; ++e) t[e] = __builtin_fma(-f, pv[e], t[e]);
            }
        }
        bst<NT, V>(t, rs, voff, r * ld8);
    }
}


// Row classes of a band (pass_s_body's rule) for the 64-step passes: every row from nzc,
// then each step's pivot row raised to the step index (LDS atomic max: the last step that
// pivoted on the row wins; steps >= 0 exceed every class code).  One load per thread
// instead of a scan of the step table per row.  The caller syncs.
// densepiv (form 23): a pivot row whose every coefficient is non-zero (nzc == kb, so every step
// after its pivot step touches it) gets class kDensePiv + step: its group may stay on the DPP
// chain (pass_q_kernel).  Only the step that won the row marks it, so the marks do not race.
constexpr int kDensePiv = 64;
__device__ inline void classify_band(int32_t* cls, const BlockDesc* __restrict__ bd,
                                     const int32_t* __restrict__ nzc, int64_t i0, int nr, int kb,
                                     bool densepiv = false) {
    for (int r = threadIdx.x; r < nr; r += blockDim.x) {
        const int nz = nzc[i0 + r];
        // (an empty block, out of place, is a copy: C and nzc are the previous block's)
        cls[r] = kb == 0 || nz == 0 ? kUntouched : (nz == kb ? kDense : kSparse);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < kb; l += blockDim.x) {
        const int64_t r = (int64_t)bd->pl[l] - i0;
        if (bd->pl[l] >= 0 && r >= 0 && r < nr) atomicMax(&cls[r], l);
    }
    if (!densepiv) return;
    __syncthreads();
    for (int l = threadIdx.x; l < kb; l += blockDim.x) {
        const int64_t r = (int64_t)bd->pl[l] - i0;
        if (bd->pl[l] >= 0 && r >= 0 && r < nr && cls[r] == l && nzc[i0 + r] == kb) cls[r] = kDensePiv + l;
    }
}

// Form 21: the pass at K = 64 with the coefficients broadcast by DPP.  At 64 steps per
// element the scalar coefficient path of forms 3-5 stalls: every chunk of 2 rows x 8
// steps is a scalar load that misses to L2 (~800 cycles under the stream) against ~128
// cycles of fmas, and a pass took 16 ms where the same chain with no coefficient loads
// takes 7.1 (tools/passlab.hip, profiles/r02j/).  Here the coefficients travel as
// ordinary vector loads, well ahead of use: lane n of each 16-lane row loads steps
// (2n, 2n+1) of a 32-step half of its row's coefficient row with one 16-B load, and
// v_fmac_f64_dpp ... row_newbcast:n reads lane n's value for the whole row, so the fma
// takes its coefficient straight from another lane's register (neg modifier: fma(-c, p, t),
// the eager operation).  1 double x 2 rows per lane, P[0..64) in 128 VGPRs, buffer
// accesses with one 32-bit column offset per lane: 166 VGPRs, 3 waves per SIMD.
// Coefficient registers are written only by loads (no VALU write within two
// instructions of a DPP read: tests/test_isa.py audits the built code object).  Partial
// blocks run the same code: their unused steps were zeroed at block start (C and P tails).
template <int N>
__device__ __forceinline__ void fmac_bc(double& t, double c, double p) {
    asm("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
        : "+v"(t)
        : "v"(c), "v"(p), "n"(N));
}
template <int N>
__device__ __forceinline__ double bc_mov(double v) {
    return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + N, 0xf, 0xf, false);
}
// step l of both rows: half h = l / 32, (even, odd) register e = l & 1, lane (l & 31) / 2
template <int L>
__device__ __forceinline__ void dpp_step(double (&t)[2], const double (&c)[2][2][2], const double (&pr)[64]) {
    constexpr int h = L / 32, e = L & 1, n = (L & 31) >> 1;
    fmac_bc<n>(t[0], c[0][h][e], pr[L]);
    fmac_bc<n>(t[1], c[1][h][e], pr[L]);
}
template <int L0, int... I>
__device__ __forceinline__ void dpp_half(double (&t)[2], const double (&c)[2][2][2], const double (&pr)[64],
                                         std::integer_sequence<int, I...>) {
    (dpp_step<L0 + I>(t, c, pr), ...);
}

// Generic replay of one row of class cl (a pivot row at step cl >= 0: start from P[cl]; a
// sparse row: skip the steps whose coefficient is 0) over the 64 steps, P[0..64) of the
// lane's column in registers (unrolled: no dynamic register index), the row's coefficients
// from f(l) (uniform).  The tails of a partial block have f == 0 and are skipped.
template <typename F>
__device__ __forceinline__ double replay_row(double t, int cl, const double (&pr)[64], F f) {
#pragma unroll
    for (int l = 0; l < 64; ++l) {
        const double c = f(l);
        if (l == cl)
            t = pr[l];
        else if (l > cl && c != 0.0)
            t = __builtin_fma(-c, pr[l], t);
    }
    return t;
}

// PUB (lookahead): the output rows are stored write-through (sc1) and every workgroup, once
// all its waves have drained their stores, adds 1 to its band's count, so the next block's
// selections can read a finished band from Tout instead of replaying this block on it
// (band_done; MI355X_MICROARCH.md, inter-workgroup visibility, first row of the sc1 table).
template <bool NT, bool PUB = false>
__global__ __launch_bounds__(256) void pass_d_kernel(const double* __restrict__ T, double* __restrict__ Tout,
                                                     int64_t ld, int64_t rows, int64_t width,
                                                     const BlockDesc* __restrict__ bd,
                                                     const double* __restrict__ C, int64_t ldc,
                                                     const double* __restrict__ P,
                                                     const int32_t* __restrict__ nzc, int rb,
                                                     uint32_t* bcnt = nullptr) {
    constexpr int K = 64, U = 2;
    constexpr int kSt = (NT ? 2 : 0) | (PUB ? kAuxSc1 : 0);   // store policy
    __shared__ int32_t cls[1024];
    const int kb = bd->blk;
    const bool outplace = Tout != T;
    if (kb == 0 && !outplace) return;   // full and partial blocks alike (zeroed tails)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool colok = j < width;
    const int jc = (int)(colok ? j : width - 1);
    double pr[K];   // all 64 rows: a partial block's P[l >= kb] is +0 (zeroed at block start)
#pragma unroll
    for (int l = 0; l < K; ++l) pr[l] = P[(int64_t)l * ld + jc];
    const int64_t i0 = (int64_t)blockIdx.y * rb;
    const int64_t iend = (i0 + rb < rows) ? i0 + rb : rows;
    const int nr = (int)(iend - i0);
    classify_band(cls, bd, nzc, i0, nr, kb);
    __syncthreads();
    // band descriptors (the caller keeps rb * ld * 8 < 2^31): rows at soffset r * ld8;
    // stores of lanes past the width go out of range and are dropped
    const int ld8 = (int)(ld * 8);
    const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(T + i0 * ld), (short)0, (int)((int64_t)nr * ld * 8), 0x00020000);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(Tout + i0 * ld), (short)0, (int)((int64_t)nr * ld * 8), 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(C + i0 * ldc), (short)0, (int)((int64_t)nr * ldc * 8), 0x00020000);
    const int voff = jc * 8;
    const int soff_bad = 0x7fffff00;
    const int voff_st = colok ? voff : soff_bad;
    const int coff = (threadIdx.x & 15) * 16;
    auto dense_at = [&](int r0) {
        if (r0 + U > nr) return false;
        return cls[r0] == kDense && cls[r0 + 1] == kDense;
    };
    double c[U][2][2];   // [row][half][even/odd step]
    auto loadc = [&](int r0, int h) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u4v x = __builtin_amdgcn_raw_buffer_load_b128(rc, coff + h * 256, (r0 + u) * (int)ldc * 8, 0);
            const d2 v = __builtin_bit_cast(d2, x);
            c[u][h][0] = v.x;
            c[u][h][1] = v.y;
        }
    };
    auto loadt = [&](double (&t)[U], int r0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u2v x = __builtin_amdgcn_raw_buffer_load_b64(rt, voff, (r0 + u) * ld8, NT ? 2 : 0);
            t[u] = __builtin_bit_cast(double, x);
        }
    };
    // one dense group (rows r0, r0+1 in t; their coefficients in c), with the loads of the
    // next group rn issued in vmcnt order: its rows first, the first half of its
    // coefficients once this group's first half has run, the second half at the end
    auto group = [&](double (&t)[U], double (&tn)[U], int r0, int rn) {
        loadt(tn, rn);
        __builtin_amdgcn_sched_barrier(0);
        dpp_half<0>(t, c, pr, std::make_integer_sequence<int, 32>{});
        __builtin_amdgcn_sched_barrier(0);
        loadc(rn, 0);
        __builtin_amdgcn_sched_barrier(0);
        dpp_half<32>(t, c, pr, std::make_integer_sequence<int, 32>{});
        __builtin_amdgcn_sched_barrier(0);
        loadc(rn, 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u)
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, t[u]), ro, voff_st, (r0 + u) * ld8,
                                                  kSt);
    };
    double ta[U], tb[U];
    int r = 0;
    while (r < nr) {
        if (dense_at(r)) {
            // a run of dense groups (the next group's loads are clamped to the current
            // one at the end of a run: harmless re-reads)
            loadt(ta, r);
            loadc(r, 0);
            loadc(r, 1);
            while (true) {
                const bool nb = dense_at(r + U);
                group(ta, tb, r, nb ? r + U : r);
                r += U;
                if (!nb) break;
                const bool na = dense_at(r + U);
                group(tb, ta, r, na ? r + U : r);
                r += U;
                if (!na) break;
            }
            continue;
        }
        // generic replay, one row (as pass_s_body)
        const int cl = cls[r];
        if (cl == kUntouched && outplace) {
            const u2v x = __builtin_amdgcn_raw_buffer_load_b64(rt, voff, r * ld8, NT ? 2 : 0);
            __builtin_amdgcn_raw_buffer_store_b64(x, ro, voff_st, r * ld8, kSt);
        } else if (cl != kUntouched) {
            const double* cr = C + (i0 + r) * ldc;
            double t = 0.0;
            if (cl < 0)
                t = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rt, voff, r * ld8, NT ? 2 : 0));
            t = replay_row(t, cl, pr, [&](int l) { return cr[l]; });
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, t), ro, voff_st, r * ld8, kSt);
        }
        r += 1;
    }
    if constexpr (PUB) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its sc1 stores are through
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(&bcnt[blockIdx.y], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Form 23: form 21's arithmetic (P[0..64) of one column per lane in 128 VGPRs, the
// coefficients broadcast by v_fmac_f64_dpp) with the tableau rows and their coefficient
// rows staged through an LDS ring instead of registers.  Form 21 holds one 2-row group
// ahead in registers: 1 KB in flight per wave, so the stream is latency-bound (4.2 TB/s).
// Here each wave keeps D groups of U rows in flight by LDS-DMA (global_load_lds_dwordx4:
// no VGPRs): ring slot = U rows x the wave's 64 columns, then the U rows' 64 coefficients
// (DMA k: rows 2k, 2k+1, lane l's 16 B = row 2k + l / 32, columns / steps 2 (l % 32), +1).
// The DMAs are issued from inline asm so that hipcc does not count them (it would wait
// vmcnt(0) before the next LDS read, draining the ring: cdna_hip_programming.md, glds);
// the kernel waits with its own counted vmcnt, which relies on every group issuing exactly
// U DMAs and U stores (rows with nothing to store aim a store out of range).  Groups whose
// U rows are all dense, or dense pivot rows (recomputed after the chain: redo_pivot_row),
// run the chains from LDS; any other group replays row by row
// (replay_row: T and the coefficients from the slot, P from the registers).  Lab:
// 7.3-7.5 ms per C3 pass against form 21's 8.2-8.5 (tools/passlab.hip f4r, bit-exact).
// newer than group g's U DMAs: U per prologue group still to come and 2 U (U stores + U
// DMAs) per finished group: U (D - 1) + U g while g < D - 1, then 2 U (D - 1)
template <int D, int U>
__device__ __forceinline__ void vmwait_group(int g) {
    static_assert(D <= 8 && 2 * U * (D - 1) <= 63, "vmcnt holds 6 bits");
    if (g >= D - 1) {
        vmwait<2 * U * (D - 1)>();
        return;
    }
    switch (g) {
        case 0: vmwait<U * (D - 1)>(); break;
        case 1: vmwait<U * (D - 1) + U>(); break;
        case 2: vmwait<U * (D - 1) + 2 * U>(); break;
        case 3: vmwait<U * (D - 1) + 3 * U>(); break;
        case 4: vmwait<U * (D - 1) + 4 * U>(); break;
        case 5: vmwait<U * (D - 1) + 5 * U>(); break;
        default: vmwait<U * (D - 1) + 6 * U>(); break;
    }
}
// The same wait under a shared coefficient ring (pass_q_kernel, CS): a group is U / 2 tableau DMAs and
// U stores, and the first group of every supergroup of G issues U / 2 coefficient DMAs ahead of them
// (behind its own wait).  Newer than group g's tableau DMAs: the D - 1 groups between, and the
// coefficient DMAs of a supergroup that opened among them: when g lies 1 .. D - 1 past a supergroup's
// start (p = g % G; D <= G, so at most one).  The coefficient DMAs of g's own supergroup are older
// than its first group's tableau DMAs, so that group's wait covers them.
template <int D, int U>
__device__ __forceinline__ void vmwait_group_cs(int g, int p) {
    constexpr int h = U / 2;
    static_assert(D >= 2 && D <= 4 && 3 * h * (D - 1) + h <= 63, "vmcnt holds 6 bits");
    if (g >= D - 1) {
        if (p >= 1 && p <= D - 1)
            vmwait<3 * h * (D - 1) + h>();
        else
            vmwait<3 * h * (D - 1)>();
        return;
    }
    // the prologue's groups still to come, the finished groups, supergroup 1's coefficients (g >= 1)
    if (g == 0)
        vmwait<h * (D - 1)>();
    else if (g == 1)
        vmwait<h * (D > 2 ? D - 2 : 0) + 3 * h + h>();
    else
        vmwait<h * (D > 3 ? D - 3 : 0) + 6 * h + h>();
}
template <int U, int L>
__device__ __forceinline__ void ring_step(double (&t)[U], const double (&c)[U][2], const double (&pr)[64]) {
    constexpr int e = L & 1, n = (L & 31) >> 1;
#pragma unroll
    for (int u = 0; u < U; ++u) fmac_bc<n>(t[u], c[u][e], pr[L]);
}
template <int U, int L0, int... I>
__device__ __forceinline__ void ring_half(double (&t)[U], const double (&c)[U][2], const double (&pr)[64],
                                          std::integer_sequence<int, I...>) {
    (ring_step<U, L0 + I>(t, c, pr), ...);
}

// A dense pivot row (classify_band, kDensePiv) of a group that ran the chain: its value again,
// as replay_row computes it: t = P[cl], then the DPP steps l > cl only, the unrolled sequence
// entered by a uniform test per step (cl in a scalar).  cr: the row's 64 coefficients in the
// ring slot; each half's registers are written by its LDS load alone.
template <int L>
__device__ __forceinline__ void redo_step(double& t, const double (&c)[2], const double (&pr)[64], int cl) {
    constexpr int e = L & 1, n = (L & 31) >> 1;
    if (L == cl)
        t = pr[L];
    else if (L > cl)
        fmac_bc<n>(t, c[e], pr[L]);
}
template <int L0, int... I>
__device__ __forceinline__ void redo_half(double& t, const double (&c)[2], const double (&pr)[64], int cl,
                                          std::integer_sequence<int, I...>) {
    (redo_step<L0 + I>(t, c, pr, cl), ...);
}
__device__ __forceinline__ double redo_pivot_row(const double* cr, int cl, const double (&pr)[64]) {
    // the lane id, made here: a rare path must not hold an address register across the chain
    // (the kernel sits at its 168 VGPRs)
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    double t = 0.0;
    if (cl < 32) {
        const d2 v = *(const d2*)(cr + 2 * (lane & 15));
        const double c0[2] = {v.x, v.y};
        redo_half<0>(t, c0, pr, cl, std::make_integer_sequence<int, 32>{});
    }
    const d2 v = *(const d2*)(cr + 32 + 2 * (lane & 15));
    const double c1[2] = {v.x, v.y};
    redo_half<32>(t, c1, pr, cl, std::make_integer_sequence<int, 32>{});
    return t;
}

// PUB: band publication as form 21's (pass_d_kernel)
// pivg: groups of dense and dense pivot rows run the chain too (DLP_PASS_PIVG, default 1)
// SA: the LDS-DMAs in the scalar-base form (DLP_PASS_SADDR, default 1)
// CS (with SA): the coefficient rows fetched once per workgroup (DLP_PASS_CSHARE).  The four waves of a
// workgroup run the same rows of the band, so their coefficient DMAs are the same 512 B per row four
// times over.  Here each wave keeps a private ring of D tableau slots (U rows x 64 columns), and the
// workgroup shares one coefficient ring behind them: NS = 2 slots of a supergroup of G = 4 consecutive
// groups (G U rows x 64 coefficients).  Wave w fetches group G sg + w of supergroup sg, U / 2 DMAs, all
// waves at the same place: behind the barrier that opens supergroup sg - 1.  One barrier per
// supergroup: every wave waits for its own DMAs of supergroup sg (the counted wait of the
// supergroup's first group covers them, vmwait_group_cs), then the barrier, then reads any wave's
// rows; the same barrier says that every wave is done with supergroup sg - 1, whose slot is refilled
// behind it.  A bare s_barrier: __syncthreads() would drain the ring and the stores.  Every wave of a
// workgroup runs the same ng groups on every path, so the barriers match.
// NL (with NT): the tableau DMAs carry the nt policy (DLP_PASS_NTLOAD): the tableau is read once per
// pass, and a default-policy stream of its size evicts what the chain beside the pass and the pass
// itself re-read (C, P, cls, nzc: those loads, and the coefficient DMAs, keep the default policy).
// Only the asm string differs: the DMAs per group, and with them the counted waits, stay.
// (three waves per SIMD, at most 168 VGPRs, as before the pivot-row recompute was added)
template <bool NT, int U, int D, bool SA = false, bool CS = false, bool NL = false, bool PUB = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void pass_q_kernel(
                                                     const double* __restrict__ T, double* __restrict__ Tout,
                                                     int64_t ld, int64_t rows, int64_t width,
                                                     const BlockDesc* __restrict__ bd,
                                                     const double* __restrict__ C, int64_t ldc,
                                                     const double* __restrict__ P,
                                                     const int32_t* __restrict__ nzc, int rb,
                                                     uint32_t* bcnt = nullptr, int pivg = 0) {
    constexpr int K = 64, SLOT = (CS ? 64 : 128) * U;   // doubles per ring slot
    constexpr int G = 4, NS = 2;                          // CS: groups per supergroup, supergroup slots
    static_assert(!CS || (SA && G == 4 && D <= G), "one group per wave; the shared ring's counted waits");
    constexpr int kSt = (NT ? 2 : 0) | (PUB ? kAuxSc1 : 0);   // store policy
    static_assert(U % 2 == 0, "one DMA carries two rows");
    __shared__ __attribute__((aligned(16))) int32_t cls[1024];
    typedef int32_t clsv __attribute__((ext_vector_type(U)));
    extern __shared__ double ring[];   // [4 waves][D slots][SLOT]; CS: then [NS][G groups][U rows][64]
    const int kb = bd->blk;
    const bool outplace = Tout != T;
    if (kb == 0 && !outplace) return;   // full and partial blocks alike (zeroed tails)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool colok = j < width;
    const int jc = (int)(colok ? j : width - 1);
    double pr[K];   // all 64 rows: a partial block's P[l >= kb] is +0 (zeroed at block start)
#pragma unroll
    for (int l = 0; l < K; ++l) pr[l] = P[(int64_t)l * ld + jc];
    const int64_t i0 = (int64_t)blockIdx.y * rb;
    const int64_t iend = (i0 + rb < rows) ? i0 + rb : rows;
    const int nr = (int)(iend - i0);
    classify_band(cls, bd, nzc, i0, nr, kb, pivg != 0);
    __syncthreads();
    // the P loads complete here, before the ring starts (else hipcc waits for them, and
    // with them for everything, at the top of every group)
#pragma unroll
    for (int l = 0; l < K; ++l) asm volatile("" ::"v"(pr[l]));
    const int ng = (nr + U - 1) / U;
    // DMA sources: this lane's row of each DMA (row 2k + lane / 32 of a group, clamped to the
    // band) and its 16 B of the wave's 64 columns (clamped inside the row stride) / of the
    // row's 64 coefficients
    const int64_t wc = (int64_t)blockIdx.x * 256 + w * 64 + 2 * (lane & 31);
    const int64_t wcc = wc < ld - 1 ? wc : ld - 2;
    double* wbase = ring + (size_t)w * D * SLOT;
    const uint32_t lbase = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)wbase;
    const double* cring = ring + (size_t)4 * D * SLOT;
    const uint32_t cbase = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)cring;
    // SA: every DMA in the scalar-base form (glds16s).  The base is the DMA's first row, wave-uniform;
    // the lane's byte offset is fixed for the band: its row of the pair and its clamped column
    // (tvoff; ld * 8 + wcc * 8 < 2^32 since rb * ld * 8 < 2^31), its 16 B of the pair's 128
    // coefficients (cvoff).  Steady state: the refilled group lies wholly inside the band, its bases
    // run ahead by scalar adds (tb, cb: U rows on per group) and no VALU instruction belongs to a
    // DMA.  Elsewhere (the prologue, the last D refills, a short last group) the row clamp of the
    // per-lane form is taken on the base, and on a pair whose second row is past the band both
    // halves read the band's last row: the same source bytes as the per-lane form's.
    uint32_t tvoff = 0, cvoff = 0;
    const double *tsrc = nullptr, *csrc = nullptr;
    if constexpr (SA) {
        tvoff = (uint32_t)(lane >> 5) * (uint32_t)(ld * 8) + (uint32_t)(wcc * 8);
        cvoff = 16u * lane;
    } else {
        tsrc = T + i0 * ld + wcc;
        csrc = C + i0 * ldc + 2 * (lane & 31);
    }
    auto dma = [&](int g, int s) {
        const int gg = g < ng ? g : ng - 1;
#pragma unroll
        for (int k = 0; k < U / 2; ++k) {
            const uint32_t m0 = __builtin_amdgcn_readfirstlane(lbase + s * SLOT * 8 + k * 1024);
            if constexpr (SA) {
                const int rk = gg * U + 2 * k;
                const bool pair = rk + 1 < nr;   // (uniform)
                const uint32_t up = lane >> 5 ? (uint32_t)(ld * 8) : 0u;
                glds16s<NL>(pair ? tvoff : tvoff - up, T + (i0 + (rk < nr ? rk : nr - 1)) * ld, m0);
            } else {
                int r = gg * U + 2 * k + (lane >> 5);
                r = r < nr ? r : nr - 1;
                glds16<NL>(tsrc + (int64_t)r * ld, m0);
            }
        }
        if constexpr (CS) return;
#pragma unroll
        for (int k = 0; k < U / 2; ++k) {
            const uint32_t m0 = __builtin_amdgcn_readfirstlane(lbase + s * SLOT * 8 + U * 512 + k * 1024);
            if constexpr (SA) {
                const int rk = gg * U + 2 * k;
                const bool pair = rk + 1 < nr;
                glds16s(pair ? cvoff : cvoff & 511u, C + (i0 + (rk < nr ? rk : nr - 1)) * ldc, m0);
            } else {
                int r = gg * U + 2 * k + (lane >> 5);
                r = r < nr ? r : nr - 1;
                glds16(csrc + (int64_t)r * ldc, m0);
            }
        }
    };
    const int ngs = SA ? nr / U : 0;   // refills of groups [D, ngs) are in the steady state
    const int64_t tstep = (int64_t)U * ld * 8, cstep = (int64_t)U * ldc * 8;
    const char* tb = (const char*)(T + i0 * ld) + D * tstep;   // group g + D's first row
    const char* cb = (const char*)(C + i0 * ldc) + D * cstep;
    auto dma_s = [&](int s) {
#pragma unroll
        for (int k = 0; k < U / 2; ++k)
            glds16s<NL>(tvoff, tb + (int64_t)2 * k * ld * 8,
                    __builtin_amdgcn_readfirstlane(lbase + s * SLOT * 8 + k * 1024));
        if constexpr (CS) return;
#pragma unroll
        for (int k = 0; k < U / 2; ++k)
            glds16s(cvoff, cb + (int64_t)2 * k * ldc * 8,
                    __builtin_amdgcn_readfirstlane(lbase + s * SLOT * 8 + U * 512 + k * 1024));
    };
    // CS: this wave's group of supergroup sg (group G sg + w) into shared slot cs; a group that does not
    // lie wholly inside the band takes dma's row clamp on the base
    auto dma_c = [&](int sg, int cs) {
        const int gq = G * sg + w;
        const uint32_t dst = cbase + (uint32_t)((cs * G + w) * U * 512);
        const bool inside = (gq + 1) * U <= nr;   // (uniform)
        const int gg = gq < ng ? gq : ng - 1;
#pragma unroll
        for (int k = 0; k < U / 2; ++k) {
            const uint32_t m0 = __builtin_amdgcn_readfirstlane(dst + k * 1024);
            if (inside) {
                glds16s(cvoff, C + (i0 + gq * U + 2 * k) * ldc, m0);
            } else {
                const int rk = gg * U + 2 * k;
                const bool pair = rk + 1 < nr;
                glds16s(pair ? cvoff : cvoff & 511u, C + (i0 + (rk < nr ? rk : nr - 1)) * ldc, m0);
            }
        }
    };
    // band descriptor (the caller keeps rb * ld * 8 < 2^31): rows at soffset r * ld8; stores
    // of lanes past the width, and of rows with nothing to store, go out of range (dropped)
    const int ld8 = (int)(ld * 8);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(Tout + i0 * ld), (short)0, (int)((int64_t)nr * ld * 8), 0x00020000);
    const int voff_st = colok ? jc * 8 : 0x7fffff00;
    auto store = [&](double v, int r, bool keep) {
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, v), ro, keep ? voff_st : 0x7fffff00,
                                              (r < nr ? r : 0) * ld8, kSt);
    };
    if constexpr (CS) dma_c(0, 0);   // (older than group 0's tableau DMAs)
#pragma unroll
    for (int s = 0; s < D; ++s) dma(s, s);
    int s = 0;
    for (int g = 0; g < ng; ++g) {
        if constexpr (CS) {
            const int p = g % G;   // the group's place in its supergroup
            vmwait_group_cs<D, U>(g, p);
            if (p == 0) {   // (uniform) behind the barrier this supergroup's rows are in, the last one's slot is free
                asm volatile("s_barrier" ::: "memory");
                dma_c(g / G + 1, (g / G + 1) % NS);
            }
        } else {
            vmwait_group<D, U>(g);
        }
        const double* sl = wbase + s * SLOT;
        // the group's coefficient rows (CS: group g % G of slot g / G % NS)
        const double* cf = CS ? cring + g % (NS * G) * U * 64 : sl + U * 64;
        const int r0 = g * U;
        // the group's U classes in one LDS read (a short last group is never dense; rb <= 1024)
        const clsv cv = *(const clsv*)(cls + r0);
        bool dense = r0 + U <= nr, anyp = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cu = __builtin_amdgcn_readfirstlane(cv[u]);
            dense = dense && (cu == kDense || cu >= kDensePiv);
            anyp = anyp || cu >= kDensePiv;
        }
        if (dense) {   // (uniform)
            double t[U];
#pragma unroll
            for (int u = 0; u < U; ++u) t[u] = sl[u * 64 + lane];
            double c[U][2];
            auto loadc = [&](int h) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const d2 v = *(const d2*)(cf + u * 64 + h * 32 + 2 * (lane & 15));
                    c[u][0] = v.x;
                    c[u][1] = v.y;
                }
            };
            loadc(0);
            ring_half<U, 0>(t, c, pr, std::make_integer_sequence<int, 32>{});
            loadc(1);
            ring_half<U, 32>(t, c, pr, std::make_integer_sequence<int, 32>{});
            if (anyp) {   // (uniform; rare: at most kb rows of the whole tableau)
#pragma nounroll
                for (int u = 0; u < U; ++u) {
                    const int cl = __builtin_amdgcn_readfirstlane(cls[r0 + u]) - kDensePiv;
                    if (cl < 0) continue;
                    const double tp = redo_pivot_row(cf + u * 64, cl, pr);
#pragma unroll
                    for (int k = 0; k < U; ++k) t[k] = k == u ? tp : t[k];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) store(t[u], r0 + u, true);
        } else {
            // generic replay, row by row (form 21's); exactly U stores for the counted waits
            for (int u = 0; u < U; ++u) {
                const int r = r0 + u;
                int cl = r < nr ? cls[r] : kUntouched;
                if (cl >= kDensePiv) cl -= kDensePiv;
                double t = sl[u * 64 + lane];
                if (cl == kUntouched) {
                    store(t, r, outplace && r < nr);
                    continue;
                }
                const double* cr = cf + u * 64;   // the row's coefficients (broadcast reads)
                t = replay_row(t, cl, pr, [&](int l) { return cr[l]; });
                store(t, r, true);
            }
        }
        if (SA && g + D < ngs) {   // (uniform)
            dma_s(s);
        } else {
            dma(g + D, s);
        }
        if constexpr (SA) {
            tb += tstep;
            cb += cstep;
        }
        s = s + 1 == D ? 0 : s + 1;
    }
    if constexpr (PUB) {
        vmwait<0>();   // every wave: its sc1 stores are through (and the clamped tail DMAs landed)
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(&bcnt[blockIdx.y], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}


// Form 22: the K = 64 pass on the matrix cores.  v_mfma_f64_16x16x4f64 rounds exactly as
// four sequential fmas in k order (tools/mfma_probe.hip: 51.2 M random elements, denormal
// and signed-zero operands included), so T_tile := mfma(-C_frag, P_frag, T_tile) over the
// 16 k-blocks of a block is the eager sequence t = fma(-C[i][l], P[l][c], t), l = 0..63.
// Workgroup: 4 waves x NT 16-column tiles (64 NT columns) of a band; each wave keeps the
// P fragments of its tiles (16 x NT doubles per lane) for the band; the 4 waves share
// each 16-row group, whose coefficient rows are staged in LDS (rows padded to 66 doubles:
// conflict-free A-fragment reads) by LDS-DMA with per-lane source addresses, one group
// ahead, next to the next group's T tiles in registers.  Accumulator layout: lane l, reg i
// = row l/16 + 4 i, column l%16.  Every group runs through the MFMAs; only rows of class
// dense are stored, the rest (the block's pivot rows, sparse rows; copies of untouched
// rows out of place) go through the generic replay afterwards.  Partial blocks run the
// same code (tails zeroed at block start).
typedef double d4 __attribute__((ext_vector_type(4)));
// PUB (lookahead, round 5): band publication as form 21's — every output store write-through
// (sc1, beside nt) through a band buffer resource, every wave drained, then one agent-scope add
// to the band's count (pass_d_kernel).  The caller keeps rb * ld * 8 < 2^31.
template <bool NT_, int NT, bool PUB = false>
__global__ __launch_bounds__(256, 2) void pass_m_kernel(const double* __restrict__ T, double* __restrict__ Tout,
                                                     int64_t ld, int64_t rows, int64_t width,
                                                     const BlockDesc* __restrict__ bd,
                                                     const double* __restrict__ C, int64_t ldc,
                                                     const double* __restrict__ P,
                                                     const int32_t* __restrict__ nzc, int rb,
                                                     uint32_t* bcnt = nullptr) {
    constexpr int kSt = (NT_ ? 2 : 0) | (PUB ? kAuxSc1 : 0);   // store policy (PUB)
    constexpr int K = 64, KB = K / 4, W = 16 * NT, RS = K + 2;
    constexpr int NPC = (16 * RS + 127) / 128;   // 1 KiB LDS-DMA pieces per group
    // ONE __shared__ object (the coefficient stages, then the row classes): with a second one
    // beside the LDS-DMA target, hipcc waits vmcnt(0) before the class reads of the stores,
    // draining the next group's prefetch every group (cdna_hip_programming.md, glds traps)
    __shared__ double lds_all[2 * NPC * 128 + 512];
    double(*As)[NPC * 128] = reinterpret_cast<double(*)[NPC * 128]>(lds_all);
    int32_t* cls = reinterpret_cast<int32_t*>(lds_all + 2 * NPC * 128);
    const int kb = bd->blk;
    const bool outplace = Tout != T;
    if (kb == 0 && !outplace) return;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int64_t cw = (int64_t)blockIdx.x * (4 * W);   // the workgroup's first column
    const int64_t c0 = cw + w * W;
    double b[KB][NT];   // P fragments: rows 4 b + lq, column c0 + 16 t + lr
#pragma unroll
    for (int k4 = 0; k4 < KB; ++k4)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t col = c0 + 16 * t + lr;
            b[k4][t] = P[(int64_t)(4 * k4 + lq) * ld + (col < width ? col : width - 1)];
        }
    const int64_t i0 = (int64_t)blockIdx.y * rb;
    const int64_t iend = (i0 + rb < rows) ? i0 + rb : rows;
    const int nr = (int)(iend - i0);
    classify_band(cls, bd, nzc, i0, nr, kb);
    const int ng = (nr + 15) / 16;
    // PUB: the band's output through one buffer resource (byte offsets column * 8 + row * ld8;
    // the caller keeps rb * ld * 8 < 2^31)
    const int ld8 = (int)(ld * 8);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(Tout + i0 * ld), (short)0, (int)((int64_t)nr * ld * 8), 0x00020000);
    (void)ro;
    (void)ld8;
    auto stage = [&](int g, int buf) {
        const int gg = g < ng ? g : ng - 1;
        for (int pc = w; pc < NPC; pc += 4) {
            const int e0 = pc * 128 + 2 * lane;   // this lane's LDS doubles e0, e0 + 1
            int r = e0 / RS, c = e0 % RS;
            if (c >= K || r >= 16) {   // padding: any valid source
                r = 0;
                c = 0;
            }
            int64_t row = i0 + (int64_t)gg * 16 + r;
            row = row < iend ? row : iend - 1;
            __builtin_amdgcn_global_load_lds(C + row * ldc + c,
                                             (__attribute__((address_space(3))) void*)&As[buf][pc * 128], 16, 0, 0);
        }
    };
    auto loadt = [&](d4 (&acc)[NT], int g) {
        const int gg = g < ng ? g : ng - 1;
        const int64_t r0 = i0 + (int64_t)gg * 16;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int64_t col = c0 + 16 * t + lr;
            const int64_t cc = col < width ? col : width - 1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int64_t row = r0 + lq + 4 * i;
                row = row < iend ? row : iend - 1;
                acc[t][i] = NT_ ? __builtin_nontemporal_load(T + row * ld + cc) : T[row * ld + cc];
            }
        }
    };
    d4 ta[NT], tb[NT];
    stage(0, 0);
    loadt(ta, 0);
    constexpr int STG = (NPC + 3) / 4;   // staging instructions per wave per group
    for (int g = 0; g < ng; g += 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int gg = g + h;
            if (gg >= ng) break;
            d4(&acc)[NT] = h == 0 ? ta : tb;
            d4(&nxt)[NT] = h == 0 ? tb : ta;
            // cls is complete; buffer (gg + 1) & 1 is free (group gg - 1 done).  Raw barriers: a
            // __syncthreads() waits vmcnt(0), which would drain the prefetch issued below
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            stage(gg + 1, (gg + 1) & 1);
            loadt(nxt, gg + 1);
            // this group's staging and tile: all but the loads just issued
            constexpr int NEWV = NT * 4 + STG;
            __builtin_amdgcn_s_waitcnt(0x3F70 | (NEWV & 0xF) | ((NEWV >> 4) << 14));
            asm volatile("s_barrier" ::: "memory");   // every wave's pieces of this group landed
            const double* a = &As[gg & 1][lr * RS + lq];
#pragma unroll
            for (int k4 = 0; k4 < KB; ++k4) {
                const double av = -a[4 * k4];
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[k4][t], acc[t], 0, 0, 0);
            }
            const int rl0 = gg * 16;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int64_t col = c0 + 16 * t + lr;
                if (col < width)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int rl = rl0 + lq + 4 * i;
                        if (rl < nr && cls[rl] == kDense) {
                            if constexpr (PUB) {   // (per-lane row: in the VGPR offset, not the SGPR one)
                                const double v = acc[t][i];
                                __builtin_amdgcn_raw_buffer_store_b64(dbits(v), ro,
                                                                      (int)col * 8 + (lq + 4 * i) * ld8, rl0 * ld8,
                                                                      kSt);
                            } else {
                                double* q = Tout + (i0 + rl) * ld + col;
                                if (NT_)
                                    __builtin_nontemporal_store(acc[t][i], q);
                                else
                                    *q = acc[t][i];
                            }
                        }
                    }
            }
        }
    }
    // everything else, row by row (as pass_s_body's generic replay): the 256 threads as
    // 256 / WC row slices x the workgroup's WC = 4 W columns
    constexpr int WC = 4 * W;
    const int64_t j = cw + (threadIdx.x % WC);
    const bool jok = j < width && threadIdx.x < (256 / WC) * WC;
    for (int r = threadIdx.x / WC; jok && r < nr; r += 256 / WC) {
        const int cl = cls[r];
        if (cl == kDense || (cl == kUntouched && !outplace)) continue;
        const double* row = T + (i0 + r) * ld;
        double t;
        if (cl == kUntouched) {
            t = row[j];
        } else {
            int l = 0;
            if (cl >= 0) {
                t = P[(int64_t)cl * ld + j];
                l = cl + 1;
            } else {
                t = row[j];
            }
            const double* cr = C + (i0 + r) * ldc;
            for (; l < kb; ++l) {
                const double f = cr[l];
                if (f != 0.0) t = __builtin_fma(-f, P[(int64_t)l * ld + j], t);
            }
        }
        if constexpr (PUB)   // (r differs between the lanes: VGPR offset)
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, t), ro, (int)j * 8 + r * ld8, 0, kSt);
        else
            Tout[(i0 + r) * ld + j] = t;
    }
    if constexpr (PUB) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its sc1 stores are through
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(&bcnt[blockIdx.y], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void blk_reset_kernel(DevState* st) {
    if (threadIdx.x == 0) {
        st->blk = 0;
        st->bser = st->bser + 1;   // (condensed tableau: the next block's restarts are its own)
    }
}

// Condensed tableau: before a block's pass, each slot restarted in the block gets the unit
// vector of its new variable (1 in the step's pivot row, +0 elsewhere) in the pass's INPUT, in
// step order (a slot restarted twice keeps the later one): the pass then replays every step on it,
// the steps before the restart being no-ops (their P entries of the slot were zeroed by the
// commit).  One lane per local row; a column write, 8 B per row per restart.
__global__ __launch_bounds__(256) void reset_cols_kernel(double* __restrict__ T, int64_t ld, int64_t rows,
                                                         const int32_t* __restrict__ blkp,
                                                         const int32_t* __restrict__ pl,
                                                         const int32_t* __restrict__ qs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const int kb = *blkp;
    double* r = T + i * ld;
    for (int l = 0; l < kb; ++l) r[qs[l]] = (pl[l] == (int32_t)i) ? 1.0 : 0.0;
}

// A step that found no eligible row (DLP_UNBOUNDED) is no step of its block, but its ratio
// kernel has written the entering column as the coefficients of step kb (C, counted in nzc),
// where the passes expect the zeroed tail: fma(-a, P[kb] = +0, t) turns t = -0 into +0 where
// a < 0 or a = -0.  Before the block's pass, that column goes back to +0 and out of the counts
// (one lane per local row and the objective row; nothing to do in any other state).
__global__ __launch_bounds__(256) void drop_failed_step_kernel(const DevState* __restrict__ st,
                                                               const int32_t* __restrict__ blkp,
                                                               double* __restrict__ C, int64_t ldc,
                                                               int32_t* __restrict__ nzc, int64_t rows) {
    if (st->status != DLP_UNBOUNDED) return;
    const int kb = *blkp;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > rows || kb < 0 || kb >= ldc) return;
    const double a = C[i * ldc + kb];
    if (i < rows && a != 0.0) nzc[i] = nzc[i] - 1;
    C[i * ldc + kb] = 0.0;
}

// Lookahead: the block just selected becomes st->seal[slot] (read by its pass and
// replayed by the next block's selections); the next block starts empty.
// (bcnt: the slot's band counts restart at 0 for the pass about to be launched, whose
// output the next block's selections poll; the slot's previous pass has finished.)
// A block that ended on a failed step (drop_failed_step_kernel's case: DLP_UNBOUNDED, rare and
// terminal) is cleaned here, behind the selection that failed and before the block's pass: column
// kb of C back to +0 and out of the counts, the 64 lanes over the rows and the objective row.
__global__ __launch_bounds__(64) void seal_kernel(DevState* st, int slot, uint32_t* bcnt, int64_t nb,
                                                  double* __restrict__ C, int64_t ldc,
                                                  int32_t* __restrict__ nzc, int64_t rows) {
    const int kb = st->blk;
    if (C && nzc && st->status == DLP_UNBOUNDED && kb >= 0 && kb < ldc)
        for (int64_t i = threadIdx.x; i <= rows; i += 64) {
            const double a = C[i * ldc + kb];
            if (i < rows && a != 0.0) nzc[i] = nzc[i] - 1;
            C[i * ldc + kb] = 0.0;
        }
    for (int l = threadIdx.x; l < kMaxDefer; l += 64) {
        st->seal[slot].pl[l] = l < kb ? st->pl[l] : -1;
        st->seal[slot].qs[l] = st->qs[l];
    }
    if (bcnt)
        for (int64_t b = threadIdx.x; b < nb; b += 64) bcnt[b] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        st->seal[slot].blk = kb;
        st->seal[slot].ser = st->bser;
        st->blk = 0;
        st->bser = st->bser + 1;
    }
}

}  // namespace

template <bool NT, int K, int V, int U, int D>
static void launch_pass_r(const Geometry& g, const Defer& d, DevState* st, int rb, size_t dyn,
                          int order, hipStream_t s) {
    const int ntiles = (int)((g.width + 256 * V - 1) / (256 * V));
    const int nbands = (int)((g.rows + rb - 1) / rb);
    const int64_t total = (int64_t)ntiles * nbands;
    const int64_t t8 = (ntiles + 7) / 8;
    const dim3 grid((unsigned)(order == 1 ? 8 * ((total + 7) / 8) : order == 2 ? 8 * t8 * nbands : total));
    pass_r_kernel<NT, K, V, U, D, false><<<grid, 256, dyn, s>>>(
        g.T, g.ld, g.rows, g.width, st, d.C, d.ldc, d.P, d.nzc, rb, ntiles, nbands, order);
    pass_r_kernel<NT, K, V, U, D, true><<<grid, 256, dyn, s>>>(
        g.T, g.ld, g.rows, g.width, st, d.C, d.ldc, d.P, d.nzc, rb, ntiles, nbands, order);
}

// DLP_PASS_LDS=<bytes> (tuning only): the dynamic LDS of the forms-21/23 pass workgroups, which caps
// how many share a CU while leaving the rest of the 160 KiB to the chain kernels beside them
static size_t pass_lds_env() {
    static const long v = env_long("DLP_PASS_LDS", 0);
    return v > 0 && v <= 150 * 1024 ? (size_t)v : 0;
}

// The form-23 instance (pass_q_kernel) runs for this session's passes (K = 64 blocks, ldc == 64
// exactly: the kernel addresses C with 64 steps per row; a band within one 2 GiB descriptor)
static bool pass_q_runs(const Geometry& g, const Defer& d, int rb) {
    return d.form == 23 && d.K == 64 && d.ldc == 64 && (int64_t)rb * g.ld * 8 < ((int64_t)1 << 31) && rb <= 1024;
}
// DLP_PASS_SADDR=0 (A/B): every LDS-DMA of the form-23 pass in the clamped per-lane form
static bool pass_saddr_env() {
    static const int v = env_int("DLP_PASS_SADDR", 1);
    return v != 0;
}

// Dynamic LDS that leaves room for at most `occ` workgroups on a CU (160 KiB each), the kernel's
// static LDS counting against the same 160 KiB.
static size_t occ_lds(int occ, size_t static_bytes) { return (size_t)160 * 1024 / occ - static_bytes; }
constexpr size_t kClsLds = 1024 * sizeof(int32_t);                            // cls[1024]
constexpr size_t kStreamLds = kClsLds + 512 * sizeof(int16_t) + 16;           // cls[1024], dgl[512], s_wtot[4]
constexpr size_t kMfmaLds = kClsLds + 2 * 9 * 128 * sizeof(double);           // cls[1024], the form-22 panels

// a band within one 2 GiB buffer descriptor
static bool band_in_descriptor(const Geometry& g, int rb) { return (int64_t)rb * g.ld * 8 < ((int64_t)1 << 31); }

// DLP_PASS_CSHARE (A/B): 1 / 0: the form-23 pass's coefficient rows fetched once per workgroup (the
// shared ring, pass_q_kernel's CS) wherever such an instance exists and the scalar-base DMAs are on /
// nowhere; unset: the shipped choice per geometry (pass_cshare_default)
static int pass_cshare_env() {
    static const int v = env_int("DLP_PASS_CSHARE", -1);
    return v;
}
// The shipped choice, by the rows per group (U = 4 from 16,384 local rows, else 2): shared with 4 rows (C3:
// the pass equal, the chain beside it faster, the bench line +1% in 12 of 12 alternating pairs; c3r2: the
// pass 2.1% faster), not with 2 (c3r4: the pass 2% slower); DESIGN.md 16.4, profiles/c3_pass_cshare/
static bool pass_cshare_default(int U) { return U == 4; }
// The shared ring is compiled for the (U, D) that can be chosen: the two U = 4 depths and U = 2's default
constexpr bool pass_q_shared_exists(int U, int D) { return (U == 4 && (D == 2 || D == 3)) || (U == 2 && D == 4); }
constexpr int kCsG = 4, kCsNS = 2;   // pass_q_kernel's G and NS
// The ring of one form-23 workgroup: 4 waves x D slots of U rows (x 64 columns, and without the shared
// ring their 64 coefficients), then the shared coefficient ring
static size_t pass_q_lds(int U, int D, bool shared) {
    return shared ? ((size_t)4 * D + kCsNS * kCsG) * 64 * U * sizeof(double) : (size_t)4 * D * 128 * U * sizeof(double);
}

// DLP_PASS_NTLOAD (A/B): 1 / 0: the form-23 pass's tableau DMAs with the nt policy wherever such an
// instance exists (and the session is nontemporal) / nowhere; unset: the shipped choice
static int pass_ntload_env() {
    static const int v = env_int("DLP_PASS_NTLOAD", -1);
    return v;
}
// The shipped choice: on at every geometry (C3: the pass 39 us shorter, the chain kernels beside it 1.1-1.3 us
// each, the bench line +1.8% against the parent in four alternating pairs; c3r2 +2.1 / +2.6%, c3r4 +0.8 / +2.6%);
// DESIGN.md 16.5, profiles/c3_pass_ntload/
constexpr bool kPassNtloadDefault = true;
// The nt DMAs are compiled for the instances the auto policy picks on a streaming tableau: (U, D) = (4, 2)
// and (2, 4), scalar-base or per-lane, and with the shared coefficient ring where it is the shipped choice
constexpr bool pass_q_ntload_exists(bool NT, int U, int D, bool cs) {
    return NT && ((U == 4 && D == 2) || (U == 2 && D == 4 && !cs));
}

// The form-23 instance of (U, D): scalar-base DMAs or per-lane ones (sad), the shared coefficient ring
// (csh; with sad), publishing or not (bcnt); the nt tableau DMAs where asked for and compiled
template <bool NT, int U, int D>
static void launch_pass_q(const Geometry& g, const Defer& d, const BlockDesc* bd, double* To, int rb,
                          uint32_t* bcnt, bool sad, bool csh, int pivg, dim3 grid, size_t dyn, hipStream_t s) {
    const int nle = pass_ntload_env();
    const bool ntl = nle >= 0 ? nle != 0 : kPassNtloadDefault;
    auto go = [&](auto sa, auto cs, auto pub) {
        constexpr bool SA = decltype(sa)::value, CS = decltype(cs)::value, PUB = decltype(pub)::value;
        if constexpr (pass_q_ntload_exists(NT, U, D, CS)) {
            if (ntl) {
                pass_q_kernel<NT, U, D, SA, CS, true, PUB><<<grid, 256, dyn, s>>>(
                    g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc, d.P, d.nzc, rb, bcnt, pivg);
                return;
            }
        }
        pass_q_kernel<NT, U, D, SA, CS, false, PUB><<<grid, 256, dyn, s>>>(
            g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc, d.P, d.nzc, rb, bcnt, pivg);
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if constexpr (pass_q_shared_exists(U, D)) {
        if (sad && csh) {
            bcnt ? go(yes, yes, yes) : go(yes, yes, no);
            return;
        }
    }
    if (sad)
        bcnt ? go(yes, no, yes) : go(yes, no, no);
    else
        bcnt ? go(no, no, yes) : go(no, no, no);
}

template <bool NT, int K>
static hipError_t pass(const Geometry& g, const Defer& d, DevState* st, int rb, int occ,
                       hipStream_t s, double* Tout, int seal, uint32_t* bcnt) {
    // lookahead: out of place, the sealed block; pass_s forms only (lookahead_form)
    if (seal >= 0 && !lookahead_form(d.form)) return hipErrorInvalidValue;
    const BlockDesc* bd = seal >= 0 ? &st->seal[seal] : (const BlockDesc*)&st->blk;
    double* To = Tout ? Tout : g.T;
    const unsigned nbands = (unsigned)((g.rows + rb - 1) / rb);
    // Each arm launches its form's kernels (none when the rank holds no rows); an arm that cannot run
    // returns its error before it launches anything.  The block restarts at the one exit below.
    if (K >= 16 && d.form >= 6 && d.form <= 19 && d.form != 14 && d.form != 15 && band_in_descriptor(g, rb)) {
        // streamed forms (K >= 16, a band within one 2 GiB buffer descriptor; else form 3)
        if constexpr (K >= 16) {
            if ((d.form == 6 || d.form == 7 || d.form == 10 || d.form == 11 || d.form == 16 ||
                 d.form == 17) && K > 32)
                return hipErrorInvalidValue;
            const size_t dyn = occ > 0 ? occ_lds(occ, kStreamLds) : 0;
            if (g.rows > 0) {
                // forms 6-9: XCD work order by band groups; 10-13: the same with the
                // tile-fastest order; 16-19: XCD work order by tile ranges
                const int order = d.form <= 9 ? 1 : d.form <= 13 ? 0 : 2;
                const int f = d.form <= 9 ? d.form : d.form <= 13 ? d.form - 4 : d.form - 10;
                if (f == 6) {
                    if constexpr (K <= 32) launch_pass_r<NT, K, 2, 2, 4>(g, d, st, rb, dyn, order, s);
                } else if (f == 7) {
                    if constexpr (K <= 32) launch_pass_r<NT, K, 2, 2, 2>(g, d, st, rb, dyn, order, s);
                } else if (f == 8) {
                    launch_pass_r<NT, K, 1, 4, 4>(g, d, st, rb, dyn, order, s);
                } else {
                    launch_pass_r<NT, K, 1, 4, 2>(g, d, st, rb, dyn, order, s);
                }
            }
        }
    } else if (d.form == 22 && K == 64 && d.K == 64 && d.ldc == 64 && rb <= 1024) {
        // MFMA pass (K = 64 blocks; 128-column workgroups)
        if constexpr (K == 64) {
            const size_t dyn = occ > 0 ? occ_lds(occ, kMfmaLds) : 0;
            const dim3 grid((unsigned)((g.width + 127) / 128), nbands);
            if (g.rows > 0) {
                if (bcnt && band_in_descriptor(g, rb))
                    pass_m_kernel<NT, 2, true><<<grid, 256, dyn, s>>>(g.T, To, g.ld, g.rows, g.width, bd, d.C,
                                                                      d.ldc, d.P, d.nzc, rb, bcnt);
                else
                    pass_m_kernel<NT, 2><<<grid, 256, dyn, s>>>(g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc,
                                                                 d.P, d.nzc, rb);
            }
        }
    } else if (d.form == 21 && K == 64 && d.K == 64 && d.ldc == 64 && band_in_descriptor(g, rb) &&
               (int64_t)rb * d.ldc * 8 < ((int64_t)1 << 31)) {
        // (d.K == 64 exactly: the kernel addresses C with 64 steps per row, ldc == 64)
        // DPP-coefficient pass (K = 64 blocks; 1 double per lane: 256-column tiles)
        if constexpr (K == 64) {
            const size_t dyn = occ > 0 ? occ_lds(occ, kClsLds) : pass_lds_env();
            const dim3 grid((unsigned)((g.width + 255) / 256), nbands);
            if (g.rows > 0) {
                if (bcnt)
                    pass_d_kernel<NT, true><<<grid, 256, dyn, s>>>(g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc,
                                                                   d.P, d.nzc, rb, bcnt);
                else
                    pass_d_kernel<NT><<<grid, 256, dyn, s>>>(g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc, d.P,
                                                             d.nzc, rb);
            }
        }
    } else if (K == 64 && pass_q_runs(g, d, rb)) {
        // LDS-ring DPP pass (K = 64 blocks; 256-column tiles): U rows per group, D groups in
        // flight per wave: at U = 2, D = 4, 32 KiB of ring + 4 KiB of row classes per workgroup, so
        // three pass workgroups leave the lookahead chain's LDS free on a CU
        if constexpr (K == 64) {
            // ring depth D: 4 groups in flight (DLP_Q_DEPTH = 2 or 3: tuning only)
            static const int qd = env_int("DLP_Q_DEPTH", 4);
            // rows per group: 4 (twice the independent fma chains per wave, 2 or 3 groups in flight)
            // from 16,384 rows, else 2 (alternating pairs, profiles/r06w/: C3 pass 4.455-4.458 vs
            // 4.519-4.523 ms, 13,951-13,956 vs 13,753-13,755 pivots/s; c3r2 equal; c3r4's pass 2%
            // slower with U = 4); DLP_Q_U = 2 / 4 overrides
            static const int qu_env = env_int("DLP_Q_U", 0);
            // groups holding dense pivot rows stay on the DPP chain (DLP_PASS_PIVG=0: the row-by-row replay)
            static const int pivg = env_int("DLP_PASS_PIVG", 1);
            const bool sad = pass_saddr_env();
            const int U = qu_env == 2 || qu_env == 4 ? qu_env : (g.rows >= 16384 ? 4 : 2);
            const int D = U == 4 ? (qd == 3 ? 3 : 2) : (qd == 2 || qd == 3 || qd == 6 || qd == 8 ? qd : 4);
            // the shared coefficient ring: where DLP_PASS_CSHARE or the shipped choice asks for it
            const int cse = pass_cshare_env();
            const bool csh = sad && pass_q_shared_exists(U, D) && (cse >= 0 ? cse != 0 : pass_cshare_default(U));
            size_t dyn = std::max(pass_q_lds(U, D, csh), pass_lds_env());
            if (occ > 0) dyn = std::max(dyn, occ_lds(occ, kClsLds));
            const dim3 grid((unsigned)((g.width + 255) / 256), nbands);
            if (g.rows <= 0)
                ;
            else if (U == 4 && D == 3)
                launch_pass_q<NT, 4, 3>(g, d, bd, To, rb, bcnt, sad, csh, pivg, grid, dyn, s);
            else if (U == 4)
                launch_pass_q<NT, 4, 2>(g, d, bd, To, rb, bcnt, sad, csh, pivg, grid, dyn, s);
            else if (D == 2)
                launch_pass_q<NT, 2, 2>(g, d, bd, To, rb, bcnt, sad, csh, pivg, grid, dyn, s);
            else if (D == 3)
                launch_pass_q<NT, 2, 3>(g, d, bd, To, rb, bcnt, sad, csh, pivg, grid, dyn, s);
            else if (D == 6)
                launch_pass_q<NT, 2, 6>(g, d, bd, To, rb, bcnt, sad, csh, pivg, grid, dyn, s);
            else if (D == 8)
                launch_pass_q<NT, 2, 8>(g, d, bd, To, rb, bcnt, sad, csh, pivg, grid, dyn, s);
            else
                launch_pass_q<NT, 2, 4>(g, d, bd, To, rb, bcnt, sad, csh, pivg, grid, dyn, s);
        }
    } else {
        // streamed forms need K >= 16 (an even number of coefficient chunks): form 3 below
        const int form = (d.form >= 6 && d.form != 14 && d.form != 15 && d.form != 20) ? 3 : d.form;
        const int cols = (form == 0 || form == 4 || form >= 14) ? kDeferTile : 256;
        const int ntiles = (int)((g.width + cols - 1) / cols);
        const int64_t bands = (g.rows + rb - 1) / rb;
        size_t dyn = form >= 3 ? 0 : (size_t)K * rb * sizeof(double) + (size_t)rb * sizeof(int32_t);
        if (dyn > 160 * 1024) return hipErrorInvalidValue;
        // the kernel's static LDS: cls[1024] (forms 3-5), s_pl[K] (forms 0-2)
        if (occ > 0)
            dyn = std::max(dyn, occ_lds(occ, form >= 14 ? kStreamLds : form >= 3 ? kClsLds : K * sizeof(int32_t)));
        const dim3 grid(ntiles, (unsigned)bands);
        // the session's K is this template's: partial blocks run the full-block instance (their
        // unused steps were zeroed at block start), one launch per pass
        const int tails = d.K == K ? 1 : 0;
        if (g.rows > 0) {
            if (form == 0) {
                if constexpr (K <= 32)   // 2 doubles per lane: P[0..K) in 4K VGPRs
                    pass_kernel<NT, K><<<grid, 256, dyn, s>>>(g.T, g.ld, g.rows, g.width, st, d.C,
                                                              d.ldc, d.P, rb);
                else
                    return hipErrorInvalidValue;
            } else if (form == 3) {
                pass_s_kernel<NT, K, 1, 4, false><<<grid, 256, dyn, s>>>(g.T, To, g.ld, g.rows, g.width, bd,
                                                                         d.C, d.ldc, d.P, d.nzc, rb, tails);
                if (!tails)
                    pass_s_kernel<NT, K, 1, 4, true><<<grid, 256, dyn, s>>>(g.T, To, g.ld, g.rows, g.width, bd,
                                                                            d.C, d.ldc, d.P, d.nzc, rb, 0);
            } else if (form == 20) {
                if constexpr (K <= 32) {
                    pass_s_kernel<NT, K, 2, 2, false, true><<<grid, 256, dyn, s>>>(
                        g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc, d.P, d.nzc, rb, tails);
                    if (!tails)
                        pass_s_kernel<NT, K, 2, 2, true><<<grid, 256, dyn, s>>>(
                            g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc, d.P, d.nzc, rb, 0);
                } else
                    return hipErrorInvalidValue;
            } else if (form == 4 || form == 14 || form == 15) {
                if constexpr (K <= 32) {
                    // form 14 keeps its streamed partial-block kernel, form 15 (the 3-waves build,
                    // which spills) its partial-block instance: its full-block build ran a partial
                    // C3-geometry block with a wrong tableau (tests/test_gpu_defer.py)
                    const int tl = (form == 14 || form == 15) ? 0 : tails;
                    if (form == 15)
                        pass_s3_kernel<NT, K, 2, 2, false><<<grid, 256, dyn, s>>>(
                            g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc, d.P, d.nzc, rb, tl);
                    else
                        pass_s_kernel<NT, K, 2, 2, false><<<grid, 256, dyn, s>>>(
                            g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc, d.P, d.nzc, rb, tl);
                    if (form >= 14 && K >= 16 && band_in_descriptor(g, rb)) {
                        // partial block through the streamed kernel's partial instance
                        const int nb = (int)bands;
                        if constexpr (K >= 16)
                            pass_r_kernel<NT, K, 2, 2, 4, true><<<dim3((unsigned)(ntiles * bands)), 256, dyn, s>>>(
                                g.T, g.ld, g.rows, g.width, st, d.C, d.ldc, d.P, d.nzc, rb, ntiles, nb, 0);
                    } else if (!tl) {
                        pass_s_kernel<NT, K, 2, 2, true><<<grid, 256, dyn, s>>>(
                            g.T, To, g.ld, g.rows, g.width, bd, d.C, d.ldc, d.P, d.nzc, rb, 0);
                    }
                } else
                    return hipErrorInvalidValue;
            } else if (form == 5) {
                pass_s_kernel<NT, K, 1, 8, false><<<grid, 256, dyn, s>>>(g.T, To, g.ld, g.rows, g.width, bd,
                                                                         d.C, d.ldc, d.P, d.nzc, rb, tails);
                if (!tails)
                    pass_s_kernel<NT, K, 1, 8, true><<<grid, 256, dyn, s>>>(g.T, To, g.ld, g.rows, g.width, bd,
                                                                            d.C, d.ldc, d.P, d.nzc, rb, 0);
            }
            else if (form == 1)
                pass1_kernel<NT, K, 2><<<grid, 256, dyn, s>>>(g.T, g.ld, g.rows, g.width, st, d.C,
                                                              d.ldc, d.P, rb);
            else
                pass1_kernel<NT, K, 4><<<grid, 256, dyn, s>>>(g.T, g.ld, g.rows, g.width, st, d.C,
                                                              d.ldc, d.P, rb);
        }
    }
    if (seal < 0) blk_reset_kernel<<<1, 64, 0, s>>>(st);
    return hipGetLastError();
}

template <bool NT>
static hipError_t pass_k(const Geometry& g, const Defer& d, DevState* st, int rb, int occ,
                         hipStream_t s, double* Tout, int seal, uint32_t* bcnt) {
    if (d.K <= 4) return pass<NT, 4>(g, d, st, rb, occ, s, Tout, seal, nullptr);
    if (d.K <= 8) return pass<NT, 8>(g, d, st, rb, occ, s, Tout, seal, nullptr);
    if (d.K <= 16) return pass<NT, 16>(g, d, st, rb, occ, s, Tout, seal, nullptr);
    if (d.K <= 32) return pass<NT, 32>(g, d, st, rb, occ, s, Tout, seal, nullptr);
    return pass<NT, 64>(g, d, st, rb, occ, s, Tout, seal, bcnt);
}

bool lookahead_form(int form) {
    return form == 3 || form == 4 || form == 5 || form == 20 || form == 21 || form == 22 || form == 23;
}

// pass workgroups per band of a publishing form: 256-column tiles (21, 23), 128 (22)
int band_pub_tiles(int form, int64_t width) {
    return (int)(form == 22 ? (width + 127) / 128 : (width + 255) / 256);
}
bool band_pub_ok(const BandPub& bp, const Geometry& g, const Defer& d, int rb) {
    return (d.form == 21 || d.form == 22 || d.form == 23) && d.K == 64 && d.ldc == 64 && rb == bp.rb &&
           (g.rows + rb - 1) / rb <= bp.stride && band_pub_tiles(d.form, g.width) == bp.ntiles &&
           (int64_t)rb * g.ld * 8 < ((int64_t)1 << 31);
}

hipError_t launch_flush_defer(const Geometry& g, const Defer& d, DevState* st, bool nontemporal,
                              int rows_per_block, int occupancy, hipStream_t s, double* Tout,
                              int seal, const BandPub* bp) {
    if (d.K < 1 || d.K > kMaxDefer || rows_per_block < 1 || rows_per_block > 1024 || seal > 1)
        return hipErrorInvalidValue;
    // band publication: lookahead passes of forms 21-23 (band_pub_ok), counted per seal slot
    uint32_t* bcnt = nullptr;
    if (bp && bp->cnt && seal >= 0 && Tout && Tout != g.T && band_pub_ok(*bp, g, d, rows_per_block))
        bcnt = bp->cnt + seal * bp->stride;
    // (a sealed block's failed step was dropped by its seal: launch_seal_defer)
    if (seal < 0 && g.rows > 0 && d.C && d.nzc) {
        drop_failed_step_kernel<<<(unsigned)((g.rows + 256) / 256), 256, 0, s>>>(st, &st->blk, d.C, d.ldc, d.nzc,
                                                                                g.rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (g.cd.on) {
        const hipError_t e = launch_reset_cols(g, st, seal, s);
        if (e != hipSuccess) return e;
    }
    return nontemporal ? pass_k<true>(g, d, st, rows_per_block, occupancy, s, Tout, seal, bcnt)
                       : pass_k<false>(g, d, st, rows_per_block, occupancy, s, Tout, seal, bcnt);
}

hipError_t launch_reset_cols(const Geometry& g, const DevState* st, int seal, hipStream_t s) {
    if (!g.cd.on || g.rows <= 0) return hipSuccess;
    const int32_t* blkp = seal >= 0 ? &st->seal[seal].blk : &st->blk;
    const int32_t* pl = seal >= 0 ? st->seal[seal].pl : st->pl;
    const int32_t* qs = seal >= 0 ? st->seal[seal].qs : st->qs;
    reset_cols_kernel<<<(unsigned)((g.rows + 255) / 256), 256, 0, s>>>(g.T, g.ld, g.rows, blkp, pl, qs);
    return hipGetLastError();
}

hipError_t launch_seal_defer(const Geometry& g, const Defer& d, DevState* st, int slot, hipStream_t s,
                             const BandPub* bp) {
    if (slot < 0 || slot > 1) return hipErrorInvalidValue;
    const bool drop = g.rows > 0 && d.C && d.nzc;   // (launch_flush_defer's condition for the in-place path)
    seal_kernel<<<1, 64, 0, s>>>(st, slot, bp && bp->cnt ? bp->cnt + slot * bp->stride : nullptr,
                                 bp ? bp->stride : 0, drop ? d.C : nullptr, d.ldc, drop ? d.nzc : nullptr, g.rows);
    return hipGetLastError();
}

}  // namespace dlp
