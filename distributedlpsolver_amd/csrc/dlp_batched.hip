// dlp_batched.hip — C5: thousands of independent small LPs, one workgroup per
// LP, the tableau's nonbasic columns + RHS resident in LDS ((m+1) x (n+1) fp64:
// 65 x 129 x 8 B = 67 KB at 64 x 128, two workgroups per CU of 160 KB; 34 KB at
// 64 x 64, four).  HBM is touched once per LP (load the generated tableau,
// store the outputs); every pivot is LDS traffic plus workgroup barriers
// (SURVEY.md §8a row a6).
//
// Pivot rule and arithmetic are exactly the big-tableau path's (dlp.h header):
// Dantzig/Bland pricing with index ties, ratio test with basis-index ties,
// IEEE division for the pivot row, fma elimination, colq == 0 rows untouched.
// Reference analog: the per-impression subproblems solved independently in
// GlobalProblem::ConstructPrimal, R/global_problem.cpp:270-274.
// A dlp_batch keeps every LP's final state in HBM between calls and continues from it after new
// objectives (the resident source and the keep switch below).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "dlp_host.h"
#include "dlp_internal.h"

namespace dlp {
namespace {

__device__ inline uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__device__ inline uint64_t skey(uint64_t seed, uint64_t s) {
    return mix64(seed ^ (0x9E3779B97F4A7C15ULL * (s + 1)));
}
__device__ inline double u01(uint64_t key, uint64_t idx) {
    return (double)(mix64(key + idx) >> 11) * 0x1.0p-53;
}

// Tableaus of the batch in HBM: LP k at T + k*(m+1)*ld, generated with seed+k
// (same spec as generate_rows_kernel: one wave per row, strided fma chains +
// fixed halving tree for b).  blockIdx.y = LP, waves of blockIdx.x = rows.
__global__ __launch_bounds__(256) void batched_generate_kernel(double* __restrict__ T, int64_t ld,
                                                               int64_t m, int64_t n, int kind,
                                                               uint64_t seed) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t sk = seed + blockIdx.y;
    double* base = T + (int64_t)blockIdx.y * (m + 1) * ld;
    const int64_t N = n + m;
    if (i < m) {
        const uint64_t kA = skey(sk, 1), kX = skey(sk, 2), kU = skey(sk, 3), kD = skey(sk, 5);
        double* r = base + i * ld;
        // degenerate family: ~50% "cone" rows with A in [-1,1) and b = 0
        const bool cone = kind == DLP_GEN_DEGENERATE && (mix64(kD + (uint64_t)i) >> 63) == 0;
        double acc = 0.0;
        for (int64_t j = lane; j < n; j += 64) {
            const double u = u01(kA, (uint64_t)(i * n + j));
            const double a = cone ? 2.0 * u - 1.0 : u;
            r[j] = a;
            acc = __builtin_fma(a, u01(kX, (uint64_t)j), acc);
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) acc = acc + __shfl_down(acc, w);
        double bi = __shfl(acc, 0) + u01(kU, (uint64_t)i);
        if (cone) bi = 0.0;
        for (int64_t j = n + lane; j < ld; j += 64) r[j] = (j == n + i) ? 1.0 : (j == N ? bi : 0.0);
    } else if (i == m) {
        double* z = base + m * ld;
        const uint64_t kC = skey(sk, 4);
        for (int64_t j = lane; j < ld; j += 64) z[j] = (j < n) ? -u01(kC, (uint64_t)j) : 0.0;
    }
}

struct BatchOut {
    double* objective;
    int32_t* status;
    int64_t* npivots;
    int32_t* basis;
    dlp_pivot* logs;
    int64_t log_cap;
    uint64_t* stamps;   // diagnostics (DLP_BATCH_STAMPS): LP 0's phase clocks, [64 pivots][8]
    double* x;          // [nlp * n], [nlp * m]: the solution vectors (NULL: not written)
    double* y;
};

// Where a batch kernel takes LP k's data from.  GenIn: the generated full-layout tableaus (LP k
// at T + k * (m+1) * ld).  DenseIn: the caller's A_k (m x n row-major, no padding), b_k, c_k at
// strides sA, sb, sc doubles (0: one array shared by every LP), read straight into the
// condensed tableau: slot j of row i is A_k[i][j], the RHS b_k[i], the objective row -c_k[j]
// with value +0 (the single-LP dense fill), and no full-layout copy passes through HBM.
struct GenIn {
    static constexpr bool dense = false, resident = false, keep = false, dual = false, grow = false, widen = false;
    const double* T;
    int64_t ld;
};
struct DenseIn {
    static constexpr bool dense = true, resident = false, keep = false, dual = false, grow = false, widen = false;
    const double *A, *b, *c;
    int64_t sA, sb, sc;
};
// The resident state of a dlp_batch, LP k's record at S + k * state_doubles(m, n):
// the condensed tableau, row i's n slots then its RHS (row stride W = n + 1, the objective row
// last, its RHS entry the objective value), then as int32 var[n] | basis[m] | the Bland flag |
// the status.  Consecutive slots are consecutive doubles: the LDS kernel's slot loops and the
// register kernel's buffer accesses (lane = slot in the vector offset, row in the scalar
// offset) are both coalesced.  (One base pointer: the register kernel carries it through its
// pivot loop in two SGPRs; two pointers were two SGPRs too many and spilled.)
struct BatchState {
    double* S;
};
__host__ __device__ inline int64_t state_doubles(int64_t m, int64_t n) {
    return (m + 1) * (n + 1) + (n + m + 2 + 1) / 2;
}
// DenseKeepIn: DenseIn whose epilogue stores the final state (`keep`; dlp_batch_create_dense).
// ResIn: the resident state itself, continued and stored again (dlp_batch_resolve); with c != NULL
// the prologue first rebuilds LP k's objective row from c + k * sc by the rule of
// dlp_session_set_objective, fused into the one read of the tableau.
struct DenseKeepIn : DenseIn {
    static constexpr bool keep = true;
    BatchState st;
};
struct ResIn {
    static constexpr bool dense = false, resident = true, keep = true, dual = false, grow = false, widen = false;
    BatchState st;
    const double* c;
    int64_t sc;
};
// RhsIn: the resident state continued by the dual simplex after new right-hand sides
// (dlp_batch_resolve_rhs): the prologue rebuilds LP k's RHS column from
// b + k * sb by the fold of dlp.h, then the pivot loop selects the leaving row first.
struct RhsIn {
    static constexpr bool dense = false, resident = true, keep = true, dual = true, grow = false, widen = false;
    BatchState st;
    const double* b;
    int64_t sb;
    double tol_feas;
    double* last;   // [nlp * m]: the b_k each LP's RHS column was last built from (continuation, below)
    static constexpr const double* c = nullptr;   // (no new objective in this call)
    static constexpr int64_t sc = 0;
};
// AddIn: the resident state grown by r constraint rows per LP and continued by the dual simplex
// (dlp_batch_add_rows).  The kernel's m is the grown row count; the prologue reads
// LP k's record of m - r rows at src (row stride W unchanged, the objective row to row m), folds
// the r new rows G_k x <= h_k into the current basis by the row rule of dlp.h and stores the record
// of the grown shape at st.  r == 0: src is st.S itself, nothing is folded, `last` is not touched.
struct AddIn {
    static constexpr bool dense = false, resident = true, keep = true, dual = true, grow = true, widen = false;
    BatchState st;
    const double* src;
    int r;
    const double *G, *h;   // LP k: r x n row-major at G + k * sG, r doubles at h + k * sh
    int64_t sG, sh;
    double tol_feas;
    double* last;    // [nlp * m] of the grown shape, filled with NaN: no finite b_k continues it
    int32_t* flag;   // the smallest LP index with a G_k / h_k entry that is not finite (atomicMin)
    static constexpr const double* c = nullptr;   // (no new objective in this call)
    static constexpr int64_t sc = 0;
};
// ColsIn: the resident state widened by k structural variables per LP and continued by the primal
// simplex (dlp_batch_add_cols).  The kernel's n is the grown column count; the
// prologue reads LP j's record of n - k slots at src (row stride n - k + 1), re-strides it to
// W = n + 1 with the RHS at slot n, renames every variable index >= n - k by + k, gives the new
// variables the slots n - k .. n - 1 and fills them by the column rule of dlp.h from P_j
// (m x k row-major at P + j * sP) and d_j (k doubles at d + j * sd); the record of the grown
// shape is stored at st.  k > 0 always (k == 0 is dlp_batch_resolve); `last` is not touched.
struct ColsIn {
    static constexpr bool dense = false, resident = true, keep = true, dual = false, grow = false, widen = true;
    BatchState st;
    const double* src;
    int k;
    const double *P, *d;
    int64_t sP, sd;
    int32_t* flag;   // the smallest LP index with a P_j / d_j entry that is not finite (atomicMin)
    static constexpr const double* c = nullptr;   // (no new objective in this call)
    static constexpr int64_t sc = 0;
};
// The status word of a record whose dual phase was stopped by the budget: its RHS has negative
// entries, so only dlp_batch_resolve_rhs may continue it.  Reported outwards as DLP_PIVOT_LIMIT.
constexpr int kDualPending = 100;

// acc = acc + (cb * t): two roundings, never contracted (dlp_reopt.hip's fold step)
__device__ __forceinline__ double fold_step(double acc, double cb, double t) {
#pragma clang fp contract(off)
    const double prod = cb * t;
    return acc + prod;
}
// acc = acc - (gb * t): the row rule's step of dlp_batch_add_rows, v_mul_f64 then v_add_f64
__device__ __forceinline__ double unfold_step(double acc, double gb, double t) {
#pragma clang fp contract(off)
    const double prod = gb * t;
    return acc - prod;
}
typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));   // a b64 buffer store's data
__device__ __forceinline__ double mul_rounded(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ bool not_finite(double v) { return !(__builtin_fabs(v) < __builtin_inf()); }

// One workgroup = one LP.  The LDS holds only the NONBASIC columns of the
// tableau (+ the RHS): a basic variable's column is a unit vector, so storing
// it buys nothing, and dropping it takes the 64 x 128 tableau from 100 KB to
// 67 KB (two LPs per CU instead of one) and 64 x 64 from 67 KB to 34 KB.
// LDS image: T[(m+1)][W] with W = n + 1 (slots 0..n-1, RHS at slot n),
// colq[m+1], prow[W], var[n] (the variable in each slot), basis[m], scratch.
//
// Same values as the full tableau: when q enters at slot s_q and l leaves row
// p, slot s_q takes l's column.  In the full tableau that column is e_p (1.0
// exactly at row p, a signed zero elsewhere), so its new entries are
// prow_l = 1.0 / piv at row p and fma(-colq[i], prow_l, 0) elsewhere (or the
// zero, when colq[i] == 0): the same bits as the full update, up to the sign
// of a zero, which reaches no output (every later value that depends on it is
// a fma / division whose result does not).  Pricing runs over the slots with
// the full tableau's order: min z, ties -> smallest VARIABLE index; Bland ->
// the smallest variable index with z < -tol.
template <class In>
__global__ __launch_bounds__(512) void batched_solve_kernel(In in, int m, int n,
                                                            int64_t max_pivots, int pricing,
                                                            double tol_dj, double tol_piv,
                                                            BatchOut out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int N = n + m, W = n + 1;
    double* T = smem;                                   // (m+1) x W
    double* colq = T + (m + 1) * W;                     // m+1
    double* prow = colq + (m + 1);                      // W
    int32_t* var = (int32_t*)(prow + W);                // n
    int32_t* basis = var + n;                           // m
    // scratch: [0] q (variable), [1] slot of q, [2] p, [3] status, [4] bland, [5] dense: some b_i not >= 0
    // (resident: 1 rejected at creation, 2 a c_k / b_k entry that is not finite, 3 DLP_ERR_STATE:
    // a pending dual phase in front of a primal call, or an LP that is not dual feasible in
    // front of a dual one)
    int32_t* sI = basis + m;
    double* sD = (double*)(sI + 6 + ((n + m) & 1));     // piv, ratio (8-B aligned)

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t lp = blockIdx.x;
    // the final state to the batch's resident buffers (In::keep)
    auto store_state = [&](int stt) {
        if constexpr (In::keep) {
            double* __restrict__ dst = in.st.S + lp * state_doubles(m, n);
            int32_t* __restrict__ di = (int32_t*)(dst + (m + 1) * W);
            for (int e = tid; e < (m + 1) * W; e += blockDim.x) dst[e] = T[e];
            for (int s = tid; s < n; s += blockDim.x) di[s] = var[s];
            for (int i = tid; i < m; i += blockDim.x) di[n + i] = basis[i];
            if (tid == 0) {
                di[N] = sI[4];
                di[N + 1] = stt;
            }
            if constexpr (In::grow) {   // no finite b_k matches the grown record: a later resolve_rhs rebuilds
                if (in.r > 0)
                    for (int i = tid; i < m; i += blockDim.x) in.last[lp * m + i] = __builtin_nan("");
            } else if constexpr (In::dual) {   // the b_k this RHS column was built from
                const double* __restrict__ b = in.b + lp * in.sb;
                for (int i = tid; i < m; i += blockDim.x) in.last[lp * m + i] = b[i];
            }
        }
    };
    bool has_c = false;   // (resident) a new objective: the rows are read by the fold below
    if constexpr (In::widen) {
        // The record of n - k slots, re-strided: row i's old slots keep their place, its RHS moves
        // to slot n, every variable index >= n - k (the slacks) goes up by k, the new variables sit
        // nonbasic in the slots n - k .. n - 1 (filled by the column rule after the barrier).
        // sF borrows sD as in the row growth: [0] a P_j / d_j entry that is not finite.
        const int kc = in.k, no = n - kc, Wo = no + 1, No = no + m;
        const double* __restrict__ src = in.src + lp * state_doubles(m, no);
        const int32_t* __restrict__ si = (const int32_t*)(src + (m + 1) * Wo);
        for (int s = tid; s < no; s += blockDim.x) {
            const int v = si[s];
            var[s] = v >= no ? v + kc : v;
        }
        for (int t = tid; t < kc; t += blockDim.x) var[no + t] = no + t;
        for (int i = tid; i < m; i += blockDim.x) {
            const int v = si[no + i];
            basis[i] = v >= no ? v + kc : v;
        }
        for (int e = tid; e < (m + 1) * Wo; e += blockDim.x) {
            const int i = e / Wo, s = e - i * Wo;
            T[i * W + (s < no ? s : n)] = src[e];
        }
        if (tid == 0) {
            // 1: rejected at creation; 3: left infeasible or pending by a dual phase (negative RHS
            // entries: the primal rule must not pivot on it).  Both keep their stored status and
            // Bland state in the widened record; an accepted LP starts over, whatever it was.
            const int sv = si[No + 1];
            const int bad = sv == DLP_ERR_ARG ? 1 : (sv == DLP_INFEASIBLE || sv == kDualPending) ? 3 : 0;
            sI[5] = bad;
            sI[3] = bad ? sv : (int)DLP_RUNNING;
            sI[4] = bad ? si[No] : (pricing == DLP_PRICING_BLAND ? 1 : 0);
            ((int32_t*)sD)[0] = 0;
        }
    } else if constexpr (In::grow) {
        // The record of m - r rows: its constraint rows keep their place (the stride W is the
        // grown shape's too), its objective row moves to row m, the new slacks are basic in
        // their own rows.  sF borrows sD (next written after the pivot loop's first barrier):
        // [0] a G_k / h_k entry that is not finite, [1] a refused LP's new RHS below -tol_feas.
        const int r = in.r, mo = m - r, No = n + mo;
        const double* __restrict__ src = in.src + lp * state_doubles(mo, n);
        const int32_t* __restrict__ si = (const int32_t*)(src + (mo + 1) * W);
        int32_t* sF = (int32_t*)sD;
        for (int s = tid; s < n; s += blockDim.x) var[s] = si[s];
        for (int i = tid; i < mo; i += blockDim.x) basis[i] = si[n + i];
        for (int t = tid; t < r; t += blockDim.x) basis[mo + t] = No + t;
        for (int e = tid; e < mo * W; e += blockDim.x) T[e] = src[e];
        for (int s = tid; s < W; s += blockDim.x) T[m * W + s] = src[mo * W + s];
        if (wid == 0) {
            // 1: rejected at creation; 3: some stored slot has z < -tol_dj (not dual feasible)
            const int sv = si[No + 1];
            int bad = sv == DLP_ERR_ARG ? 1 : 0;
            bool neg = false;
            for (int s = lane; s < n; s += 64) neg |= src[mo * W + s] < -tol_dj;
            if (__ballot(neg) != 0 && bad == 0) bad = 3;
            if (lane == 0) {
                // r == 0 continues a pending dual phase with its Bland state; a refused LP keeps
                // its stored status and Bland state in the grown record
                const bool cont = r == 0 && sv == kDualPending;
                sI[5] = bad;
                sI[3] = bad ? sv : (int)DLP_RUNNING;
                sI[4] = bad ? si[No] : ((cont && si[No]) || pricing == DLP_PRICING_BLAND ? 1 : 0);
                sF[0] = 0;
                sF[1] = 0;
            }
        }
    } else if constexpr (In::resident) {
        const double* __restrict__ src = in.st.S + lp * state_doubles(m, n);
        const int32_t* __restrict__ si = (const int32_t*)(src + (m + 1) * W);
        has_c = !In::dual && in.c != nullptr;
        for (int s = tid; s < n; s += blockDim.x) var[s] = si[s];
        for (int i = tid; i < m; i += blockDim.x) basis[i] = si[n + i];
        if (!has_c)
            for (int e = tid; e < (m + 1) * W; e += blockDim.x) T[e] = src[e];
        if (wid == 0) {
            // 1: rejected at creation; 2: a c_k entry that is not finite (this call only)
            int bad = si[N + 1] == DLP_ERR_ARG ? 1 : 0;
            if (has_c) {
                const double* __restrict__ c = in.c + lp * in.sc;
                bool nf = false;
                for (int j = lane; j < n; j += 64) nf |= not_finite(c[j]);
                if (__ballot(nf) != 0 && bad == 0) bad = 2;
                // cB_i, staged where the entering column will live
                for (int i = lane; i < m; i += 64) {
                    const int bv = si[n + i];
                    colq[i] = bv < n ? c[bv] : 0.0;
                }
            }
            if constexpr (In::dual) {
                // 2: a b_k entry that is not finite; 3: some stored slot has z < -tol_dj (the LP
                // is not dual feasible: stopped inside a primal solve, or unbounded)
                const double* __restrict__ b = in.b + lp * in.sb;
                bool nf = false, neg = false;
                for (int i = lane; i < m; i += 64) nf |= not_finite(b[i]);
                for (int s = lane; s < n; s += 64) neg |= src[m * W + s] < -tol_dj;
                if (__ballot(nf) != 0 && bad == 0) bad = 2;
                if (__ballot(neg) != 0 && bad == 0) bad = 3;
                // continuation: a pending dual phase handed the very b_k (bit for bit) it was
                // stopped with goes on from its RHS column and Bland state as they stand, so that
                // budgets of any size give the pivots of one unbounded call
                bool cont = si[N + 1] == kDualPending;
                if (cont) {
                    const double* __restrict__ last = in.last + lp * m;
                    bool diff = false;
                    for (int i = lane; i < m; i += 64)
                        diff |= __builtin_bit_cast(uint64_t, b[i]) != __builtin_bit_cast(uint64_t, last[i]);
                    cont = __ballot(diff) == 0;
                }
                if (lane == 0) sI[0] = cont ? 1 : 0;
            } else {
                // 3: left infeasible or pending by a dual phase (negative RHS entries: the primal
                // rule must not pivot on it)
                const int sv = si[N + 1];
                if (bad == 0 && (sv == DLP_INFEASIBLE || sv == kDualPending)) bad = 3;
            }
            if (lane == 0) {
                const bool fresh = has_c || In::dual;   // the status and the Bland state start over
                sI[5] = bad;
                sI[3] = fresh ? (int)DLP_RUNNING : si[N + 1];
                sI[4] = fresh ? (pricing == DLP_PRICING_BLAND ? 1 : 0) : si[N];
                if constexpr (In::dual)
                    if (sI[0] && si[N]) sI[4] = 1;   // (continued: the Bland state as it was left)
            }
        }
    } else if constexpr (!In::dense) {
        const double* __restrict__ src = in.T + lp * (m + 1) * in.ld;
        for (int i = 0; i <= m; ++i)
            for (int s = tid; s < W; s += blockDim.x) T[i * W + s] = src[(int64_t)i * in.ld + (s < n ? s : N)];
    } else {
        const double* __restrict__ A = in.A + lp * in.sA;
        const double* __restrict__ b = in.b + lp * in.sb;
        const double* __restrict__ c = in.c + lp * in.sc;
        for (int i = 0; i < m; ++i)
            for (int s = tid; s < W; s += blockDim.x) T[i * W + s] = s < n ? A[(int64_t)i * n + s] : b[i];
        for (int s = tid; s < W; s += blockDim.x) T[m * W + s] = s < n ? -c[s] : 0.0;
        if (wid == 0) {   // an LP with a negative or NaN b_i is rejected, not solved
            bool bad = false;
            for (int i = lane; i < m; i += 64) bad |= !(b[i] >= 0.0);
            const uint64_t anyb = __ballot(bad);
            if (lane == 0) sI[5] = anyb != 0 ? 1 : 0;
        }
    }
    if constexpr (!In::resident) {
        for (int s = tid; s < n; s += blockDim.x) var[s] = s;
        for (int i = tid; i < m; i += blockDim.x) basis[i] = n + i;
        if (tid == 0) {
            sI[3] = DLP_RUNNING;
            sI[4] = pricing == DLP_PRICING_BLAND ? 1 : 0;
        }
    }
    __syncthreads();
    if constexpr (In::widen) {
        // The column rule (dlp.h, dlp_batch_add_cols): new variable t's column in the current basis
        // is B^-1 p, B^-1 the slack columns of the full layout, so entry r is the fold of
        // Tfull[r][slack l] * p_l over l ascending from +0.0, the product rounded, then the sum; the
        // objective row's entry less d_t.  inv[l] is dlp_batch_resolve_rhs's map (>= 0 slack l's
        // slot, else -(row + 1) of the row it is basic in: that row's unit vector, every other
        // entry a zero that changes no bit and is skipped) and borrows the entering column's
        // place.  One work item owns one row of one new column and reads only old slots; it holds
        // for any basis, so rejected and refused LPs take it too.
        const int kc = in.k, no = n - kc;
        const double* __restrict__ P = in.P + lp * in.sP;
        const double* __restrict__ d = in.d + lp * in.sd;
        int32_t* sF = (int32_t*)sD;
        int32_t* inv = (int32_t*)colq;
        bool nf = false;
        for (int e = tid; e < m * kc; e += blockDim.x) nf |= not_finite(P[e]);
        for (int t = tid; t < kc; t += blockDim.x) nf |= not_finite(d[t]);
        if (__ballot(nf) != 0 && lane == 0) {
            atomicMin(in.flag, (int32_t)lp);
            sF[0] = 1;
        }
        for (int s = tid; s < no; s += blockDim.x)
            if (var[s] >= n) inv[var[s] - n] = s;
        for (int i = tid; i < m; i += blockDim.x)
            if (basis[i] >= n) inv[basis[i] - n] = -(i + 1);
        __syncthreads();
        for (int item = tid; item < (m + 1) * kc; item += blockDim.x) {
            const int t = item / (m + 1), r = item - t * (m + 1);
            double acc = 0.0;
            for (int l0 = 0; l0 < m; l0 += 8) {   // loads first, then the dependent chain
                double cf[8], pl[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int l = min(l0 + u, m - 1);
                    const int iv = inv[l];
                    pl[u] = P[(int64_t)l * kc + t];
                    cf[u] = iv >= 0 ? T[r * W + iv] : (iv == -(r + 1) ? 1.0 : 0.0);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (l0 + u < m && cf[u] != 0.0) acc = fold_step(acc, cf[u], pl[u]);
            }
            if (r == m) acc = acc - d[t];
            T[r * W + no + t] = acc;
        }
        __syncthreads();
        if (sF[0]) return;   // (uniform) the call fails as a whole: nothing of it is kept
    }
    if constexpr (In::grow) {
        if (in.r > 0) {
            // The row rule (dlp.h, dlp_batch_add_rows): new row t in the current basis is
            // g - sum_i gB_i * T[i] over the old rows ascending, gB_i = g[basis[i]] (a slack: +0.0),
            // rows with gB_i == 0.0 skipped, the product rounded, then the difference.  One work
            // item owns one slot of one new row; gB is staged where the entering column and the
            // pivot row will live, as many new rows at a time as fit there.  It holds for any
            // basis, so rejected and refused LPs take it too.
            const int r = in.r, mo = m - r;
            const double* __restrict__ G = in.G + lp * in.sG;
            const double* __restrict__ h = in.h + lp * in.sh;
            int32_t* sF = (int32_t*)sD;
            bool nf = false;
            for (int e = tid; e < r * n; e += blockDim.x) nf |= not_finite(G[e]);
            for (int t = tid; t < r; t += blockDim.x) nf |= not_finite(h[t]);
            if (__ballot(nf) != 0 && lane == 0) {
                atomicMin(in.flag, (int32_t)lp);
                sF[0] = 1;
            }
            double* gB = colq;
            const int ch = min(r, (m + 1 + W) / mo);   // >= 1: m + 1 > mo
            for (int t0 = 0; t0 < r; t0 += ch) {
                const int tc = min(ch, r - t0);
                for (int e = tid; e < tc * mo; e += blockDim.x) {
                    const int t = e / mo, i = e - t * mo;
                    const int bv = basis[i];
                    gB[e] = bv < n ? G[(int64_t)(t0 + t) * n + bv] : 0.0;
                }
                __syncthreads();
                for (int item = tid; item < tc * W; item += blockDim.x) {
                    const int t = item / W, s = item - t * W;
                    const double* gb = gB + t * mo;
                    double acc = 0.0;
                    if (s == n) acc = h[t0 + t];
                    else if (var[s] < n) acc = G[(int64_t)(t0 + t) * n + var[s]];
                    for (int i0 = 0; i0 < mo; i0 += 8) {   // loads first, then the dependent chain
                        double tt[8], f[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int i = min(i0 + u, mo - 1);
                            f[u] = gb[i];
                            tt[u] = T[i * W + s];
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (i0 + u < mo && f[u] != 0.0) acc = unfold_step(acc, f[u], tt[u]);
                    }
                    T[(mo + t0 + t) * W + s] = acc;
                }
                __syncthreads();
            }
            if (sI[5] == 3) {   // (uniform) refused: does a new row make the record primal infeasible?
                for (int t = tid; t < r; t += blockDim.x)
                    if (T[(mo + t) * W + n] < -in.tol_feas) sF[1] = 1;
                __syncthreads();
            }
            if (sF[0]) return;   // (uniform) the call fails as a whole: nothing of it is kept
        }
    }
    if constexpr (In::dense || In::resident) {
        if (sI[5]) {   // (uniform) DLP_ERR_ARG, no pivots, the slack basis, NaN values
            const double nan = __builtin_nan("");
            const bool resident_basis = In::resident && sI[5] >= 2;   // refused for this call: the basis as it stands
            const int err = In::resident && sI[5] == 3 ? DLP_ERR_STATE : DLP_ERR_ARG;
            if (tid == 0) {
                if (out.status) out.status[lp] = err;
                if (out.npivots) out.npivots[lp] = 0;
                if (out.objective) out.objective[lp] = nan;
            }
            if (out.basis)
                for (int i = tid; i < m; i += blockDim.x) out.basis[lp * m + i] = resident_basis ? basis[i] : n + i;
            if (out.x)
                for (int j = tid; j < n; j += blockDim.x) out.x[lp * n + j] = nan;
            if (out.y)
                for (int i = tid; i < m; i += blockDim.x) out.y[lp * m + i] = nan;
            // a fresh batch keeps the rejected LP as loaded, marked DLP_ERR_ARG; a resident one
            // is left exactly as it was
            if constexpr (!In::resident) store_state(DLP_ERR_ARG);
            // a grown one takes the LP's record of the new shape: its stored status and Bland state
            // (sI[3], sI[4]), or pending when a new row has made it primal infeasible as well
            if constexpr (In::grow)
                if (in.r > 0) store_state(sI[5] == 3 && ((const int32_t*)sD)[1] ? kDualPending : sI[3]);
            // (a widened one too: a shape change is all or nothing)
            if constexpr (In::widen) store_state(sI[3]);
            return;
        }
    }
    if constexpr (In::resident) {
        if (has_c) {
            // The objective rebuild fused into the load (dlp.h, dlp_session_set_objective's rule):
            // a slot loop owns a column, copies its m constraint entries from the state into the
            // LDS and folds them in row order, 8 loads requested ahead of the 8 dependent adds.
            const double* __restrict__ src = in.st.S + lp * state_doubles(m, n);
            const double* __restrict__ c = in.c + lp * in.sc;
            for (int s = tid; s < W; s += blockDim.x) {
                double acc = 0.0;
                if (s < n && var[s] < n) acc = -c[var[s]];
                for (int i0 = 0; i0 < m; i0 += 8) {
                    double t[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) t[u] = src[(int64_t)min(i0 + u, m - 1) * W + s];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + u;
                        if (i < m) {
                            T[i * W + s] = t[u];
                            const double cb = colq[i];
                            if (cb != 0.0) acc = fold_step(acc, cb, t[u]);
                        }
                    }
                }
                T[m * W + s] = acc;
            }
            __syncthreads();
        }
    }
    if constexpr (In::dual && !In::grow) if (sI[0] == 0) {   // (uniform; sI[0] is next written after the pivot loop's first barrier)
        // The RHS rebuild (dlp.h, dlp_batch_resolve_rhs's rule): the slack columns of the full
        // layout are B^-1, so row r's new RHS is the fold of Tfull[r][n + l] * b_l over l
        // ascending, one thread per row (the objective row included: its entry is the new
        // objective value).  inv[l] says where slack l lives: >= 0 its slot, else -(row + 1) of
        // the row it is basic in, whose column is that row's unit vector (objective entry +0.0:
        // a term that cannot change a bit, so it is left out).  inv borrows the entering
        // column's place, b_l is one uniform load per step.
        int32_t* inv = (int32_t*)colq;
        const double* __restrict__ b = in.b + lp * in.sb;
        for (int s = tid; s < n; s += blockDim.x)
            if (var[s] >= n) inv[var[s] - n] = s;
        for (int i = tid; i < m; i += blockDim.x)
            if (basis[i] >= n) inv[basis[i] - n] = -(i + 1);
        __syncthreads();
        for (int r = tid; r <= m; r += blockDim.x) {
            double acc = 0.0;
            for (int l = 0; l < m; ++l) {
                const int iv = inv[l];
                if (iv >= 0) acc = fold_step(acc, T[r * W + iv], b[l]);
                else if (iv == -(r + 1)) acc = fold_step(acc, 1.0, b[l]);
            }
            T[r * W + n] = acc;
        }
        __syncthreads();
    }

    int64_t k = 0;
    if constexpr (In::resident && !In::dual) {
        // resumed without a new objective: an optimal or unbounded LP does no pivot
        if (sI[3] == DLP_OK || sI[3] == DLP_UNBOUNDED) max_pivots = 0;
    }
    int q = -1, sq = -1, p = -1;
    for (; In::dual || k < max_pivots; ++k) {
      if constexpr (In::dual) {
        // ---- d1 leaving row (wave 0): the most negative RHS below -tol_feas, ties -> the smallest
        // basic VARIABLE; Bland -> the eligible row with the smallest basic variable
        if (wid == 0) {
            double rmin = __builtin_inf();
            int bmin = kNoIndex, imin = -1, bb = kNoIndex, ib = -1;
            for (int i = lane; i < m; i += 64) {
                const double v = T[i * W + n];
                const int bv = basis[i];
                if (v < -in.tol_feas) {
                    if (v < rmin || (v == rmin && bv < bmin)) { rmin = v; bmin = bv; imin = i; }
                    if (bv < bb) { bb = bv; ib = i; }
                }
            }
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) {
                const double orr = __shfl_xor(rmin, sh);
                const int obm = __shfl_xor(bmin, sh), oim = __shfl_xor(imin, sh);
                const int obb = __shfl_xor(bb, sh), oib = __shfl_xor(ib, sh);
                if (orr < rmin || (orr == rmin && obm < bmin)) { rmin = orr; bmin = obm; imin = oim; }
                if (obb < bb) { bb = obb; ib = oib; }
            }
            if (lane == 0) sI[2] = sI[4] ? ib : imin;
        }
        __syncthreads();
        p = sI[2];
        if (p < 0) {   // primal feasible too: optimal (tested before the budget)
            if (tid == 0) sI[3] = DLP_OK;
            break;
        }
        if (k >= max_pivots) break;
        // ---- d2 entering slot (wave 0): min over a = T[p][s] < -tol_piv of max(z_s, 0) / -a,
        // ties -> the smallest variable; then select + log as the primal's a4
        if (wid == 0) {
            double rbest = __builtin_inf(), abest = 0.0;
            int vbest = kNoIndex, sbest = -1;
            const double* z = T + m * W;
            const double* rowp = T + p * W;
            for (int s = lane; s < n; s += 64) {
                const double a = rowp[s];
                if (a < -tol_piv) {
                    double zz = z[s];
                    if (!(zz > 0.0)) zz = 0.0;
                    const double r = zz / (-a);
                    const int vr = var[s];
                    if (r < rbest || (r == rbest && vr < vbest)) { rbest = r; vbest = vr; sbest = s; abest = a; }
                }
            }
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) {
                const double orr = __shfl_xor(rbest, sh), oa = __shfl_xor(abest, sh);
                const int ov = __shfl_xor(vbest, sh), os = __shfl_xor(sbest, sh);
                if (orr < rbest || (orr == rbest && ov < vbest)) { rbest = orr; vbest = ov; sbest = os; abest = oa; }
            }
            if (lane == 0) {
                sI[1] = sbest;
                if (sbest >= 0) {
                    const int leaving = basis[p];
                    basis[p] = vbest;
                    var[sbest] = leaving;   // the entering slot now holds the leaving variable
                    sI[0] = vbest;
                    sI[4] = (pricing == DLP_PRICING_BLAND) ? 1 : (rbest == 0.0 ? 1 : 0);
                    sD[0] = abest;
                    sD[1] = rbest;
                    if (out.logs && k < out.log_cap) {
                        dlp_pivot e;
                        e.q = vbest; e.p = p; e.leaving = leaving; e.pad = 0;
                        e.ratio = rbest; e.objective = 0.0;
                        out.logs[lp * out.log_cap + k] = e;
                    }
                }
            }
        }
        __syncthreads();
        sq = sI[1];
        if (sq < 0) {   // no entry of row p can take its RHS up: no x satisfies the row
            if (tid == 0) sI[3] = DLP_INFEASIBLE;
            break;
        }
        q = sI[0];
        for (int i = tid; i <= m; i += blockDim.x) colq[i] = T[i * W + sq];
      } else {
        // ---- a1 pricing (wave 0): lexicographic (z, variable) min + first variable < -tol
        if (wid == 0) {
            double zmin = __builtin_inf();
            int vmin = kNoIndex, smin = -1, vb = kNoIndex, sb = -1;
            const double* z = T + m * W;
            for (int s = lane; s < n; s += 64) {
                const double v = z[s];
                const int vr = var[s];
                if (v < zmin || (v == zmin && vr < vmin)) { zmin = v; vmin = vr; smin = s; }
                if (v < -tol_dj && vr < vb) { vb = vr; sb = s; }
            }
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) {
                const double oz = __shfl_xor(zmin, sh);
                const int ov = __shfl_xor(vmin, sh), os = __shfl_xor(smin, sh);
                const int ob = __shfl_xor(vb, sh), osb = __shfl_xor(sb, sh);
                if (oz < zmin || (oz == zmin && ov < vmin)) { zmin = oz; vmin = ov; smin = os; }
                if (ob < vb) { vb = ob; sb = osb; }
            }
            if (lane == 0) {
                int q = kNoIndex, sq = -1;
                if (sI[4]) {
                    q = vb;
                    sq = sb;
                } else if (vmin != kNoIndex && zmin < -tol_dj) {
                    q = vmin;
                    sq = smin;
                }
                sI[0] = (q == kNoIndex) ? -1 : q;
                sI[1] = sq;
            }
        }
        __syncthreads();
        q = sI[0], sq = sI[1];
        if (q < 0) {
            if (tid == 0) sI[3] = DLP_OK;
            break;
        }
        // ---- a2 ratio test (wave 0) + colq capture (all)
        for (int i = tid; i <= m; i += blockDim.x) colq[i] = T[i * W + sq];
        if (wid == 0) {
            Cand best;
            best.valid = 0; best.ratio = 0.0; best.basis_var = kNoIndex; best.row = -1;
            best.pad0 = 0; best.pivot = 0.0;
            for (int i = lane; i < m; i += 64) {
                const double a = T[i * W + sq];
                if (a > tol_piv) {
                    double rhs = T[i * W + n];
                    if (!(rhs > 0.0)) rhs = 0.0;
                    Cand c;
                    c.ratio = rhs / a; c.basis_var = basis[i]; c.row = i; c.valid = 1;
                    c.pad0 = 0; c.pivot = a;
                    if (cand_better(c, best)) best = c;
                }
            }
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) {
                Cand o;
                o.ratio = __shfl_xor(best.ratio, sh);
                o.basis_var = __shfl_xor(best.basis_var, sh);
                o.row = __shfl_xor(best.row, sh);
                o.valid = __shfl_xor(best.valid, sh);
                o.pad0 = 0;
                o.pivot = __shfl_xor(best.pivot, sh);
                if (cand_better(o, best)) best = o;
            }
            if (lane == 0) {
                if (!best.valid) {
                    sI[2] = -1;
                } else {   // a4 select + log
                    const int p = best.row;
                    const int leaving = basis[p];
                    basis[p] = q;
                    var[sq] = leaving;   // the entering slot now holds the leaving variable
                    sI[2] = p;
                    sI[4] = (pricing == DLP_PRICING_BLAND) ? 1 : (best.ratio == 0.0 ? 1 : 0);
                    sD[0] = best.pivot;
                    sD[1] = best.ratio;
                    if (out.logs && k < out.log_cap) {
                        dlp_pivot e;
                        e.q = q; e.p = p; e.leaving = leaving; e.pad = 0;
                        e.ratio = best.ratio; e.objective = 0.0;
                        out.logs[lp * out.log_cap + k] = e;
                    }
                }
            }
        }
        __syncthreads();
        p = sI[2];
        if (p < 0) {
            if (tid == 0) sI[3] = DLP_UNBOUNDED;
            break;
        }
      }
        // ---- a3 pivot row (IEEE division), then the elimination: work items (slot,
        // row group), R row groups so that the lanes share it evenly; rows 8 at a time,
        // loads first
        const double piv = sD[0];
        for (int s = tid; s < W; s += blockDim.x) prow[s] = (s == sq ? 1.0 : T[p * W + s]) / piv;
        __syncthreads();
        {
            // R row groups with W * R <= blockDim.x: no lane takes a second item
            const int R = W >= (int)blockDim.x ? 1 : (int)(blockDim.x / W);
            const int rpg = (m + 1 + R - 1) / R;
            for (int item = tid; item < W * R; item += blockDim.x) {
                const int rg = item / W, s = item - rg * W;
                const bool ent = s == sq;               // slot of q -> column of the leaving var
                const double pj = prow[s];
                const int ib = rg * rpg, ie = min(ib + rpg, m + 1);
                for (int i0 = ib; i0 < ie; i0 += 8) {
                    double t[8], f[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = min(i0 + u, ie - 1);
                        f[u] = colq[i];
                        t[u] = ent ? 0.0 : T[i * W + s];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + u;
                        const double v = __builtin_fma(-f[u], pj, t[u]);
                        const double nv = (i == p) ? pj : (f[u] != 0.0 ? v : t[u]);
                        if (i < ie) T[i * W + s] = nv;
                    }
                }
            }
        }
        __syncthreads();
        if (tid == 0 && out.logs && k < out.log_cap)
            out.logs[lp * out.log_cap + k].objective = T[m * W + n];
    }
    int stt = DLP_RUNNING;   // (thread 0's is the status)
    if (tid == 0) {
        stt = sI[3];
        if (stt == DLP_RUNNING) stt = DLP_PIVOT_LIMIT;
        if (out.status) out.status[lp] = stt;
        if (out.npivots) out.npivots[lp] = k;
        if (out.objective) out.objective[lp] = T[m * W + n];
    }
    // (a dual phase the budget stopped is stored as pending: the primal rule must not continue it)
    store_state(In::dual && stt == DLP_PIVOT_LIMIT ? kDualPending : stt);
    if (out.basis)
        for (int i = tid; i < m; i += blockDim.x) out.basis[lp * m + i] = basis[i];
    // x and y from the tableau as it stands, every index written exactly once (no zero fill):
    // a nonbasic variable by its slot (x_j = 0, y_i = the slack's reduced cost), a basic one by
    // its row (x_j = the row's RHS, y_i = +0)
    if (out.x || out.y) {
        double* x = out.x ? out.x + lp * n : nullptr;
        double* y = out.y ? out.y + lp * m : nullptr;
        for (int s = tid; s < n; s += blockDim.x) {
            const int v = var[s];
            if (v < n) { if (x) x[v] = 0.0; }
            else if (y) y[v - n] = T[m * W + s];
        }
        for (int i = tid; i < m; i += blockDim.x) {
            const int v = basis[i];
            if (v < n) { if (x) x[v] = T[i * W + n]; }
            else if (y) y[v - n] = 0.0;
        }
    }
}

// C5, register-resident (round 3): at m = 64 one LANE owns one slot (column) of the
// nonbasic tableau, all 65 of its rows in 130 VGPRs (rows unrolled: no dynamic register
// index), so the elimination is 65 fmas per lane from registers with the column q read
// from LDS as a broadcast, and the pivot row is computed in place (each lane divides its
// own T[p][s]).  A workgroup of NW = ceil((n + 1) / 64) waves is one LP (192 lanes at
// 64 x 128, 129 of them owning a slot); no LDS holds the tableau, so 3 waves per SIMD fit:
// 4 LPs per CU at 64 x 128 (the LDS kernel: 2), 6 at 64 x 64 (4).  Per pivot: pricing
// (wave shuffles + one LDS partial per wave), the entering column written to LDS by its
// owner lane, the ratio test by wave 0 (one row per lane, which also keeps that row's RHS),
// 3 barriers.
// Same operations on the same values as batched_solve_kernel (same bits).
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a register array indexed
// by I stays in registers (a #pragma unroll of 65 iterations may be left rolled, and the
// array then lives in scratch)
template <typename F, int... I>
__device__ __forceinline__ void each_(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void each(F&& f) {
    each_(f, std::make_integer_sequence<int, N>{});
}

// Wave-wide minimum by DPP (xor 1, xor 2, half-row and row mirrors, then the row broadcasts
// 15 and 31: the full minimum lands in lane 63, read back as a uniform value) — a few cycles
// per step against the LDS round trip of each ds_bpermute a shuffle costs.  No NaN reaches
// them (the callers map NaN to +inf first).
template <int CTRL, int RMASK>
__device__ __forceinline__ double dpp_f64(double v, double id) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v), d = __builtin_bit_cast(uint64_t, id);
    const uint32_t lo = __builtin_amdgcn_update_dpp((int)(uint32_t)d, (int)(uint32_t)u, CTRL, RMASK, 0xf, false);
    const uint32_t hi = __builtin_amdgcn_update_dpp((int)(uint32_t)(d >> 32), (int)(uint32_t)(u >> 32), CTRL, RMASK, 0xf, false);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double wave_min_f64(double v) {
    const double id = __builtin_inf();
    double o;
    o = dpp_f64<0xB1, 0xf>(v, id); v = o < v ? o : v;    // quad_perm [1,0,3,2]
    o = dpp_f64<0x4E, 0xf>(v, id); v = o < v ? o : v;    // quad_perm [2,3,0,1]
    o = dpp_f64<0x141, 0xf>(v, id); v = o < v ? o : v;   // row_half_mirror
    o = dpp_f64<0x140, 0xf>(v, id); v = o < v ? o : v;   // row_mirror
    o = dpp_f64<0x142, 0xa>(v, id); v = o < v ? o : v;   // row_bcast:15
    o = dpp_f64<0x143, 0xc>(v, id); v = o < v ? o : v;   // row_bcast:31
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, 63), hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), 63);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
template <int CTRL, int RMASK>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(kNoIndex, v, CTRL, RMASK, 0xf, false);
}
// lane `l`'s value (l uniform, in an SGPR): two v_readlane_b32
__device__ __forceinline__ double readlane_f64(double v, int l) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)b, l), hi = __builtin_amdgcn_readlane((uint32_t)(b >> 32), l);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int wave_min_i32(int v) {
    v = min(v, dpp_i32<0xB1, 0xf>(v));
    v = min(v, dpp_i32<0x4E, 0xf>(v));
    v = min(v, dpp_i32<0x141, 0xf>(v));
    v = min(v, dpp_i32<0x140, 0xf>(v));
    v = min(v, dpp_i32<0x142, 0xa>(v));
    v = min(v, dpp_i32<0x143, 0xc>(v));
    return __builtin_amdgcn_readlane(v, 63);
}

// Rows of the register-resident elimination in inline asm.  The entering column's entry f
// and the pivot row index are the same for every lane of the LP, so each test is a uniform
// exec mask (all lanes or none) set by SALU, with no branch.  (hipcc, left to itself, turned the 2 x 65 tests into live vector masks
// and spilled them, or moved the register rows to scratch.)
// t := fma(-f, pj, t) unless f == +-0 (the eager rule leaves the row untouched).
// 8 rows, their masks from zm (bit r set: the entering column's row r is +-0, the row is skipped;
// the ratio test ballots it once per pivot), so a row costs two SALU instructions and its fma
// (round 5; rounds 3-4 compared every row on the VALU first, a VALU -> SALU dependency per row),
// with the entering column's entries taken from another lane's register by DPP:
// lane k of every 16-lane row holds entry 16 g + k (cq = colq[16 g + (lane & 15)], g = R0 / 16), and
// v_fmac_f64_dpp ... row_newbcast:k reads it for the whole row (neg modifier: fma(-f, pj, t), the
// eager operation), so the elimination waits for one LDS read per 16 rows instead of one per 8.
// cq is written only by an LDS load (no VALU write within two instructions of a DPP read:
// tests/test_isa.py); an SALU write of exec before a DPP op needs no wait state.
template <int R0>
__device__ __forceinline__ void elim8dpp(double* t, double cq, double pj, uint64_t zm) {
    uint64_t sv;
    // (a group with no +-0 entry, the common case on a dense LP, branches to the 8 fmas back to
    // back; the branch is inside the asm so the register allocator sees one block)
    asm volatile(
        "s_bfe_u64 %[sv], %[zm], %[bfe]\n\t"
        "s_cbranch_scc1 1f\n\t"
        "v_fmac_f64_dpp %[t0], -%[c], %[pj] row_newbcast:%[k0] row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %[t1], -%[c], %[pj] row_newbcast:%[k1] row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %[t2], -%[c], %[pj] row_newbcast:%[k2] row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %[t3], -%[c], %[pj] row_newbcast:%[k3] row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %[t4], -%[c], %[pj] row_newbcast:%[k4] row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %[t5], -%[c], %[pj] row_newbcast:%[k5] row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %[t6], -%[c], %[pj] row_newbcast:%[k6] row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %[t7], -%[c], %[pj] row_newbcast:%[k7] row_mask:0xf bank_mask:0xf\n\t"
        "s_branch 2f\n"
        "1:\n\t"
        "s_mov_b64 %[sv], exec\n\t"
        "s_bitcmp1_b64 %[zm], %[r0]\n\ts_cselect_b64 exec, 0, %[sv]\n\tv_fmac_f64_dpp %[t0], -%[c], %[pj] row_newbcast:%[k0] row_mask:0xf bank_mask:0xf\n\t"
        "s_bitcmp1_b64 %[zm], %[r1]\n\ts_cselect_b64 exec, 0, %[sv]\n\tv_fmac_f64_dpp %[t1], -%[c], %[pj] row_newbcast:%[k1] row_mask:0xf bank_mask:0xf\n\t"
        "s_bitcmp1_b64 %[zm], %[r2]\n\ts_cselect_b64 exec, 0, %[sv]\n\tv_fmac_f64_dpp %[t2], -%[c], %[pj] row_newbcast:%[k2] row_mask:0xf bank_mask:0xf\n\t"
        "s_bitcmp1_b64 %[zm], %[r3]\n\ts_cselect_b64 exec, 0, %[sv]\n\tv_fmac_f64_dpp %[t3], -%[c], %[pj] row_newbcast:%[k3] row_mask:0xf bank_mask:0xf\n\t"
        "s_bitcmp1_b64 %[zm], %[r4]\n\ts_cselect_b64 exec, 0, %[sv]\n\tv_fmac_f64_dpp %[t4], -%[c], %[pj] row_newbcast:%[k4] row_mask:0xf bank_mask:0xf\n\t"
        "s_bitcmp1_b64 %[zm], %[r5]\n\ts_cselect_b64 exec, 0, %[sv]\n\tv_fmac_f64_dpp %[t5], -%[c], %[pj] row_newbcast:%[k5] row_mask:0xf bank_mask:0xf\n\t"
        "s_bitcmp1_b64 %[zm], %[r6]\n\ts_cselect_b64 exec, 0, %[sv]\n\tv_fmac_f64_dpp %[t6], -%[c], %[pj] row_newbcast:%[k6] row_mask:0xf bank_mask:0xf\n\t"
        "s_bitcmp1_b64 %[zm], %[r7]\n\ts_cselect_b64 exec, 0, %[sv]\n\tv_fmac_f64_dpp %[t7], -%[c], %[pj] row_newbcast:%[k7] row_mask:0xf bank_mask:0xf\n\t"
        "s_mov_b64 exec, %[sv]\n"
        "2:"
        : [t0] "+v"(t[0]), [t1] "+v"(t[1]), [t2] "+v"(t[2]), [t3] "+v"(t[3]), [t4] "+v"(t[4]), [t5] "+v"(t[5]),
          [t6] "+v"(t[6]), [t7] "+v"(t[7]), [sv] "=&s"(sv)
        : [c] "v"(cq), [pj] "v"(pj), [zm] "s"(zm), [bfe] "n"(R0 | (8 << 16)), [r0] "n"(R0), [r1] "n"(R0 + 1), [r2] "n"(R0 + 2),
          [r3] "n"(R0 + 3), [r4] "n"(R0 + 4), [r5] "n"(R0 + 5), [r6] "n"(R0 + 6), [r7] "n"(R0 + 7),
          [k0] "n"(R0 % 16), [k1] "n"(R0 % 16 + 1), [k2] "n"(R0 % 16 + 2), [k3] "n"(R0 % 16 + 3),
          [k4] "n"(R0 % 16 + 4), [k5] "n"(R0 % 16 + 5), [k6] "n"(R0 % 16 + 6), [k7] "n"(R0 % 16 + 7)
        : "scc");
}
__device__ __forceinline__ void elim_row(double& t, double f, double pj) {
    uint64_t sv;
    asm volatile(
        "v_cmp_neq_f64_e32 vcc, 0, %[f]\n\t"
        "s_and_saveexec_b64 %[sv], vcc\n\t"
        "v_fma_f64 %[t], -%[f], %[pj], %[t]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [t] "+v"(t), [sv] "=&s"(sv)
        : [f] "v"(f), [pj] "v"(pj)
        : "vcc");
}
// 8 rows at a time, one exec save/restore per block (exec is all lanes or none per row: p is
// uniform), so a row costs a compare, an exec select and one move.  tp := t[p]
template <int R0>
__device__ __forceinline__ void pick8(double& tp, const double* t, int p) {
    uint64_t sv;
    asm volatile("s_mov_b64 %[sv], exec\n\t"
                 "s_cmp_eq_u32 %[p], %[r0]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[d], %[t0]\n\t"
                 "s_cmp_eq_u32 %[p], %[r1]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[d], %[t1]\n\t"
                 "s_cmp_eq_u32 %[p], %[r2]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[d], %[t2]\n\t"
                 "s_cmp_eq_u32 %[p], %[r3]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[d], %[t3]\n\t"
                 "s_cmp_eq_u32 %[p], %[r4]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[d], %[t4]\n\t"
                 "s_cmp_eq_u32 %[p], %[r5]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[d], %[t5]\n\t"
                 "s_cmp_eq_u32 %[p], %[r6]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[d], %[t6]\n\t"
                 "s_cmp_eq_u32 %[p], %[r7]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[d], %[t7]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [d] "+v"(tp), [sv] "=&s"(sv)
                 : [t0] "v"(t[0]), [t1] "v"(t[1]), [t2] "v"(t[2]), [t3] "v"(t[3]), [t4] "v"(t[4]),
                   [t5] "v"(t[5]), [t6] "v"(t[6]), [t7] "v"(t[7]), [p] "s"(p), [r0] "n"(R0), [r1] "n"(R0 + 1),
                   [r2] "n"(R0 + 2), [r3] "n"(R0 + 3), [r4] "n"(R0 + 4), [r5] "n"(R0 + 5), [r6] "n"(R0 + 6),
                   [r7] "n"(R0 + 7)
                 : "scc");
}
// t[R0 + k] := v where R0 + k == p
template <int R0>
__device__ __forceinline__ void set8(double* t, double v, int p) {
    uint64_t sv;
    asm volatile("s_mov_b64 %[sv], exec\n\t"
                 "s_cmp_eq_u32 %[p], %[r0]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[t0], %[v]\n\t"
                 "s_cmp_eq_u32 %[p], %[r1]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[t1], %[v]\n\t"
                 "s_cmp_eq_u32 %[p], %[r2]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[t2], %[v]\n\t"
                 "s_cmp_eq_u32 %[p], %[r3]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[t3], %[v]\n\t"
                 "s_cmp_eq_u32 %[p], %[r4]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[t4], %[v]\n\t"
                 "s_cmp_eq_u32 %[p], %[r5]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[t5], %[v]\n\t"
                 "s_cmp_eq_u32 %[p], %[r6]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[t6], %[v]\n\t"
                 "s_cmp_eq_u32 %[p], %[r7]\n\ts_cselect_b64 exec, %[sv], 0\n\tv_mov_b64 %[t7], %[v]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [t0] "+v"(t[0]), [t1] "+v"(t[1]), [t2] "+v"(t[2]), [t3] "+v"(t[3]), [t4] "+v"(t[4]),
                   [t5] "+v"(t[5]), [t6] "+v"(t[6]), [t7] "+v"(t[7]), [sv] "=&s"(sv)
                 : [v] "v"(v), [p] "s"(p), [r0] "n"(R0), [r1] "n"(R0 + 1), [r2] "n"(R0 + 2), [r3] "n"(R0 + 3),
                   [r4] "n"(R0 + 4), [r5] "n"(R0 + 5), [r6] "n"(R0 + 6), [r7] "n"(R0 + 7)
                 : "scc");
}
// dst := src where ROW == p (p uniform)
template <int ROW>
__device__ __forceinline__ void move_if_row(double& dst, double src, int p) {
    uint64_t m, sv;
    asm volatile(
        "s_cmp_eq_u32 %[p], %[row]\n\t"
        "s_cselect_b64 %[m], -1, 0\n\t"
        "s_and_saveexec_b64 %[sv], %[m]\n\t"
        "v_mov_b64 %[d], %[s]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [d] "+v"(dst), [m] "=&s"(m), [sv] "=&s"(sv)
        : [s] "v"(src), [p] "s"(p), [row] "n"(ROW)
        : "scc");
}
// acc := acc + (cb * t), the product rounded, then the sum (fold_step's two roundings), cb
// uniform in an SGPR pair.  In asm so that a step holds one temporary: left to the scheduler,
// the 64 independent products were computed ahead of the dependent adds and the register rows
// spilled.
__device__ __forceinline__ void fold_row(double& acc, double cb, double t) {
    double p;
    // (s_nop 1: cb was written by v_readlane, and a VALU read of an SGPR a VALU wrote needs two
    // wait states, which the compiler's hazard recognizer does not insert inside asm)
    asm volatile(
        "s_nop 1\n\t"
        "v_mul_f64 %[p], %[cb], %[t]\n\t"
        "v_add_f64 %[acc], %[acc], %[p]"
        : [acc] "+v"(acc), [p] "=&v"(p)
        : [cb] "s"(cb), [t] "v"(t));
}
template <int M, int NW, class In>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(3))) void batched_reg_kernel(In in, int n,
                                                           int64_t max_pivots, int pricing, double tol_dj,
                                                           double tol_piv, BatchOut out) {
    static_assert(M == 64, "one ratio-test row per lane of wave 0");
    constexpr int R = M + 1;   // rows, the objective row last
    __shared__ double s_colq[R];
    __shared__ double s_zv[NW];
    __shared__ int32_t s_zvar[NW], s_zslot[NW], s_bvar[NW], s_bslot[NW];
    __shared__ int32_t s_basis[M];
    __shared__ int32_t s_p, s_leave, s_bland;
    __shared__ double s_piv;
    __shared__ uint64_t s_zm;   // rows 0..63 of the entering column that are +-0 (the elimination's skip rule)
    __shared__ int32_t s_bad;   // dense input: some b_i is not >= 0 (resident: 1 rejected at creation, 2 a bad c_k, 3 a dual phase left it infeasible or pending)
    __shared__ double s_cb[M];  // resident, new objective: cB_i = c[basis[i]] (+0.0 for a slack)
    // dual (RhsIn) only, absent from every other instantiation: b_k, where each slack lives (>= 0 its
    // slot, else -(row + 1) of the row it is basic in), the continuation flag, and the staging tile
    // of the RHS rebuild: kPanel slack columns of R entries (stride R = 65 doubles, odd: the 16
    // writers of one row land in 16 different bank pairs, the 64 readers of one column are consecutive)
    constexpr int kPanel = 16;
    __shared__ double s_b[M];
    __shared__ int32_t s_inv[M];
    __shared__ int32_t s_cont;
    __shared__ double s_zr;
    __shared__ double s_stage[kPanel * R];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = n + M;
    const int sl = tid;              // this lane's slot: < n a variable's column
    const bool own = sl < n;
    int var = sl < n ? sl : kNoIndex;   // the variable in the slot
    const int64_t lp = blockIdx.x;
    // buffer loads, one lane offset and the row in the scalar offset (a flat load per row
    // would hold 65 64-bit addresses in VGPRs next to the 65 values); lanes past the slots
    // read out of range, which returns +0
    const int voff = own ? sl * 8 : 0x7fffff00;
    double t[R];
    // wave 0, lane i keeps row i's RHS (the ratio test's) and every lane of wave 0 the objective
    // value T[M][N], each updated with the operations a column slot's elimination applies (same
    // bits): the RHS column needs no slot of its own, so n columns take ceil(n / 64) waves (round
    // 4: 64 x 128 in 2 waves instead of 3, 64 x 64 in 1 instead of 2; more LPs per CU)
    double rr = 0.0, zr = 0.0;
    // the final state to the batch's resident buffers (In::keep): the loads' pattern as stores,
    // lanes past the slots out of range (dropped)
    auto store_state = [&](int stt) __attribute__((always_inline)) {
        if constexpr (In::keep) {
            // (W opaque: the 65 row offsets are computed again here, not kept in SGPRs across the
            // pivot loop from the resident prologue's loads, where they would spill)
            int W = n + 1;
            asm volatile("" : "+s"(W));
            double* const rec = in.st.S + lp * state_doubles(M, n);
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc((void*)rec, (short)0, R * W * 8, 0x00020000);
            each<R>([&](auto I) {
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, t[I]), rs, voff, (int)I * W * 8, 0);
            });
            if (wid == 0) {
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, rr), rs, (lane * W + n) * 8, 0, 0);
                if (lane == 0)
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, zr), rs, (M * W + n) * 8, 0, 0);
            }
            int32_t* __restrict__ di = (int32_t*)(rec + R * W);
            if (own) di[sl] = var;
            for (int i = tid; i < M; i += blockDim.x) di[n + i] = s_basis[i];
            if (tid == 0) {
                di[N] = s_bland;
                di[N + 1] = stt;
            }
            if constexpr (In::dual)   // the b_k this RHS column was built from
                if (wid == 0) in.last[lp * M + lane] = s_b[lane];
        }
    };
    bool has_c = false;   // (resident) a new objective
    int saved = DLP_RUNNING;
    double acc = 0.0;     // (resident, has_c) this slot's fold, started at -c[var]
    if constexpr (In::resident) {
        // the state's loads: GenIn's pattern with row stride W = n + 1 and the RHS at slot n
        const int W = n + 1;
        const double* const rec = in.st.S + lp * state_doubles(M, n);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void*)rec, (short)0, R * W * 8, 0x00020000);
        each<R>([&](auto I) {
            t[I] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, (int)I * W * 8, 0));
        });
        const int32_t* __restrict__ si = (const int32_t*)(rec + R * W);
        if (own) var = si[sl];
        saved = si[N + 1];
        has_c = in.c != nullptr;
        if (wid == 0) {
            rr = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, (lane * W + n) * 8, 0, 0));
            zr = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, (M * W + n) * 8, 0, 0));
            const int bv = si[n + lane];
            s_basis[lane] = bv;
            // 1: rejected at creation; 2: a c_k entry that is not finite (this call only)
            int bad = saved == DLP_ERR_ARG ? 1 : 0;
            if (has_c) {
                const double* __restrict__ c = in.c + lp * in.sc;
                bool nf = false;
                for (int j = lane; j < n; j += 64) nf |= not_finite(c[j]);
                if (__ballot(nf) != 0 && bad == 0) bad = 2;
                s_cb[lane] = bv < n ? c[bv] : 0.0;   // cB_i, staged once per LP
            }
            // 3: left infeasible or pending by a dual phase (negative RHS entries: DLP_ERR_STATE)
            if constexpr (!In::dual) {
                if (bad == 0 && (saved == DLP_INFEASIBLE || saved == kDualPending)) bad = 3;
                if (lane == 0) {
                    s_bad = bad;
                    s_bland = has_c ? (pricing == DLP_PRICING_BLAND ? 1 : 0) : si[N];
                }
            } else {
                // 2: a b_k entry that is not finite; 3: some stored slot has z < -tol_dj (the LP is
                // not dual feasible: stopped inside a primal solve, or unbounded).  Lane i takes
                // b_k[i] once, for the checks, the rebuild (through LDS) and `last`.
                const double bl = in.b[lp * in.sb + lane];
                s_b[lane] = bl;
                bool neg = false;
                for (int s = lane; s < n; s += 64) neg |= rec[M * W + s] < -tol_dj;
                if (__ballot(not_finite(bl)) != 0 && bad == 0) bad = 2;
                if (__ballot(neg) != 0 && bad == 0) bad = 3;
                // continuation: a pending dual phase handed the very b_k (bit for bit) it was
                // stopped with goes on from its RHS column and Bland state as they stand
                bool cont = saved == kDualPending;
                if (cont) {
                    const double ll = in.last[lp * M + lane];
                    cont = __ballot(__builtin_bit_cast(uint64_t, bl) != __builtin_bit_cast(uint64_t, ll)) == 0;
                }
                if (lane == 0) {
                    s_bad = bad;
                    s_cont = cont ? 1 : 0;
                    s_bland = (cont && si[N]) || pricing == DLP_PRICING_BLAND ? 1 : 0;
                }
            }
        }
        if (has_c && own && var < n) acc = -in.c[lp * in.sc + var];
    } else if constexpr (!In::dense) {
        const int64_t ldg = in.ld;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(in.T + lp * (int64_t)R * ldg), (short)0, (int)((int64_t)R * ldg * 8), 0x00020000);
        each<R>([&](auto I) {
            t[I] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, (int)(I * ldg * 8), 0));
        });
        if (wid == 0) {
            rr = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(((int64_t)lane * ldg + N) * 8), 0, 0));
            zr = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(((int64_t)M * ldg + N) * 8), 0, 0));
        }
    } else {
        // the same loads from the caller's arrays: the resource on A_k (M x n doubles, row I at
        // scalar offset I * n * 8), a second one on c_k for the objective row -c[slot]; wave 0,
        // lane i takes b_k[i], the objective value starts at +0
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(in.A + lp * in.sA), (short)0, M * n * 8, 0x00020000);
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(in.c + lp * in.sc), (short)0, n * 8, 0x00020000);
        each<M>([&](auto I) {
            t[I] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, (int)I * n * 8, 0));
        });
        t[M] = -__builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rc, voff, 0, 0));
        if (wid == 0) {
            rr = in.b[lp * in.sb + lane];
            // an LP with a negative or NaN b_i is rejected, not solved
            const uint64_t anyb = __ballot(!(rr >= 0.0));
            if (lane == 0) s_bad = anyb != 0 ? 1 : 0;
        }
    }
    if constexpr (!In::resident) {
        for (int i = tid; i < M; i += blockDim.x) s_basis[i] = n + i;
        if (tid == 0) s_bland = pricing == DLP_PRICING_BLAND ? 1 : 0;
    }
    __syncthreads();
    if constexpr (In::dense || In::resident) {
        if (s_bad) {   // (uniform) DLP_ERR_ARG, no pivots, the slack basis, NaN values
            const double nan = __builtin_nan("");
            const bool resident_basis = In::resident && s_bad >= 2;   // refused for this call: the basis as it stands
            const int err = In::resident && s_bad == 3 ? DLP_ERR_STATE : DLP_ERR_ARG;
            if (tid == 0) {
                if (out.status) out.status[lp] = err;
                if (out.npivots) out.npivots[lp] = 0;
                if (out.objective) out.objective[lp] = nan;
            }
            if (out.basis)
                for (int i = tid; i < M; i += blockDim.x) out.basis[lp * M + i] = resident_basis ? s_basis[i] : n + i;
            if (out.x && own) out.x[lp * n + sl] = nan;
            if (out.y && wid == 0) out.y[lp * M + lane] = nan;
            // a fresh batch keeps the rejected LP as loaded, marked DLP_ERR_ARG; a resident one
            // is left exactly as it was
            if constexpr (!In::resident) store_state(DLP_ERR_ARG);
            return;
        }
    }
    int status = DLP_RUNNING;
    if constexpr (In::dual) {
        if (s_cont == 0) {   // (uniform)
            // The RHS rebuild (dlp.h, dlp_batch_resolve_rhs's rule) on the columns in registers:
            // row r's new RHS is the fold of Tfull[r][n + l] * b_l over l ascending, and slack l's
            // column sits in the lane that owns its slot, or is the unit vector of the row it is
            // basic in (a term of exactly b_l there; elsewhere its +-0 product cannot change a bit
            // and is left out, as in the LDS kernel).  The columns cross to the rows' lanes through
            // the staging tile, kPanel slacks at a time: the owner of a slack of the panel writes
            // its R entries, then wave 0's lane i folds row i, and every lane of wave 0 the
            // objective row (each keeps zr), the accumulators carried from panel to panel.
            if (own && var >= n) s_inv[var - n] = sl;
            if (wid == 0) {
                const int bv = s_basis[lane];
                if (bv >= n) s_inv[bv - n] = -(lane + 1);
            }
            double ra = 0.0, za = 0.0;
            for (int l0 = 0; l0 < M; l0 += kPanel) {
                const int c = var - n - l0;   // (kNoIndex in a lane past the slots: never in a panel)
                if (own && c >= 0 && c < kPanel) each<R>([&](auto I) { s_stage[c * R + I] = t[I]; });
                __syncthreads();
                if (wid == 0) {
                    // (rolled: unrolled, the panel's 32 LDS reads are requested ahead of the
                    // dependent adds and the register rows spill)
#pragma unroll 1
                    for (int j = 0; j < kPanel; ++j) {
                        const int iv = s_inv[l0 + j];
                        const double bl = s_b[l0 + j];
                        if (iv >= 0) {
                            ra = fold_step(ra, s_stage[j * R + lane], bl);
                            za = fold_step(za, s_stage[j * R + M], bl);
                        } else if (iv == -(lane + 1)) {
                            ra = fold_step(ra, 1.0, bl);
                        }
                    }
                }
                __syncthreads();
            }
            if (wid == 0) {
                rr = ra;
                zr = za;
            }
        }
        // (the objective value lives in LDS through the dual pivot loop, thread 0's alone to read
        // and write: the loop holds more than the primal's, and the two VGPRs are what keeps
        // the instantiation inside 168 without scratch)
        if (tid == 0) s_zr = zr;
    } else if constexpr (In::resident) {
        if (has_c) {
            // The objective rebuild, on the rows just loaded (dlp.h, dlp_session_set_objective's
            // rule): the lane owns its slot's column and folds rows 0..M-1 ascending, cB_i from
            // lane i's register by v_readlane (uniform: a skipped row is a scalar branch).
            const double cbv = s_cb[lane];
            // (the objective value: the same fold of the RHS, wave 0's lane i holding row i's
            // product, added in row order)
            const double prod = mul_rounded(cbv, rr);
            double z = 0.0;
            each<M>([&](auto I) {
                const double cb = readlane_f64(cbv, (int)I);
                if (cb != 0.0) {
                    fold_row(acc, cb, t[I]);
                    if (wid == 0) z = z + readlane_f64(prod, (int)I);
                }
            });
            t[M] = acc;
            if (wid == 0) zr = z;
        } else if (saved == DLP_OK || saved == DLP_UNBOUNDED) {
            // resumed without a new objective: an optimal or unbounded LP does no pivot
            status = saved;
            max_pivots = 0;
        }
    }
    int64_t k = 0;
    auto stamp = [&](int ph) {
        if (out.stamps && lp == 0 && tid == 0 && k < 64) out.stamps[k * 8 + ph] = wall_clock64();
    };
    for (; In::dual || k < max_pivots; ++k) {
        stamp(0);
        int q = kNoIndex, sq = -1, p = -1;
        uint64_t zm = 0;
      if constexpr (In::dual) {
        // ---- d1 leaving row (wave 0, row = lane): the most negative RHS below -tol_feas, exact
        // ties -> the smallest basic VARIABLE; Bland -> the eligible row with the smallest basic
        // variable (the ratio test's ballot / wave_min_i32 pattern)
        if (wid == 0) {
            const bool elig = rr < -in.tol_feas;
            const int bv = s_basis[lane];
            int pl = -1;
            if (__ballot(elig) != 0) {
                if (s_bland) {
                    const int bmin = wave_min_i32(elig ? bv : kNoIndex);
                    pl = __ffsll((unsigned long long)__ballot(elig && bv == bmin)) - 1;
                } else {
                    const double rmin = wave_min_f64(elig ? rr : __builtin_inf());
                    const bool tie = elig && rr == rmin;
                    const uint64_t ties = __ballot(tie);
                    pl = __ffsll((unsigned long long)ties) - 1;
                    if (__popcll(ties) > 1) {
                        const int bmin = wave_min_i32(tie ? bv : kNoIndex);
                        pl = __ffsll((unsigned long long)__ballot(tie && bv == bmin)) - 1;
                    }
                }
            }
            if (lane == 0) s_p = pl;
        }
        __syncthreads();
        stamp(1);
        p = __builtin_amdgcn_readfirstlane(s_p);   // (uniform: an SGPR operand below)
        if (p < 0) {   // primal feasible too: optimal (tested before the budget)
            status = DLP_OK;
            break;
        }
        if (k >= max_pivots) break;
        // ---- d2 entering slot: min over a = T[p][s] < -tol_piv of max(z_s, 0) / -a, exact ties ->
        // the smallest variable; per wave field by field, then across the waves (the pricing
        // reduction's structure).  A NaN ratio is no candidate, a +inf one is (it loses to any
        // finite ratio and ties by variable), as the LDS kernel's comparison has it.
        {
            double a = 0.0;
            each<M / 8>([&](auto G) { if ((p >> 3) == (int)G) pick8<8 * G>(a, &t[8 * G], p); });
            bool cand = own && a < -tol_piv;
            double r = __builtin_inf();
            if (cand) {
                double zz = t[M];
                if (!(zz > 0.0)) zz = 0.0;
                r = zz / (-a);
                if (r != r) {
                    cand = false;
                    r = __builtin_inf();
                }
            }
            const double rmin = wave_min_f64(r);
            const int vr = cand && r == rmin ? var : kNoIndex;
            const int vmin = wave_min_i32(vr);
            const uint64_t wz = __ballot(vr == vmin && vmin != kNoIndex);
            if (lane == 0) {
                s_zv[wid] = rmin;
                s_zvar[wid] = vmin;
                s_zslot[wid] = wz ? wid * 64 + __ffsll((unsigned long long)wz) - 1 : -1;
            }
        }
        __syncthreads();
        stamp(2);
        double rbest = s_zv[0];
        q = s_zvar[0], sq = s_zslot[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            if (s_zv[w] < rbest || (s_zv[w] == rbest && s_zvar[w] < q)) {
                rbest = s_zv[w]; q = s_zvar[w]; sq = s_zslot[w];
            }
        }
        if (sq < 0) {   // no entry of row p can take its RHS up: no x satisfies the row
            status = DLP_INFEASIBLE;
            break;
        }
        // ---- the entering column to LDS (its owner lane) + select and log as the primal's a4
        if (sl == sq) each<R>([&](auto I) { s_colq[I] = t[I]; });
        if (tid == 0) {
            const int leaving = s_basis[p];
            s_basis[p] = q;
            s_leave = leaving;
            s_bland = (pricing == DLP_PRICING_BLAND) ? 1 : (rbest == 0.0 ? 1 : 0);
            if (out.logs && k < out.log_cap) {
                dlp_pivot e;
                e.q = q; e.p = p; e.leaving = leaving; e.pad = 0;
                e.ratio = rbest; e.objective = 0.0;
                out.logs[lp * out.log_cap + k] = e;
            }
        }
        __syncthreads();
        stamp(3);
        // the elimination's skip masks, balloted by every wave for itself (-0 == 0: both skipped)
        zm = __ballot(s_colq[lane] == 0.0);
      } else {
        // ---- a1 pricing: lexicographic (z, variable) min; Bland: first variable with z < -tol.
        // Reduced field by field (min z, then the smallest variable among the lanes holding it;
        // the Bland variable apart): fewer cross-lane moves than shuffling the whole tuple.
        {
            const bool cand = sl < n;
            const double z = cand && t[M] < __builtin_inf() ? t[M] : __builtin_inf();   // (as z < zmin: NaN skipped)
            const double zmin = wave_min_f64(z);
            const int vz = cand && z == zmin ? var : kNoIndex;
            const int vbl = cand && z < -tol_dj ? var : kNoIndex;
            const int vmin = wave_min_i32(vz), vb = wave_min_i32(vbl);
            // the slots of the two winners (variables are distinct: one lane each)
            const uint64_t wz = __ballot(vz == vmin && vmin != kNoIndex);
            const uint64_t wb = __ballot(vbl == vb && vb != kNoIndex);
            if (lane == 0) {
                s_zv[wid] = zmin;
                s_zvar[wid] = vmin;
                s_zslot[wid] = wz ? wid * 64 + __ffsll((unsigned long long)wz) - 1 : -1;
                s_bvar[wid] = vb;
                s_bslot[wid] = wb ? wid * 64 + __ffsll((unsigned long long)wb) - 1 : -1;
            }
        }
        __syncthreads();
        stamp(1);
        {
            double zmin = s_zv[0];
            int vmin = s_zvar[0], smin = s_zslot[0], vb = s_bvar[0], sb = s_bslot[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                if (s_zv[w] < zmin || (s_zv[w] == zmin && s_zvar[w] < vmin)) {
                    zmin = s_zv[w]; vmin = s_zvar[w]; smin = s_zslot[w];
                }
                if (s_bvar[w] < vb) { vb = s_bvar[w]; sb = s_bslot[w]; }
            }
            if (s_bland) {
                q = vb; sq = sb;
            } else if (vmin != kNoIndex && zmin < -tol_dj) {
                q = vmin; sq = smin;
            }
        }
        if (q == kNoIndex) {
            status = DLP_OK;
            break;
        }
        // ---- the entering column to LDS (its owner lane)
        if (sl == sq) each<R>([&](auto I) { s_colq[I] = t[I]; });
        __syncthreads();
        stamp(2);
        // ---- a2 ratio test (wave 0, row = lane) + a4 select and log
        if (wid == 0) {
            // min ratio over the valid rows, then the smallest basis variable among the rows
            // holding it (cand_better's order), field by field
            const double a = s_colq[lane];
            const uint64_t zm = __ballot(a == 0.0);   // (-0 == 0: both skipped, as the eager rule)
            if (lane == 0) s_zm = zm;
            const bool valid = a > tol_piv;
            double ratio = __builtin_inf();
            if (valid) {
                double rhs = rr;
                if (!(rhs > 0.0)) rhs = 0.0;
                ratio = rhs / a;
            }
            const uint64_t anyv = __ballot(valid);
            const double rmin = wave_min_f64(ratio);
            const bool tie = valid && ratio == rmin;
            const int bv = s_basis[lane];
            const uint64_t ties = __ballot(tie);
            int wl = __ffsll((unsigned long long)ties) - 1;
            if (__popcll(ties) > 1) {   // exact ties: the smallest basis variable
                const int bmin = wave_min_i32(tie ? bv : kNoIndex);
                wl = __ffsll((unsigned long long)__ballot(tie && bv == bmin)) - 1;
            }
            Cand best;
            best.valid = anyv != 0 ? 1 : 0;
            best.row = wl;
            // (wl is uniform: v_readlane, no LDS round trip as __shfl's ds_bpermute)
            const int wls = __builtin_amdgcn_readfirstlane(wl < 0 ? 0 : wl);
            best.basis_var = anyv != 0 ? __builtin_amdgcn_readlane(bv, wls) : kNoIndex;
            best.ratio = anyv != 0 ? readlane_f64(ratio, wls) : 0.0;
            best.pivot = anyv != 0 ? readlane_f64(a, wls) : 0.0;
            best.pad0 = 0;
            if (lane == 0) {
                if (!best.valid) {
                    s_p = -1;
                } else {
                    const int p = best.row;
                    const int leaving = s_basis[p];
                    s_basis[p] = q;
                    s_leave = leaving;
                    s_p = p;
                    s_bland = (pricing == DLP_PRICING_BLAND) ? 1 : (best.ratio == 0.0 ? 1 : 0);
                    s_piv = best.pivot;
                    if (out.logs && k < out.log_cap) {
                        dlp_pivot e;
                        e.q = q; e.p = p; e.leaving = leaving; e.pad = 0;
                        e.ratio = best.ratio; e.objective = 0.0;
                        out.logs[lp * out.log_cap + k] = e;
                    }
                }
            }
        }
        __syncthreads();
        stamp(3);
        p = __builtin_amdgcn_readfirstlane(s_p);   // (uniform: an SGPR operand below)
        // the elimination's inputs, requested with p's (their LDS latency overlaps the pivot-row
        // division): the skip rule's row masks from the entering column's zero mask (SALU, no VALU
        // compare per row) and the entries for the DPP broadcast, 4 LDS reads per lane (elim8dpp)
        // (readfirstlane returns int: both halves through uint32_t, or a set bit 31 — row 31's
        // entry +-0 — sign-extends over rows 32..63 and their eliminations are skipped)
        zm = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(s_zm >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)s_zm);
      }
        double cq[M / 16];
        each<M / 16>([&](auto G) { cq[G] = s_colq[16 * G + (lane & 15)]; });
        // (with them: the pivot, the objective row's entry and wave 0's row entry for its RHS update)
        // (the dual's pivot is the entering column's entry of row p, negative)
        const double piv = In::dual ? s_colq[p] : s_piv, fM = s_colq[M];
        const double fr = wid == 0 ? s_colq[lane] : 0.0;
        if (p < 0) {
            status = DLP_UNBOUNDED;
            break;
        }
        // ---- a3 pivot row (IEEE division, in place) and the elimination; the entering slot
        // takes the leaving variable's column (e_p before the pivot)
        const bool ent = sl == sq;
        if (ent) var = s_leave;
        double tp = 0.0;
        // tp = t[p]: only the group of 8 rows holding p (a uniform branch per group)
        each<M / 8>([&](auto G) { if ((p >> 3) == (int)G) pick8<8 * G>(tp, &t[8 * G], p); });
        move_if_row<M>(tp, t[M], p);
        const double pj = (ent ? 1.0 : tp) / piv;
        stamp(4);
        if (ent) each<R>([&](auto I) { t[I] = 0.0; });   // e_p before the pivot (see the LDS kernel)
        each<M / 8>([&](auto G) { elim8dpp<8 * G>(&t[8 * G], cq[G / 2], pj, zm); });
        elim_row(t[M], fM, pj);   // the objective row
        each<M / 8>([&](auto G) { if ((p >> 3) == (int)G) set8<8 * G>(&t[8 * G], pj, p); });   // row p := the pivot row
        move_if_row<M>(t[M], pj, p);
        if (wid == 0) {   // the RHS of row `lane` and the objective value, as a column slot updates its rows
            const double pjr = readlane_f64(rr, p) / piv;   // (p uniform)
            const double v = __builtin_fma(-fr, pjr, rr);
            rr = lane == p ? pjr : (fr != 0.0 ? v : rr);
            const double fz = fM;
            if constexpr (In::dual) {
                if (lane == 0 && fz != 0.0) s_zr = __builtin_fma(-fz, pjr, s_zr);
            } else {
                if (fz != 0.0) zr = __builtin_fma(-fz, pjr, zr);
            }
        }
        stamp(5);
        if (tid == 0 && out.logs && k < out.log_cap) out.logs[lp * out.log_cap + k].objective = In::dual ? s_zr : zr;
    }
    if constexpr (In::dual)
        if (tid == 0) zr = s_zr;   // (store_state's and the output's copy are thread 0's)
    if (tid == 0) {
        int stt = status;
        if (stt == DLP_RUNNING) stt = DLP_PIVOT_LIMIT;
        if (out.status) out.status[lp] = stt;
        if (out.npivots) out.npivots[lp] = k;
        if (out.objective) out.objective[lp] = zr;
    }
    // (a dual phase the budget stopped is stored as pending: the primal rule must not continue it)
    store_state(status == DLP_RUNNING ? (In::dual ? kDualPending : (int)DLP_PIVOT_LIMIT) : status);
    if (out.basis)
        for (int i = tid; i < M; i += blockDim.x) out.basis[lp * M + i] = s_basis[i];
    // x and y from the tableau as it stands, every index written exactly once (no zero fill):
    // a nonbasic variable by its slot's lane (x_j = 0, y_i = the slack's reduced cost), a basic
    // one by its row's lane of wave 0 (x_j = the row's RHS, y_i = +0)
    if (out.x || out.y) {
        double* x = out.x ? out.x + lp * n : nullptr;
        double* y = out.y ? out.y + lp * M : nullptr;
        if (own) {
            if (var < n) { if (x) x[var] = 0.0; }
            else if (y) y[var - n] = t[M];
        }
        if (wid == 0) {
            const int bv = s_basis[lane];
            if (bv < n) { if (x) x[bv] = rr; }
            else if (y) y[bv - n] = 0.0;
        }
    }
}

}  // namespace
}  // namespace dlp

// A device's batch context, reused across dlp_batched_solve calls: the stream,
// the two timing events, the tableau buffer, one packed output buffer (objective | pivot count |
// status per LP, read back in ONE copy through a pinned staging buffer), basis and log buffers,
// each grown on demand and kept.  A fresh stream costs ~2 ms and the 7 allocations + frees ~1 ms
// on MI355X, more than the 64 x 128 batch's 0.8 ms kernel.  One context per device, taken for the
// whole call; a concurrent call on the same device builds and frees a private one as before.
// dlp_release_cached_memory frees them (dlp::batched_release).
namespace {
struct BatchCtx {
    int device = -1;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    void* dT = nullptr;   size_t capT = 0;
    void* dOut = nullptr; size_t capOut = 0;
    void* dB = nullptr;   size_t capB = 0;
    void* dL = nullptr;   size_t capL = 0;
    void* hOut = nullptr; size_t capH = 0;   // pinned
    // dlp_batched_solve_dense: host inputs staged as A | b | c, and the x / y outputs
    void* dIn = nullptr;  size_t capIn = 0;
    void* dX = nullptr;   size_t capX = 0;
    void* dY = nullptr;   size_t capY = 0;
    void free_all() {
        if (device >= 0) (void)hipSetDevice(device);
        if (s) (void)hipStreamSynchronize(s);
        for (void* p : {dT, dOut, dB, dL, dIn, dX, dY})
            if (p) (void)hipFree(p);
        if (hOut) (void)hipHostFree(hOut);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (s) (void)hipStreamDestroy(s);
        (void)hipGetLastError();
        *this = BatchCtx{};
    }
};
constexpr int kBatchDevs = 64;
std::mutex g_batch_mu[kBatchDevs];
BatchCtx g_batch[kBatchDevs];

// grow *p to at least `bytes` (contents not kept)
hipError_t ensure_buf(void** p, size_t* cap, size_t bytes, bool pinned = false) {
    if (*cap >= bytes && *p) return hipSuccess;
    if (*p) (void)(pinned ? hipHostFree(*p) : hipFree(*p));
    *p = nullptr;
    *cap = 0;
    const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    if (e == hipSuccess) *cap = bytes;
    return e;
}

// DLP_BATCH_RHS_LDS=1: dlp_batch_resolve_rhs runs the LDS kernel at every shape (A/B against the
// register instantiation); read once per process, as DLP_BATCH_LDS
bool rhs_force_lds() {
    static const bool f = dlp::env_int("DLP_BATCH_RHS_LDS", 0) == 1;
    return f;
}

// restores the caller's current device on every return path
struct DeviceGuard {
    int dev = -1;
    DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
};
}  // namespace

// A resident batch (dlp_batch_create_dense): its shape and options, its own context (stream,
// events, output buffers) and the state buffers of dlp::BatchState plus the staging buffer of
// host objectives.  They belong to the handle: dlp_release_cached_memory does not see them.
struct dlp_batch {
    int64_t nlp = 0, m = 0, n = 0;
    dlp_options opt{};
    BatchCtx ctx;
    void *dS = nullptr, *dC = nullptr;   // the state records (dlp::BatchState), host objectives staged
    void* dRb = nullptr;                 // host right-hand sides staged (allocated by the first such call)
    void* dBlast = nullptr;              // dlp::RhsIn::last (allocated by the first dlp_batch_resolve_rhs)
    int64_t bytes = 0;
    bool reg = false;
};

namespace dlp {
// Free the cached batch contexts of `device` (-1: all); returns the device bytes freed.
size_t batched_release(int device) {
    size_t n = 0;
    DeviceGuard g;
    for (int d = 0; d < kBatchDevs; ++d) {
        if (device >= 0 && d != device) continue;
        std::lock_guard<std::mutex> lk(g_batch_mu[d]);
        if (g_batch[d].device >= 0) {
            n += g_batch[d].capT + g_batch[d].capOut + g_batch[d].capB + g_batch[d].capL +
                 g_batch[d].capIn + g_batch[d].capX + g_batch[d].capY;
            g_batch[d].free_all();
        }
    }
    return n;
}
}  // namespace dlp

#define HIP_BTRY(expr)                                                               \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess) {                                                      \
            dlp::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));       \
            rc = DLP_ERR_HIP;                                                        \
            goto done;                                                               \
        }                                                                            \
    } while (0)

// The kernel dlp_batched_solve runs for an m x n batch, its lanes per LP and how many LPs one
// CU holds at once (the occupancy query with its VGPR / LDS footprint): C5's bound is per-pivot
// serial latency x this residency (bench.py --workload c5).
extern "C" int dlp_batched_occupancy(int64_t m, int64_t n, int device, int32_t* lps_per_cu,
                                     int32_t* threads_per_lp, int32_t* register_kernel) {
    if (m <= 0 || n <= 0) return DLP_ERR_ARG;
    const size_t lds = sizeof(double) * ((m + 1) * (n + 1) + (m + 1) + (n + 1)) + sizeof(int32_t) * (n + m + 8) +
                       sizeof(double) * 2 + 16;
    static const bool force_lds = dlp::env_int("DLP_BATCH_LDS", 0) == 1;
    const int nw = (int)((n + 63) / 64);
    const bool reg = !force_lds && m == 64 && nw >= 1 && nw <= 3;
    if (!reg && lds > 160 * 1024) return DLP_ERR_UNSUPPORTED;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        dlp::set_error("no HIP device visible (libdlp has no CPU fallback)");
        return DLP_ERR_NODEVICE;
    }
    DeviceGuard guard;   // the caller's current device is restored
    if (hipSetDevice(device) != hipSuccess) return DLP_ERR_HIP;
    int nb = 0, threads = 0;
    hipError_t e;
    if (reg) {
        threads = 64 * nw;
        using dlp::GenIn;
        e = nw == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dlp::batched_reg_kernel<64, 1, GenIn>, threads, 0)
          : nw == 2 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dlp::batched_reg_kernel<64, 2, GenIn>, threads, 0)
                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dlp::batched_reg_kernel<64, 3, GenIn>, threads, 0);
    } else {
        threads = lds > 40 * 1024 ? 512 : 256;
        e = hipFuncSetAttribute((const void*)dlp::batched_solve_kernel<dlp::GenIn>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dlp::batched_solve_kernel<dlp::GenIn>, threads, lds);
    }
    if (e != hipSuccess) {
        dlp::set_error(std::string("dlp_batched_occupancy: ") + hipGetErrorString(e));
        return DLP_ERR_HIP;
    }
    if (lps_per_cu) *lps_per_cu = nb;
    if (threads_per_lp) *threads_per_lp = threads;
    if (register_kernel) *register_kernel = reg ? 1 : 0;
    return DLP_OK;
}

namespace {
// One batch of nlp LPs of m x n: generated on the device from (kind, seed + k), or the caller's
// arrays (din); the host outputs (NULL: skipped).  The arguments are already validated.
struct BatchJob {
    const char* who;
    int64_t nlp, m, n;
    int kind;
    uint64_t seed;
    const dlp_batch_dense_in* din;   // NULL: generated (or, with `resolve`, the resident state)
    dlp_batch_out out;
    // a resident batch (dlp_batch_*): its own context instead of the device's cached one; the
    // dense kernels keep the final state in it (creation), or continue from it (resolve, with
    // the call's per-LP vector vec: the new objectives, n doubles per LP, NULL = resume)
    dlp_batch* batch;
    bool resolve;
    const double* vec;
    int64_t vstride;
    int vec_device;
    // dlp_batch_resolve_rhs: vec holds the new right-hand sides (m doubles per LP) and the dual
    // instantiation runs
    bool rhs;
    // dlp_batch_add_rows: m is the grown row count, r of its rows are new (LP k's r x n at
    // G + k * sG, its r right-hand sides at h + k * sh; rows_device: device pointers)
    bool grow;
    int64_t r;
    const double *G, *h;
    int64_t sG, sh;
    int rows_device;
    // dlp_batch_add_cols: n is the grown column count, k of its columns are new; G / h / sG / sh /
    // rows_device carry P / d / strideP / strided / cols_are_device (LP j's m x k and k doubles)
    bool widen;
    int64_t k;
};

int batched_run(const dlp_options& o, const BatchJob& job) {
    const int64_t nlp = job.nlp, m = job.m, n = job.n;
    const dlp_batch_dense_in* din = job.din;
    double* const objective = job.out.objective;
    int32_t* const status = job.out.status;
    int64_t* const npivots = job.out.npivots;
    int32_t* const basis = job.out.basis;
    dlp_pivot* const logs = job.out.logs;
    const int64_t log_cap = job.out.log_cap;
    double* const kernel_ms = job.out.kernel_ms;
    const std::string who = job.who;
    const int64_t N = n + m, ldg = (N + 1 + 15) / 16 * 16;
    const size_t lds = sizeof(double) * ((m + 1) * (n + 1) + (m + 1) + (n + 1)) + sizeof(int32_t) * (n + m + 8) +
                       sizeof(double) * 2 + 16;
    int rc = DLP_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        dlp::set_error("no HIP device visible (libdlp has no CPU fallback)");
        return DLP_ERR_NODEVICE;
    }
    if (o.device < 0 || o.device >= ndev) {
        dlp::set_error(who + ": no such device");
        return DLP_ERR_ARG;
    }
    if (lds > 160 * 1024) {
        dlp::set_error(who + ": tableau does not fit in 160 KiB of LDS");
        return DLP_ERR_UNSUPPORTED;
    }
    DeviceGuard guard;
    BatchCtx priv;
    BatchCtx* c = &priv;
    std::unique_lock<std::mutex> lk;
    dlp_batch* const bt = job.batch;
    if (bt) {
        c = &bt->ctx;   // (a handle is not thread-safe: no lock)
    } else if (o.device < kBatchDevs) {
        lk = std::unique_lock<std::mutex>(g_batch_mu[o.device], std::try_to_lock);
        if (lk.owns_lock()) c = &g_batch[o.device];
    }
    uint64_t* dStamps = nullptr;
    void *newS = nullptr, *newL = nullptr;   // dlp_batch_add_rows: the grown records, swapped in on success
    void* newC = nullptr;                    // dlp_batch_add_cols: newS and the wider staging buffer of host objectives
    bool refused = false;                    // ... a non-finite row: the call fails, the context stays
    dlp::BatchOut bo{};
    const size_t bOut = (sizeof(double) + sizeof(int64_t) + sizeof(int32_t)) * (size_t)nlp;
    const size_t bFlag = job.grow || job.widen ? 16 : 0;   // (the device flag of dlp::AddIn / ColsIn behind the packed outputs)
    double* dObj = nullptr;
    int64_t* dNp = nullptr;
    int32_t* dSt = nullptr;
    const bool want_log = logs && log_cap > 0;
    // host inputs are staged packed (A | b | c, a shared array once); device inputs are read in place
    const bool stage = din && !din->device;
    const size_t cntA = din ? (size_t)(din->strideA ? nlp : 1) * m * n : 0;
    const size_t cntb = din ? (size_t)(din->strideb ? nlp : 1) * m : 0;
    const size_t cntc = din ? (size_t)(din->stridec ? nlp : 1) * n : 0;
    HIP_BTRY(hipSetDevice(o.device));
    c->device = o.device;
    if (!c->s) HIP_BTRY(hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking));
    if (!c->e0) HIP_BTRY(hipEventCreate(&c->e0));
    if (!c->e1) HIP_BTRY(hipEventCreate(&c->e1));
    if (!din && !job.resolve) HIP_BTRY(ensure_buf(&c->dT, &c->capT, sizeof(double) * nlp * (m + 1) * ldg));
    if (stage) HIP_BTRY(ensure_buf(&c->dIn, &c->capIn, sizeof(double) * (cntA + cntb + cntc)));
    HIP_BTRY(ensure_buf(&c->dOut, &c->capOut, bOut + bFlag));
    HIP_BTRY(ensure_buf(&c->hOut, &c->capH, bOut + bFlag, true));
    if (basis) HIP_BTRY(ensure_buf(&c->dB, &c->capB, sizeof(int32_t) * nlp * m));
    if (want_log) HIP_BTRY(ensure_buf(&c->dL, &c->capL, sizeof(dlp_pivot) * nlp * log_cap));
    if (job.out.x) HIP_BTRY(ensure_buf(&c->dX, &c->capX, sizeof(double) * nlp * n));
    if (job.out.y) HIP_BTRY(ensure_buf(&c->dY, &c->capY, sizeof(double) * nlp * m));
    dObj = (double*)c->dOut;
    dNp = (int64_t*)(dObj + nlp);
    dSt = (int32_t*)(dNp + nlp);
    if (bt && !job.resolve) {
        // the resident state (and the staging buffer of host objectives), owned by the handle
        const size_t bS = sizeof(double) * nlp * dlp::state_doubles(m, n), bC = sizeof(double) * nlp * n;
        if (hipMalloc(&bt->dS, bS) != hipSuccess || hipMalloc(&bt->dC, bC) != hipSuccess) {
            (void)hipGetLastError();
            dlp::set_error(who + ": the batch's resident state does not fit in device memory");
            rc = DLP_ERR_OOM;
            goto done;
        }
        bt->bytes = (int64_t)(bS + bC);
    }
    {
        hipStream_t s = c->s;
        // host arrays: `per` doubles per LP at `stride` (0: one shared array) -> packed at dst
        auto put = [&](double* dst, const double* src, int64_t per, int64_t stride) {
            if (stride == 0 || stride == per)
                return hipMemcpyAsync(dst, src, sizeof(double) * per * (stride ? nlp : 1),
                                      hipMemcpyHostToDevice, s);
            return hipMemcpy2DAsync(dst, sizeof(double) * per, src, sizeof(double) * stride,
                                    sizeof(double) * per, (size_t)nlp, hipMemcpyHostToDevice, s);
        };
        dlp::GenIn gin{(const double*)c->dT, ldg};
        dlp::DenseIn dn{};
        dlp::BatchState bst{bt ? (double*)bt->dS : nullptr};
        // the call's per-LP vector on the device (resolve: c_k; resolve_rhs: b_k) and its stride
        const double* dvec = nullptr;
        int64_t dstride = 0;
        if (job.rhs && !bt->dBlast) {
            // (read only for an LP this call's kernel has marked pending, after writing its b_k)
            const size_t bL = sizeof(double) * nlp * m;
            if (hipMalloc(&bt->dBlast, bL) != hipSuccess) {
                (void)hipGetLastError();
                bt->dBlast = nullptr;
                dlp::set_error(who + ": the batch's right-hand sides do not fit in device memory");
                rc = DLP_ERR_OOM;
                goto done;
            }
            bt->bytes += (int64_t)bL;
        }
        dlp::AddIn ain{};
        dlp::ColsIn cin{};
        if (job.grow) {
            const int64_t r = job.r;
            ain.st = bst;
            ain.src = (const double*)bt->dS;
            ain.r = (int)r;
            ain.tol_feas = o.tol_feas;
            ain.last = (double*)bt->dBlast;
            if (r > 0) {
                // the records and the `last` buffer of the grown shape: the kernel fills them, the
                // handle takes them only when no LP's rows were refused
                const size_t bS = sizeof(double) * nlp * dlp::state_doubles(m, n), bL = sizeof(double) * nlp * m;
                if (hipMalloc(&newS, bS) != hipSuccess || hipMalloc(&newL, bL) != hipSuccess) {
                    (void)hipGetLastError();
                    dlp::set_error(who + ": the grown state does not fit in device memory");
                    rc = DLP_ERR_OOM;
                    goto done;
                }
                ain.st = dlp::BatchState{(double*)newS};
                ain.last = (double*)newL;
                ain.flag = (int32_t*)((char*)c->dOut + bOut);
                HIP_BTRY(hipMemsetAsync(ain.flag, 0x7f, sizeof(int32_t), s));   // (above every LP index)
                if (job.rows_device) {
                    ain.G = job.G; ain.h = job.h; ain.sG = job.sG; ain.sh = job.sh;
                } else {   // host rows: packed G | h, a shared array once
                    const size_t cntG = (size_t)(job.sG ? nlp : 1) * r * n, cnth = (size_t)(job.sh ? nlp : 1) * r;
                    HIP_BTRY(ensure_buf(&c->dIn, &c->capIn, sizeof(double) * (cntG + cnth)));
                    double* dG = (double*)c->dIn;
                    HIP_BTRY(put(dG, job.G, r * n, job.sG));
                    HIP_BTRY(put(dG + cntG, job.h, r, job.sh));
                    ain.G = dG; ain.h = dG + cntG;
                    ain.sG = job.sG ? r * n : 0; ain.sh = job.sh ? r : 0;
                }
            }
        } else if (job.widen) {
            // the records of the grown shape and the staging buffer of host objectives at its n: the
            // kernel fills the records, the handle takes both only when no LP's columns were refused
            const int64_t k = job.k;
            const size_t bS = sizeof(double) * nlp * dlp::state_doubles(m, n), bC = sizeof(double) * nlp * n;
            if (hipMalloc(&newS, bS) != hipSuccess || hipMalloc(&newC, bC) != hipSuccess) {
                (void)hipGetLastError();
                dlp::set_error(who + ": the grown state does not fit in device memory");
                rc = DLP_ERR_OOM;
                goto done;
            }
            cin.st = dlp::BatchState{(double*)newS};
            cin.src = (const double*)bt->dS;
            cin.k = (int)k;
            cin.flag = (int32_t*)((char*)c->dOut + bOut);
            HIP_BTRY(hipMemsetAsync(cin.flag, 0x7f, sizeof(int32_t), s));   // (above every LP index)
            if (job.rows_device) {
                cin.P = job.G; cin.d = job.h; cin.sP = job.sG; cin.sd = job.sh;
            } else {   // host columns: packed P | d, a shared array once
                const size_t cntP = (size_t)(job.sG ? nlp : 1) * m * k, cntd = (size_t)(job.sh ? nlp : 1) * k;
                HIP_BTRY(ensure_buf(&c->dIn, &c->capIn, sizeof(double) * (cntP + cntd)));
                double* dP = (double*)c->dIn;
                HIP_BTRY(put(dP, job.G, m * k, job.sG));
                HIP_BTRY(put(dP + cntP, job.h, k, job.sh));
                cin.P = dP; cin.d = dP + cntP;
                cin.sP = job.sG ? m * k : 0; cin.sd = job.sh ? k : 0;
            }
        } else if (job.resolve) {
            if (job.vec && !job.vec_device) {   // a host vector: packed into the handle's staging buffer
                const int64_t cnt = job.rhs ? m : n;   // (right-hand sides: m per LP, their own buffer)
                const size_t per = sizeof(double) * cnt;
                if (job.rhs && !bt->dRb) {
                    if (hipMalloc(&bt->dRb, per * nlp) != hipSuccess) {
                        (void)hipGetLastError();
                        bt->dRb = nullptr;
                        dlp::set_error(who + ": the staging buffer of b does not fit in device memory");
                        rc = DLP_ERR_OOM;
                        goto done;
                    }
                    bt->bytes += (int64_t)(per * nlp);
                }
                void* const dst = job.rhs ? bt->dRb : bt->dC;
                if (job.vstride == 0 || job.vstride == cnt)
                    HIP_BTRY(hipMemcpyAsync(dst, job.vec, per * (job.vstride ? nlp : 1), hipMemcpyHostToDevice, s));
                else
                    HIP_BTRY(hipMemcpy2DAsync(dst, per, job.vec, sizeof(double) * job.vstride, per, (size_t)nlp,
                                              hipMemcpyHostToDevice, s));
                dvec = (const double*)dst;
                dstride = job.vstride ? cnt : 0;
            } else {
                dvec = job.vec;
                dstride = job.vstride;
            }
        } else if (!din) {
            dim3 gg((unsigned)((m + 1 + 3) / 4), (unsigned)nlp);
            dlp::batched_generate_kernel<<<gg, 256, 0, s>>>((double*)c->dT, ldg, m, n, job.kind, job.seed);
            HIP_BTRY(hipGetLastError());
        } else if (stage) {
            double* dA = (double*)c->dIn;
            HIP_BTRY(put(dA, din->A, m * n, din->strideA));
            HIP_BTRY(put(dA + cntA, din->b, m, din->strideb));
            HIP_BTRY(put(dA + cntA + cntb, din->c, n, din->stridec));
            dn = dlp::DenseIn{dA, dA + cntA, dA + cntA + cntb, din->strideA ? m * n : 0,
                              din->strideb ? m : 0, din->stridec ? n : 0};
        } else {
            dn = dlp::DenseIn{din->A, din->b, din->c, din->strideA, din->strideb, din->stridec};
        }
        bo.objective = dObj;
        bo.status = dSt;
        bo.npivots = dNp;
        bo.basis = basis ? (int32_t*)c->dB : nullptr;
        bo.logs = want_log ? (dlp_pivot*)c->dL : nullptr;
        bo.log_cap = want_log ? log_cap : 0;
        bo.x = job.out.x ? (double*)c->dX : nullptr;
        bo.y = job.out.y ? (double*)c->dY : nullptr;
        static const char* stamp_file = std::getenv("DLP_BATCH_STAMPS");
        if (stamp_file) {
            HIP_BTRY(hipMalloc(&dStamps, sizeof(uint64_t) * 64 * 8));
            HIP_BTRY(hipMemsetAsync(dStamps, 0, sizeof(uint64_t) * 64 * 8, s));
            bo.stamps = dStamps;
        }
        // m = 64 with n <= 192 columns: the register-resident kernel (DLP_BATCH_LDS=1: the LDS
        // kernel, for A/B); otherwise the LDS-resident one
        static const bool force_lds = dlp::env_int("DLP_BATCH_LDS", 0) == 1;
        const int nw = (int)((n + 63) / 64);
        // (the dual re-solve runs the register kernel's RhsIn instantiation on the same records;
        // DLP_BATCH_RHS_LDS=1 sends that call alone through the LDS kernel)
        // (dlp_batch_add_rows and dlp_batch_add_cols always run the LDS kernel: DESIGN.md §25, §27)
        const bool reg = !force_lds && m == 64 && nw >= 1 && nw <= 3 && !(job.rhs && rhs_force_lds()) && !job.grow &&
                         !job.widen;
        // the kernel of this input kind (its own instantiation, so its own dynamic-LDS attribute),
        // timed alone between e0 and e1
        auto launch = [&](auto in) -> hipError_t {
            using In = decltype(in);
            hipError_t e = hipSuccess;
            if (!reg)
                e = hipFuncSetAttribute((const void*)dlp::batched_solve_kernel<In>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e == hipSuccess) e = hipEventRecord(c->e0, s);
            if (e != hipSuccess) return e;
            if (reg) {
              if constexpr (!In::grow && !In::widen) {   // (no register-kernel instantiation of the growth sources)
                if (nw == 1)
                    dlp::batched_reg_kernel<64, 1, In><<<(unsigned)nlp, 64, 0, s>>>(in, (int)n, o.max_pivots, o.pricing,
                                                                                  o.tol_dj, o.tol_piv, bo);
                else if (nw == 2)
                    dlp::batched_reg_kernel<64, 2, In><<<(unsigned)nlp, 128, 0, s>>>(in, (int)n, o.max_pivots, o.pricing,
                                                                                   o.tol_dj, o.tol_piv, bo);
                else
                    dlp::batched_reg_kernel<64, 3, In><<<(unsigned)nlp, 192, 0, s>>>(in, (int)n, o.max_pivots, o.pricing,
                                                                                   o.tol_dj, o.tol_piv, bo);
              }
            } else {
                // 512 lanes per LP when few LPs share a CU (LDS > 40 KB each), else 256
                const unsigned threads = lds > 40 * 1024 ? 512 : 256;
                dlp::batched_solve_kernel<In><<<(unsigned)nlp, threads, lds, s>>>(
                    in, (int)m, (int)n, o.max_pivots, o.pricing, o.tol_dj, o.tol_piv, bo);
            }
            return hipGetLastError();
        };
        if (job.grow)
            HIP_BTRY(launch(ain));
        else if (job.widen)
            HIP_BTRY(launch(cin));
        else if (job.rhs)
            HIP_BTRY(launch(dlp::RhsIn{bst, dvec, dstride, o.tol_feas, (double*)bt->dBlast}));
        else if (job.resolve)
            HIP_BTRY(launch(dlp::ResIn{bst, dvec, dstride}));
        else if (bt)
            HIP_BTRY(launch(dlp::DenseKeepIn{dn, bst}));
        else
            HIP_BTRY(din ? launch(dn) : launch(gin));
        if (bt && !job.rhs && !job.grow && !job.widen) bt->reg = reg;   // (the kernel of creation and of dlp_batch_resolve)
        HIP_BTRY(hipEventRecord(c->e1, s));
        if (job.grow && job.r > 0) {
            // all or nothing: a non-finite row in any LP leaves the batch and `out` as they were
            int32_t* const hflag = (int32_t*)((char*)c->hOut + bOut);
            HIP_BTRY(hipMemcpyAsync(hflag, ain.flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_BTRY(hipStreamSynchronize(s));
            if (*hflag >= 0 && *hflag < nlp) {
                dlp::set_error(who + ": LP " + std::to_string(*hflag) + ": a G or h entry is not finite");
                refused = true;
                rc = DLP_ERR_ARG;
                goto done;
            }
            // the swap: the handle owns the grown buffers, the old ones (and the staging buffer of
            // host right-hand sides, sized by the old m) go
            const int64_t mo = m - job.r;
            bt->bytes -= (int64_t)(sizeof(double) * nlp * dlp::state_doubles(mo, n));
            (void)hipFree(bt->dS);
            if (bt->dBlast) {
                bt->bytes -= (int64_t)(sizeof(double) * nlp * mo);
                (void)hipFree(bt->dBlast);
            }
            if (bt->dRb) {
                bt->bytes -= (int64_t)(sizeof(double) * nlp * mo);
                (void)hipFree(bt->dRb);
                bt->dRb = nullptr;
            }
            bt->dS = newS;
            bt->dBlast = newL;
            newS = newL = nullptr;
            bt->bytes += (int64_t)(sizeof(double) * nlp * (dlp::state_doubles(m, n) + m));
            bt->m = m;
            bt->reg = !force_lds && m == 64 && nw >= 1 && nw <= 3;   // the kernel of the later resolve calls
        }
        if (job.widen) {
            // all or nothing, as above: a non-finite column in any LP leaves the batch and `out` as they were
            int32_t* const hflag = (int32_t*)((char*)c->hOut + bOut);
            HIP_BTRY(hipMemcpyAsync(hflag, cin.flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_BTRY(hipStreamSynchronize(s));
            if (*hflag >= 0 && *hflag < nlp) {
                dlp::set_error(who + ": LP " + std::to_string(*hflag) + ": a P or d entry is not finite");
                refused = true;
                rc = DLP_ERR_ARG;
                goto done;
            }
            // the swap: the handle owns the wider records and objective staging buffer, the old ones go
            // (`last` and the staging buffer of host right-hand sides are sized by m: they stay)
            const int64_t no = n - job.k;
            bt->bytes -= (int64_t)(sizeof(double) * nlp * (dlp::state_doubles(m, no) + no));
            (void)hipFree(bt->dS);
            (void)hipFree(bt->dC);
            bt->dS = newS;
            bt->dC = newC;
            newS = newC = nullptr;
            bt->bytes += (int64_t)(sizeof(double) * nlp * (dlp::state_doubles(m, n) + n));
            bt->n = n;
            bt->reg = !force_lds && m == 64 && nw >= 1 && nw <= 3;   // the kernel of the later resolve calls
        }
        // read back only what the caller asked for: the packed outputs it wants in one copy
        // (objective | pivot counts | status are contiguous), basis, logs, x and y when requested
        const bool wo = objective != nullptr, wn = npivots != nullptr, ws = status != nullptr;
        if (wo || wn || ws) {
            const size_t from = wo ? 0 : wn ? sizeof(double) * nlp : (sizeof(double) + sizeof(int64_t)) * nlp;
            const size_t to = ws ? bOut : wn ? (sizeof(double) + sizeof(int64_t)) * nlp : sizeof(double) * nlp;
            HIP_BTRY(hipMemcpyAsync((char*)c->hOut + from, (char*)c->dOut + from, to - from,
                                    hipMemcpyDeviceToHost, s));
        }
        if (basis) HIP_BTRY(hipMemcpyAsync(basis, c->dB, sizeof(int32_t) * nlp * m, hipMemcpyDeviceToHost, s));
        if (want_log)
            HIP_BTRY(hipMemcpyAsync(logs, c->dL, sizeof(dlp_pivot) * nlp * log_cap, hipMemcpyDeviceToHost, s));
        if (job.out.x)
            HIP_BTRY(hipMemcpyAsync(job.out.x, c->dX, sizeof(double) * nlp * n, hipMemcpyDeviceToHost, s));
        if (job.out.y)
            HIP_BTRY(hipMemcpyAsync(job.out.y, c->dY, sizeof(double) * nlp * m, hipMemcpyDeviceToHost, s));
        HIP_BTRY(hipStreamSynchronize(s));
        if (kernel_ms) {
            float ms = 0.f;
            HIP_BTRY(hipEventElapsedTime(&ms, c->e0, c->e1));
            *kernel_ms = ms;
        }
        if (wo) std::memcpy(objective, c->hOut, sizeof(double) * nlp);
        if (wn) std::memcpy(npivots, (char*)c->hOut + sizeof(double) * nlp, sizeof(int64_t) * nlp);
        if (ws) std::memcpy(status, (char*)c->hOut + (sizeof(double) + sizeof(int64_t)) * nlp, sizeof(int32_t) * nlp);
        if (dStamps) {   // diagnostics only
            std::vector<uint64_t> h(64 * 8);
            HIP_BTRY(hipMemcpy(h.data(), dStamps, sizeof(uint64_t) * 64 * 8, hipMemcpyDeviceToHost));
            if (FILE* f = std::fopen(stamp_file, "wb")) {
                std::fwrite(h.data(), sizeof(uint64_t), h.size(), f);
                std::fclose(f);
            }
        }
    }
done:
    if (dStamps) (void)hipFree(dStamps);
    if (newS) (void)hipFree(newS);
    if (newL) (void)hipFree(newL);
    if (newC) (void)hipFree(newC);
    if ((rc != DLP_OK && !refused) || c == &priv) c->free_all();   // a failed context is rebuilt next call
    return rc;
}
}  // namespace

extern "C" int dlp_batched_solve(int kind, int64_t nlp, int64_t m, int64_t n, uint64_t seed,
                                 const dlp_options* opt, double* objective, int32_t* status,
                                 int64_t* npivots, int32_t* basis, dlp_pivot* logs,
                                 int64_t log_cap, double* kernel_ms) {
    dlp_options o;
    if (opt) o = *opt; else dlp_options_default(&o);
    if (nlp <= 0 || m <= 0 || n <= 0 || (kind != DLP_GEN_DENSE && kind != DLP_GEN_DEGENERATE) ||
        nlp > 65535 * 16 || log_cap < 0) {
        dlp::set_error("dlp_batched_solve: bad arguments");
        return DLP_ERR_ARG;
    }
    BatchJob job{};
    job.who = "dlp_batched_solve";
    job.nlp = nlp; job.m = m; job.n = n;
    job.kind = kind; job.seed = seed;
    job.out.objective = objective; job.out.status = status; job.out.npivots = npivots;
    job.out.basis = basis; job.out.logs = logs; job.out.log_cap = log_cap;
    job.out.kernel_ms = kernel_ms;
    return batched_run(o, job);
}

extern "C" int dlp_batched_solve_dense(int64_t nlp, int64_t m, int64_t n, const dlp_batch_dense_in* in,
                                       const dlp_options* opt, const dlp_batch_out* out) {
    dlp_options o;
    if (opt) o = *opt; else dlp_options_default(&o);
    const auto bad_stride = [](int64_t s, int64_t need) { return s != 0 && s < need; };
    if (nlp <= 0 || m <= 0 || n <= 0 || nlp > 65535 * 16 || !in || !out || out->log_cap < 0 || !in->A ||
        !in->b || !in->c || (in->device != 0 && in->device != 1) || bad_stride(in->strideA, m * n) ||
        bad_stride(in->strideb, m) || bad_stride(in->stridec, n)) {
        dlp::set_error("dlp_batched_solve_dense: bad arguments");
        return DLP_ERR_ARG;
    }
    BatchJob job{};
    job.who = "dlp_batched_solve_dense";
    job.nlp = nlp; job.m = m; job.n = n;
    job.din = in;
    job.out = *out;
    return batched_run(o, job);
}

// ---- resident batches
namespace {
void batch_destroy(dlp_batch* b) {
    DeviceGuard guard;
    if (b->opt.device >= 0) (void)hipSetDevice(b->opt.device);
    b->ctx.free_all();   // (drains the stream first)
    for (void* p : {b->dS, b->dC, b->dRb, b->dBlast})
        if (p) (void)hipFree(p);
    (void)hipGetLastError();
    delete b;
}
}  // namespace

extern "C" int dlp_batch_create_dense(int64_t nlp, int64_t m, int64_t n, const dlp_batch_dense_in* in,
                                      const dlp_options* opt, const dlp_batch_out* out, dlp_batch** batch) {
    dlp_options o;
    if (opt) o = *opt; else dlp_options_default(&o);
    if (batch) *batch = nullptr;
    const auto bad_stride = [](int64_t s, int64_t need) { return s != 0 && s < need; };
    if (nlp <= 0 || m <= 0 || n <= 0 || nlp > 65535 * 16 || !in || !batch || (out && out->log_cap < 0) || !in->A ||
        !in->b || !in->c || (in->device != 0 && in->device != 1) || bad_stride(in->strideA, m * n) ||
        bad_stride(in->strideb, m) || bad_stride(in->stridec, n)) {
        dlp::set_error("dlp_batch_create_dense: bad arguments");
        return DLP_ERR_ARG;
    }
    dlp_batch* b = new (std::nothrow) dlp_batch;
    if (!b) return DLP_ERR_OOM;
    b->nlp = nlp; b->m = m; b->n = n;
    b->opt = o;
    BatchJob job{};
    job.who = "dlp_batch_create_dense";
    job.nlp = nlp; job.m = m; job.n = n;
    job.din = in;
    if (out) job.out = *out;
    job.batch = b;
    const int rc = batched_run(o, job);
    if (rc != DLP_OK) {
        b->opt.device = rc == DLP_ERR_NODEVICE || rc == DLP_ERR_ARG ? -1 : b->opt.device;
        batch_destroy(b);
        return rc;
    }
    *batch = b;
    return DLP_OK;
}

extern "C" int dlp_batch_resolve(dlp_batch* batch, const double* c, int64_t stridec, int c_is_device,
                                 int64_t max_pivots, const dlp_batch_out* out) {
    if (!batch || max_pivots < 0 || (out && out->log_cap < 0) ||
        (c && ((stridec != 0 && stridec < batch->n) || (c_is_device != 0 && c_is_device != 1)))) {
        dlp::set_error("dlp_batch_resolve: bad arguments");
        return DLP_ERR_ARG;
    }
    dlp_options o = batch->opt;
    o.max_pivots = max_pivots;
    BatchJob job{};
    job.who = "dlp_batch_resolve";
    job.nlp = batch->nlp; job.m = batch->m; job.n = batch->n;
    if (out) job.out = *out;
    job.batch = batch;
    job.resolve = true;
    job.vec = c;
    job.vstride = stridec;
    job.vec_device = c_is_device;
    return batched_run(o, job);
}

extern "C" int dlp_batch_resolve_rhs(dlp_batch* batch, const double* b, int64_t strideb, int b_is_device,
                                     int64_t max_pivots, const dlp_batch_out* out) {
    if (!batch || !b || max_pivots < 0 || (out && out->log_cap < 0) || (strideb != 0 && strideb < batch->m) ||
        (b_is_device != 0 && b_is_device != 1)) {
        dlp::set_error("dlp_batch_resolve_rhs: bad arguments");
        return DLP_ERR_ARG;
    }
    dlp_options o = batch->opt;
    o.max_pivots = max_pivots;
    BatchJob job{};
    job.who = "dlp_batch_resolve_rhs";
    job.nlp = batch->nlp; job.m = batch->m; job.n = batch->n;
    if (out) job.out = *out;
    job.batch = batch;
    job.resolve = true;
    job.rhs = true;
    job.vec = b;
    job.vstride = strideb;
    job.vec_device = b_is_device;
    return batched_run(o, job);
}

extern "C" int dlp_batch_add_rows(dlp_batch* batch, int64_t r, const double* G, int64_t strideG, const double* h,
                                  int64_t strideh, int rows_are_device, int64_t max_pivots, const dlp_batch_out* out) {
    if (!batch || r < 0 || max_pivots < 0 || (out && out->log_cap < 0) ||
        (rows_are_device != 0 && rows_are_device != 1) ||
        (r > 0 && (!G || !h || (strideG != 0 && strideG < r * batch->n) || (strideh != 0 && strideh < r)))) {
        dlp::set_error("dlp_batch_add_rows: bad arguments");
        return DLP_ERR_ARG;
    }
    if (r > 160 * 1024 / 8) {   // (a row takes more than 8 bytes of LDS: the launch's formula cannot hold it)
        dlp::set_error("dlp_batch_add_rows: tableau does not fit in 160 KiB of LDS");
        return DLP_ERR_UNSUPPORTED;
    }
    dlp_options o = batch->opt;
    o.max_pivots = max_pivots;
    BatchJob job{};
    job.who = "dlp_batch_add_rows";
    job.nlp = batch->nlp; job.m = batch->m + r; job.n = batch->n;
    if (out) job.out = *out;
    job.batch = batch;
    job.resolve = true;
    job.grow = true;
    job.r = r;
    job.G = G; job.h = h;
    job.sG = strideG; job.sh = strideh;
    job.rows_device = rows_are_device;
    return batched_run(o, job);
}

extern "C" int dlp_batch_add_cols(dlp_batch* batch, int64_t k, const double* P, int64_t strideP, const double* d,
                                  int64_t strided, int cols_are_device, int64_t max_pivots, const dlp_batch_out* out) {
    if (!batch || k < 0 || max_pivots < 0 || (out && out->log_cap < 0) ||
        (cols_are_device != 0 && cols_are_device != 1) ||
        (k > 0 && (!P || !d || (strideP != 0 && strideP < batch->m * k) ||
                   (strided != 0 && strided < k)))) {
        dlp::set_error("dlp_batch_add_cols: bad arguments");
        return DLP_ERR_ARG;
    }
    if (k == 0) return dlp_batch_resolve(batch, nullptr, 0, 0, max_pivots, out);
    if (k > 160 * 1024 / 8) {   // (a column takes more than 8 bytes of LDS: the launch's formula cannot hold it)
        dlp::set_error("dlp_batch_add_cols: tableau does not fit in 160 KiB of LDS");
        return DLP_ERR_UNSUPPORTED;
    }
    dlp_options o = batch->opt;
    o.max_pivots = max_pivots;
    BatchJob job{};
    job.who = "dlp_batch_add_cols";
    job.nlp = batch->nlp; job.m = batch->m; job.n = batch->n + k;
    if (out) job.out = *out;
    job.batch = batch;
    job.resolve = true;
    job.widen = true;
    job.k = k;
    job.G = P; job.h = d;
    job.sG = strideP; job.sh = strided;
    job.rows_device = cols_are_device;
    return batched_run(o, job);
}

extern "C" int dlp_batch_read(dlp_batch* batch, int64_t k, double* T, int32_t* basis) {
    if (!batch || k < 0 || k >= batch->nlp) {
        dlp::set_error("dlp_batch_read: bad arguments");
        return DLP_ERR_ARG;
    }
    const int64_t m = batch->m, n = batch->n, N = n + m, W = n + 1, ld = dlp_tableau_ld(m, n);
    std::vector<double> t((size_t)dlp::state_doubles(m, n));
    const int32_t* const si = (const int32_t*)(t.data() + (m + 1) * W);
    DeviceGuard guard;
    if (hipSetDevice(batch->opt.device) != hipSuccess ||
        hipMemcpy(t.data(), (const double*)batch->dS + k * dlp::state_doubles(m, n), sizeof(double) * t.size(),
                  hipMemcpyDeviceToHost) != hipSuccess) {
        dlp::set_error(std::string("dlp_batch_read: ") + hipGetErrorString(hipGetLastError()));
        return DLP_ERR_HIP;
    }
    if (basis) std::memcpy(basis, si + n, sizeof(int32_t) * m);
    if (T) {
        // the full layout: slot s is the column of var[s], a basic variable's column the unit
        // vector of its row (objective entry +0.0), the RHS at column N, padding +0.0
        std::fill(T, T + (m + 1) * ld, 0.0);
        for (int64_t i = 0; i <= m; ++i) {
            for (int64_t s = 0; s < n; ++s) T[i * ld + si[s]] = t[i * W + s];
            T[i * ld + N] = t[i * W + n];
        }
        for (int64_t i = 0; i < m; ++i) T[i * ld + si[n + i]] = 1.0;
    }
    return DLP_OK;
}

extern "C" int dlp_batch_info(const dlp_batch* batch, int64_t* nlp, int64_t* m, int64_t* n,
                              int32_t* register_kernel, int64_t* device_bytes) {
    if (!batch) {
        dlp::set_error("dlp_batch_info: bad arguments");
        return DLP_ERR_ARG;
    }
    if (nlp) *nlp = batch->nlp;
    if (m) *m = batch->m;
    if (n) *n = batch->n;
    if (register_kernel) *register_kernel = batch->reg ? 1 : 0;
    if (device_bytes) *device_bytes = batch->bytes;
    return DLP_OK;
}

// The kernel dlp_batch_resolve_rhs runs for this batch (batched_run's choice) and how many LPs one
// CU of the batch's device holds of it: the occupancy query on that very instantiation.
extern "C" int dlp_batch_rhs_kernel(const dlp_batch* batch, int32_t* register_kernel, int32_t* lps_per_cu,
                                    int32_t* threads_per_lp) {
    if (!batch) {
        dlp::set_error("dlp_batch_rhs_kernel: bad arguments");
        return DLP_ERR_ARG;
    }
    using dlp::RhsIn;
    const int64_t m = batch->m, n = batch->n;
    const size_t lds = sizeof(double) * ((m + 1) * (n + 1) + (m + 1) + (n + 1)) + sizeof(int32_t) * (n + m + 8) +
                       sizeof(double) * 2 + 16;
    static const bool force_lds = dlp::env_int("DLP_BATCH_LDS", 0) == 1;
    const int nw = (int)((n + 63) / 64);
    const bool reg = !force_lds && m == 64 && nw >= 1 && nw <= 3 && !rhs_force_lds();
    DeviceGuard guard;
    if (hipSetDevice(batch->opt.device) != hipSuccess) return DLP_ERR_HIP;
    int nb = 0, threads = 0;
    hipError_t e;
    if (reg) {
        threads = 64 * nw;
        e = nw == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dlp::batched_reg_kernel<64, 1, RhsIn>, threads, 0)
          : nw == 2 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dlp::batched_reg_kernel<64, 2, RhsIn>, threads, 0)
                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dlp::batched_reg_kernel<64, 3, RhsIn>, threads, 0);
    } else {
        threads = lds > 40 * 1024 ? 512 : 256;
        e = hipFuncSetAttribute((const void*)dlp::batched_solve_kernel<RhsIn>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dlp::batched_solve_kernel<RhsIn>, threads, lds);
    }
    if (e != hipSuccess) {
        dlp::set_error(std::string("dlp_batch_rhs_kernel: ") + hipGetErrorString(e));
        return DLP_ERR_HIP;
    }
    if (register_kernel) *register_kernel = reg ? 1 : 0;
    if (lps_per_cu) *lps_per_cu = nb;
    if (threads_per_lp) *threads_per_lp = threads;
    return DLP_OK;
}

extern "C" void dlp_batch_free(dlp_batch* batch) {
    if (batch) batch_destroy(batch);
}
