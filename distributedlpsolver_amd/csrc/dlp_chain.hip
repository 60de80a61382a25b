// dlp_chain.hip — the selection chain of the deferred rank-k pivot (the tableau pass that
// applies a block is dlp_pass.hip): the ratio, pivot-row, commit and fused pivot kernels, their
// phase-stamp diagnostics and their launchers.
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
#include <utility>

#include "dlp_host.h"
#include "dlp_internal.h"

namespace dlp {
namespace {

#include "dlp_device.h"
#include "dlp_defer_device.h"

// a1 + a2 (+ a4 single rank) on the replayed column q.  Pricing as in the
// eager ratio_kernel.  Lane i: a = T_j[i][q] by replaying steps 0..j-1 on
// T0[i][q]; C[j][i] = a; the RHS cache advances by step j-1 (or is read from
// T0 when the block is empty); then the ratio candidate.  The objective row
// (local index rows) is current in place: C[j][rows] = z_q.
//
// Latency, not bytes, sets this kernel's time, so everything that does not
// depend on q is requested before the pricing reduce: the lane's whole replay
// chain of coefficients (from Cc, the column-major copy of C, so each load is
// one coalesced 512-B wave access), the RHS inputs, the basis entry, the step
// tables.  Only T0[i][q] and P[l][q] wait for q.  The workgroup partials are
// handed to the last-arriving workgroup without fences: write-through (sc1)
// stores drained by vmcnt(0) before the ticket add, sc1 loads after it
// (MI355X_MICROARCH.md, inter-workgroup visibility, first table row).

// Fused single-rank pivot (pivot_defer_kernel): the workgroup that ends the ratio
// phase (the last arriver, or block 0 when nothing prices in) publishes the
// selection to the pivot-row workgroups of the same launch: st->zq, then an
// agent release and the flag st->go.
__device__ inline void release_go(DevState* st) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(&st->go, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Diagnostics (DLP_CHAIN_STAMPS=<file>, never set in a timed run): wall-clock stamps (100 MHz)
// of the phases of the lookahead chain kernels, one row per pivot (mod 64): ratio kernel
// workgroup 0 at start / q known / T0 and P[l][q] in / replay done / block reduce done /
// ticket taken, the last workgroup at its end; the pivot-row kernel's workgroup 0 at start /
// step table in / replay done / end.  Written by one lane; dumped by the session at free.
__device__ uint64_t g_chain_stamps[64][16];
__device__ int g_chain_stamps_on;
#define CHAIN_STAMP(slot, k)                                                                  \
    do {                                                                                      \
        if (g_chain_stamps_on && threadIdx.x == 0) g_chain_stamps[(slot) & 63][k] = wall_clock64(); \
    } while (0)
// Per-workgroup stamps of one selection per block (slot 40 mod 64; the grouped-ring kernel only):
// start / q known / T0 in / replay done / block reduce done / ticket taken, the CU (HW_ID), and
// wave 0's replayed steps (J - L0).
__device__ uint64_t g_wg_stamps[1024][8];
#define WG_STAMP(slot, k, v)                                                                   \
    do {                                                                                       \
        if (g_chain_stamps_on && threadIdx.x == 0 && ((slot) & 63) == 40 && blockIdx.x < 1024) \
            g_wg_stamps[blockIdx.x][k] = (v);                                                  \
    } while (0)

// LEAN (lookahead beside the form-21 pass): no register-resident chain (coefficients in
// pairs during the replay) and DPP wave minima for the block reductions (round 3: LDS trees),
// 30 VGPRs, so the kernel fits in the 32 VGPRs per SIMD that three pass waves (3 x 160) leave
// free.  Same operations in
// the same order.  (Staging the chain in LDS by LDS-DMA, 32 steps per round trip, measured
// no faster beside the pass: 96 vs 95 us per selection, profiles/r02j/.)
// LEAN, LCH = 0: the coefficient chain streams through a per-wave LDS ring by LDS-DMA, two
// steps per DMA, kRatioRingPairs DMAs in flight (launch-time LDS, kRatioRing bytes: see
// kProwRing).
// (RP = kRatioRingPairs: 16 measured equal at C3, 8,239-8,267 vs 8,262-8,263 pivots/s, profiles/r04c/)
constexpr int kRatioRingPairs = 8;
constexpr size_t ratio_ring_bytes(int rp) { return (size_t)(kRatioDeferThreads / 64) * rp * 128 * sizeof(double); }
// ROWS / RG (the ring only, round 6): ROWS rows per wave (64, 32, 16; 128 / ROWS steps per 1-KB
// DMA, lane x bringing step x / (ROWS / 2) of rows 2 (x % (ROWS / 2)), +1) and RG DMAs retired per
// wait, their LDS reads issued together: one wait and one LDS round trip per 2 RG (ROWS 64) steps
// instead of per pair.  A workgroup of blockDim.x lanes covers blockDim.x ROWS / 64 rows; lanes
// wl >= ROWS hold no row.  ROWS = 64, RG = 1 is the LEAN loop beside the pass.
template <int KMAX, bool FUSED, bool LEAN = false, int LCH = 4, int RP = kRatioRingPairs, bool DB = false,
          int ROWS = 64, int RG = 1>
__device__ __forceinline__ void ratio_defer_body(
    const double* __restrict__ T, int64_t ld, int64_t rows, int64_t rows_elig, int64_t ncols,
    int64_t row_first, int32_t* basis, const PricePart* __restrict__ pp, int ntiles,
    DevState* st, double* __restrict__ C, int64_t ldc, double* __restrict__ Cc, int64_t ldcc,
    const double* __restrict__ P, double* __restrict__ rhs, int32_t* __restrict__ nzc,
    Cand* partials, Cand* cand_out, int nranks, double tol_dj, double tol_piv, int pricing,
    dlp_pivot* log, int64_t log_cap, int nblocks, const double* __restrict__ Ccp = nullptr,
    const double* __restrict__ Pp = nullptr, int prev_seal = -1, const XPeers* xp = nullptr,
    uint32_t xseq = 0, uint32_t* bcnt = nullptr, int brb = 1, int bnt = 0, const double* Tn = nullptr,
    int xsel = 0, uint32_t rseq = 0, Cond cd = Cond{}) {
    // (the grouped ring reads up to 128 / ROWS * (RG + 1) table entries past J - 1, dropped)
    constexpr bool GRING = ROWS != 64 || RG != 1;
    constexpr int kPad = GRING ? 128 / ROWS * (RG + 1) : 0;
    constexpr int kWaves = GRING ? 16 : kRatioDeferThreads / 64;
    __shared__ PricePart lds_pp[kWaves];
    __shared__ Cand lds_c[kWaves];
    __shared__ int s_last;
    __shared__ double s_pq[KMAX + kPad], s_pn[KMAX];
    __shared__ int32_t s_pl[KMAX + kPad];
    auto cand_red = [&](Cand v) { return block_cand(v, lds_c); };
    // this lane's pricing partial is requested first: it depends on nothing, and the reduce
    // below then waits for it alongside the step-table loads instead of after them
    const PricePart pp0 = (int)threadIdx.x < ntiles ? pp[threadIdx.x] : pp_empty();
    if (st->status != DLP_RUNNING) return;
    const int64_t slot = st->npivots;
    if constexpr (LEAN) if (blockIdx.x == 0) CHAIN_STAMP(slot, 0);
    if constexpr (ROWS != 64 || RG != 1) WG_STAMP(slot, 0, wall_clock64());

    // replayed steps: the sealed previous block (lookahead: not yet applied to T, its kp
    // steps first), then this block's j steps; C / Cc / nzc are written at index j
    const int j = st->blk;
    const int kp = prev_seal >= 0 ? st->seal[prev_seal].blk : 0;
    const int J = kp + j;
    const int wl = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the wave's rows [i0, i0 + ROWS); this lane's row i (none: far past every bound)
    const bool lane_row = !GRING || wl < ROWS;
    const int64_t i0 = GRING ? (int64_t)blockIdx.x * (blockDim.x / 64 * ROWS) + wv * ROWS
                             : (int64_t)blockIdx.x * blockDim.x + wv * 64;
    const int64_t i = !GRING ? (int64_t)blockIdx.x * blockDim.x + threadIdx.x
                             : (lane_row ? i0 + wl : ((int64_t)1 << 62));
    for (int l = threadIdx.x; l < J; l += blockDim.x) {
        s_pn[l] = l < kp ? Pp[(int64_t)l * ld + ncols] : P[(int64_t)(l - kp) * ld + ncols];
        s_pl[l] = l < kp ? st->seal[prev_seal].pl[l] : st->pl[l - kp];
    }
    // ring: lanes 0-31 of a DMA bring step 2p, lanes 32-63 step 2p+1, 16 B = two rows each,
    // so the ring slot holds the wave's 64 rows of both steps; Cc does not depend on q, so the
    // first DMAs are issued here and land during the pricing reduce.  Steps past J-1 re-read
    // step J-1 (harmless), so every pair issues exactly one DMA.
    constexpr bool RING = LEAN && LCH == 0;
    constexpr int SPD = 128 / ROWS, HL = ROWS / 2;   // steps per DMA; lanes per step
    extern __shared__ double s_dyn[];
    const bool wave_rows = i0 < rows;   // (i0 + ROWS - 1 < ldcc = round64(rows + 1))
    // band publication (RING): the wave's 64 rows final in Tn (their bands of the sealed
    // block's pass are done): start there and replay this block's steps only
    bool wdone = false;
    if constexpr (LEAN)
        if (bcnt && kp > 0 && i0 + ROWS - 1 < rows) {
            const int64_t b0 = i0 / brb, b1 = (i0 + ROWS - 1) / brb;
            const uint32_t c0 = __hip_atomic_load(&bcnt[b0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t c1 = b1 == b0 ? c0 : __hip_atomic_load(&bcnt[b1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            wdone = __builtin_amdgcn_readfirstlane(c0 == (uint32_t)bnt && c1 == (uint32_t)bnt ? 1 : 0) != 0;
        }
    const int L0 = wdone ? kp : 0;
    auto ring_at = [&](int p) { return s_dyn + (wv * RP + p % RP) * 128; };
    auto sbase = [&](int l) -> const double* {   // wave-uniform: step l's row i0 (l clamped)
        l = l < J ? l : J - 1;
        return (l < kp ? Ccp + (int64_t)l * ldcc : Cc + (int64_t)(l - kp) * ldcc) + i0;
    };
    auto csrc = [&](int p) -> const double* {
        if constexpr (ROWS == 64)
            return ((wl >> 5) ? sbase(L0 + 2 * p + 1) : sbase(L0 + 2 * p)) + 2 * (wl & 31);
        else
            return sbase(L0 + SPD * p + wl / HL) + 2 * (wl % HL);
    };
    if constexpr (RING)
        if (wave_rows && J > L0)
#pragma unroll
            for (int p = 0; p < RP; ++p) glds16(csrc(p), lds_addr(ring_at(p)));
    const int64_t ic = i < rows ? i : rows;   // clamped: loads need no guard
    double f[LEAN ? 1 : KMAX];
    if constexpr (!LEAN) {
#pragma unroll
        for (int l = 0; l < KMAX; ++l)
            f[l] = (l < J) ? (l < kp ? Ccp[(int64_t)l * ldcc + ic] : Cc[(int64_t)(l - kp) * ldcc + ic]) : 0.0;
    }
    auto fld = [&](int l) { return l < kp ? Ccp[(int64_t)l * ldcc + ic] : Cc[(int64_t)(l - kp) * ldcc + ic]; };
    double r_in = 0.0;
    int32_t nz_in = 0, bvar = 0;
    if (i < rows && j > 0) nz_in = nzc[i];
    if (i < rows_elig) {
        r_in = J == 0 ? T[i * ld + ncols] : rhs[i];
        bvar = basis[row_first + i];
    }

    PricePart acc = pp_empty();
    pp_combine(acc, pp0);
    for (int k = threadIdx.x + blockDim.x; k < ntiles; k += blockDim.x) pp_combine(acc, pp[k]);
    acc = block_price(acc, lds_pp);   // (DPP wave minima: LEAN too, within its 32 VGPRs)
    int32_t q;
    if (st->bland)
        q = acc.jbland;
    else
        q = (acc.jmin != kNoIndex && acc.zmin < -tol_dj) ? acc.jmin : kNoIndex;
    if (q == kNoIndex) {
        if constexpr (RING) vmwait<0>();   // no DMA into LDS outlives the wave
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->q = -1;
            st->status = DLP_OK;
            if constexpr (FUSED) release_go(st);
            if (xsel == 2) sel_publish(st, rseq, DLP_OK, 0.0);   // the pivot-row workgroups end too
        }
        return;
    }

    if constexpr (LEAN) if (blockIdx.x == 0) CHAIN_STAMP(slot, 1);
    if constexpr (GRING) WG_STAMP(slot, 1, wall_clock64());
    // condensed tableau: q's slot, and the step (of the replayed sequence: sealed steps first) at
    // which that slot restarted from the unit vector of its new variable (R < 0: none replayed here)
    // (the LCH = 8 tuning instance has no condensed build: its 32 VGPRs are full; the launcher
    // never picks it for a condensed session)
    int32_t sq = q, R = -1;
    if (!(LEAN && LCH == 8) && cd.on) {
        sq = __builtin_amdgcn_readfirstlane(cd.slot_of[q]);
        if (sq < 0 || sq >= ncols) {   // (an invariant: a priced variable is nonbasic) — never fault
            if constexpr (RING) vmwait<0>();
            if (blockIdx.x == 0 && threadIdx.x == 0) st->status = DLP_ERR_STATE;
            return;
        }
        const int32_t rv = __builtin_amdgcn_readfirstlane(cd.rst[sq]);
        if (rv >= 0) {
            if ((rv >> 7) == st->bser)
                R = kp + (rv & 127);
            else if (kp > 0 && (rv >> 7) == st->seal[prev_seal].ser)
                R = rv & 127;
        }
    }
    // T0[i][q] is requested before the P[l][q] loads and their barrier: both wait only for q
    double a = 0.0;
    if (wdone)   // sc1 load (the pass stored Tn write-through)
        a = __builtin_bit_cast(double, __hip_atomic_load((const uint64_t*)(Tn + i * ld + sq), __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT));
    else if (i <= rows)
        a = T[i * ld + sq];
    for (int l = threadIdx.x; l < J; l += blockDim.x)
        s_pq[l] = l < kp ? Pp[(int64_t)l * ld + sq] : P[(int64_t)(l - kp) * ld + sq];
    __syncthreads();
    if constexpr (LEAN) if (blockIdx.x == 0) CHAIN_STAMP(slot, 2);
    if constexpr (GRING) WG_STAMP(slot, 2, wall_clock64());

    Cand c = cand_empty();
    double flast = 0.0;   // LEAN: C of step J-1 (the RHS cache's step)
    if constexpr (RING) {
        // branch-free (the fma is computed and dropped where the eager rule skips it), so
        // the LDS reads of a pair's two steps issue together instead of one per branch
        // (ok = false: a pair's second step past J-1, read from the tables' spare entries and
        // dropped: l <= J <= KMAX - 1)
        // (condensed: at step R the slot's new column starts from the unit vector, +0 here)
        auto step = [&](int l, double fv, bool ok) {
            if (l == R) a = 0.0;   // (uniform; the objective row's lane reloads z_q below)
            const double pq = s_pq[l];
            const bool piv = i == s_pl[l];
            const double u = __builtin_fma(-fv, pq, a);
            a = ok && i < rows ? (piv ? pq : (fv != 0.0 ? u : a)) : a;
            flast = ok ? fv : flast;
        };
        if (wave_rows) {
            const int npairs = (J - L0 + SPD - 1) / SPD;   // (DMAs holding replayed steps)
            if constexpr (!GRING) {
                for (int p = 0; p < npairs; ++p) {
                    vmwait<RP - 1>();   // pair p landed: only ring DMAs issue in this loop
                    double* rs = ring_at(p);
                    const double f0 = rs[wl], f1 = rs[64 + wl];
                    step(L0 + 2 * p, f0, true);
                    step(L0 + 2 * p + 1, f1, L0 + 2 * p + 1 < J);
                    glds16(csrc(p + RP), lds_addr(rs));
                }
            } else {
                // RG DMAs per wait: their LDS reads together, then the SPD RG steps, then RG refills
                // (a group past the last DMA re-reads clamped steps, dropped: every group issues RG)
                const int r = wl % ROWS;
                for (int p0 = 0; p0 < npairs; p0 += RG) {
                    vmwait<RP - RG>();
                    double fq[SPD * RG];
#pragma unroll
                    for (int g = 0; g < RG; ++g) {
                        const double* rs = ring_at(p0 + g);
#pragma unroll
                        for (int k = 0; k < SPD; ++k) fq[g * SPD + k] = rs[k * ROWS + r];
                    }
#pragma unroll
                    for (int u = 0; u < SPD * RG; ++u) step(L0 + SPD * p0 + u, fq[u], L0 + SPD * p0 + u < J);
#pragma unroll
                    for (int g = 0; g < RG; ++g) glds16(csrc(p0 + g + RP), lds_addr(ring_at(p0 + g)));
                }
            }
            vmwait<0>();
            // no step replayed (first selection of a block on a finished band): the RHS cache
            // still advances by the sealed block's last step
            if (npairs == 0 && J > 0 && lane_row) flast = Ccp[(int64_t)(kp - 1) * ldcc + i];
            // (condensed: the restart step zeroed every lane of the wave; the objective row is
            // never replayed, its z_q is current)
            if (R >= L0 && i == rows) a = T[i * ld + sq];
        }
        if (blockIdx.x == 0) CHAIN_STAMP(slot, 3);
        if constexpr (GRING) {
            WG_STAMP(slot, 3, wall_clock64());
            WG_STAMP(slot, 6, (uint64_t)__smid());
            WG_STAMP(slot, 7, (uint64_t)(J - L0));
        }
    } else if constexpr (LEAN) {
        // LCH coefficient loads per round trip (the register budget of this kernel), from the
        // first step not applied to the row's source (L0: a published band starts after the
        // sealed block); the next chunk's loads are issued before this chunk is applied
        // (condensed: a restart of q's slot at R >= L0 starts the replay there from +0)
        const int Ls = R >= L0 ? R : L0;
        if (R >= L0 && i < rows) a = 0.0;
        if (i < rows && J > L0 && !DB) {   // one chunk at a time (LEAN's 32 VGPRs)
            for (int l0 = Ls; l0 < J; l0 += LCH) {
                double fq[LCH];
#pragma unroll
                for (int u = 0; u < LCH; ++u) fq[u] = l0 + u < J ? fld(l0 + u) : 0.0;
#pragma unroll
                for (int u = 0; u < LCH; ++u) {
                    const int l = l0 + u;
                    const double fv = fq[u];
                    if (l < J) {
                        if (i == s_pl[l])
                            a = s_pq[l];
                        else if (fv != 0.0)
                            a = __builtin_fma(-fv, s_pq[l], a);
                        flast = fv;
                    }
                }
            }
        } else if (i < rows && J > L0) {   // DB (MID): double-buffered
            double fa[LCH], fb[LCH];
            auto fetch = [&](double (&fq)[LCH], int l0) {
#pragma unroll
                for (int u = 0; u < LCH; ++u) fq[u] = l0 + u < J ? fld(l0 + u) : 0.0;
            };
            auto apply = [&](const double (&fq)[LCH], int l0) {
#pragma unroll
                for (int u = 0; u < LCH; ++u) {
                    const int l = l0 + u;
                    const double fv = fq[u];
                    if (l < J) {
                        if (i == s_pl[l])
                            a = s_pq[l];
                        else if (fv != 0.0)
                            a = __builtin_fma(-fv, s_pq[l], a);
                        flast = fv;
                    }
                }
            };
            fetch(fa, Ls);
            for (int l0 = Ls; l0 < J; l0 += 2 * LCH) {
                if (l0 + LCH < J) fetch(fb, l0 + LCH);
                apply(fa, l0);
                if (l0 + LCH >= J) break;
                if (l0 + 2 * LCH < J) fetch(fa, l0 + 2 * LCH);
                apply(fb, l0 + LCH);
            }
        } else if (i < rows && J > 0 && L0 == J) {
            flast = Ccp[(int64_t)(kp - 1) * ldcc + i];   // nothing replayed: the RHS cache's step
        }
        if (blockIdx.x == 0) CHAIN_STAMP(slot, 3);
    }
    if (i <= rows) {
        if (i < rows) {
            if constexpr (!LEAN) {   // (LEAN replayed above)
#pragma unroll
                for (int l = 0; l < KMAX; ++l) {
                    if (l < J) {
                        if (l == R) a = 0.0;
                        if (i == s_pl[l])
                            a = s_pq[l];
                        else if (f[l] != 0.0)
                            a = __builtin_fma(-f[l], s_pq[l], a);
                    }
                }
            }
        }
        C[i * ldc + j] = a;
        // block start: the row's coefficients of steps 1..K-1 := +0, so a pass over a partial
        // block (kb < K steps) runs the full-block code: P[l >= kb] is +0 too (commit_row),
        // and fma(-(+0), +0, t) = t + (-0) = t for every t
        if (j == 0)
            for (int64_t l = 1; l < ldc; ++l) C[i * ldc + l] = 0.0;
        Cc[(int64_t)j * ldcc + i] = a;
        if (i < rows) nzc[i] = (j == 0 ? 0 : nz_in) + (a != 0.0 ? 1 : 0);   // the pass's row class
        if (i < rows_elig) {
            double r = r_in;
            if (J > 0) {
                const int l = J - 1;
                double fp = 0.0;   // f[j-1], selected without dynamic register indexing
                if constexpr (LEAN) {
                    fp = flast;
                } else {
#pragma unroll
                    for (int u = 0; u < KMAX; ++u) fp = (u == l) ? f[u] : fp;
                }
                if (i == s_pl[l])
                    r = s_pn[l];
                else if (fp != 0.0)
                    r = __builtin_fma(-fp, s_pn[l], r);
            }
            rhs[i] = r;
            if (a > tol_piv) {
                double b = r;
                if (!(b > 0.0)) b = 0.0;
                c.ratio = b / a;
                c.row = (int32_t)(row_first + i);
                c.basis_var = bvar;
                c.valid = 1;
                c.pivot = a;
            }
        }
    }
    c = cand_red(c);
    if constexpr (LEAN) if (blockIdx.x == 0) CHAIN_STAMP(slot, 4);
    if constexpr (GRING) WG_STAMP(slot, 4, wall_clock64());
    if (xp && xsel) {
        // peer exchange, selection in this launch: every workgroup's candidate straight into slot
        // [seq & 1][me][blockIdx] of every rank (no partials, no ticket); workgroup 0 of every rank
        // waits for all of them, reduces them in the candidate order and selects (every rank
        // reaches the same p).  A workgroup's reads of the state are done before it pushes, so the
        // selection never races them.
        if (threadIdx.x == 0) x_push_cand(xp, xseq, c, (int)blockIdx.x);
        if (blockIdx.x != 0) return;
        __shared__ int s_xok;
        Cand w;
        if (!x_gather_all(xp, xseq, &w, &s_xok)) {
            if (threadIdx.x == 0) {
                st->status = kStatusXFail;
                if (xsel == 2) sel_publish(st, rseq, kStatusXFail, 0.0);
            }
            return;
        }
        w = cand_red(w);
        if (threadIdx.x == 0) {
            // one-launch pivot: z_q (the objective row is current; this launch's commit writes it
            // only after the record) before the selection, which writes the log entry's other fields
            const double zq = xsel == 2 ? T[rows * ld + sq] : 0.0;
            st->sq = sq;
            do_select(st, w, q, basis, row_first, rows, pricing, log, log_cap, true, xsel != 2, cd);
            if (xsel == 2) sel_publish(st, rseq, st->status, zq);
        }
        if constexpr (LEAN) CHAIN_STAMP(slot, 6);
        return;
    }

    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)partials, (short)0, (int)(nblocks * sizeof(Cand)), 0x00020000);
    if (threadIdx.x == 0) {
        const u4v* cv = (const u4v*)&c;
        __builtin_amdgcn_raw_buffer_store_b128(cv[0], prs, (int)(blockIdx.x * sizeof(Cand)), 0, kAuxSc1);
        __builtin_amdgcn_raw_buffer_store_b128(cv[1], prs, (int)(blockIdx.x * sizeof(Cand)) + 16, 0,
                                               kAuxSc1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned prev =
            __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (prev == (unsigned)nblocks - 1);
    }
    __syncthreads();
    if constexpr (LEAN) if (blockIdx.x == 0) CHAIN_STAMP(slot, 5);
    if constexpr (GRING) WG_STAMP(slot, 5, wall_clock64());
    if (!s_last) return;
    Cand best = cand_empty();
    for (int k = threadIdx.x; k < nblocks; k += blockDim.x) {
        Cand o;
        u4v* ov = (u4v*)&o;
        ov[0] = __builtin_amdgcn_raw_buffer_load_b128(prs, (int)(k * sizeof(Cand)), 0, kAuxSc1);
        ov[1] = __builtin_amdgcn_raw_buffer_load_b128(prs, (int)(k * sizeof(Cand)) + 16, 0, kAuxSc1);
        if (cand_better(o, best)) best = o;
    }
    best = cand_red(best);
    if (threadIdx.x == 0) {
        st->ticket = 0;
        st->q = q;
        st->sq = sq;
        if (nranks == 1)
            do_select(st, best, q, basis, row_first, rows, pricing, log, log_cap, true, true, cd);
        else if (xp)
            x_push_cand(xp, xseq, best);   // peer exchange: straight into every rank's slot
        else
            cand_out[0] = best;
        if constexpr (FUSED) {
            st->zq = T[rows * ld + sq];   // the objective row is current; nobody writes it yet
            release_go(st);
        }
    }

    if constexpr (LEAN) CHAIN_STAMP(slot, 6);
}

template <int KMAX>
__global__ __launch_bounds__(kRatioDeferThreads) void ratio_defer_kernel(
    const double* __restrict__ T, int64_t ld, int64_t rows, int64_t rows_elig, int64_t ncols,
    int64_t row_first, int32_t* basis, const PricePart* __restrict__ pp, int ntiles,
    DevState* st, double* __restrict__ C, int64_t ldc, double* __restrict__ Cc, int64_t ldcc,
    const double* __restrict__ P, double* __restrict__ rhs, int32_t* __restrict__ nzc,
    Cand* partials, Cand* cand_out, int nranks, double tol_dj, double tol_piv, int pricing,
    dlp_pivot* log, int64_t log_cap, const double* __restrict__ Ccp, const double* __restrict__ Pp,
    int prev_seal, const XPeers* xp, uint32_t xseq, int xsel, Cond cd) {
    ratio_defer_body<KMAX, false>(T, ld, rows, rows_elig, ncols, row_first, basis, pp, ntiles, st, C,
                                  ldc, Cc, ldcc, P, rhs, nzc, partials, cand_out, nranks, tol_dj,
                                  tol_piv, pricing, log, log_cap, (int)gridDim.x, Ccp, Pp, prev_seal,
                                  xp, xseq, nullptr, 1, 0, nullptr, xsel, 0, cd);
}

// MID (round 5): beside the MFMA pass (form 22 leaves 104 VGPRs per SIMD), the replay's
// coefficients in registers, LCH per round trip, double-buffered, no LDS ring.
template <int KMAX, int LCH>
__global__ __launch_bounds__(kRatioDeferThreads) __attribute__((amdgpu_num_vgpr(104))) void ratio_mid_kernel(
    const double* __restrict__ T, int64_t ld, int64_t rows, int64_t rows_elig, int64_t ncols,
    int64_t row_first, int32_t* basis, const PricePart* __restrict__ pp, int ntiles,
    DevState* st, double* __restrict__ C, int64_t ldc, double* __restrict__ Cc, int64_t ldcc,
    const double* __restrict__ P, double* __restrict__ rhs, int32_t* __restrict__ nzc,
    Cand* partials, Cand* cand_out, int nranks, double tol_dj, double tol_piv, int pricing,
    dlp_pivot* log, int64_t log_cap, const double* __restrict__ Ccp, const double* __restrict__ Pp,
    int prev_seal, const XPeers* xp, uint32_t xseq, uint32_t* bcnt, int brb, int bnt, const double* Tn,
    int xsel, Cond cd) {
    ratio_defer_body<KMAX, false, true, LCH, kRatioRingPairs, true>(T, ld, rows, rows_elig, ncols, row_first, basis, pp, ntiles, st, C,
                                             ldc, Cc, ldcc, P, rhs, nzc, partials, cand_out, nranks, tol_dj,
                                             tol_piv, pricing, log, log_cap, (int)gridDim.x, Ccp, Pp, prev_seal,
                                             xp, xseq, bcnt, brb, bnt, Tn, xsel, 0, cd);
}

// The LEAN selection kernel, held to 32 VGPRs (lookahead at K = 64, beside the pass).
template <int KMAX, int LCH, int RP = kRatioRingPairs>
__global__ __launch_bounds__(kRatioDeferThreads) __attribute__((amdgpu_num_vgpr(32))) void ratio_lean_kernel(
    const double* __restrict__ T, int64_t ld, int64_t rows, int64_t rows_elig, int64_t ncols,
    int64_t row_first, int32_t* basis, const PricePart* __restrict__ pp, int ntiles,
    DevState* st, double* __restrict__ C, int64_t ldc, double* __restrict__ Cc, int64_t ldcc,
    const double* __restrict__ P, double* __restrict__ rhs, int32_t* __restrict__ nzc,
    Cand* partials, Cand* cand_out, int nranks, double tol_dj, double tol_piv, int pricing,
    dlp_pivot* log, int64_t log_cap, const double* __restrict__ Ccp, const double* __restrict__ Pp,
    int prev_seal, const XPeers* xp, uint32_t xseq, uint32_t* bcnt, int brb, int bnt, const double* Tn,
    int xsel, Cond cd) {
    ratio_defer_body<KMAX, false, true, LCH, RP>(T, ld, rows, rows_elig, ncols, row_first, basis, pp, ntiles, st, C,
                                        ldc, Cc, ldcc, P, rhs, nzc, partials, cand_out, nranks, tol_dj,
                                        tol_piv, pricing, log, log_cap, (int)gridDim.x, Ccp, Pp, prev_seal,
                                        xp, xseq, bcnt, brb, bnt, Tn, xsel, 0, cd);
}

// The grouped ring (round 6): the selection kernel of a chain on CUs of its own (the lookahead's
// disjoint CU masks: no pass waves beside it, so no 32-VGPR budget).  ROWS rows per wave, RP DMAs
// in flight, RG retired per wait (tools/chainlab.hip, profiles/r06q/-r06s/).  Launched with
// rthreads x 64 / ROWS lanes, so a workgroup covers the session's rthreads rows and the grid, the
// partials and the exchange's candidate slots are those of every other ratio kernel.
template <int ROWS, int RP, int RG>
__global__ __launch_bounds__(1024) void ratio_ring_kernel(
    const double* __restrict__ T, int64_t ld, int64_t rows, int64_t rows_elig, int64_t ncols,
    int64_t row_first, int32_t* basis, const PricePart* __restrict__ pp, int ntiles,
    DevState* st, double* __restrict__ C, int64_t ldc, double* __restrict__ Cc, int64_t ldcc,
    const double* __restrict__ P, double* __restrict__ rhs, int32_t* __restrict__ nzc,
    Cand* partials, Cand* cand_out, int nranks, double tol_dj, double tol_piv, int pricing,
    dlp_pivot* log, int64_t log_cap, const double* __restrict__ Ccp, const double* __restrict__ Pp,
    int prev_seal, const XPeers* xp, uint32_t xseq, uint32_t* bcnt, int brb, int bnt, const double* Tn,
    int xsel, Cond cd) {
    ratio_defer_body<128, false, true, 0, RP, false, ROWS, RG>(
        T, ld, rows, rows_elig, ncols, row_first, basis, pp, ntiles, st, C, ldc, Cc, ldcc, P, rhs, nzc, partials,
        cand_out, nranks, tol_dj, tol_piv, pricing, log, log_cap, (int)gridDim.x, Ccp, Pp, prev_seal, xp, xseq, bcnt,
        brb, bnt, Tn, xsel, 0, cd);
}

// commit_row: P[s] := pr for columns j, j+1; objective row z -= z_q * P[s] (z_q != 0);
// pricing partial of this 512-column tile (pp[tile]); objective value into log[klog].
// Same per-element operations as the eager update kernel's objective band.
// ZQ: 0 = z_q from C[rows][s]; 1 = the caller's early loads of T[rows][j..j+1] (zpre) and z_q
// (zqv); 2 = z_q given (zqv: the selection record of a one-launch pivot), z loaded here
// Condensed tableau (cd.on): slot sq is the entering variable's, now the leaving variable's: its
// objective entry restarts from +0 (a basic column's), its restart is recorded (rst, block
// serial bser, step s) and its entries of the block's earlier pivot rows become +0 (the pass
// starts the slot from the unit vector written by reset_cols); pricing by variable (var_of).
// (commit_row itself: dlp_defer_device.h, shared with the deferred dual chain of dlp_dual.hip)

// a3 first half on the replayed pivot row: T_s[p] = steps 0..s-1 applied to
// T0[p], divided by the pivot element (IEEE division).  fused (single rank):
// commit_row as well.  Otherwise the owner writes the fp64 bits and every
// other rank INT64_MIN for the int64 MAX exchange.
constexpr int kProwRingSteps = 8;   // (RS: 16 measured equal, with the ratio ring's 16)
constexpr size_t prow_ring_bytes(int rs) { return (size_t)4 * rs * 128 * sizeof(double); }
// PG (the ring only, round 6): pivot rows retired per wait, their LDS reads issued together (PG = 1:
// one wait and one LDS round trip per row, the 32-VGPR kernel beside the pass)
template <bool LEAN, int RS = kProwRingSteps, int CHR = 16, int PG = 1>
__device__ __forceinline__ void prow_defer_body(
    double* __restrict__ T, int64_t ld, int64_t rows, int64_t ncols, int64_t nprice,
    const DevState* st, const double* __restrict__ C, int64_t ldc, double* __restrict__ P,
    int64_t* __restrict__ bits, PricePart* pp, double tol_dj, dlp_pivot* log, int64_t log_cap,
    int fused, const double* __restrict__ Cp, const double* __restrict__ Pp, int prev_seal,
    const XPeers* xp, uint32_t xseq, uint32_t* bcnt, int brb, int bnt, const double* Tn, int xcommit,
    int tile, int onelaunch = 0, Cond cd = Cond{}) {
    __shared__ PricePart lds_pp[4];
    __shared__ SelView s_sel;
    __shared__ int s_selok;
    __shared__ double s_cp[kMaxReplay + (PG > 1 ? PG : 0)];   // (a group past S - 1 reads spares, dropped)
    __shared__ int32_t s_pl[kMaxReplay + (PG > 1 ? PG : 0)];
    // LEAN: the replayed pivot rows stream through a per-wave LDS ring by LDS-DMA, RING steps
    // in flight (each lane's own 16 B of a row land at ring + 16 lane), instead of 4 rows per
    // round trip in the 32 VGPRs this kernel has beside the pass
    // (launch-time LDS, kProwRing bytes: static LDS of that size makes hipcc's descriptor ask for
    // the VGPRs its LDS-bound occupancy would leave, 176, and the kernel no longer fits beside
    // the pass)
    constexpr int RING = RS;
    extern __shared__ double s_dyn[];
    auto s_ring = reinterpret_cast<double(*)[RING][128]>(s_dyn);
    if (st->status != DLP_RUNNING) return;   // an earlier launch ended the solve
    // the selection: from the state (a launch of its own), or, in a one-launch pivot (peer
    // exchange), from the record the ratio workgroups of this launch publish (DevState::SelRec)
    SelView sv;
    if (onelaunch) {
        if (!sel_wait(xp, st, xseq, &sv, &s_sel, &s_selok)) {
            if (threadIdx.x == 0) const_cast<DevState*>(st)->status = kStatusXFail;   // (writable memory)
            return;
        }
        if (sv.status != DLP_RUNNING) return;
    } else {
        sv.status = DLP_RUNNING;
        sv.p_local = st->p_local;
        sv.blk = st->blk;
        sv.piv = st->piv;
        sv.zq = 0.0;
        sv.npivots = st->npivots;
        sv.sq = -1;
    }
    const int64_t slot = sv.npivots - 1;
    if constexpr (LEAN) if (tile == 0) CHAIN_STAMP(slot, 8);
    const int s = sv.blk - 1;
    // replayed steps: the sealed previous block first (lookahead), then this block's s
    const int kp = prev_seal >= 0 ? st->seal[prev_seal].blk : 0;
    const int S = kp + s;
    const int32_t pl = sv.p_local;
    const int64_t j = ((int64_t)tile * blockDim.x + threadIdx.x) * 2;
    const bool owner_lane = pl >= 0 && j < ld;
    // LEAN, band publication: row p final in Tn (its band of the sealed block's pass is done):
    // start there and replay this block's steps only
    bool pdone = false;
    if (bcnt && kp > 0 && pl >= 0)
            pdone = __builtin_amdgcn_readfirstlane(
                        __hip_atomic_load(&bcnt[pl / brb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == (uint32_t)bnt;
    const int L0 = pdone ? kp : 0;
    // the ring's first RING rows are requested first (they depend on nothing but the step
    // counts); rows past the last step re-read it (harmless), so every step issues one DMA
    auto psrc = [&](int l) -> const double* {
        l = l < S ? l : S - 1;
        return (l < kp ? Pp + (int64_t)l * ld : P + (int64_t)(l - kp) * ld) + j;
    };
    const int wv = threadIdx.x >> 6, wl = threadIdx.x & 63;
    if constexpr (LEAN)
        if (owner_lane && S > L0)
#pragma unroll
            for (int r = 0; r < RING; ++r) glds16(psrc(L0 + r), lds_addr(&s_ring[wv][(L0 + r) % RING][0]));
    // everything that depends only on (p, s) is requested before the step-table barrier:
    // T0[p][j..j+1] and, for the fused commit, the objective row and z_q
    d2 t0 = d2{0.0, 0.0}, zpre = d2{0.0, 0.0};
    double zqpre = 0.0;
    if (pdone && j < ld) {   // sc1 loads (the pass stored Tn write-through)
        const uint64_t* tn = (const uint64_t*)(Tn + (int64_t)pl * ld + j);
        const double x0 = __builtin_bit_cast(double, __hip_atomic_load(tn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const double x1 = __builtin_bit_cast(double, __hip_atomic_load(tn + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        t0.x = x0;
        t0.y = x1;
    } else if (pl >= 0 && j < ld) {
        t0 = *(const d2*)(T + (int64_t)pl * ld + j);
    }
    // condensed tableau: the lane's two slots' restarts (the step of the replayed sequence at which
    // each restarts from +0, -1: none here) and the entering slot (its entry of row p is the
    // leaving variable's unit 1)
    int32_t Rx = -1, Ry = -1, sq = -1;
    if (cd.on) {
        sq = onelaunch ? sv.sq : st->sq;   // (one launch: the record's, published with the selection)
        if (owner_lane) {
            const int bs = st->bser, ss = kp > 0 ? st->seal[prev_seal].ser : -2;
            // (a sealed-block restart matters only where row p is replayed through the sealed
            // block: a published row p already holds its result)
            auto rof = [&](int32_t rv) -> int32_t {
                if (rv < 0) return -1;
                if ((rv >> 7) == bs) return kp + (rv & 127);
                return (!pdone && (rv >> 7) == ss) ? (rv & 127) : -1;
            };
            Rx = rof(cd.rst[j]);
            Ry = rof(cd.rst[j + 1]);
        }
    }
    // The restarts: inside the replay loops (the slot's value becomes +0 at its restart step), or,
    // in the MID instance (CHR 8), whose registers are budgeted beside the MFMA pass, after the
    // loop: a restarted slot is replayed again from +0 at its restart step, its pivot rows from
    // global memory.  Then the entering slot's entry is the leaving variable's unit 1.
    constexpr bool kFixAfter = !LEAN && CHR == 8;
    auto cond_fix = [&](d2& t) {
        if (kFixAfter && (Rx >= 0 || Ry >= 0)) {
            const int r0 = Rx < 0 ? Ry : (Ry < 0 ? Rx : min(Rx, Ry));
            if (Rx >= 0) t.x = 0.0;
            if (Ry >= 0) t.y = 0.0;
            for (int l = r0; l < S; ++l) {
                const d2 pv = *(const d2*)((l < kp ? Pp + (int64_t)l * ld : P + (int64_t)(l - kp) * ld) + j);
                const double cp = s_cp[l];
                const bool piv = pl == s_pl[l];
                if (Rx >= 0 && l >= Rx) t.x = piv ? pv.x : (cp != 0.0 ? __builtin_fma(-cp, pv.x, t.x) : t.x);
                if (Ry >= 0 && l >= Ry) t.y = piv ? pv.y : (cp != 0.0 ? __builtin_fma(-cp, pv.y, t.y) : t.y);
            }
        }
        if (j == sq) t.x = 1.0;
        if (j + 1 == sq) t.y = 1.0;
    };
    if (fused && !LEAN) {   // (LEAN: within the 32 VGPRs that let it run beside the pass)
        zqpre = C[rows * ldc + s];
        if (j < ((ncols + 16) & ~(int64_t)15)) zpre = *(const d2*)(T + rows * ld + j);
    }
    if (pl >= 0)
        for (int l = threadIdx.x; l < S; l += blockDim.x) {
            s_cp[l] = l < kp ? Cp[(int64_t)pl * ldc + l] : C[(int64_t)pl * ldc + (l - kp)];
            s_pl[l] = l < kp ? st->seal[prev_seal].pl[l] : st->pl[l - kp];
        }
    __syncthreads();
    if constexpr (LEAN) if (tile == 0) CHAIN_STAMP(slot, 9);
    d2 pr;
    pr.x = 0.0;
    pr.y = 0.0;
    if (owner_lane && LEAN) {
        d2 t = t0;
        asm volatile("" ::"v"(t.x), "v"(t.y));   // T0[p] in here (hipcc's own wait), not in the loop
        if constexpr (PG == 1) {
            for (int l = L0; l < S; ++l) {
                vmwait<RING - 1>();   // step l's DMA retired: only ring DMAs issue in this loop
                const d2 pv = *(const d2*)&s_ring[wv][l % RING][2 * wl];
                const double cp = s_cp[l];
                const bool piv = pl == s_pl[l];
                if (l == Rx) t.x = 0.0;
                if (l == Ry) t.y = 0.0;
                const double ux = __builtin_fma(-cp, pv.x, t.x), uy = __builtin_fma(-cp, pv.y, t.y);
                t.x = piv ? pv.x : (cp != 0.0 ? ux : t.x);   // (branch-free, as the ratio ring's step)
                t.y = piv ? pv.y : (cp != 0.0 ? uy : t.y);
                glds16(psrc(l + RING), lds_addr(&s_ring[wv][l % RING][0]));
            }
        } else {
            // PG rows per wait: their LDS reads together, then the PG steps, then PG refills (a group
            // past S - 1 reads clamped rows and drops them: every group issues PG DMAs)
            for (int l0 = L0; l0 < S; l0 += PG) {
                vmwait<RING - PG>();
                d2 pv[PG];
#pragma unroll
                for (int g = 0; g < PG; ++g) pv[g] = *(const d2*)&s_ring[wv][(l0 + g) % RING][2 * wl];
#pragma unroll
                for (int g = 0; g < PG; ++g) {
                    const int l = l0 + g;
                    const double cp = s_cp[l];
                    const bool piv = pl == s_pl[l];
                    const bool ok = l < S;
                    if (l == Rx) t.x = 0.0;
                    if (l == Ry) t.y = 0.0;
                    const double ux = __builtin_fma(-cp, pv[g].x, t.x), uy = __builtin_fma(-cp, pv[g].y, t.y);
                    t.x = ok ? (piv ? pv[g].x : (cp != 0.0 ? ux : t.x)) : t.x;
                    t.y = ok ? (piv ? pv[g].y : (cp != 0.0 ? uy : t.y)) : t.y;
                }
#pragma unroll
                for (int g = 0; g < PG; ++g) glds16(psrc(l0 + g + RING), lds_addr(&s_ring[wv][(l0 + g) % RING][0]));
            }
        }
        vmwait<0>();   // the ring drained (the clamped tail DMAs) before the block exits
        if (cd.on) cond_fix(t);
        const double piv = sv.piv;
        pr.x = t.x / piv;
        pr.y = t.y / piv;
    } else if (owner_lane) {
        d2 t = t0;
        // chunks of CH pivot rows (row index clamped), double-buffered: the next chunk's loads are
        // issued before this chunk is applied, so up to 2 CH rows are in flight (c3r8: the replay
        // was 7 us per pivot with one chunk of 8 in flight, profiles/r04e/)
        constexpr int CH = CHR;
        d2 pa[CH], pb[CH];
        auto fetch = [&](d2 (&pv)[CH], int l0) {
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int l = min(l0 + u, S - 1);
                pv[u] = *(const d2*)((l < kp ? Pp + (int64_t)l * ld : P + (int64_t)(l - kp) * ld) + j);
            }
        };
        auto apply = [&](const d2 (&pv)[CH], int l0) {
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int l = l0 + u;
                if (l < S) {
                    if (!kFixAfter && l == Rx) t.x = 0.0;
                    if (!kFixAfter && l == Ry) t.y = 0.0;
                    if (pl == s_pl[l]) {
                        t = pv[u];
                    } else if (s_cp[l] != 0.0) {
                        t.x = __builtin_fma(-s_cp[l], pv[u].x, t.x);
                        t.y = __builtin_fma(-s_cp[l], pv[u].y, t.y);
                    }
                }
            }
        };
        if (S > L0) fetch(pa, L0);
        for (int l0 = L0; l0 < S; l0 += 2 * CH) {
            if (l0 + CH < S) fetch(pb, l0 + CH);
            apply(pa, l0);
            if (l0 + CH >= S) break;
            if (l0 + 2 * CH < S) fetch(pa, l0 + 2 * CH);
            apply(pb, l0 + CH);
        }
        if (cd.on) cond_fix(t);
        const double piv = sv.piv;
        pr.x = t.x / piv;
        pr.y = t.y / piv;
    }
    if constexpr (LEAN) if (tile == 0) CHAIN_STAMP(slot, 10);
    if (!fused && xp) {   // peer exchange: the owner's row into every rank's row region
        // (scalars first: hipcc of ROCm 7.2 compiles __builtin_bit_cast(T, v.y) of an
        // ext_vector element as a cast of element 0; tests/test_isa.py guards this site)
        const double px = pr.x, py = pr.y;
        if (pl >= 0)      // (uniform per launch)
            x_push_row_chunk(xp, xseq, j, ld, __builtin_bit_cast(uint64_t, px),
                             __builtin_bit_cast(uint64_t, py), tile);
        if constexpr (LEAN) if (tile == 0) CHAIN_STAMP(slot, 11);
        if (!xcommit) return;
        // the commit in this launch (no commit launch): the owner commits the row it holds, every
        // other rank waits for this chunk's flag and reads the chunk from its own row region
        if (pl < 0) {
            __shared__ int s_xok;
            if (threadIdx.x == 0) s_xok = x_wait(xp, x_rflag(xp, xp->me, tile), xseq) ? 1 : 0;
            __syncthreads();
            if (!s_xok) {
                if (threadIdx.x == 0) const_cast<DevState*>(st)->status = kStatusXFail;   // (st is writable memory)
                return;
            }
            if (j < ld) {
                uint64_t a = 0, b = 0;
                x_read_row_pair(xp, j, &a, &b);
                pr.x = __builtin_bit_cast(double, a);
                pr.y = __builtin_bit_cast(double, b);
            }
        }
        if constexpr (LEAN) if (tile == 0) CHAIN_STAMP(slot, 13);
        if (onelaunch)   // z_q from the record (C[rows][s] is another workgroup's store of this launch)
            commit_row<2>(T, ld, rows, ncols, nprice, slot, C, ldc, P, s, j, pr, pp, tile, tol_dj, log, log_cap,
                          lds_pp, d2{0.0, 0.0}, sv.zq, cd, sq, cd.on ? st->bser : 0);
        else
            commit_row(T, ld, rows, ncols, nprice, slot, C, ldc, P, s, j, pr, pp, tile, tol_dj, log, log_cap, lds_pp,
                       d2{0.0, 0.0}, 0.0, cd, sq, cd.on ? st->bser : 0);
        if constexpr (LEAN) if (tile == 0) CHAIN_STAMP(slot, 14);
        return;
    }
    if (!fused) {
        if (j < ld) {
            if (pl >= 0) {
                *(d2*)(bits + j) = pr;   // the fp64 bits, as int64
            } else {
                bits[j] = INT64_MIN;
                bits[j + 1] = INT64_MIN;
            }
        }
        return;
    }
    commit_row<LEAN ? 0 : 1>(T, ld, rows, ncols, nprice, slot, C, ldc, P, s, j, pr, pp, tile, tol_dj, log,
                             log_cap, lds_pp, zpre, zqpre, cd, sq, cd.on ? st->bser : 0);
    if constexpr (LEAN) if (tile == 0) CHAIN_STAMP(slot, 11);
}
#define DLP_PROW_ARGS                                                                              \
    double *__restrict__ T, int64_t ld, int64_t rows, int64_t ncols, int64_t nprice, const DevState *st, \
        const double *__restrict__ C, int64_t ldc, double *__restrict__ P, int64_t *__restrict__ bits,  \
        PricePart *pp, double tol_dj, dlp_pivot *log, int64_t log_cap, int fused,                    \
        const double *__restrict__ Cp, const double *__restrict__ Pp, int prev_seal, const XPeers *xp, \
        uint32_t xseq, uint32_t *bcnt, int brb, int bnt, const double *Tn, int xcommit, Cond cd
#define DLP_PROW_PASS T, ld, rows, ncols, nprice, st, C, ldc, P, bits, pp, tol_dj, log, log_cap, fused, Cp, Pp, \
                      prev_seal, xp, xseq, bcnt, brb, bnt, Tn, xcommit, (int)blockIdx.x, 0, cd
// The LEAN instance (lookahead at K = 64, beside the form-21 pass) is held to 32 VGPRs in its
// kernel descriptor: the pass leaves 32 per SIMD (with the LDS-DMA asm, hipcc's descriptor
// otherwise requested 176 for a body that uses 30, and the kernel could not share a CU).
template <bool LEAN = false>
__global__ __launch_bounds__(256) void prow_defer_kernel(DLP_PROW_ARGS) {
    prow_defer_body<false>(DLP_PROW_PASS);
}
template <int RS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(32))) void prow_lean_kernel(DLP_PROW_ARGS) {
    prow_defer_body<true, RS>(DLP_PROW_PASS);
}
// The grouped ring (round 6): the pivot-row kernel of a chain on CUs of its own, RS rows in flight,
// PG retired per wait (no 32-VGPR budget: no pass waves beside it)
template <int RS, int PG>
__global__ __launch_bounds__(256) void prow_ring_kernel(DLP_PROW_ARGS) {
    prow_defer_body<true, RS, 16, PG>(DLP_PROW_PASS);
}
// MID (round 5): beside the MFMA pass (form 22: 3 waves x 136 VGPRs per SIMD leave 104), the
// register replay of the fat kernel with 2 x 8 pivot rows in flight instead of 2 x 16, and no
// LDS ring (the MFMA pass stages its coefficients through LDS).
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(104))) void prow_mid_kernel(DLP_PROW_ARGS) {
    prow_defer_body<false, kProwRingSteps, 8>(DLP_PROW_PASS);
}
#undef DLP_PROW_ARGS
#undef DLP_PROW_PASS

// Peer exchange, one launch per pivot (dlp::launch_pivot_x): workgroups [0, nrat) run the ratio
// test and the selection (every workgroup pushes its candidate to every rank, workgroup 0 reduces
// all of them, selects and publishes the selection record); workgroups [nrat, nrat + nprow) are the
// pivot-row workgroups, which wait for the record, replay and push the owner's row and commit it.
// Workgroups are dispatched in index order, so the ratio workgroups never wait for a slot behind
// the pivot-row workgroups that wait for them.  LEAN: beside the form-21 pass (32 VGPRs; both
// bodies' LDS rings are the same size).
#define DLP_PX_RATIO_ARGS                                                                                       \
    double *__restrict__ T, int64_t ld, int64_t rows, int64_t rows_elig, int64_t ncols, int64_t nprice,         \
        int64_t row_first, int32_t *basis, PricePart *pp, int ntiles, DevState *st, double *__restrict__ C,     \
        int64_t ldc, double *__restrict__ Cc, int64_t ldcc, double *__restrict__ P, double *__restrict__ rhs,   \
        int32_t *__restrict__ nzc, int nrat, double tol_dj, double tol_piv, int pricing, dlp_pivot *log,         \
        int64_t log_cap, const double *__restrict__ Ccp, const double *__restrict__ Pp,                          \
        const double *__restrict__ Cp, int prev_seal, const XPeers *xp, uint32_t xseq, uint32_t *bcnt, int brb, \
        int bnt, const double *Tn, int xs, Cond cd
// (xs = 2, passed at launch: as a compile-time constant hipcc gave the LEAN instance 34 VGPRs, at
// run time 30 of the 32 the form-21 pass leaves per SIMD)
#define DLP_PX_BODIES(KM, LEAN_, LCH_, RP_, RS_, CD_)                                                               \
    if ((int)blockIdx.x < nrat) {                                                                                \
        ratio_defer_body<KM, false, LEAN_, LCH_, RP_>(T, ld, rows, rows_elig, ncols, row_first, basis, pp,       \
                                                     ntiles, st, C, ldc, Cc, ldcc, P, rhs, nzc, nullptr,          \
                                                     nullptr, 2, tol_dj, tol_piv, pricing, log, log_cap, nrat,    \
                                                     Ccp, Pp, prev_seal, xp, xseq, bcnt, brb, bnt, Tn, xs, xseq, CD_); \
        return;                                                                                                  \
    }                                                                                                            \
    prow_defer_body<LEAN_, RS_>(T, ld, rows, ncols, nprice, st, C, ldc, P, nullptr, pp,      \
                                tol_dj, log, log_cap, 0, Cp, Pp, prev_seal, xp, xseq, bcnt, brb, bnt, Tn, 1,     \
                                (int)blockIdx.x - nrat, 1, CD_)
template <int KMAX>
__global__ __launch_bounds__(256) void pivot_x_kernel(DLP_PX_RATIO_ARGS) {
    DLP_PX_BODIES(KMAX, false, 4, kRatioRingPairs, kProwRingSteps, cd);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(32))) void pivot_x_lean_kernel(DLP_PX_RATIO_ARGS) {
    // (no condensed build: its 32 VGPRs are full; launch_pivot_x refuses a condensed session here)
    DLP_PX_BODIES(128, true, 0, kRatioRingPairs, kProwRingSteps, Cond{});
}
// The chain on CUs of its own (round 6): the grouped-ring selection with ROWS rows per wave (256 lanes
// cover the session's rthreads = 4 ROWS rows, so the exchange's candidate slots are unchanged) and the
// register pivot-row kernel, no VGPR budget; every workgroup resident (the caller's chain CUs hold two
// each at the ring's 64 KB)
template <int ROWS>
__global__ __launch_bounds__(256) void pivot_x_ring_kernel(DLP_PX_RATIO_ARGS) {
    if ((int)blockIdx.x < nrat) {
        ratio_defer_body<128, false, true, 0, 16, false, ROWS, 4>(
            T, ld, rows, rows_elig, ncols, row_first, basis, pp, ntiles, st, C, ldc, Cc, ldcc, P, rhs, nzc, nullptr,
            nullptr, 2, tol_dj, tol_piv, pricing, log, log_cap, nrat, Ccp, Pp, prev_seal, xp, xseq, bcnt, brb, bnt, Tn,
            xs, xseq, cd);
        return;
    }
    prow_defer_body<false>(T, ld, rows, ncols, nprice, st, C, ldc, P, nullptr, pp, tol_dj, log, log_cap, 0, Cp, Pp,
                           prev_seal, xp, xseq, bcnt, brb, bnt, Tn, 1, (int)blockIdx.x - nrat, 1, cd);
}
#undef DLP_PX_BODIES

// Multi-rank: P[s] from the exchanged bits, then the objective row + pricing.
__global__ __launch_bounds__(256) void commit_defer_kernel(
    double* __restrict__ T, int64_t ld, int64_t rows, int64_t ncols, int64_t nprice,
    DevState* st, const double* __restrict__ C, int64_t ldc, double* __restrict__ P,
    const int64_t* __restrict__ bits, PricePart* pp, double tol_dj, dlp_pivot* log,
    int64_t log_cap, const XPeers* xp, uint32_t xseq, Cond cd) {
    __shared__ PricePart lds_pp[4];
    __shared__ int s_ok;
    if (st->status != DLP_RUNNING) return;
    const int64_t slot = st->npivots - 1;
    if (blockIdx.x == 0) CHAIN_STAMP(slot, 12);
    const int s = st->blk - 1;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    d2 pr;
    pr.x = 0.0;
    pr.y = 0.0;
    if (xp) {   // peer exchange: this chunk's flag, then the row from this rank's region
        if (threadIdx.x == 0) s_ok = x_wait(xp, x_rflag(xp, xp->me, blockIdx.x), xseq) ? 1 : 0;
        __syncthreads();
        if (blockIdx.x == 0) CHAIN_STAMP(slot, 13);
        if (!s_ok) {
            if (threadIdx.x == 0) st->status = kStatusXFail;
            return;
        }
        if (j < ld) {
            uint64_t a = 0, b = 0;
            x_read_row_pair(xp, j, &a, &b);
            pr.x = __builtin_bit_cast(double, a);
            pr.y = __builtin_bit_cast(double, b);
        }
    } else if (j < ld) {
        pr = *(const d2*)(bits + j);
    }
    commit_row(T, ld, rows, ncols, nprice, st->npivots - 1, C, ldc, P, s, j, pr, pp, (int)blockIdx.x, tol_dj, log,
               log_cap, lds_pp, d2{0.0, 0.0}, 0.0, cd, cd.on ? st->sq : -1, cd.on ? st->bser : 0);
    if (blockIdx.x == 0) CHAIN_STAMP(slot, 14);
}

// Single rank: ratio test, selection and pivot row in ONE launch (saves a kernel
// boundary per pivot, and the pivot-row workgroups load the block's P rows while
// the ratio phase runs).  Blocks [0, nrat) run ratio_defer_body; blocks
// [nrat, nrat + nprow) are pivot-row workgroups, one 512-column tile each, which
// wait for st->go (bounded spin: a stall turns into DLP_ERR_HIP, never a hang),
// then replay T0[p] exactly as prow_defer_kernel and commit it (commit_row, with
// z_q from st->zq).  The last pivot-row workgroup to finish resets go and its
// ticket for the next launch.  Every block of the grid is resident at once
// (<= 2 * 129 workgroups of 256 threads at C3 against 8 per CU), and blocks are
// dispatched in index order, so the ratio blocks always run.
template <int KMAX>
__global__ __launch_bounds__(256) void pivot_defer_kernel(
    double* __restrict__ T, int64_t ld, int64_t rows, int64_t rows_elig, int64_t ncols,
    int64_t nprice, int64_t row_first, int32_t* basis, PricePart* pp, int ntiles, DevState* st,
    double* __restrict__ C, int64_t ldc, double* __restrict__ Cc, int64_t ldcc,
    double* __restrict__ P, double* __restrict__ rhs, int32_t* __restrict__ nzc, Cand* partials,
    int nrat, double tol_dj, double tol_piv, int pricing, dlp_pivot* log, int64_t log_cap) {
    if ((int)blockIdx.x < nrat) {
        ratio_defer_body<KMAX, true>(T, ld, rows, rows_elig, ncols, row_first, basis, pp, ntiles, st,
                                     C, ldc, Cc, ldcc, P, rhs, nzc, partials, nullptr, 1, tol_dj,
                                     tol_piv, pricing, log, log_cap, nrat);
        return;
    }
    __shared__ PricePart lds_pp[4];
    __shared__ double s_cp[KMAX];
    __shared__ int32_t s_pl[KMAX];
    __shared__ int s_ok;
    if (st->status != DLP_RUNNING) return;   // the same answer in every block of this launch
    const int tile = (int)blockIdx.x - nrat;
    const int64_t j = ((int64_t)tile * blockDim.x + threadIdx.x) * 2;
    const int64_t jc = j < ld ? j : ld - 2;
    // the block's earlier pivot rows at this lane's columns, before the wait (blk may
    // already be one past them if this block starts late: that row is not used)
    const int s0 = min(st->blk, KMAX);
    d2 pv[KMAX];
#pragma unroll
    for (int l = 0; l < KMAX; ++l)
        if (l < s0) pv[l] = *(const d2*)(P + (int64_t)l * ld + jc);
    if (threadIdx.x == 0) {
        int ok = 0;
        for (int it = 0; it < (1 << 24); ++it) {
            if (__hip_atomic_load(&st->go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                ok = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_ok = ok;
    }
    __syncthreads();
    const bool run = s_ok && st->status == DLP_RUNNING;
    if (!s_ok && threadIdx.x == 0) st->status = DLP_ERR_HIP;
    if (run) {
        const int s = st->blk - 1;
        const int32_t pl = st->p_local;
        for (int l = threadIdx.x; l < s; l += blockDim.x) {
            s_cp[l] = C[(int64_t)pl * ldc + l];
            s_pl[l] = st->pl[l];
        }
        __syncthreads();
        d2 pr;
        pr.x = 0.0;
        pr.y = 0.0;
        if (j < ld) {
            d2 t = *(const d2*)(T + (int64_t)pl * ld + j);
#pragma unroll
            for (int l = 0; l < KMAX; ++l) {
                if (l < s) {
                    const d2 v = l < s0 ? pv[l] : *(const d2*)(P + (int64_t)l * ld + j);
                    if (pl == s_pl[l]) {
                        t = v;
                    } else if (s_cp[l] != 0.0) {
                        t.x = __builtin_fma(-s_cp[l], v.x, t.x);
                        t.y = __builtin_fma(-s_cp[l], v.y, t.y);
                    }
                }
            }
            const double piv = st->piv;
            pr.x = t.x / piv;
            pr.y = t.y / piv;
        }
        // commit_row with z_q from the state (C[rows][s] is another block's store)
        const int64_t width = (ncols + 16) & ~(int64_t)15;
        if (j < ld) {
            *(d2*)(P + (int64_t)s * ld + j) = pr;
            if (s == 0)   // block start: pivot rows 1..K-1 := +0 (commit_row)
                for (int64_t l = 1; l < ldc; ++l) *(d2*)(P + l * ld + j) = d2{0.0, 0.0};
        }
        const double zq = st->zq;
        PricePart acc = pp_empty();
        if (j < width) {
            double* zp = T + rows * ld + j;
            d2 z = *(const d2*)zp;
            if (zq != 0.0) {
                z.x = __builtin_fma(-zq, pr.x, z.x);
                z.y = __builtin_fma(-zq, pr.y, z.y);
                *(d2*)zp = z;
            }
            price_pair(acc, z.x, z.y, j, nprice, tol_dj);
            if (log && j <= ncols && ncols < j + 2) {
                const int64_t k = st->npivots - 1;
                if (k >= 0 && k < log_cap) log[k].objective = (ncols == j) ? z.x : z.y;
            }
        }
        acc = block_price(acc, lds_pp);
        if (threadIdx.x == 0) pp[tile] = acc;
    }
    // the last pivot-row block to finish re-arms the flag for the next launch
    if (threadIdx.x == 0) {
        const int nprow = (int)gridDim.x - nrat;
        const unsigned prev =
            __hip_atomic_fetch_add(&st->ticket2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == (unsigned)nprow - 1) {
            __hip_atomic_store(&st->go, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&st->ticket2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

// The band-publication arguments of a lookahead chain kernel (bcnt, brb, bnt, Tn): the counts of
// the sealed block's pass in flight, or "nothing published" without one.
struct BandArgs {
    uint32_t* cnt;
    int rb, ntiles;
    const double* Tn;
};
static BandArgs band_args(const BandPub* bp, int prev_seal) {
    if (!(bp && bp->cnt && bp->Tn && prev_seal >= 0)) return {nullptr, 1, 0, nullptr};
    return {bp->cnt + prev_seal * bp->stride, bp->rb, bp->ntiles, bp->Tn};
}

// Rows per wave of the grouped ring.  In isolation (chainlab, cold inputs, 127 / 64 replayed steps)
// it replays 1.6-2x faster than the LEAN ring: 64 rows per wave on 256-lane workgroups (C3 rows on
// 64 CUs: 20.4 / 10.0 us vs 36.4 / 14.0), 32 on the rank geometries' 128-lane ones (c3r4 on 128
// CUs: 11.9 / 6.8 vs 22.6 / 11.5; profiles/r06q/-r06s/).  In the product the selection launch is
// bound by its other round trips, so the pivot rate barely moves (profiles/r06t/, alternating):
// c3r2 +1.5% (both pairs), C3 equal (pass-bound), c3r4 equal, c3r8 -1.5% (both pairs).  Auto: the
// grouped ring on 256-lane workgroups, the LEAN ring on 128-lane ones.
static int ratio_ring_rows(const Geometry& g) {
    return g.rthreads >= 256 ? 64 : 0;
}

int ratio_defer_blocks(const Geometry& g) {
    return (int)((g.rows + 1 + g.rthreads - 1) / g.rthreads);
}
// the fused single-rank pivot and the one-launch peer pivot keep 256-lane ratio workgroups
static int ratio_blocks_256(const Geometry& g) {
    return (int)((g.rows + 1 + kRatioDeferThreads - 1) / kRatioDeferThreads);
}

hipError_t launch_ratio_defer(const Geometry& g, const Defer& d, int32_t* basis,
                              const PricePart* pp, DevState* st, Cand* partials, int nblocks,
                              Cand* cand_out, int nranks, double tol_dj, double tol_piv,
                              int pricing, dlp_pivot* log, int64_t log_cap, hipStream_t s,
                              const Defer* prev, int prev_seal, const XPeers* xp, uint32_t xseq,
                              const BandPub* bp, bool xfuse, bool own_cus) {
    const int ntiles = (int)((g.width + kDeferTile - 1) / kDeferTile);
    const BandArgs b = band_args(bp, prev_seal);
    xfuse = xfuse && xp && nranks > 1;
    if (nblocks < ratio_defer_blocks(g)) return hipErrorInvalidValue;   // partials too small
    nblocks = ratio_defer_blocks(g);
    if (prev_seal >= 0 && (!prev || prev_seal > 1 || 2 * d.K > kMaxReplay)) return hipErrorInvalidValue;
    const double* Ccp = prev_seal >= 0 ? prev->Cc : nullptr;
    const double* Pp = prev_seal >= 0 ? prev->P : nullptr;
    const int steps = prev_seal >= 0 ? 2 * d.K : d.K;   // at most kp + j replayed steps
    if (g.rthreads != 64 && g.rthreads != 128 && g.rthreads != 256) return hipErrorInvalidValue;
#define DLP_RATIO_ARGS                                                                                      \
    g.T, g.ld, g.rows, g.rows_elig, g.ncols, g.row_first, basis, pp, ntiles, st, d.C, d.ldc, d.Cc, d.ldcc, \
        d.P, d.rhs, d.nzc, partials, cand_out, nranks, tol_dj, tol_piv, pricing, log, log_cap, Ccp, Pp,     \
        prev_seal, xp, xseq
    // (the lookahead instances also take the band publication)
#define DLP_RATIO_LA_ARGS DLP_RATIO_ARGS, b.cnt, b.rb, b.ntiles, b.Tn, xfuse ? 1 : 0, g.cd
    if (steps <= 8)
        ratio_defer_kernel<8><<<nblocks, g.rthreads, 0, s>>>(DLP_RATIO_ARGS, xfuse ? 1 : 0, g.cd);
    else if (steps <= 16)
        ratio_defer_kernel<16><<<nblocks, g.rthreads, 0, s>>>(DLP_RATIO_ARGS, xfuse ? 1 : 0, g.cd);
    else if (steps <= 32)
        ratio_defer_kernel<32><<<nblocks, g.rthreads, 0, s>>>(DLP_RATIO_ARGS, xfuse ? 1 : 0, g.cd);
    else if (steps <= 64)
        ratio_defer_kernel<64><<<nblocks, g.rthreads, 0, s>>>(DLP_RATIO_ARGS, xfuse ? 1 : 0, g.cd);
    else   // lookahead at K = 64, beside the form-21 pass
    {
        static const int lch = env_int("DLP_LEAN_LCH", 0);
        static const int mid_env = env_int("DLP_MID_CHAIN", -1);
        if (mid_env >= 0 ? mid_env == 1 : d.form == 22) {   // beside the MFMA pass: registers, no ring
            ratio_mid_kernel<128, 16><<<nblocks, g.rthreads, 0, s>>>(DLP_RATIO_LA_ARGS);
            return hipGetLastError();
        }
        // the chain on CUs of its own: the grouped ring, ROWS rows per wave (DLP_RATIO_ROWS = 64 / 32 / 16
        // overrides the policy, 0 keeps the LEAN ring)
        static const int rows_env = env_int("DLP_RATIO_ROWS", -1);
        const int rrows = rows_env >= 0 ? rows_env : (own_cus ? ratio_ring_rows(g) : 0);
        if (rrows == 64 || rrows == 32 || rrows == 16) {
            const int lanes = g.rthreads * 64 / rrows;
            if (lanes > 1024) return hipErrorInvalidValue;
#define DLP_RATIO_RING(R_, RP_, RG_) \
    ratio_ring_kernel<R_, RP_, RG_><<<nblocks, lanes, (size_t)(lanes / 64) * RP_ * 1024, s>>>(DLP_RATIO_LA_ARGS)
            // (DLP_RATIO_RP=12: 12 DMAs in flight, 48 KB of ring per 256-lane workgroup, so three share a
            // CU and C3's 129 workgroups are resident at once on 64 CUs; tuning)
            static const int rp_env = env_int("DLP_RATIO_RP", 16);
            if (rrows == 64 && rp_env == 12)
                DLP_RATIO_RING(64, 12, 4);
            else if (rrows == 64)
                DLP_RATIO_RING(64, 16, 4);
            else if (rrows == 32)
                DLP_RATIO_RING(32, 16, 4);
            else
                DLP_RATIO_RING(16, 16, 2);
#undef DLP_RATIO_RING
            return hipGetLastError();
        }
        static const int ring_env = env_int("DLP_CHAIN_RING", 0);
#define DLP_RATIO_LEAN(L, DYN, ...) \
    ratio_lean_kernel<128, L, ##__VA_ARGS__><<<nblocks, g.rthreads, DYN, s>>>(DLP_RATIO_LA_ARGS)
        // the LDS ring (0); 4 or 8 coefficient loads per round trip for tuning only (DLP_LEAN_LCH)
        if (lch == 8 && !g.cd.on)
            DLP_RATIO_LEAN(8, 0);
        else if (lch == 4)
            DLP_RATIO_LEAN(4, 0);
        else if (ring_env == 16)   // (tuning: DLP_CHAIN_RING=16, 16 ring DMAs in flight per wave)
            DLP_RATIO_LEAN(0, ratio_ring_bytes(16) / (kRatioDeferThreads / g.rthreads), 16);
        else
            DLP_RATIO_LEAN(0, ratio_ring_bytes(kRatioRingPairs) / (kRatioDeferThreads / g.rthreads));
#undef DLP_RATIO_LEAN
    }
#undef DLP_RATIO_LA_ARGS
#undef DLP_RATIO_ARGS
    return hipGetLastError();
}

hipError_t launch_pivot_defer(const Geometry& g, const Defer& d, int32_t* basis, PricePart* pp,
                              DevState* st, Cand* partials, int nblocks, double tol_dj,
                              double tol_piv, int pricing, dlp_pivot* log, int64_t log_cap,
                              hipStream_t s) {
    const int ntiles = (int)((g.width + kDeferTile - 1) / kDeferTile);
    if (nblocks < ratio_blocks_256(g)) return hipErrorInvalidValue;   // partials too small
    const int nrat = ratio_blocks_256(g);
    const int nprow = (int)((g.ld + kDeferTile - 1) / kDeferTile);
    // every block resident at once (the pivot-row blocks wait on the ratio blocks): the
    // caller keeps the grid within 2 blocks per CU (fused_pivot_fits); K <= 32
    if (d.K > 32 || g.cd.on) return hipErrorInvalidValue;   // (no condensed-tableau instance)
#define DLP_PIVOT_DEFER(KM)                                                                       \
    pivot_defer_kernel<KM><<<nrat + nprow, 256, 0, s>>>(                                          \
        g.T, g.ld, g.rows, g.rows_elig, g.ncols, g.nprice, g.row_first, basis, pp, ntiles, st,    \
        d.C, d.ldc, d.Cc, d.ldcc, d.P, d.rhs, d.nzc, partials, nrat, tol_dj, tol_piv, pricing,    \
        log, log_cap)
    if (d.K <= 8)
        DLP_PIVOT_DEFER(8);
    else if (d.K <= 16)
        DLP_PIVOT_DEFER(16);
    else
        DLP_PIVOT_DEFER(32);
#undef DLP_PIVOT_DEFER
    return hipGetLastError();
}

int fused_pivot_blocks(const Geometry& g) {
    return ratio_blocks_256(g) + (int)((g.ld + kDeferTile - 1) / kDeferTile);
}

// How many workgroups of the fused pivot kernel (the instance launch_pivot_defer picks for K)
// the device holds at once, from the compiled kernel's real occupancy (0 when unknown): its
// pivot-row blocks spin on the ratio blocks' selection, so the whole grid must be resident.
int fused_pivot_capacity(int K, int cus) {
    int per = 0;
    const hipError_t e =
        K <= 8    ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, pivot_defer_kernel<8>, 256, 0)
        : K <= 16 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, pivot_defer_kernel<16>, 256, 0)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, pivot_defer_kernel<32>, 256, 0);
    return e == hipSuccess ? per * cus : 0;
}

hipError_t launch_prow_defer(const Geometry& g, const Defer& d, const DevState* st,
                             int64_t* prow_bits, PricePart* pp, double tol_dj, dlp_pivot* log,
                             int64_t log_cap, int nranks, hipStream_t s, const Defer* prev,
                             int prev_seal, const XPeers* xp, uint32_t xseq, const BandPub* bp,
                             bool xfuse, bool own_cus) {
    const int blocks = (int)((g.ld + kDeferTile - 1) / kDeferTile);
    const int xc = (xfuse && xp && nranks > 1) ? 1 : 0;
    if (prev_seal >= 0 && (!prev || prev_seal > 1 || 2 * d.K > kMaxReplay)) return hipErrorInvalidValue;
    if (!(prev_seal >= 0 && d.K > 32)) {
        prow_defer_kernel<<<blocks, 256, 0, s>>>(g.T, g.ld, g.rows, g.ncols, g.nprice, st, d.C, d.ldc,
                                                 d.P, prow_bits, pp, tol_dj, log, log_cap,
                                                 nranks == 1 ? 1 : 0, prev_seal >= 0 ? prev->C : nullptr,
                                                 prev_seal >= 0 ? prev->P : nullptr, prev_seal,
                                                 nranks == 1 ? nullptr : xp, xseq, nullptr, 1, 0, nullptr, xc, g.cd);
        return hipGetLastError();
    }
    // lookahead at K = 64: the sealed block replayed first, the pass in flight publishing its bands
    const BandArgs b = band_args(bp, prev_seal);
#define DLP_PROW_LA_ARGS                                                                                       \
    g.T, g.ld, g.rows, g.ncols, g.nprice, st, d.C, d.ldc, d.P, prow_bits, pp, tol_dj, log, log_cap,            \
        nranks == 1 ? 1 : 0, prev->C, prev->P, prev_seal, nranks == 1 ? nullptr : xp, xseq, b.cnt, b.rb, b.ntiles, \
        b.Tn, xc, g.cd
    static const int fat_env = env_int("DLP_FAT_PROW", -1);
    // the chain on CUs of its own: the grouped ring (DLP_PROW_GROUP = 4) or the register kernel
    static const int pg_env = env_int("DLP_PROW_GROUP", 0);
    if (own_cus && fat_env < 0 && pg_env == 4) {
        prow_ring_kernel<16, 4><<<blocks, 256, prow_ring_bytes(16), s>>>(DLP_PROW_LA_ARGS);
        return hipGetLastError();
    }
    const bool fat = fat_env >= 0 ? fat_env == 1 : own_cus;
    static const int mid_env = env_int("DLP_MID_CHAIN", -1);
    const bool mid = !fat && (mid_env >= 0 ? mid_env == 1 : d.form == 22);
    static const int ring_env = env_int("DLP_CHAIN_RING", 0);
    if (mid)   // beside the MFMA pass (form 22 leaves 104 VGPRs per SIMD): the register replay, 2 x 8 rows
        prow_mid_kernel<<<blocks, 256, 0, s>>>(DLP_PROW_LA_ARGS);
    else if (fat)   // the chain on CUs of its own (no pass waves beside it): the register kernel, 2 x 16
                    // pivot rows in flight
        prow_defer_kernel<<<blocks, 256, 0, s>>>(DLP_PROW_LA_ARGS);
    else if (ring_env == 16)   // beside the form-21 pass: the LEAN ring
        prow_lean_kernel<16><<<blocks, 256, prow_ring_bytes(16), s>>>(DLP_PROW_LA_ARGS);
    else
        prow_lean_kernel<kProwRingSteps><<<blocks, 256, prow_ring_bytes(kProwRingSteps), s>>>(DLP_PROW_LA_ARGS);
#undef DLP_PROW_LA_ARGS
    return hipGetLastError();
}

hipError_t launch_pivot_x(const Geometry& g, const Defer& d, int32_t* basis, PricePart* pp, DevState* st,
                          double tol_dj, double tol_piv, int pricing, dlp_pivot* log, int64_t log_cap,
                          hipStream_t s, const Defer* prev, int prev_seal, const XPeers* xp, uint32_t seq,
                          const BandPub* bp, bool own_cus) {
    // 256-lane ratio blocks (the ring instance: 128 or 256 rows each, on the chain's own CUs); the
    // selection record carries the condensed tableau's entering slot
    const bool ring = own_cus && d.K == 64 && (g.rthreads == 128 || g.rthreads == kRatioDeferThreads);
    if (!xp || (!ring && g.rthreads != kRatioDeferThreads)) return hipErrorInvalidValue;
    if (prev_seal >= 0 && (!prev || prev_seal > 1 || 2 * d.K > kMaxReplay)) return hipErrorInvalidValue;
    const int ntiles = (int)((g.width + kDeferTile - 1) / kDeferTile);
    const int nrat = ratio_defer_blocks(g);
    const int nprow = (int)((g.ld + kDeferTile - 1) / kDeferTile);
    const BandArgs b = band_args(bp, prev_seal);
    const double* Ccp = prev_seal >= 0 ? prev->Cc : nullptr;
    const double* Pp = prev_seal >= 0 ? prev->P : nullptr;
    const double* Cp = prev_seal >= 0 ? prev->C : nullptr;
    const int steps = prev_seal >= 0 ? 2 * d.K : d.K;
#define DLP_PX_ARGS                                                                                          \
    g.T, g.ld, g.rows, g.rows_elig, g.ncols, g.nprice, g.row_first, basis, pp, ntiles, st, d.C, d.ldc, d.Cc, \
        d.ldcc, d.P, d.rhs, d.nzc, nrat, tol_dj, tol_piv, pricing, log, log_cap, Ccp, Pp, Cp, prev_seal, xp, \
        seq, b.cnt, b.rb, b.ntiles, b.Tn, 2, g.cd
    if (!ring && steps > 64 && g.cd.on) return hipErrorInvalidValue;   // (the LEAN instance has no condensed build)
    if (ring) {
        if (g.rthreads == 128)
            pivot_x_ring_kernel<32><<<nrat + nprow, 256, (size_t)4 * 16 * 1024, s>>>(DLP_PX_ARGS);
        else
            pivot_x_ring_kernel<64><<<nrat + nprow, 256, (size_t)4 * 16 * 1024, s>>>(DLP_PX_ARGS);
    } else if (steps > 64)   // lookahead at K = 64, beside the form-21 pass
        pivot_x_lean_kernel<<<nrat + nprow, 256, std::max(ratio_ring_bytes(kRatioRingPairs),
                                                          prow_ring_bytes(kProwRingSteps)), s>>>(DLP_PX_ARGS);
    else if (steps <= 16)
        pivot_x_kernel<16><<<nrat + nprow, 256, 0, s>>>(DLP_PX_ARGS);
    else if (steps <= 32)
        pivot_x_kernel<32><<<nrat + nprow, 256, 0, s>>>(DLP_PX_ARGS);
    else
        pivot_x_kernel<64><<<nrat + nprow, 256, 0, s>>>(DLP_PX_ARGS);
#undef DLP_PX_ARGS
    return hipGetLastError();
}

hipError_t launch_commit_defer(const Geometry& g, const Defer& d, DevState* st,
                               const int64_t* prow_bits, PricePart* pp, double tol_dj,
                               dlp_pivot* log, int64_t log_cap, hipStream_t s, const XPeers* xp,
                               uint32_t xseq) {
    const int blocks = (int)((g.ld + kDeferTile - 1) / kDeferTile);
    commit_defer_kernel<<<blocks, 256, 0, s>>>(g.T, g.ld, g.rows, g.ncols, g.nprice, st, d.C,
                                               d.ldc, d.P, prow_bits, pp, tol_dj, log, log_cap, xp,
                                               xseq, g.cd);
    return hipGetLastError();
}

hipError_t chain_stamps_enable() {
    const int on = 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_chain_stamps_on), &on, sizeof(on));
}
hipError_t chain_stamps_dump(uint64_t* host64x16) {
    return hipMemcpyFromSymbol(host64x16, HIP_SYMBOL(g_chain_stamps), sizeof(uint64_t) * 64 * 16);
}
hipError_t chain_wg_stamps_dump(uint64_t* host1024x8) {
    return hipMemcpyFromSymbol(host1024x8, HIP_SYMBOL(g_wg_stamps), sizeof(uint64_t) * 1024 * 8);
}

}  // namespace dlp
