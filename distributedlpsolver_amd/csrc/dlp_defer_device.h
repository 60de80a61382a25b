// dlp_defer_device.h — device-side helpers shared by the two deferred rank-k units, the
// selection chain (dlp_chain.hip) and the tableau pass (dlp_pass.hip): bit casts for buffer
// operands, (non)temporal vector loads / stores, the asm LDS-DMA and its counted waits.
// Internal; included after dlp_device.h inside `namespace dlp { namespace { ... } }`.
#pragma once

typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));
// A double's bits as the b64 buffer-store operand, built from scalars: hipcc miscompiles a
// __builtin_bit_cast of an element of an ext_vector value (tests/test_isa.py source guard).
__device__ __forceinline__ u2v dbits(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof(u));
    u2v w;
    w.x = (unsigned)u;
    w.y = (unsigned)(u >> 32);
    return w;
}

template <bool NT>
__device__ inline d2 ldv(const double* p) {
    if constexpr (NT)
        return __builtin_nontemporal_load((const d2*)p);
    else
        return *(const d2*)p;
}
template <bool NT>
__device__ inline double ldv1(const double* p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}
template <bool NT>
__device__ inline void stv1(double* p, double v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}
template <bool NT>
__device__ inline void stv(double* p, d2 v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, (d2*)p);
    else
        *(d2*)p = v;
}

// 16-B LDS-DMA (global_load_lds_dwordx4: lane x's 16 bytes land at the wave-uniform LDS
// address m0 + 16 x) issued from inline asm, so that hipcc does not count it: with the
// builtin it waits vmcnt(0) before the next LDS read or ordinary-load use, draining every
// DMA in flight (cdna_hip_programming.md, glds).  The callers retire their DMAs with counted
// waits of their own (vmwait), which hold because between two of them they issue no other
// vector-memory instruction, or a fixed number of them.  The lgkmcnt(0) orders the DMA's
// LDS write after this wave's earlier LDS reads of the slot it refills.
// NTL: the DMA carries the nt cache policy (a single-use stream: it leaves the re-read data of the
// kernels beside it in the caches; profiles/r04s lab8).  Only the asm string differs.
template <bool NTL = false>
__device__ __forceinline__ void glds16(const void* g, uint32_t m0) {
    if constexpr (NTL)
        asm volatile("s_waitcnt lgkmcnt(0)\n\tglobal_load_lds_dwordx4 %0, off nt" ::"v"(g), "{m0}"(m0) : "memory");
    else
        asm volatile("s_waitcnt lgkmcnt(0)\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "{m0}"(m0) : "memory");
}
// The same DMA in the scalar-base form: lane x reads 16 B at base + voff (voff: unsigned 32-bit bytes),
// the wave-uniform base in an SGPR pair, so a stream that only advances by a uniform stride needs no
// per-lane address arithmetic.  The s_nop covers a base that an SALU add has just written (the
// compiler pads nothing inside the statement).
template <bool NTL = false>
__device__ __forceinline__ void glds16s(uint32_t voff, const void* base, uint32_t m0) {
    if constexpr (NTL)
        asm volatile("s_nop 4\n\ts_waitcnt lgkmcnt(0)\n\tglobal_load_lds_dwordx4 %0, %1 nt" ::"v"(voff), "s"(base),
                     "{m0}"(m0)
                     : "memory");
    else
        asm volatile("s_nop 4\n\ts_waitcnt lgkmcnt(0)\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base),
                     "{m0}"(m0)
                     : "memory");
}
template <int N>
__device__ __forceinline__ void vmwait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p);
}

constexpr int kAuxSc1 = 16;   // buffer-op cache policy: sc1 (write-through store / L2 load)

// The commit of a block step (the primal chain of dlp_chain.hip, which documents it, and the dual
// chain of dlp_dual.hip): P[s] := pr for columns j, j+1; objective row z -= z_q * P[s] (z_q != 0);
// pricing partial of this 512-column tile (pp[tile]); objective value into log[klog].
template <int ZQ = 0>
__device__ inline void commit_row(double* __restrict__ T, int64_t ld, int64_t rows, int64_t ncols,
                                  int64_t nprice, int64_t klog, const double* __restrict__ C,
                                  int64_t ldc, double* __restrict__ P, int s, int64_t j, d2 pr,
                                  PricePart* pp, int tile, double tol_dj, dlp_pivot* log, int64_t log_cap,
                                  PricePart* lds_pp, d2 zpre = d2{0.0, 0.0}, double zqv = 0.0,
                                  Cond cd = Cond{}, int32_t sq = -1, int32_t bser = 0) {
    const int64_t width = (ncols + 16) & ~(int64_t)15;
    const bool rx = cd.on && j == sq, ry = cd.on && j + 1 == sq;
    if (j < ld) {
        *(d2*)(P + (int64_t)s * ld + j) = pr;
        if (s == 0)   // block start: pivot rows 1..K-1 := +0 (see the ratio kernel's C tails)
            for (int64_t l = 1; l < ldc; ++l) *(d2*)(P + l * ld + j) = d2{0.0, 0.0};
        if (rx || ry) {
            for (int l = 0; l < s; ++l) P[(int64_t)l * ld + sq] = 0.0;
            cd.rst[sq] = (bser << 7) | s;
        }
    }
    const double zq = ZQ == 0 ? C[rows * ldc + s] : zqv;
    PricePart acc = pp_empty();
    if (j < width) {
        double* zp = T + rows * ld + j;
        d2 z = ZQ == 1 ? zpre : *(const d2*)zp;
        if (rx) z.x = 0.0;
        if (ry) z.y = 0.0;
        if (zq != 0.0) {
            z.x = __builtin_fma(-zq, pr.x, z.x);
            z.y = __builtin_fma(-zq, pr.y, z.y);
        }
        if (zq != 0.0 || rx || ry) *(d2*)zp = z;
        if (cd.on)
            price_pair_var(acc, z.x, z.y, cd.var_of[j], cd.var_of[j + 1], tol_dj);
        else
            price_pair(acc, z.x, z.y, j, nprice, tol_dj);
        if (log && j <= ncols && ncols < j + 2) {
            if (klog >= 0 && klog < log_cap) log[klog].objective = (ncols == j) ? z.x : z.y;
        }
    }
    acc = block_price(acc, lds_pp);
    if (threadIdx.x == 0) pp[tile] = acc;
}
