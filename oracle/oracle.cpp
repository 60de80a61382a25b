// oracle.cpp — TEST INFRASTRUCTURE ONLY (see oracle.h).  CPU restatement of
// the dense-tableau simplex rule spec and the instance
// generators (§8a row a7, §8f row f1).  Written independently of the product
// sources under distributedlpsolver_amd/csrc: nothing is shared, so agreement
// between the two is evidence, not tautology.
//
// Build: g++ -O2 -std=c++17 -ffp-contract=off -fopenmp -shared -fPIC (oracle/Makefile).
#include "oracle.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <vector>
#ifdef _OPENMP
#include <omp.h>
#endif

namespace {

// ---------------------------------------------------------------- generators
// in-repo splitmix64 -> fp64 via (u >> 11) * 2^-53.
// Nearest reference analog: Instance::GenerateInstance, R/instance.cpp:32-57.
inline uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
inline uint64_t stream_key(uint64_t seed, uint64_t stream) {
    return mix64(seed ^ (0x9E3779B97F4A7C15ULL * (stream + 1)));
}
inline double unit(uint64_t key, uint64_t idx) {
    return (double)(mix64(key + idx) >> 11) * 0x1.0p-53;
}
enum { S_A = 1, S_X0 = 2, S_U = 3, S_C = 4, S_DEGEN = 5 };

// Degenerate family (kind 1): row i is a "cone" row when the top bit of its
// mask draw is 0 (~50%): A_ij = 2u - 1 (mixed sign, exact) and b_i = 0, so the
// origin is a highly degenerate vertex while OPT stays > 0; other rows as dense.
inline bool degen_row(int kind, uint64_t seed, int64_t i) {
    return kind == 1 && (mix64(stream_key(seed, S_DEGEN) + (uint64_t)i) >> 63) == 0;
}
inline double gen_a(bool cone, uint64_t kA, int64_t i, int64_t n, int64_t j) {
    const double u = unit(kA, (uint64_t)(i * n + j));
    return cone ? 2.0 * u - 1.0 : u;
}

// b_i = (sum of 64 strided fma chains, reduced by a fixed halving tree) + u_i.
// Chain l accumulates j = l, l+64, l+128, ... ascending: s_l = fma(A_ij, x0_j, s_l).
// Tree: for w = 32, 16, 8, 4, 2, 1: s_l = s_l + s_{l+w} for l < w.  Result s_0.
// (The build's generator spec; one 64-lane wavefront per row on the device.)
double gen_b(bool cone, int64_t n, uint64_t seed, int64_t i, const double* Arow,
             const std::vector<double>& x0) {
    if (cone) return 0.0;
    double s[64];
    for (int l = 0; l < 64; ++l) {
        double acc = 0.0;
        for (int64_t j = l; j < n; j += 64) acc = std::fma(Arow[j], x0[j], acc);
        s[l] = acc;
    }
    for (int w = 32; w >= 1; w >>= 1)
        for (int l = 0; l < w; ++l) s[l] = s[l] + s[l + w];
    return s[0] + unit(stream_key(seed, S_U), (uint64_t)i);
}

inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

// ------------------------------------------------------------------ tableau
struct Tab {
    int64_t m = 0, n = 0, N = 0, ld = 0;
    int64_t row_first = 0, rows = 0;      // local constraint rows; objective row is rows
    int64_t nprice = 0;                   // priced columns [0, nprice)
    int64_t rows_elig = 0;                // rows [0, rows_elig) enter the ratio test
    std::vector<double> T;                // (rows+1) x ld
    std::vector<int32_t> basis;           // global, m entries (replicated)
    std::vector<double> colq, prow;
    int pricing = 0, bland = 0, status = 4 /*running*/;
    double tol_dj = 1e-9, tol_piv = 1e-9;
    int32_t q = -1, p = -1, p_local = -1, leaving = -1;
    double ratio = 0.0;
    int nthreads = 1;
    std::vector<oracle_pivot> log;
    double* row(int64_t i) { return T.data() + i * ld; }
};

void tab_init(Tab& t, int64_t m, int64_t n, int64_t row_first, int64_t rows, const oracle_opts* o) {
    t.m = m; t.n = n; t.N = n + m; t.ld = round16(t.N + 1);
    t.row_first = row_first; t.rows = rows;
    t.nprice = t.N; t.rows_elig = rows;
    t.T.assign((size_t)(rows + 1) * t.ld, 0.0);
    t.basis.resize(m);
    for (int64_t i = 0; i < m; ++i) t.basis[i] = (int32_t)(n + i);   // slack basis
    t.colq.assign(rows + 1, 0.0);
    t.prow.assign(t.ld, 0.0);
    if (o) {
        t.pricing = o->pricing; t.tol_dj = o->tol_dj; t.tol_piv = o->tol_piv;
        t.nthreads = o->nthreads > 0 ? o->nthreads : 1;
    }
    t.bland = t.pricing == 1;
}

void tab_fill_dense(Tab& t, const double* A, const double* b, const double* c) {
    for (int64_t il = 0; il < t.rows; ++il) {
        int64_t i = t.row_first + il;
        double* r = t.row(il);
        for (int64_t j = 0; j < t.n; ++j) r[j] = A[i * t.n + j];
        r[t.n + i] = 1.0;
        r[t.N] = b[i];
    }
    double* z = t.row(t.rows);
    for (int64_t j = 0; j < t.n; ++j) z[j] = -c[j];
}

// a1: pricing.  Dantzig: q = argmin z_j (first index on ties), optimal when
// z_q >= -tol_dj.  Bland: first j with z_j < -tol_dj.
// Nearest reference analog: the first-wins strict '<' scans of
// R/global_problem.cpp:335-341,352-361.
int32_t price(Tab& t) {
    const double* z = t.row(t.rows);
    if (t.bland) {
        for (int64_t j = 0; j < t.nprice; ++j)
            if (z[j] < -t.tol_dj) return (int32_t)j;
        return -1;
    }
    double best = std::numeric_limits<double>::infinity();
    int64_t q = -1;
    for (int64_t j = 0; j < t.nprice; ++j)
        if (z[j] < best) { best = z[j]; q = j; }
    if (q < 0 || !(best < -t.tol_dj)) return -1;
    return (int32_t)q;
}

// Candidate order: valid first, then smaller ratio, then smaller basis index.
bool cand_better(const oracle_cand& a, const oracle_cand& b) {
    if (a.valid != b.valid) return a.valid != 0;
    if (!a.valid) return false;
    if (a.ratio != b.ratio) return a.ratio < b.ratio;
    return a.basis_var < b.basis_var;
}

// a2: ratio test over local rows (nearest analog: the tolerance-gated tight
// set test of R/global_problem.cpp:372-380).
oracle_cand local_ratio(Tab& t, int32_t q) {
    oracle_cand best{};
    best.valid = 0;
    for (int64_t il = 0; il <= t.rows; ++il) t.colq[il] = t.row(il)[q];
    for (int64_t il = 0; il < t.rows_elig; ++il) {
        double a = t.colq[il];
        if (!(a > t.tol_piv)) continue;
        double rhs = t.row(il)[t.N];
        if (!(rhs > 0.0)) rhs = 0.0;
        oracle_cand c{};
        c.ratio = rhs / a;
        c.row = (int32_t)(t.row_first + il);
        c.basis_var = t.basis[c.row];
        c.valid = 1;
        c.pivot = a;
        if (cand_better(c, best)) best = c;
    }
    return best;
}

// a4: select + basis bookkeeping + pivot log.
void record_pivot(Tab& t, const oracle_cand& w) {
    t.p = w.row;
    t.leaving = t.basis[w.row];
    t.basis[w.row] = t.q;
    t.ratio = w.ratio;
    t.bland = (t.pricing == 1) ? 1 : (w.ratio == 0.0 ? 1 : 0);
    int64_t pl = (int64_t)w.row - t.row_first;
    t.p_local = (pl >= 0 && pl < t.rows) ? (int32_t)pl : -1;
    oracle_pivot e{};
    e.q = t.q; e.p = t.p; e.leaving = t.leaving; e.ratio = w.ratio;
    e.objective = std::numeric_limits<double>::quiet_NaN();
    t.log.push_back(e);
}

void make_prow(Tab& t) {
    const double* r = t.row(t.p_local);
    double piv = r[t.q];
    for (int64_t j = 0; j < t.ld; ++j) t.prow[j] = r[j] / piv;
}

// a3: rank-1 elimination.  Rows with colq == 0 are untouched; row p := prow.
// Nearest analog: the 2x2 basis solve of R/global_problem.cpp:393-405.
void eliminate(Tab& t) {
    const int64_t rows = t.rows, ld = t.ld;
    const double* pr = t.prow.data();
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(t.nthreads)
#endif
    for (int64_t il = 0; il <= rows; ++il) {
        double* r = t.T.data() + il * ld;
        if (il == t.p_local) {
            std::memcpy(r, pr, sizeof(double) * ld);
            continue;
        }
        double f = t.colq[il];
        if (f == 0.0) continue;
        for (int64_t j = 0; j < ld; ++j) r[j] = std::fma(-f, pr[j], r[j]);
    }
    t.log.back().objective = t.row(rows)[t.N];
}

// One full pivot on a single slice holding every row. Returns status.
int pivot_once(Tab& t) {
    t.q = price(t);
    if (t.q < 0) { t.status = 0; return 0; }
    oracle_cand w = local_ratio(t, t.q);
    if (!w.valid) { t.status = 2; return 2; }
    record_pivot(t, w);
    make_prow(t);
    eliminate(t);
    return 4;
}

}  // namespace

#include "oracle_general.inc"

struct oracle_slice { Tab t; };

extern "C" {

int64_t oracle_ld(int64_t m, int64_t n) { return round16(n + m + 1); }

int oracle_gen_dense(int kind, int64_t m, int64_t n, uint64_t seed, double* A, double* b, double* c) {
    if (m <= 0 || n <= 0 || (kind != 0 && kind != 1)) return -1;
    std::vector<double> x0(n);
    const uint64_t kA = stream_key(seed, S_A), kX = stream_key(seed, S_X0), kC = stream_key(seed, S_C);
    for (int64_t j = 0; j < n; ++j) x0[j] = unit(kX, (uint64_t)j);
    std::vector<double> rowbuf(n);
    for (int64_t i = 0; i < m; ++i) {
        double* Ar = A ? A + i * n : rowbuf.data();
        const bool cone = degen_row(kind, seed, i);
        for (int64_t j = 0; j < n; ++j) Ar[j] = gen_a(cone, kA, i, n, j);
        if (b) b[i] = gen_b(cone, n, seed, i, Ar, x0);
    }
    if (c)
        for (int64_t j = 0; j < n; ++j) c[j] = unit(kC, (uint64_t)j);
    return 0;
}

int oracle_gen_tableau(int kind, int64_t m, int64_t n, uint64_t seed, int64_t row_first,
                       int64_t row_count, int64_t ld, double* T, int32_t nthreads) {
    const int64_t N = n + m;
    if (ld < N + 1 || row_first < 0 || row_first + row_count > m) return -1;
    std::vector<double> x0(n);
    const uint64_t kA = stream_key(seed, S_A), kX = stream_key(seed, S_X0), kC = stream_key(seed, S_C);
    for (int64_t j = 0; j < n; ++j) x0[j] = unit(kX, (uint64_t)j);
    (void)nthreads;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(nthreads > 0 ? nthreads : 1)
#endif
    for (int64_t il = 0; il < row_count; ++il) {
        const int64_t i = row_first + il;
        double* r = T + il * ld;
        std::memset(r, 0, sizeof(double) * ld);
        const bool cone = degen_row(kind, seed, i);
        for (int64_t j = 0; j < n; ++j) r[j] = gen_a(cone, kA, i, n, j);
        r[N] = gen_b(cone, n, seed, i, r, x0);
        r[n + i] = 1.0;
    }
    double* z = T + row_count * ld;
    std::memset(z, 0, sizeof(double) * ld);
    for (int64_t j = 0; j < n; ++j) z[j] = -unit(kC, (uint64_t)j);
    return 0;
}

// f1: restatement of Instance::GenerateInstance (R/instance.cpp:32-57) and
// SetBudgets (R/instance.cpp:136-141), using libc srand(1)/rand() directly.
// - loop bound evaluated in long double: (long double)sparsity * I (R/instance.cpp:44);
// - bid = (long double)(rand()+1) / (long double)RAND_MAX (R/instance.cpp:46), then to fp64;
// - a repeated (advertiser, impression) draw overwrites (hash_map operator[] assignment);
// - budget B_a = 0.5L * (I / A) * scaling, with integer I / A (R/instance.cpp:136-141).
int oracle_gen_adalloc(int A, int I, double sparsity, double scaling, int64_t* nnz,
                       int32_t* adv, int32_t* imp, double* bid, double* budgets,
                       int32_t* draws_per_adv, double* max_bid) {
    if (A <= 0 || I <= 0 || !nnz) return -1;
    std::vector<std::map<int, double>> rows(A);
    srand(1);
    long double mb = 0;
    const long double bound = (long double)sparsity * (long double)I;
    for (int a = 0; a < A; ++a) {
        int draws = 0;
        for (int i = 0; i < bound; ++i) {
            int index = rand() % I;
            long double b = (long double)(rand() + 1) / ((long double)RAND_MAX);
            if (mb < b) mb = b;
            rows[a][index] = (double)b;
            ++draws;
        }
        if (draws_per_adv) draws_per_adv[a] = draws;
    }
    int64_t k = 0;
    for (int a = 0; a < A; ++a)
        for (auto& kv : rows[a]) {
            if (adv) { adv[k] = a; imp[k] = kv.first; bid[k] = kv.second; }
            ++k;
        }
    *nnz = k;
    if (budgets)
        for (int a = 0; a < A; ++a)
            budgets[a] = (double)(0.5L * (long double)(I / A) * (long double)scaling);
    if (max_bid) *max_bid = (double)mb;
    return 0;
}

int oracle_solve_dense(int64_t m, int64_t n, const double* A, const double* b, const double* c,
                       const oracle_opts* opt, double* x, double* y, double* obj,
                       int32_t* basis, oracle_pivot* log, int64_t log_cap, int64_t* npivots,
                       int* status) {
    if (m <= 0 || n <= 0 || !A || !b || !c || !opt) return -1;
    for (int64_t i = 0; i < m; ++i)
        if (!(b[i] >= 0.0)) return -1;
    Tab t;
    tab_init(t, m, n, 0, m, opt);
    tab_fill_dense(t, A, b, c);
    int st = 4;
    int64_t k = 0;
    while (k < opt->max_pivots) {
        st = pivot_once(t);
        if (st != 4) break;
        ++k;
    }
    if (st == 4) st = 3;
    if (status) *status = st;
    if (npivots) *npivots = (int64_t)t.log.size();
    if (x) {
        for (int64_t j = 0; j < n; ++j) x[j] = 0.0;
        for (int64_t i = 0; i < m; ++i)
            if (t.basis[i] < n) x[t.basis[i]] = t.row(i)[t.N];
    }
    if (y)
        for (int64_t i = 0; i < m; ++i) y[i] = t.row(m)[n + i];
    if (obj) *obj = t.row(m)[t.N];
    if (basis) std::memcpy(basis, t.basis.data(), sizeof(int32_t) * m);
    if (log) {
        int64_t cnt = std::min<int64_t>(log_cap, (int64_t)t.log.size());
        std::memcpy(log, t.log.data(), sizeof(oracle_pivot) * cnt);
    }
    return 0;
}

int oracle_slice_create(int64_t m, int64_t n, const double* A, const double* b, const double* c,
                        int64_t row_first, int64_t row_count, const oracle_opts* opt,
                        oracle_slice** out) {
    if (!out || row_first < 0 || row_count < 0 || row_first + row_count > m) return -1;
    auto* s = new oracle_slice();
    tab_init(s->t, m, n, row_first, row_count, opt);
    tab_fill_dense(s->t, A, b, c);
    *out = s;
    return 0;
}

int oracle_slice_candidate(oracle_slice* s, oracle_cand* cand, int* optimal) {
    Tab& t = s->t;
    t.q = price(t);
    *optimal = t.q < 0;
    if (t.q < 0) { std::memset(cand, 0, sizeof(*cand)); return 0; }
    *cand = local_ratio(t, t.q);
    return 0;
}

int oracle_slice_select(oracle_slice* s, const oracle_cand* cands, int n, int64_t* prow_send,
                        int* unbounded) {
    Tab& t = s->t;
    oracle_cand best{};
    for (int r = 0; r < n; ++r)
        if (cand_better(cands[r], best)) best = cands[r];
    *unbounded = !best.valid;
    if (!best.valid) return 0;
    record_pivot(t, best);
    if (t.p_local >= 0) {
        make_prow(t);
        std::memcpy(prow_send, t.prow.data(), sizeof(double) * t.ld);
    } else {
        for (int64_t j = 0; j < t.ld; ++j) prow_send[j] = std::numeric_limits<int64_t>::min();
    }
    return 0;
}

int oracle_slice_update(oracle_slice* s, const int64_t* prow_recv) {
    Tab& t = s->t;
    std::memcpy(t.prow.data(), prow_recv, sizeof(double) * t.ld);
    eliminate(t);
    return 0;
}

int64_t oracle_slice_ld(const oracle_slice* s) { return s->t.ld; }
int64_t oracle_slice_npivots(const oracle_slice* s) { return (int64_t)s->t.log.size(); }
int oracle_slice_log(const oracle_slice* s, oracle_pivot* log, int64_t cap) {
    int64_t cnt = std::min<int64_t>(cap, (int64_t)s->t.log.size());
    std::memcpy(log, s->t.log.data(), sizeof(oracle_pivot) * cnt);
    return 0;
}
int oracle_slice_tableau(const oracle_slice* s, double* T) {
    std::memcpy(T, s->t.T.data(), sizeof(double) * s->t.T.size());
    return 0;
}
void oracle_slice_free(oracle_slice* s) { delete s; }

int oracle_run_generated(int kind, int64_t m, int64_t n, uint64_t seed, int64_t k, int32_t nthreads,
                         oracle_pivot* log, int64_t* npivots, const int64_t* rows_idx,
                         int64_t nrows, double* rows_out, int32_t* basis_out) {
    oracle_opts o{};
    o.pricing = 0; o.tol_dj = 1e-9; o.tol_piv = 1e-9; o.max_pivots = k; o.nthreads = nthreads;
    Tab t;
    tab_init(t, m, n, 0, m, &o);
    if (oracle_gen_tableau(kind, m, n, seed, 0, m, t.ld, t.T.data(), nthreads) != 0) return -1;
    for (int64_t i = 0; i < k; ++i)
        if (pivot_once(t) != 4) break;
    *npivots = (int64_t)t.log.size();
    std::memcpy(log, t.log.data(), sizeof(oracle_pivot) * t.log.size());
    for (int64_t r = 0; r < nrows; ++r)
        std::memcpy(rows_out + r * t.ld, t.row(rows_idx[r]), sizeof(double) * t.ld);
    if (basis_out) std::memcpy(basis_out, t.basis.data(), sizeof(int32_t) * m);
    return 0;
}

// Checkpointed run (tests/golden/make_digests.py: whole-tableau digests): the
// generated LP pivoted through ascending stops[]; at each stop cb sees the whole
// (m+1) x ld tableau (objective row last), the log so far and the basis.
int oracle_run_generated_stops(int kind, int64_t m, int64_t n, uint64_t seed, int32_t nthreads,
                               const int64_t* stops, int nstops, oracle_stop_cb cb, void* user) {
    oracle_opts o{};
    o.pricing = 0; o.tol_dj = 1e-9; o.tol_piv = 1e-9; o.nthreads = nthreads;
    o.max_pivots = nstops > 0 ? stops[nstops - 1] : 0;
    Tab t;
    tab_init(t, m, n, 0, m, &o);
    if (oracle_gen_tableau(kind, m, n, seed, 0, m, t.ld, t.T.data(), nthreads) != 0) return -1;
    for (int s = 0; s < nstops; ++s) {
        while ((int64_t)t.log.size() < stops[s])
            if (pivot_once(t) != 4) return -6;   // the LP ended before the stop
        cb((int64_t)t.log.size(), t.T.data(), t.ld, m + 1, t.log.data(), t.basis.data(), user);
    }
    return 0;
}

int oracle_bench_pivots(int kind, int64_t m, int64_t n, uint64_t seed, int64_t warmup, int64_t k,
                        int32_t nthreads, double* seconds, int64_t* done, double* gen_seconds) {
    using clk = std::chrono::steady_clock;
    oracle_opts o{};
    o.pricing = 0; o.tol_dj = 1e-9; o.tol_piv = 1e-9; o.max_pivots = warmup + k;
    o.nthreads = nthreads;
    Tab t;
    auto g0 = clk::now();
    tab_init(t, m, n, 0, m, &o);
    if (oracle_gen_tableau(kind, m, n, seed, 0, m, t.ld, t.T.data(), nthreads) != 0) return -1;
    auto g1 = clk::now();
    if (gen_seconds) *gen_seconds = std::chrono::duration<double>(g1 - g0).count();
    for (int64_t i = 0; i < warmup; ++i)
        if (pivot_once(t) != 4) return -6;
    auto t0 = clk::now();
    int64_t cnt = 0;
    for (; cnt < k; ++cnt)
        if (pivot_once(t) != 4) break;
    auto t1 = clk::now();
    *seconds = std::chrono::duration<double>(t1 - t0).count();
    if (done) *done = cnt;
    return 0;
}

// bench.py cpu_baseline: one generated LP (gen_threads), one warm-up pivot, then
// nrun consecutive timed windows on the same tableau, window r with threads[r]
// OpenMP threads, each ending after max_k[r] pivots or once budget_s[r] seconds
// have passed (checked after every pivot).  secs[r] / done[r] per window.
int oracle_bench_windows(int kind, int64_t m, int64_t n, uint64_t seed, int32_t gen_threads,
                         int nrun, const int32_t* threads, const int64_t* max_k,
                         const double* budget_s, double* secs, int64_t* done,
                         double* gen_seconds) {
    using clk = std::chrono::steady_clock;
    oracle_opts o{};
    o.pricing = 0; o.tol_dj = 1e-9; o.tol_piv = 1e-9; o.max_pivots = 1 << 30;
    o.nthreads = gen_threads;
    Tab t;
    auto g0 = clk::now();
    tab_init(t, m, n, 0, m, &o);
    if (oracle_gen_tableau(kind, m, n, seed, 0, m, t.ld, t.T.data(), gen_threads) != 0) return -1;
    if (gen_seconds) *gen_seconds = std::chrono::duration<double>(clk::now() - g0).count();
    if (pivot_once(t) != 4) return -6;
    for (int r = 0; r < nrun; ++r) {
        t.nthreads = threads[r] > 0 ? threads[r] : 1;
        auto t0 = clk::now();
        int64_t cnt = 0;
        double el = 0.0;
        while (cnt < max_k[r]) {
            if (pivot_once(t) != 4) break;
            ++cnt;
            el = std::chrono::duration<double>(clk::now() - t0).count();
            if (el >= budget_s[r]) break;
        }
        secs[r] = el;
        done[r] = cnt;
    }
    return 0;
}

}  // extern "C"

#include "oracle_defer.inc"
#include "oracle_dual.inc"
