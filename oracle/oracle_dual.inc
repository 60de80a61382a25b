// oracle_dual.inc — TEST INFRASTRUCTURE ONLY (included by oracle.cpp).
//
// The dual rule of include/dlp.h (dlp_batch_resolve_rhs; dlp_session_set_rhs applies it to a
// session's tableau) on a full-layout tableau, (m+1) x ld, objective row last, basic columns
// exact unit vectors: the RHS fold and dual pivots from the basis as it stands.  Restated from
// the header's text, not from the HIP code; tests/test_oracle_dual.py pins it bit for bit to the
// numpy reference tests/rhs_ref.py (itself held against HiGHS) wherever that one is affordable.
//
//   fold      for every stored row r = 0 .. m: acc = +0.0; l ascending: acc = acc + (T[r][n+l] * b_l),
//             product rounded, then the sum; T[r][N] = acc
//   leaving   rows i < m with T[i][N] < -tol_feas; the most negative, exact ties to the smallest
//             basis[i]; Bland mode: the eligible row with the smallest basis[i]
//   stops     no eligible row -> OK, tested before the budget -> PIVOT_LIMIT
//   entering  nonbasic j < N with a = T[p][j] < -tol_piv; r = zc / (-a), zc = z_j > 0 ? z_j : +0.0;
//             the smallest r, ties to the smallest j; none -> INFEASIBLE
//   update    over the nonbasic columns but q, the leaving variable's column and the RHS:
//             pivot row divided by the pivot; rows with T[i][q] != 0 (the objective row is one of
//             them) take fma(-T[i][q], prow[c], T[i][c]); column q becomes the unit vector of row p
//             (objective entry +0.0).  The other basic columns are not touched.
//   Bland     on for pricing 1; else entered after a pivot with r_q == 0, left after one with r_q > 0
// Serial.  Compiled for the FMA instruction set as oracle_defer.inc is (std::fma then is one
// instruction, not a libm call: a pivot of a 300 x 1040 tableau takes about 0.3 ms instead of 0.6);
// -ffp-contract=off as everywhere in the oracle, so nothing else is fused.

namespace {

constexpr int kDualOk = 0, kDualInfeasible = 1, kDualPivotLimit = 3, kDualErrArg = -1, kDualErrState = -6;

}  // namespace

extern "C" __attribute__((target("fma")))
int oracle_resolve_rhs(int64_t m, int64_t n, int64_t ld, double* T, int32_t* basis, const double* b,
                       const oracle_opts* opt, double tol_feas, int rebuild, int* bland_io,
                       oracle_pivot* log, int64_t log_cap, int64_t* npivots, int* status) {
    if (npivots) *npivots = 0;
    const int64_t N = n + m;
    if (m <= 0 || n <= 0 || ld < N + 1 || !T || !basis || !b || !opt) {
        if (status) *status = kDualErrArg;
        return kDualErrArg;
    }
    // the refusals, in the header's order; T and basis untouched
    for (int64_t l = 0; l < m; ++l)
        if (!std::isfinite(b[l])) {
            if (status) *status = kDualErrArg;
            return kDualErrArg;
        }
    std::vector<char> isbasic((size_t)N, 0);
    for (int64_t i = 0; i < m; ++i) {
        if (basis[i] < 0 || basis[i] >= N) {
            if (status) *status = kDualErrArg;
            return kDualErrArg;
        }
        isbasic[basis[i]] = 1;
    }
    double* const z = T + m * ld;
    for (int64_t j = 0; j < N; ++j)
        if (!isbasic[j] && z[j] < -opt->tol_dj) {
            if (status) *status = kDualErrState;
            return kDualErrState;
        }

    if (rebuild)
        for (int64_t r = 0; r <= m; ++r) {
            const double* slack = T + r * ld + n;
            double acc = 0.0;
            for (int64_t l = 0; l < m; ++l) {
                const double prod = slack[l] * b[l];
                acc = acc + prod;
            }
            T[r * ld + N] = acc;
        }

    bool bland = opt->pricing == 1 || (!rebuild && bland_io && *bland_io);
    std::vector<double> colq((size_t)m + 1), prow((size_t)N + 1);
    std::vector<int64_t> cols;
    cols.reserve((size_t)n + 2);
    int64_t k = 0;
    int st;
    for (;;) {
        // leaving row
        int64_t p = -1;
        for (int64_t i = 0; i < m; ++i) {
            const double rhs = T[i * ld + N];
            if (!(rhs < -tol_feas)) continue;
            if (p < 0) { p = i; continue; }
            const double cur = T[p * ld + N];
            const bool better = bland ? basis[i] < basis[p]
                                      : (rhs < cur || (rhs == cur && basis[i] < basis[p]));
            if (better) p = i;
        }
        if (p < 0) { st = kDualOk; break; }
        if (k >= opt->max_pivots) { st = kDualPivotLimit; break; }
        // entering column
        const double* rp = T + p * ld;
        int64_t q = -1;
        double best = std::numeric_limits<double>::infinity();
        for (int64_t j = 0; j < N; ++j) {
            if (isbasic[j]) continue;
            const double a = rp[j];
            if (!(a < -opt->tol_piv)) continue;
            const double zc = z[j] > 0.0 ? z[j] : 0.0;
            const double r = zc / (-a);
            if (r < best || (q < 0 && r == best)) { best = r; q = j; }
        }
        if (q < 0) { st = kDualInfeasible; break; }
        // update
        const int32_t leaving = basis[p];
        const double piv = rp[q];
        for (int64_t i = 0; i <= m; ++i) colq[i] = T[i * ld + q];
        cols.clear();
        for (int64_t j = 0; j < N; ++j)
            if ((!isbasic[j] && j != q) || j == leaving) cols.push_back(j);
        cols.push_back(N);
        for (int64_t c : cols) prow[c] = rp[c] / piv;
        for (int64_t i = 0; i <= m; ++i) {
            if (i == p || colq[i] == 0.0) continue;
            double* ri = T + i * ld;
            const double f = -colq[i];
            for (int64_t c : cols) ri[c] = std::fma(f, prow[c], ri[c]);
        }
        double* wp = T + p * ld;
        for (int64_t c : cols) wp[c] = prow[c];
        for (int64_t i = 0; i <= m; ++i) T[i * ld + q] = 0.0;
        wp[q] = 1.0;
        basis[p] = (int32_t)q;
        isbasic[q] = 1;
        isbasic[leaving] = 0;
        bland = opt->pricing == 1 ? true : best == 0.0;
        if (log && k < log_cap) {
            oracle_pivot e;
            e.q = (int32_t)q;
            e.p = (int32_t)p;
            e.leaving = leaving;
            e.pad = 0;
            e.ratio = best;
            e.objective = z[N];
            log[k] = e;
        }
        ++k;
    }
    if (npivots) *npivots = k;
    if (bland_io) *bland_io = bland ? 1 : 0;
    if (status) *status = st;
    return 0;
}
