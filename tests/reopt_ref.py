"""numpy reference of the objective-row rule of dlp_session_set_objective (include/dlp.h,
DESIGN.md §18), shared by tests/test_reopt_api.py (CPU) and tests/test_gpu_reopt.py (GPU),
plus the helpers both need: the perturbed objective, a plain numpy simplex that continues from
a given tableau, and the oracle's tableau after k pivots.

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import numpy as np

import oracle_py as O


def objective_row(T, basis, c):
    """The rule: T holds the m constraint rows in the full layout (columns 0..N-1 the
    variables, N the RHS, then padding), basis[i] the basic variable of row i, c the n new
    costs.  z starts at -c_j (structural) / +0.0 (slack, RHS, padding); rows are folded in
    ascending order, rows whose basic variable costs 0.0 skipped, as z = z + (cB_i * T[i])
    (numpy rounds the product, then the sum: no fma); basic variables get +0.0."""
    basis = np.asarray(basis)
    c = np.asarray(c, dtype=np.float64)
    m, n = len(basis), len(c)
    z = np.zeros(T.shape[1])
    z[:n] = -c
    for i in range(m):
        v = int(basis[i])
        cb = c[v] if v < n else 0.0
        if cb == 0.0:
            continue
        z = z + cb * T[i]
    z[basis] = 0.0
    return z


def make_c2(c, seed, scale=0.3, holes=True):
    """c * (1 + scale * u), u ~ U(-1, 1) seeded; holes: every 7th entry 0 (a skipped row once
    basic, a -0.0 start) and every 11th negated."""
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, len(c))
    c2 = np.asarray(c, dtype=np.float64) * (1.0 + scale * u)
    if holes:
        c2[::7] = 0.0
        c2[::11] = -c2[::11]
    return np.ascontiguousarray(c2)


def basis_from_log(m, n, log):
    basis = np.arange(n, n + m, dtype=np.int32)
    for e in log:
        basis[e["p"]] = e["q"]
    return basis


def oracle_tableau(A, b, c, k):
    """The oracle's tableau ((m+1) x ld, objective row last) and basis after k pivots of the
    cold solve of (A, b, c), through a one-rank OracleEngine."""
    m, n = A.shape
    e = O.OracleEngine(A, b, c, 0, 1, 0, m)
    try:
        for _ in range(k):
            cand = e.step_candidate()
            if e.state != 4:
                break
            bits = e.step_select(cand)
            if e.state != 4:
                break
            e.step_update(bits)
        T = np.zeros((m + 1, e.ld))
        O.lib().oracle_slice_tableau(e.h, O._d(T))
        return T, basis_from_log(m, n, e.log())
    finally:
        e.close()


def simplex_continue(T, basis, n, tol_dj=1e-9, tol_piv=1e-9, max_pivots=100000):
    """A plain numpy tableau simplex from the basic feasible tableau T ((m+1) x >= N+1,
    objective row last; modified in place): Dantzig pricing, Bland after a degenerate pivot,
    the ratio test of the pivot rule.  Returns (status, pivots): 0 optimal, 2 unbounded."""
    m = len(basis)
    N = n + m
    basis = np.array(basis)
    bland = False
    for k in range(max_pivots):
        z = T[m, :N]
        if bland:
            neg = np.nonzero(z < -tol_dj)[0]
            if len(neg) == 0:
                return 0, k
            q = int(neg[0])
        else:
            q = int(np.argmin(z))
            if not z[q] < -tol_dj:
                return 0, k
        col = T[:m, q]
        elig = np.nonzero(col > tol_piv)[0]
        if len(elig) == 0:
            return 2, k
        ratio = np.maximum(T[elig, N], 0.0) / col[elig]
        best = ratio.min()
        ties = elig[ratio == best]
        p = int(ties[np.argmin(basis[ties])])
        bland = best == 0.0
        T[p] = T[p] / T[p, q]
        for i in range(m + 1):
            if i != p and T[i, q] != 0.0:
                T[i] = T[i] - T[i, q] * T[p]
        basis[p] = q
    return 3, max_pivots
