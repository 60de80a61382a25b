"""numpy statement of the column rule of dlp_batch_add_cols (include/dlp.h) and of
the primal phase that follows it, on the full layout that ``Batch.read(k)`` returns; shared by
tests/test_batch_add_cols_api.py (CPU: against the C++ oracle's pivot log and against HiGHS) and
tests/test_gpu_batch_add_cols.py (GPU, bit for bit).

``add_cols`` yields the widened (T', basis'); ``primal_phase`` is dlp_batch_resolve(c = NULL)'s
loop (the pivot rule of dlp.h's header) with rhs_ref's update: IEEE division for the pivot row,
a real fma elsewhere, rows with a zero in the entering column untouched.

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import numpy as np

import rhs_ref as RR
from rows_ref import tableau_ld

OK, UNBOUNDED, PIVOT_LIMIT = 0, 2, 3
PIVOT_DTYPE = RR.PIVOT_DTYPE


def add_cols(T, basis, n, P, d):
    """(T, basis) as Batch.read returns them ((m+1) x >= N+1, the RHS in column N = n + m; not
    modified), P (m, k), d (k,).  Returns the full layout of the widened LP,
    (m+1) x tableau_ld(m, n+k), and its basis with every index >= n shifted by k.

    New variable t, every row r (the objective row included): acc = +0.0, then for l ascending
    acc = acc + (T[r][n+l] * p_l) (numpy rounds the product, then the sum); the objective entry
    less d_t.  In the full layout a basic slack's column is its row's unit vector with objective
    entry +0.0, so no term needs skipping: a +-0 coefficient changes no bit of acc."""
    T = np.asarray(T, dtype=np.float64)
    basis = np.asarray(basis, dtype=np.int32)
    m = len(basis)
    P = np.asarray(P, dtype=np.float64).reshape(m, -1)
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    k = P.shape[1]
    assert T.shape[0] == m + 1 and len(d) == k
    N, n2 = n + m, n + k
    N2 = n2 + m
    Tn = np.zeros((m + 1, tableau_ld(m, n2)))
    Tn[:, :n], Tn[:, n2:N2], Tn[:, N2] = T[:, :n], T[:, n:N], T[:, N]
    for t in range(k):
        acc = np.zeros(m + 1)
        for ell in range(m):
            prod = T[:, n + ell] * P[ell, t]
            acc = acc + prod
        acc[m] = acc[m] - d[t]
        Tn[:, n + t] = acc
    return Tn, np.where(basis >= n, basis + k, basis).astype(np.int32)


def primal_phase(T, basis, n, max_pivots=10 ** 6, pricing=0, bland=None, tol_dj=1e-9, tol_piv=1e-9):
    """The primal simplex from the basic feasible full-layout tableau (T, basis) (not modified).
    bland: the Bland state to start from (None: reset from the pricing option, as a fresh phase
    is).  Returns rhs_ref.resolve_rhs's dict: status (PIVOT_LIMIT when the budget ran out before
    the pricing saw optimality: max_pivots = 0 always does), done, objective, x, y, basis, log
    (PIVOT_DTYPE), T (the full layout afterwards), bland (the Bland state afterwards)."""
    T = np.array(T, dtype=np.float64)
    basis = np.array(basis, dtype=np.int32)
    m = len(basis)
    N = n + m
    isbasic = np.zeros(N, bool)
    isbasic[basis] = True
    bland = pricing == 1 if bland is None else bool(bland)
    log = []
    k = 0
    while True:
        if k >= max_pivots:
            status = PIVOT_LIMIT
            break
        nb = np.nonzero(~isbasic)[0]
        z = T[m, nb]
        neg = nb[z < -tol_dj]
        if bland:
            q = int(neg[0]) if len(neg) else -1
        else:   # min z, ties -> the smallest variable (argmin takes the first)
            j = int(np.argmin(z))
            q = int(nb[j]) if z[j] < -tol_dj else -1
        if q < 0:
            status = OK
            break
        elig = np.nonzero(T[:m, q] > tol_piv)[0]
        if len(elig) == 0:
            status = UNBOUNDED
            break
        rhs = T[elig, N]
        ratio = np.where(rhs > 0.0, rhs, 0.0) / T[elig, q]
        best = ratio.min()
        ties = elig[ratio == best]
        p = int(ties[np.argmin(basis[ties])])
        leaving = int(basis[p])
        piv = T[p, q]
        colq = T[:, q].copy()
        cols = np.concatenate([nb, [leaving, N]])
        cols = cols[cols != q]
        prow = T[p, cols] / piv
        rows = np.nonzero(colq != 0.0)[0]
        T[np.ix_(rows, cols)] = RR.fma(-colq[rows, None], prow[None, :], T[np.ix_(rows, cols)])
        T[p, cols] = prow
        basis[p] = q
        isbasic[q], isbasic[leaving] = True, False
        T[:, q] = 0.0            # the condensed tableau stores no basic column: an exact unit vector
        T[p, q] = 1.0
        bland = True if pricing == 1 else bool(best == 0.0)
        log.append((q, p, leaving, 0, best, T[m, N]))
        k += 1
    x = np.zeros(n)
    y = np.zeros(m)
    for i in range(m):
        if basis[i] < n:
            x[basis[i]] = T[i, N]
        if not isbasic[n + i]:
            y[i] = T[m, n + i]
    return dict(status=status, done=k, objective=T[m, N], x=x, y=y, basis=basis,
                log=np.array(log, dtype=PIVOT_DTYPE), T=T, bland=bland)


def add_cols_and_solve(T, basis, n, P, d, **kw):
    """The whole call on one accepted LP: the rule, then the primal phase on n + k variables."""
    T2, basis2 = add_cols(T, basis, n, P, d)
    return primal_phase(T2, basis2, n + np.asarray(d).size, **kw)


def duals(T, basis, n):
    """y of the basis as it stands: slack l's objective-row entry (a basic slack: +0.0)."""
    m = len(basis)
    return np.array(T[m, n:n + m], dtype=np.float64)


def columns(y, k, seed, depth=0.1):
    """k columns that price out attractive at the duals y: P ~ U[0, 1) with about 30 % zeros,
    d = (y . P) (1 + depth u), u ~ U[0, 1), seeded (depth < 0: unattractive; a column with
    y . p = 0 has reduced cost 0 and does not enter)."""
    rng = np.random.default_rng(seed)
    m = len(y)
    P = rng.uniform(0.0, 1.0, (m, k)) * (rng.uniform(size=(m, k)) >= 0.3)
    d = (np.asarray(y) @ P) * (1.0 + depth * rng.uniform(0.0, 1.0, k))
    return P, d
