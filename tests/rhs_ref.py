"""numpy reference of dlp_batch_resolve_rhs (include/dlp.h) on the full layout
that ``Batch.read(k)`` returns: the RHS fold and the dual simplex, shared by
tests/test_batch_rhs_api.py (CPU, against HiGHS) and tests/test_gpu_batch_rhs.py (GPU, bit for
bit).  No single-LP dual path exists, so this is the yardstick.

The elimination is a real fma (``fma`` of libm through ctypes: Python 3.10 has no math.fma);
the fold rounds the product, then the sum (numpy does not contract the two).

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import ctypes
import ctypes.util

import numpy as np

OK, INFEASIBLE, PIVOT_LIMIT, ERR_ARG, ERR_STATE = 0, 1, 3, -1, -6
PIVOT_DTYPE = np.dtype([("q", "<i4"), ("p", "<i4"), ("leaving", "<i4"), ("pad", "<i4"),
                        ("ratio", "<f8"), ("objective", "<f8")])

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma = np.frompyfunc(_libm.fma, 3, 1)


def fma(a, b, c):
    """Elementwise fma(a, b, c), one rounding."""
    return np.asarray(_fma(a, b, c), dtype=np.float64)


def fold_rhs(T, n, b):
    """The RHS rebuild: T is (m+1) x >= N+1 in the full layout (basic columns exact unit
    vectors, objective entries +0.0), b the m new right-hand sides.  Returns the m+1 new RHS
    entries, the objective value last: acc = +0.0, then acc = acc + (T[r][n+l] * b_l) for l
    ascending (a +-0 coefficient changes no bit, so no term needs skipping)."""
    m = T.shape[0] - 1
    b = np.asarray(b, dtype=np.float64)
    acc = np.zeros(m + 1)
    for ell in range(m):
        prod = T[:, n + ell] * b[ell]
        acc = acc + prod
    return acc


def eligible_rows(rhs, tol_feas=1e-9):
    return np.nonzero(rhs < -tol_feas)[0]


def resolve_rhs(T, basis, n, b, max_pivots=10 ** 6, pricing=0, tol_dj=1e-9, tol_piv=1e-9, tol_feas=1e-9,
                continued=None):
    """dlp_batch_resolve_rhs on one LP: (T, basis) as Batch.read returns them (not modified).
    Returns a dict: status (PIVOT_LIMIT for a pending dual phase), done, objective, x, y, basis,
    log (PIVOT_DTYPE), T (the full layout afterwards), bland (the Bland state afterwards); for
    ERR_ARG / ERR_STATE T and basis are the inputs and the values NaN.
    continued: None, or the Bland state a pending dual phase was left in when b is the very b of
    the call that left it pending (the read-out shows neither): no rebuild, no reset."""
    T = np.array(T, dtype=np.float64)
    basis = np.array(basis, dtype=np.int32)
    m = len(basis)
    N = n + m
    b = np.asarray(b, dtype=np.float64)
    nan = np.full(1, np.nan)[0]
    refused = dict(done=0, objective=nan, x=np.full(n, np.nan), y=np.full(m, np.nan), basis=basis,
                   log=np.zeros(0, PIVOT_DTYPE), T=T)
    if not np.isfinite(b).all():
        return dict(refused, status=ERR_ARG)
    isbasic = np.zeros(N, bool)
    isbasic[basis] = True
    if (T[m, :N][~isbasic] < -tol_dj).any():
        return dict(refused, status=ERR_STATE)
    if continued is None:
        T[:, N] = fold_rhs(T, n, b)
    bland = pricing == 1 or bool(continued)
    log = []
    status = None
    k = 0
    while True:
        rhs = T[:m, N]
        elig = eligible_rows(rhs, tol_feas)
        if len(elig) == 0:
            status = OK
            break
        if k >= max_pivots:
            status = PIVOT_LIMIT
            break
        if bland:
            p = int(elig[np.argmin(basis[elig])])
        else:
            ties = elig[rhs[elig] == rhs[elig].min()]
            p = int(ties[np.argmin(basis[ties])])
        # entering variable: ascending variable index, strict improvement -> ties to the smallest
        best, q = np.inf, -1
        for j in np.nonzero(~isbasic)[0]:
            a = T[p, j]
            if a < -tol_piv:
                z = T[m, j]
                zc = z if z > 0.0 else 0.0
                r = zc / (-a)
                if r < best or (q < 0 and r == best):
                    best, q = r, int(j)
        if q < 0:
            status = INFEASIBLE
            break
        leaving = int(basis[p])
        piv = T[p, q]
        colq = T[:, q].copy()
        cols = np.concatenate([np.nonzero(~isbasic)[0], [leaving, N]])
        cols = cols[cols != q]
        prow = T[p, cols] / piv
        rows = np.nonzero(colq != 0.0)[0]
        sub = T[np.ix_(rows, cols)]
        T[np.ix_(rows, cols)] = fma(-colq[rows, None], prow[None, :], sub)
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
    for i in range(m):
        if not isbasic[n + i]:
            y[i] = T[m, n + i]
    return dict(status=status, done=k, objective=T[m, N], x=x, y=y, basis=basis,
                log=np.array(log, dtype=PIVOT_DTYPE), T=T, bland=bland)


def from_dense(A, b, c):
    """The full-layout tableau and slack basis of max c^T x, A x <= b, x >= 0 before any pivot
    (dual feasible when c <= 0)."""
    m, n = A.shape
    N = n + m
    T = np.zeros((m + 1, N + 1))
    T[:m, :n] = A
    T[:m, n:N] = np.eye(m)
    T[:m, N] = b
    T[m, :n] = -np.asarray(c, dtype=np.float64)
    return T, np.arange(n, N, dtype=np.int32)
