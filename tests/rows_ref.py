"""numpy statement of the row rule of dlp_batch_add_rows (include/dlp.h) on the
full layout that ``Batch.read(k)`` returns, shared by tests/test_batch_add_rows_api.py (CPU,
against HiGHS) and tests/test_gpu_batch_add_rows.py (GPU, bit for bit).

``add_rows`` yields the grown (T', basis').  The dual phase that follows is
``rhs_ref.resolve_rhs(T', basis', n, <any finite vector>, continued=False)``: with continued not
None that function folds nothing, and a false value resets the Bland state.

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import numpy as np

import rhs_ref as RR


def tableau_ld(m, n):
    """dlp_tableau_ld: the N + 1 columns rounded up to 16."""
    return (n + m + 1 + 15) // 16 * 16


def add_rows(T, basis, n, G, h):
    """(T, basis) as Batch.read returns them ((m+1) x >= N+1, the RHS in column N = n + m; not
    modified), G (r, n), h (r,).  Returns the full layout of the grown LP,
    (m+r+1) x tableau_ld(m+r, n), and its basis of m + r entries.

    New row t, for every stored (nonbasic) column v and for the RHS: acc = g_v (structural),
    +0.0 (slack), h_t (RHS); then for the old rows i ascending with gB_i = g[basis[i]]
    (a basic slack: +0.0), rows with gB_i == 0.0 skipped, acc = acc - (gB_i * T[i][v]) (numpy
    rounds the product, then the difference).  Basic columns are exact +0.0, the row's own
    slack 1.0.  Old rows and the objective row keep their bits."""
    T = np.asarray(T, dtype=np.float64)
    basis = np.asarray(basis, dtype=np.int32)
    G = np.asarray(G, dtype=np.float64).reshape(-1, n)
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    m, r = len(basis), G.shape[0]
    assert T.shape[0] == m + 1 and len(h) == r
    N, m2 = n + m, m + r
    N2 = n + m2
    Tn = np.zeros((m2 + 1, tableau_ld(m2, n)))
    Tn[:m, :N], Tn[:m, N2] = T[:m, :N], T[:m, N]
    Tn[m2, :N], Tn[m2, N2] = T[m, :N], T[m, N]
    cols = np.r_[np.arange(N), N]                  # every variable's column, then the RHS
    for t in range(r):
        g = G[t]
        acc = np.zeros(N + 1)
        acc[:n] = g
        acc[N] = h[t]
        for i in range(m):
            gb = g[basis[i]] if basis[i] < n else 0.0
            if gb == 0.0:
                continue
            acc = acc - gb * T[i, cols]
        acc[basis] = 0.0                           # a basic column is stored nowhere: exact +0.0
        Tn[m + t, :N], Tn[m + t, N2] = acc[:N], acc[N]
        Tn[m + t, N + t] = 1.0
    return Tn, np.concatenate([basis, N + np.arange(r, dtype=np.int32)]).astype(np.int32)


def dual_phase(T2, basis2, n, continued=False, **kw):
    """The dual phase of the call on the grown tableau: no fold, the Bland state reset.
    continued: the Bland state a pending LP was left in, for an r = 0 call that continues it."""
    return RR.resolve_rhs(T2, basis2, n, np.zeros(len(basis2)), continued=bool(continued), **kw)


def add_rows_and_solve(T, basis, n, G, h, **kw):
    """The whole call on one accepted LP: the rule, then the dual phase.  An LP that is not dual
    feasible comes back from resolve_rhs as ERR_STATE with the grown (T', basis') unchanged."""
    T2, basis2 = add_rows(T, basis, n, G, h)
    return dual_phase(T2, basis2, n, **kw)


def cuts(x, n, r, seed, depth=0.1):
    """r rows that cut x off: G ~ U[0, 1) with about 30 % zeros, h = (G x) (1 - depth u),
    u ~ U[0, 1), seeded (a row with G x = 0 is tight, not violated)."""
    rng = np.random.default_rng(seed)
    G = rng.uniform(0.0, 1.0, (r, n)) * (rng.uniform(size=(r, n)) >= 0.3)
    h = (G @ x) * (1.0 - depth * rng.uniform(0.0, 1.0, r))
    return G, h
