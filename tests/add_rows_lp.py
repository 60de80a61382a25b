"""Inputs of the dlp_session_add_rows tests, shared by
tests/test_session_add_rows_api.py (CPU: every property claimed here, on the C++ oracle alone) and
tests/test_gpu_session_add_rows.py (GPU, bit for bit).

CASES       (m, n, r): the (shape, r) pairs of the GPU file
lp          the LP of a shape: tests/dual_lp.py's dense LPs; O.gen_dense at 5 x 7 and 37 x 58
cut_rows    rows_ref.cuts at the cold optimum x*, seed 7800 + r, depth 0.1
slack_rows  the same G with h = 2 G x* (every row slack: 0 dual pivots)
INFEASIBLE  g = 1, h = -1: no x >= 0 satisfies it
counted     a row with nonzeros on exactly R basic structural variables (the fold's batch edges)
grouped     r rows for one group of the fold: row 1 is zero where row 0 has its nonzeros (and the
            other way round), row 2 carries -0.0 coefficients (skipped rows)

B, RT: the batch length and the group size of row_fold_kernel (kFoldRows, kFoldRT in
dlp_addrows.hip; tests/test_session_add_rows_isa.py reads them from the source).

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import functools

import numpy as np

import dual_lp as D
import oracle_py as O
import reopt_ref as R
import rows_ref as AR

B, RT = 16, 4
BIG = D.BIG

# (m, n, r).  5 x 7: r = 5 crosses a 16-column stride (N + 1 = 13 -> 18); 37 x 58: N + 1 = 96, so
# r = 1 changes the full layout's stride; 65 x 449: r = RT - 1, RT, RT + 1
CASES = [(5, 7, 1), (5, 7, 2), (5, 7, 5), (37, 58, 1), (63, 70, 2), (64, 66, 4),
         (65, 449, 3), (65, 449, 4), (65, 449, 5), (300, 740, 3)]
SMALL_SEED = {(5, 7): 1, (37, 58): 2}
COUNT_SHAPE = (65, 449)          # its optimum has >= 2 B + 1 basic structural variables
COUNTS = [0, 1, B - 1, B, B + 1, 2 * B + 1]
INFEASIBLE_SHAPE = (65, 449)
DEGENERATE = [(65, 449, 3), (37, 58, 4)]   # (m, n, seed) of O.gen_dense(degenerate=True)


@functools.lru_cache(maxsize=None)
def lp(m, n):
    """(A, b, c), read-only."""
    if (m, n) in SMALL_SEED:
        return D._frozen(O.gen_dense(m, n, SMALL_SEED[(m, n)]))
    return D.dense_lp(m, n)[:3]


@functools.lru_cache(maxsize=None)
def cold(m, n):
    """(T0, basis0, x*, objective, pivots) of the oracle's cold solve (the GPU tests take the
    session's own read-out)."""
    A, b, c = lp(m, n)
    T, basis = R.oracle_tableau(A, b, c, BIG)
    ref = O.solve_dense(A, b, c)
    assert ref.status == 0 and ref.basis.tobytes() == basis.tobytes()
    return T, basis, ref.x, ref.objective, ref.num_pivots


def cut_rows(x, n, r, depth=0.1):
    return AR.cuts(np.asarray(x), n, r, 7800 + r, depth=depth)


def slack_rows(x, n, r):
    G, _ = cut_rows(x, n, r)
    return G, 2.0 * (G @ np.asarray(x))


def infeasible_row(n):
    return np.ones((1, n)), np.array([-1.0])


def counted(basis, x, n, R_, seed=7900):
    """One row (G (1, n), h) with nonzeros on exactly R_ basic structural variables (the first R_
    rows that hold one) and on a third of the nonbasic ones, cutting x off by 10 %."""
    rng = np.random.default_rng(seed + R_)
    basis = np.asarray(basis)
    bs = basis[basis < n]
    assert len(bs) >= R_, (len(bs), R_)
    g = np.zeros(n)
    nonbasic = np.setdiff1d(np.arange(n), bs)
    pick = nonbasic[rng.uniform(size=len(nonbasic)) < 1 / 3]
    g[pick] = rng.uniform(0.1, 1.0, len(pick))
    g[bs[:R_]] = rng.uniform(0.1, 1.0, R_)
    h = 0.9 * float(g @ np.asarray(x))
    return g.reshape(1, n), np.array([h])


def grouped(basis, x, n, r, seed=7950):
    """r rows: row 0 has nonzeros on the even-numbered basic structural variables only, row 1 on
    the odd-numbered ones only, row 2 (if any) is row 0 with -0.0 where row 0 is zero among the
    basic ones, the others are dense random rows.  Each cuts x off by 10 %."""
    rng = np.random.default_rng(seed + r)
    basis = np.asarray(basis)
    bs = basis[basis < n]
    assert len(bs) >= 4
    G = rng.uniform(0.1, 1.0, (r, n))
    if r > 0:
        G[0, bs[1::2]] = 0.0
    if r > 1:
        G[1, bs[0::2]] = 0.0
    if r > 2:
        G[2] = G[0]
        G[2, bs[1::2]] = -0.0
    h = 0.9 * (G @ np.asarray(x))
    return G, h


def reference(T0, basis0, n, G, h, pricing=0, max_pivots=BIG):
    """The reference of a whole call on a read-out: the rule (tests/rows_ref.py), then the C++ dual
    oracle continuing from the grown tableau with the Bland state reset.  Returns (T2, basis2, ref)."""
    T2, basis2 = AR.add_rows(T0, basis0, n, G, h)
    ref = O.resolve_rhs(T2, basis2, n, np.zeros(len(basis2)), continued=False, pricing=pricing,
                        max_pivots=max_pivots)
    return T2, basis2, ref
