"""Inputs of the dlp_session_add_cols tests, shared by
tests/test_session_add_cols_api.py (CPU: every property claimed here, on the oracle and numpy alone)
and tests/test_gpu_session_add_cols.py (GPU, bit for bit).

CASES        (m, n, k): the (shape, k) pairs of the GPU file
lp, cold     tests/add_rows_lp.py's LPs and their cold optimum (oracle)
new_cols     cols_ref.columns at the cold duals y*, seed 7701 + k, depth 0.1 (attractive)
dull_cols    the same P with d below y* . p (reduced cost > 0: no pivot)
ray          p = 0, d = 1: the LP becomes unbounded
counted      one column with exactly `count` nonzero p_l (the fold's list-tile edges), negative
             entries among them
basic_only / nonbasic_only   one column with nonzeros only on rows whose slack is basic / nonbasic
grouped      CT columns for one group of the fold: column 1 is zero exactly where column 0 is not,
             column 2 carries -0.0 entries, column 3 negative entries and a negative cost

T, CT: the list tile and the group size of col_fold_kernel (kColTile, kColCT in dlp_addcols.hip;
tests/test_session_add_cols_isa.py reads them from the source).

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import numpy as np

import add_rows_lp as AL
import cols_ref as CR
import dual_lp as D

T, CT = 64, 4
BIG = D.BIG

# (m, n, k).  5 x 7: k = 4 takes N + 1 from 13 to 17, a new full stride; 37 x 58: k = 1 makes
# N + 1 = 96 -> 97 (the full stride changes), k = 5 n + k + 1 = 64 (the condensed stride stays),
# k = 6 65 (it changes); m = 63, 64, 65: the row-band and list-tile edges, k around CT (odd k: the
# misaligned shifted copy); 300 x 740: several bands and tiles
CASES = [(5, 7, 1), (5, 7, 2), (5, 7, 4), (37, 58, 1), (37, 58, 5), (37, 58, 6)] + \
        [(m, n, k) for (m, n) in ((63, 70), (64, 66), (65, 449)) for k in (CT - 1, CT, CT + 1)] + \
        [(300, 740, 3)]
SHAPES = sorted({(m, n) for m, n, _ in CASES})
COUNT_SHAPE = (300, 740)
COUNTS = [0, 1, T - 1, T, T + 1, 2 * T + 1]
DEGENERATE = AL.DEGENERATE

lp, cold = AL.lp, AL.cold


def duals(T0, basis0, n):
    return CR.duals(T0, basis0, n)


def new_cols(y, k, depth=0.1):
    return CR.columns(np.asarray(y), k, 7701 + k, depth=depth)


def dull_cols(y, k):
    return new_cols(y, k, depth=-0.1)


def ray(m):
    return np.zeros((m, 1)), np.array([1.0])


def _priced(y, p, depth=0.02):
    """d that makes p attractive at y by `depth` (a column with y . p = 0 gets a negative cost:
    its reduced cost is positive and it does not enter)."""
    yp = float(np.asarray(y) @ p)
    return yp * (1.0 + depth) if yp > 0.0 else -1.0


def counted(y, count, seed=7600):
    """One column (P (m, 1), d) with exactly `count` nonzeros, spread over the rows, every third
    of them negative."""
    m = len(y)
    rng = np.random.default_rng(seed + count)
    p = np.zeros(m)
    rows = np.sort(rng.choice(m, size=count, replace=False))
    p[rows] = rng.uniform(0.1, 1.0, count)
    p[rows[::3]] *= -1.0
    return p.reshape(m, 1), np.array([_priced(y, p)])


def slack_rows(basis, n, m):
    """(rows whose slack is basic, rows whose slack is nonbasic)."""
    basis = np.asarray(basis)
    isb = np.zeros(m, bool)
    isb[basis[basis >= n] - n] = True
    return np.nonzero(isb)[0], np.nonzero(~isb)[0]


def on_rows(y, rows, seed=7650):
    """One column with nonzeros on exactly `rows`."""
    m = len(y)
    rng = np.random.default_rng(seed + len(rows))
    p = np.zeros(m)
    p[rows] = rng.uniform(0.1, 1.0, len(rows))
    return p.reshape(m, 1), np.array([_priced(y, p)])


def basic_only(y, basis, n):
    return on_rows(y, slack_rows(basis, n, len(y))[0])


def nonbasic_only(y, basis, n):
    return on_rows(y, slack_rows(basis, n, len(y))[1], seed=7660)


def grouped(y, seed=7680):
    """CT columns of one group: column 0 has its nonzeros on the even rows only, column 1 on the
    odd rows only, column 2 is column 0 with -0.0 on the odd rows, column 3 has negative entries and
    a negative cost; any further ones are dense."""
    m = len(y)
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.1, 1.0, (m, CT))
    P[1::2, 0] = 0.0
    P[0::2, 1] = 0.0
    P[:, 2] = P[:, 0]
    P[1::2, 2] = -0.0
    P[::3, 3] *= -1.0
    d = np.array([_priced(y, P[:, t]) for t in range(CT)])
    d[3] = -abs(d[3])
    return P, d


def reference(T0, basis0, n, P, d, pricing=0, max_pivots=10 ** 6):
    """The reference of a whole call on a read-out: the rule, then the primal phase (both
    tests/cols_ref.py) with the Bland state reset.  Returns (T2, basis2, ref)."""
    T2, basis2 = CR.add_cols(T0, basis0, n, P, d)
    ref = CR.primal_phase(T2, basis2, n + np.asarray(d).size, pricing=pricing, max_pivots=max_pivots)
    return T2, basis2, ref
