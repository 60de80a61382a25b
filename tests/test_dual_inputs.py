"""CPU: every property tests/dual_lp.py claims for its inputs, on the C++ dual oracle alone, before
any GPU is involved (tests/test_gpu_session_rhs_wide.py runs the same inputs bit for bit).
Conditions, not measurements: should a seed fail one, change the seed in dual_lp.py.

Measured here (printed with -s), dual pivots to the end, every run ends OK:
  shape      dense: cold + dual   cone, Dantzig -> Bland   cone, always Bland
  63 x 70    33 + 25              16                       57
  64 x 66    47 + 25              29                       36
  65 x 449   157 + 104            32                       52
  128 x 385  249 + 224            37                       169
  255 x 258  507 + 356            155                      768
  256 x 257  626 + 251            206                      597
  257 x 260  419 + 197            153                      782
  300 x 740  1,459 + 853          105                      880
  dup_rows (6 cold pivots), Dantzig pricing: 236 dual pivots, 12 leaving-row ties between the two
    row workgroups, 6 of them won by the higher one's row; always Bland: 350 pivots, 325 with
    eligible rows in both row workgroups, 118 won by the higher one's row.
  dup_cols, Dantzig -> Bland: 1,129 dual pivots (938 chosen in Bland mode), 843 entering-column
    ties between column workgroups, 228 of them over all three, 32 inside one lane's pair;
    always Bland: 747 pivots, 468 ties, 1 over three workgroups, 20 inside a lane's pair.
"""
import functools

import numpy as np
import pytest
from scipy.optimize import linprog

import dual_lp as D
import oracle_py as O
import reopt_ref as R
import rhs_ref as RR

SHAPES = list(D.SHAPES)


@functools.lru_cache(maxsize=None)
def _dense_run(m, n):
    A, b, c, b2 = D.dense_lp(m, n)
    T, basis = R.oracle_tableau(A, b, c, D.BIG)
    return T, basis, O.resolve_rhs(T, basis, n, b2)


@functools.lru_cache(maxsize=None)
def _cone_run(m, n):
    A, b, c = D.cone_lp(m, n)
    T, basis = RR.from_dense(A, np.abs(b), c)
    return T, basis, O.resolve_rhs(T, basis, n, b)


def _close(obj, ref):
    return abs(obj - ref) <= 1e-9 * max(1.0, abs(ref))


def test_shapes_cross_the_boundaries_they_name():
    """The kernels' constants (dlp_dual.hip: 64-row / 64-column fold tiles, 256 rows and 512
    columns per selection workgroup) against the shapes."""
    def counts(m, n):
        N = n + m
        return dict(fold_wg=-(-(m + 1) // 64), tiles=-(-m // 64), last_tile=m % 64 or 64,
                    row_wg=-(-m // 256), col_wg=-(-N // 512), N=N)
    c = {s: counts(*s) for s in SHAPES}
    assert c[(63, 70)]["fold_wg"] == 1 and (63 + 1) % 64 == 0
    assert c[(64, 66)]["fold_wg"] == 2 and c[(64, 66)]["tiles"] == 1 and c[(64, 66)]["last_tile"] == 64
    assert c[(65, 449)]["last_tile"] == 1 and c[(65, 449)]["N"] == 514 and c[(65, 449)]["col_wg"] == 2
    assert c[(128, 385)]["tiles"] == 2 and c[(128, 385)]["last_tile"] == 64 and c[(128, 385)]["N"] == 513
    assert c[(255, 258)]["row_wg"] == 1 and c[(255, 258)]["N"] == 513
    assert c[(256, 257)]["row_wg"] == 1 and 256 % 256 == 0 and c[(256, 257)]["N"] == 513
    assert c[(257, 260)]["row_wg"] == 2 and 257 % 256 == 1
    assert (c[(300, 740)]["row_wg"], c[(300, 740)]["col_wg"], c[(300, 740)]["tiles"]) == (2, 3, 5)
    for (m, n) in SHAPES:                      # small: the widest tableau is 2.5 MB
        assert (m + 1) * O.ld(m, n) * 8 <= 2.6e6


@pytest.mark.parametrize("m,n", SHAPES)
def test_dense_inputs(m, n):
    A, b, c, b2 = D.dense_lp(m, n)
    T, basis, res = _dense_run(m, n)
    cold = O.solve_dense(A, b, c)
    assert cold.status == RR.OK
    print(f"dense {m}x{n}: {cold.num_pivots} cold + {res['done']} dual pivots, status {res['status']}")
    assert res["status"] in (RR.OK, RR.INFEASIBLE) and res["done"] >= 10
    ref = O.solve_dense(A, b2, c)                 # the primal oracle's cold solve of the new LP
    assert res["status"] == ref.status == RR.OK and _close(res["objective"], ref.objective)
    # the fold on a tableau full of pivoted slack columns: against the exact sum in long double
    N = n + m
    exact = (T[:, n:N].astype(np.longdouble) @ b2.astype(np.longdouble)).astype(np.float64)
    rhs0 = O.resolve_rhs(T, basis, n, b2, max_pivots=0)["T"][:, N]
    scale = np.abs(T[:, n:N]) @ np.abs(b2)
    assert (np.abs(rhs0 - exact) <= m * 2.0 ** -52 * scale).all()


@pytest.mark.parametrize("m,n", SHAPES)
def test_cone_inputs(m, n):
    A, b, c = D.cone_lp(m, n)
    assert (c <= 0.0).all()
    neg = np.nonzero(b < 0.0)[0]
    if m > D.ROW_BLOCK:
        assert (neg < D.ROW_BLOCK).any() and (neg >= D.ROW_BLOCK).any()   # eligible rows in both workgroups
    T, basis, res = _cone_run(m, n)
    print(f"cone {m}x{n}: {res['done']} dual pivots, status {res['status']}")
    assert res["status"] in (RR.OK, RR.INFEASIBLE) and res["done"] >= 10
    hs = linprog(-c, A_ub=A, b_ub=b, bounds=(0, None), method="highs")
    if res["status"] == RR.OK:
        assert hs.status == 0 and _close(res["objective"], -hs.fun), (res["objective"], -hs.fun)
        assert (res["x"] >= -1e-9).all() and (A @ res["x"] <= b + 1e-7).all()
    else:
        assert hs.status == 2
    bl = O.resolve_rhs(T, basis, n, b, pricing=1)
    print(f"cone {m}x{n}, always Bland: {bl['done']} dual pivots, status {bl['status']}")
    assert bl["done"] >= 10 and bl["status"] == res["status"]
    if bl["status"] == RR.OK:
        assert _close(bl["objective"], res["objective"])


def test_one_shape_per_row_workgroup_count_ends_optimal():
    for run in (_dense_run, _cone_run):
        for wgs in (1, 2):
            ended = {run(m, n)[2]["status"] for (m, n) in SHAPES if -(-m // D.ROW_BLOCK) == wgs}
            assert RR.OK in ended, (run.__name__, wgs, ended)


@functools.lru_cache(maxsize=None)
def _trace(name, pricing):
    A, b, c = D.tied_lp(name)
    T0, basis0, np0 = D.cold_start(A, b, c)
    t = D.trace(T0, basis0, A.shape[1], b, pricing, blocks=D.tied_blocks(name))
    # one pivot per call is the pivots of one call (the continuation), the tableau bits included
    one = O.resolve_rhs(T0, basis0, A.shape[1], b, pricing=pricing)
    assert one["status"] == t.res["status"] and one["log"].tobytes() == t.res["log"].tobytes()
    assert one["T"].tobytes() == t.res["T"].tobytes() and one["basis"].tobytes() == t.res["basis"].tobytes()
    t.cold = np0
    return t


@pytest.mark.parametrize("name", ["dup_rows", "dup_rows_small"])
def test_duplicated_rows_tie_across_row_workgroups(name):
    A, b, c = D.tied_lp(name)
    kw = D.TIED[name][1]
    lo = np.arange(kw["pairs"])
    shared = np.ones(A.shape[1], bool)
    shared[A.shape[1] - kw["pairs"] + lo[::2]] = False      # the flipped rows' own columns
    assert np.array_equal(A[lo][:, shared], A[lo + kw["block"]][:, shared])
    assert np.array_equal(b[lo], b[lo + kw["block"]]) and b[lo].max() < np.delete(b, np.r_[lo, lo + kw["block"]]).min()
    t = _trace(name, 0)
    assert t.cold == len(lo[::2])               # the cold solve enters the flipped rows' own columns only
    ties = (t.row_tied > 0) & ~t.bland
    higher = t.row_higher & ~t.bland
    print(f"{name}: {t.res['done']} dual pivots, status {t.res['status']}, {int(ties.sum())} leaving-row ties "
          f"across row workgroups, {int(higher.sum())} won by the higher one")
    assert t.res["status"] == RR.OK and t.res["done"] >= 10
    assert ties.sum() >= (5 if name == "dup_rows" else 2)
    assert higher.sum() >= 1 and (ties & ~t.row_higher).sum() >= 1     # both orders
    bl = _trace(name, 1)
    print(f"{name}, always Bland: {bl.res['done']} pivots, status {bl.res['status']}, "
          f"{int(bl.both_blocks.sum())} with eligible rows in both row workgroups, "
          f"{int(bl.row_higher.sum())} won by the higher one")
    assert bl.bland.all() and bl.both_blocks.any() and bl.row_higher.any() and (bl.row_tied > 0).sum() >= 5


@pytest.mark.parametrize("name", ["dup_cols", "dup_cols_small"])
def test_duplicated_columns_tie_across_column_workgroups(name):
    A, b, c = D.tied_lp(name)
    kw = D.TIED[name][1]
    j = np.arange(kw["dups"])
    assert np.array_equal(A[:, j], A[:, j + kw["block"]]) and np.array_equal(c[j], c[j + kw["block"]])
    assert np.array_equal(A[:, kw["lane"]], A[:, kw["lane"] + 1])
    for pricing in (0, 1):
        t = _trace(name, pricing)
        ties = t.col_tied > 0
        print(f"{name}, pricing {pricing}: {t.res['done']} dual pivots, status {t.res['status']}, "
              f"{int(ties.sum())} entering-column ties across column workgroups, "
              f"{int((t.col_blocks >= 3).sum())} over three, {int(t.lane_pair.sum())} inside a lane's pair, "
              f"{int(t.bland.sum())} decisions in Bland mode")
        assert t.cold == 0 and t.res["done"] >= 10
        assert ties.sum() >= (5 if name == "dup_cols" else 2) and t.lane_pair.sum() >= 1
        if pricing == 0:
            assert t.res["status"] == RR.OK
            assert t.bland.any() and not t.bland.all()      # zero ratios: Dantzig and Bland choices
            if name == "dup_cols":
                assert (t.col_blocks >= 3).sum() >= 1       # a slack column in the third workgroup ties
        elif name == "dup_cols":
            assert t.both_blocks.any()                      # eligible rows in both row workgroups
