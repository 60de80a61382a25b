"""CPU: the C++ dual oracle (oracle/oracle_dual.inc through oracle_py.resolve_rhs) against the
numpy reference of the rule (tests/rhs_ref.py), bit for bit in status, pivot count, basis, every
log field, the tableau, x, y and the Bland state, on every input the dual tests already build
(tests/test_batch_rhs_api.py, tests/test_session_rhs_api.py: dense shapes after a cold solve,
cone LPs from the slack basis) in both pricing modes, with budgets 0, 1, 5 and unlimited, the
continuation of a pending phase, the infeasible input and both refusals, and on the small tied LPs
of tests/dual_lp.py.  rhs_ref.py stays the yardstick of the existing tests; this file is what
lets tests/test_gpu_session_rhs_wide.py use the oracle where rhs_ref.py is too slow.

Time on the largest shape the two share (96 x 160 after its cold solve, 80 dual pivots, one CPU
core): rhs_ref.py 625 ms, the oracle 1.7 ms.  On the widest shape of tests/dual_lp.py, which only
the oracle runs: 300 x 740 dense, 853 dual pivots, 0.28 s (0.33 ms per pivot); rhs_ref.py, at
7.8 ms per pivot on a tableau a tenth of that size, was not waited for there."""
import functools
import time

import numpy as np
import pytest

import dual_lp as D
import oracle_py as O
import reopt_ref as R
import rhs_ref as RR

import test_gpu_session_rhs as G

BIG = 10 ** 6
BUDGETS = [0, 1, 5, BIG]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def _same(got, ref, tag):
    """Every key of rhs_ref.resolve_rhs's dict, bit for bit (a NaN equals itself)."""
    assert set(got) == set(ref), tag
    assert got["status"] == ref["status"], (tag, got["status"], ref["status"])
    assert got["done"] == ref["done"], (tag, got["done"], ref["done"])
    assert got["basis"].dtype == ref["basis"].dtype and got["basis"].tobytes() == ref["basis"].tobytes(), tag
    assert got["log"].dtype == ref["log"].dtype == RR.PIVOT_DTYPE and len(got["log"]) == len(ref["log"]), tag
    for f in ("q", "p", "leaving", "pad", "ratio", "objective"):
        bad = np.nonzero(_bits(got["log"][f]) != _bits(ref["log"][f]))[0]
        assert len(bad) == 0, f"{tag}: log field {f} differs at pivots {bad[:8]}"
    assert got["T"].shape == ref["T"].shape, tag
    bad = np.argwhere(_bits(got["T"]) != _bits(ref["T"]))
    assert len(bad) == 0, f"{tag}: tableau differs at {bad[:8].tolist()}"
    for f in ("x", "y"):
        assert _bits(got[f]).tobytes() == _bits(ref[f]).tobytes(), (tag, f)
    assert _bits(np.float64(got["objective"])) == _bits(np.float64(ref["objective"])), tag
    if "bland" in ref:
        assert bool(got["bland"]) == bool(ref["bland"]), tag


def _both(T, basis, n, b, tag, **kw):
    got, ref = O.resolve_rhs(T, basis, n, b, **kw), RR.resolve_rhs(T, basis, n, b, **kw)
    _same(got, ref, f"{tag} {kw}")
    return ref


def _all_budgets(T, basis, n, b, tag, pricing):
    """Budgets 0, 1, 5 and unlimited; then the continuation of the phase the budget of 5 left
    pending, to the end.  Returns the unlimited run."""
    T0, basis0 = T.copy(), np.array(basis)
    for budget in BUDGETS:
        ref = _both(T, basis, n, b, tag, max_pivots=budget, pricing=pricing)
        if budget == 5 and ref["status"] == RR.PIVOT_LIMIT:
            _both(ref["T"], ref["basis"], n, b, tag + " continued", pricing=pricing, continued=ref["bland"])
    assert T.tobytes() == T0.tobytes() and np.array_equal(basis, basis0), "the inputs were modified"
    return ref


@functools.lru_cache(maxsize=None)
def _cold(m, n, seed):
    A, b, c = O.gen_dense(m, n, seed)
    return R.oracle_tableau(A, b, c, BIG)


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("m,n,seed", G.SHAPES)
def test_session_dense_inputs(m, n, seed, pricing):
    A, b, c, b2 = G.dense_lp(m, n, seed)
    T, basis = R.oracle_tableau(A, b, c, BIG)
    ref = _all_budgets(T, basis, n, b2, f"{m}x{n}", pricing)
    assert ref["status"] == RR.OK and ref["done"] >= 1
    same = _both(T, basis, n, b, f"{m}x{n} the b of creation", pricing=pricing)
    assert same["done"] == 0 and same["status"] == RR.OK


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("scale", [0.02, 0.3])
@pytest.mark.parametrize("m,n", [(5, 7), (37, 53)])
def test_batch_dense_inputs(m, n, scale, pricing):
    for seed in range(3):
        T, basis = _cold(m, n, 6100 + seed)
        _, b, _ = O.gen_dense(m, n, 6100 + seed)
        b2 = b * (1.0 + scale * np.random.default_rng(seed).uniform(-1.0, 1.0, m))
        _all_budgets(T, basis, n, b2, f"{m}x{n} seed {seed} scale {scale}", pricing)


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
def test_cone_inputs_from_the_slack_basis(pricing):
    statuses = set()
    for m, n, seed, variant in G.CONES:
        A, b, c = G.cone_lp(m, n, seed, variant)
        for start in (b, np.abs(b)):      # the batch tests fold b into b's own tableau, the session |b|'s
            T, basis = RR.from_dense(A, start, c)
            ref = _all_budgets(T, basis, n, b, f"cone {m}x{n} seed {seed} variant {variant}", pricing)
            assert ref["done"] > 0
            statuses.add(ref["status"])
    assert statuses == {RR.OK, RR.INFEASIBLE}


def test_infeasible_input():
    A, b, c = O.gen_dense(37, 53, 6500)
    T, basis = _cold(37, 53, 6500)
    b2 = b.copy()
    b2[3] = -1.0
    for pricing in (0, 1):
        assert _all_budgets(T, basis, 53, b2, "infeasible", pricing)["status"] == RR.INFEASIBLE


def test_refusals_leave_the_inputs_untouched():
    A, b, c = O.gen_dense(5, 7, 6600)
    T, basis = R.oracle_tableau(A, b, c, 1)     # stopped inside the primal solve: not dual feasible
    got = O.resolve_rhs(T, basis, 7, b)
    _same(got, RR.resolve_rhs(T, basis, 7, b), "not dual feasible")
    assert got["status"] == RR.ERR_STATE and got["T"].tobytes() == T.tobytes() and np.isnan(got["objective"])
    T, basis = _cold(5, 7, 6600)
    for bad in (np.nan, np.inf, -np.inf):
        b2 = b.copy()
        b2[2] = bad
        got = O.resolve_rhs(T, basis, 7, b2)
        _same(got, RR.resolve_rhs(T, basis, 7, b2), f"b with {bad}")
        assert got["status"] == RR.ERR_ARG and got["T"].tobytes() == T.tobytes()
    # a b that is not finite is refused before a tableau that is not dual feasible (dlp.h's order)
    T, basis = R.oracle_tableau(A, b, c, 1)
    assert O.resolve_rhs(T, basis, 7, b2)["status"] == RR.resolve_rhs(T, basis, 7, b2)["status"] == RR.ERR_ARG
    # the C entry point itself: T and basis untouched, the code returned and in *status
    import ctypes as C
    Tc, bc = T.copy(), basis.copy()
    o = O.Opts(0, 1e-9, 1e-9, BIG, 1)
    st, npiv, bland = C.c_int(7), C.c_int64(7), C.c_int(1)
    rc = O.lib().oracle_resolve_rhs(5, 7, T.shape[1], O._d(Tc), bc.ctypes.data_as(O._I32), O._d(b), C.byref(o),
                                    1e-9, 1, C.byref(bland), None, 0, C.byref(npiv), C.byref(st))
    assert (rc, st.value, npiv.value, bland.value) == (RR.ERR_STATE, RR.ERR_STATE, 0, 1)
    assert Tc.tobytes() == T.tobytes() and bc.tobytes() == basis.tobytes()


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("name", ["dup_rows_small", "dup_cols_small"])
def test_small_tied_lps(name, pricing):
    """tests/dual_lp.py's constructions at 40 x 40 and 30 x 40: exact ties in the leaving row and
    in the entering ratio (tests/test_dual_inputs.py counts them), zero ratios, Bland choices."""
    A, b, c = D.tied_lp(name)
    T, basis, _ = D.cold_start(A, b, c)
    ref = _all_budgets(T, basis, A.shape[1], b, name, pricing)
    assert ref["status"] == RR.OK and ref["done"] >= 10


def test_time_on_the_largest_shared_shape():
    """Prints the two times of the module docstring (not asserted: a measurement)."""
    m, n, seed = G.SHAPES[-1]
    A, b, c, b2 = G.dense_lp(m, n, seed)
    T, basis = R.oracle_tableau(A, b, c, BIG)
    t0 = time.perf_counter()
    ref = RR.resolve_rhs(T, basis, n, b2)
    t1 = time.perf_counter()
    got = O.resolve_rhs(T, basis, n, b2)
    t2 = time.perf_counter()
    _same(got, ref, "timed")
    print(f"{m}x{n}, {ref['done']} dual pivots: rhs_ref.py {1e3 * (t1 - t0):.1f} ms, oracle {1e3 * (t2 - t1):.2f} ms")
