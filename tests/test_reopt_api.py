"""CPU: dlp_session_set_objective's surface (export, argument checks, the Python wrapper) and
the numpy reference of its objective-row rule (tests/reopt_ref.py) against the oracle: on the
initial tableau it reproduces the cold objective row bit for bit, and after k pivots it yields
a tableau from which a plain simplex reaches the cold optimum of the new objective."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import reopt_ref as R

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L


def test_library_exports_set_objective():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "dlp_session_set_objective")
    assert "dlp_session_set_objective" in {s[0] for s in L.SIGNATURES}


def test_null_session_is_an_argument_error():
    c = np.zeros(3)
    ms = C.c_double()
    assert L.lib().dlp_session_set_objective(None, c.ctypes.data_as(C.POINTER(C.c_double)), 3,
                                             C.byref(ms)) == L.ERR_ARG
    assert L.lib().dlp_session_set_objective(None, None, 0, None) == L.ERR_ARG


class _Dims:
    n = 7


def test_wrapper_rejects_bad_shapes_before_the_call():
    assert callable(dlp.Session.set_objective)
    s = object.__new__(dlp.Session)   # no device: the checks run before the handle is touched
    s.problem, s._h = _Dims(), None
    for bad in (np.zeros(6), np.zeros(8), np.zeros((7, 1)), np.zeros(7, dtype=complex),
                np.array(["a"] * 7)):
        with pytest.raises(ValueError):
            s.set_objective(bad)


def test_gpu_tests_use_the_same_reference():
    import test_gpu_reopt
    assert test_gpu_reopt.R.objective_row is R.objective_row


@pytest.mark.parametrize("m,n,seed", [(5, 7, 1), (40, 50, 2), (300, 520, 5)])
def test_reference_on_the_initial_tableau_is_the_cold_row(m, n, seed):
    A, b, c = O.gen_dense(m, n, seed)
    c2 = R.make_c2(c, seed)
    assert (c2 == 0.0).any() and (n < 12 or (c2 < 0.0).any())
    T0, basis0 = R.oracle_tableau(A, b, c, 0)
    Tc, _ = R.oracle_tableau(A, b, c2, 0)
    z = R.objective_row(T0[:m], basis0, c2)
    assert z.view(np.int64).tolist() == Tc[m].view(np.int64).tolist()
    zero = np.nonzero(c2 == 0.0)[0]
    # -c_j = -0.0 where c2_j = +0.0 (and +0.0 where both holes meet: c2_j = -0.0)
    assert (np.signbit(z[zero]) != np.signbit(c2[zero])).all()
    assert not np.signbit(z[n:]).any()        # slacks, RHS, padding: +0.0


def test_reference_after_pivots_continues_to_the_cold_optimum():
    m, n, seed, k = 40, 50, 2, 20
    A, b, c = O.gen_dense(m, n, seed)
    c2 = R.make_c2(c, seed)
    T, basis = R.oracle_tableau(A, b, c, k)
    assert (basis < n).sum() > 0
    T[m] = R.objective_row(T[:m], basis, c2)
    assert not np.signbit(T[m, basis]).any() and (T[m, basis] == 0.0).all()
    status, _ = R.simplex_continue(T, basis, n)
    assert status == 0
    ref = O.solve_dense(A, b, c2)
    assert ref.status == 0
    assert abs(T[m, n + m] - ref.objective) <= 1e-9 * (1.0 + abs(ref.objective))
