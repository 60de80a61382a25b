"""CPU: dlp_session_set_rhs's surface (export, argument checks, the Python wrapper) and the inputs
of tests/test_gpu_session_rhs.py held against the numpy reference of the rule (tests/rhs_ref.py)
before any GPU is involved: the dense LPs pivot and end optimal, the cone LPs contain a zero-ratio
pivot followed by a Bland-mode choice, the infeasible LP is infeasible."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import reopt_ref as R
import rhs_ref as RR

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

import test_gpu_session_rhs as G


def test_library_exports_set_rhs():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "dlp_session_set_rhs")
    assert "dlp_session_set_rhs" in {s[0] for s in L.SIGNATURES}


def test_null_session_or_b_is_an_argument_error():
    b = np.zeros(3)
    ms = C.c_double()
    assert L.lib().dlp_session_set_rhs(None, b.ctypes.data_as(C.POINTER(C.c_double)), 3,
                                       C.byref(ms)) == L.ERR_ARG
    assert L.lib().dlp_session_set_rhs(None, None, 0, None) == L.ERR_ARG


class _Dims:
    m = 5


def test_wrapper_rejects_bad_shapes_before_the_call():
    assert callable(dlp.Session.set_rhs)
    s = object.__new__(dlp.Session)   # no device: the checks run before the handle is touched
    s.problem, s._h = _Dims(), None
    for bad in (np.zeros(4), np.zeros(6), np.zeros((5, 1)), np.zeros(5, dtype=complex),
                np.array(["a"] * 5)):
        with pytest.raises(ValueError):
            s.set_rhs(bad)


def test_gpu_tests_use_the_same_reference():
    assert G.RR.resolve_rhs is RR.resolve_rhs and G.RR.fold_rhs is RR.fold_rhs


@pytest.mark.parametrize("m,n,seed", G.SHAPES)
def test_dense_inputs_pivot_and_end_optimal(m, n, seed):
    A, b, c, b2 = G.dense_lp(m, n, seed)
    T, basis = R.oracle_tableau(A, b, c, 10 ** 6)
    res = RR.resolve_rhs(T, basis, n, b2)
    assert res["status"] == RR.OK
    assert res["done"] >= 1
    ref = O.solve_dense(A, b2, c)
    assert abs(res["objective"] - ref.objective) <= 1e-9 * (1.0 + abs(ref.objective))


def test_cone_inputs_hold_a_zero_ratio_pivot_followed_by_a_bland_choice():
    seen_ok = seen_zero = False
    for m, n, seed, variant in G.CONES:
        A, b, c = G.cone_lp(m, n, seed, variant)
        assert (b < 0.0).any() and (c <= 0.0).all()
        T, basis = RR.from_dense(A, np.abs(b), c)
        for pricing in (0, 1):
            res = RR.resolve_rhs(T, basis, n, b, pricing=pricing)
            assert res["status"] in (RR.OK, RR.INFEASIBLE) and res["done"] > 0
            seen_ok |= res["status"] == RR.OK
            r = res["log"]["ratio"]
            # a pivot after a zero-ratio one was chosen in Bland mode (pricing 0 enters it there)
            seen_zero |= pricing == 0 and bool((r[:-1] == 0.0).any())
    assert seen_ok and seen_zero


def test_infeasible_input_is_infeasible():
    A, b, c = O.gen_dense(37, 53, 6500)
    assert (A >= 0.0).all()
    T, basis = R.oracle_tableau(A, b, c, 10 ** 6)
    b2 = b.copy()
    b2[3] = -1.0
    assert RR.resolve_rhs(T, basis, 53, b2)["status"] == RR.INFEASIBLE
