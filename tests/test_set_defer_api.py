"""CPU: dlp_session_set_defer's surface (export, argument checks without a device, the Python
wrapper's checks) and the inputs of tests/test_gpu_set_defer.py held against the CPU oracle before
any GPU is involved: every stop lies inside the cold solve of its shape, and every shape's b2
makes the dual phase of the round trip pivot."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

import dual_lp as D
import test_dual_inputs as TD
import test_gpu_set_defer as G


def test_library_exports_set_defer():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "dlp_session_set_defer")
    assert "dlp_session_set_defer" in {s[0] for s in L.SIGNATURES}


def test_null_session_is_an_argument_error_without_a_device():
    ms = C.c_double(-1.0)
    f = L.lib().dlp_session_set_defer
    assert f(None, 1, 0, -1, C.byref(ms)) == L.ERR_ARG
    assert f(None, 0, 0, 0, None) == L.ERR_ARG
    for bad in ((65, 0, -1), (-1, 0, -1), (16, 2, -1), (16, -2, -1), (16, 1, 2), (16, 1, -2)):
        assert f(None, *bad, None) == L.ERR_ARG, bad


def test_wrapper_checks_its_arguments_before_the_call():
    assert callable(dlp.Session.set_defer) and callable(dlp.Session.storage)
    s = object.__new__(dlp.Session)   # no device: the checks run before the handle is touched
    s._h = None
    for bad in (dict(defer=65), dict(defer=-1), dict(defer=1.5), dict(defer="16"), dict(defer=True),
                dict(defer=16, condensed=2), dict(defer=16, condensed=-2), dict(defer=16, condensed=0.0),
                dict(defer=16, lookahead=2), dict(defer=16, lookahead=-2), dict(defer=16, lookahead=None)):
        with pytest.raises(ValueError):
            s.set_defer(**bad)


def test_paths_are_the_issue_set():
    assert G.P == {"eager": dict(defer=1),
                   "k4c": dict(defer=4, condensed=1),
                   "k16f": dict(defer=16, condensed=-1),
                   "k16c_la": dict(defer=16, condensed=1, lookahead=1),
                   "k64c": dict(defer=64, condensed=1)}
    assert G.STOPS == {(63, 70): (7, 29), (65, 449): (7, 37, 100), (257, 260): (7, 37, 100),
                       (300, 740): (7, 37, 100)}
    assert set(G.STOPS) <= set(D.SHAPES)


@pytest.mark.parametrize("m,n", sorted(G.STOPS))
def test_every_stop_lies_inside_the_cold_solve(m, n):
    A, b, c, b2 = D.dense_lp(m, n)
    cold = O.solve_dense(A, b, c)
    print(f"dense {m}x{n}: {cold.num_pivots} cold pivots, stops {G.STOPS[(m, n)]}")
    assert cold.status == L.OK and cold.num_pivots > max(G.STOPS[(m, n)])
    assert cold.num_pivots > G.CHAIN_STOP * (len(G.P) + 1) or (m, n) != G.CHAIN_SHAPE


@pytest.mark.parametrize("m,n", sorted(G.STOPS))
def test_the_dual_phase_of_b2_pivots(m, n):
    T, basis, res = TD._dense_run(m, n)   # (tests/test_dual_inputs.py guarantees it; restated)
    assert res["status"] == L.OK and res["done"] >= 10
