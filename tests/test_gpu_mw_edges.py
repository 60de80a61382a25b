"""MW path at the envelope, search and report size boundaries, on the GPU: the HIP path against
the fp64 spec (oracle/oracle_mw.cpp), bit for bit, at the shapes of tests/mw_shapes.py (each
listed there with the kernel or branch of csrc/dlp_mw.hip it reaches; tests/test_mw_edges.py pins
on the CPU that it does).

  * every accepted shape in sort and in binary mode: full 16- and 32-point segments, both sides of
    the two envelope dispatch edges, bitonic sorts of 64 .. 1024 points with n == np2 and n < np2,
    the <32> kernel with an empty impression and an odd I, the search at I = 255 .. 16385, the
    report in one and two blocks, and a run whose region count crosses the LDS cache limit;
  * the options the other MW tests never vary: epsilon, tolerance above 1e-12, scaling, 2 and 8
    ratios per level, an explicit transition scale;
  * x_current, and the three ways to call dlp_mw_solution;
  * a binary-mode run in pieces."""
import ctypes as C

import numpy as np
import pytest

import mw_shapes as S

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("binary", [False, True], ids=["sort", "binary"])


@MODES
@pytest.mark.parametrize("s", S.ACCEPTED, ids=S.shape_id)
def test_mw_gpu_bit_identical_to_spec_at_the_edges(s, binary, monkeypatch):
    monkeypatch.delenv("DLP_MW_NO_LDS_CACHE", raising=False)
    log, x, w, r = S.assert_gpu_equals_spec(s.A, s.I, s.sparsity, s.T, binary)
    assert np.isfinite(log["dual_value"]).all() and (w > 0).all()
    if s is S.CACHE and binary:     # both sides of the region cache in one run, without the knob
        assert r["regions"][0] <= S.CACHE_REGIONS < r["regions"][-1]


# (name, binary, options, iterations, the spec output that the option changes against the defaults)
OPTIONS = [
    ("epsilon0.05", False, dict(epsilon=0.05), 12, "dual"),
    ("epsilon0.05", True, dict(epsilon=0.05), 12, "dual"),
    ("tolerance1e-6", False, dict(tolerance=1e-6), S.TOLERANCE_T, "dual"),
    ("tolerance1e-6", True, dict(tolerance=1e-6), S.TOLERANCE_T, "dual"),
    ("scaling0.5", False, dict(scaling=0.5), 12, "dual"),
    ("scaling0.5", True, dict(scaling=0.5), 12, "dual"),
    ("scaling1.0", False, dict(scaling=1.0), 12, "dual"),
    ("scaling1.0", True, dict(scaling=1.0), 12, "dual"),
    ("intervals2", True, dict(intervals=2), 12, "levels"),
    ("intervals8", True, dict(intervals=S.MAX_RATIOS), 12, "levels"),
    ("scale", True, dict(scale=1 - 1e-3), 12, "levels"),
]


@pytest.mark.parametrize("name,binary,opts,T,changes", OPTIONS,
                         ids=[f"{o[0]}-{'binary' if o[1] else 'sort'}" for o in OPTIONS])
@pytest.mark.parametrize("A,I,sp", [(63, 63, 0.1), (180, 180, 0.1)], ids=["63x63", "180x180"])
def test_mw_gpu_options_bit_identical_to_spec(A, I, sp, name, binary, opts, T, changes):
    _, _, _, r = S.assert_gpu_equals_spec(A, I, sp, T, binary, **opts)
    # the option is not a no-op: the spec's run differs from the one under the defaults (but for
    # the tolerance at 63x63, which changes nothing there: tests/test_mw_edges.py)
    if not (name == "tolerance1e-6" and A == 63):
        assert (r[changes] != S.spec(A, I, sp, T, binary)[changes]).any()


@MODES
@pytest.mark.parametrize("A,I,sp", [(63, 63, 0.1), (180, 180, 0.1)], ids=["63x63", "180x180"])
def test_mw_gpu_x_current(A, I, sp, binary):
    """x_current is the last iteration's primal: after one iteration the average is x_current;
    after t - 1 iterations and one more, x_avg = fa * x_avg_prev + fb * x_current with fa =
    (t-1)/t, fb = 1/t, two products and one add (average_kernel, R/instance.cpp:143-152)."""
    p = dlp.Problem.adalloc(A, I, 1, sp, 0.25)
    mw = dlp.MW(p, binary=binary)
    mw.run(1)
    xa, w, xc = mw.solution(current=True)
    assert xc.tobytes() == xa.tobytes()
    if not binary:                  # binary mode's iteration 1 allocates nothing (dual value 0)
        assert (xc > 0).any()
    t = 7
    mw.run(t - 2)
    xa_prev, _ = mw.solution()
    log, _ = mw.run(1)
    xa, w, xc = mw.solution(current=True)
    fa, fb = (t - 1) / t, 1.0 / t
    S.same_bits("x_avg", xa, fa * xa_prev + fb * xc)
    assert (xc > 0).any() and (xc >= 0).all() and (xc != xa).any()
    # the run as a whole is the spec's, and the three ways to ask for the solution agree
    r = S.spec(A, I, sp, t, binary)
    S.same_bits("x_avg", xa[S.impression_major(p)], r["x_avg"])
    S.same_bits("weights", w, r["weights"])
    assert log["dual_value"][0] == r["dual"][t - 1]
    xa2, w2 = mw.solution()
    assert xa2.tobytes() == xa.tobytes() and w2.tobytes() == w.tobytes()
    w3 = np.full(A, np.nan)
    L.check(L.lib().dlp_mw_solution(mw._h, None, None, w3.ctypes.data_as(C.POINTER(C.c_double))),
            "dlp_mw_solution")
    assert w3.tobytes() == w.tobytes()
    xc3 = np.full(p.n, np.nan)
    L.check(L.lib().dlp_mw_solution(mw._h, None, xc3.ctypes.data_as(C.POINTER(C.c_double)), None),
            "dlp_mw_solution")
    assert xc3.tobytes() == xc.tobytes()
    mw.close()


@pytest.mark.parametrize("A,I,sp", [(63, 63, 0.1), (175, 175, 0.1), (396, 396, 0.1)],
                         ids=["seg16-63x63", "seg32-175x175", "wave-396x396"])
def test_mw_gpu_binary_run_in_pieces_equals_one_run(A, I, sp):
    p = dlp.Problem.adalloc(A, I, 1, sp, 0.25)
    a = dlp.MW(p, binary=True)
    la, _ = a.run(12)
    b = dlp.MW(p, binary=True)
    lb = np.concatenate([b.run(5)[0], b.run(7)[0]])
    assert la.tobytes() == lb.tobytes()
    for u, v in zip(a.solution(current=True), b.solution(current=True)):
        assert u.tobytes() == v.tobytes()
    S.assert_log_equals_spec(la, S.spec(A, I, sp, 12, True), True)
    a.close()
    b.close()
