"""CPU: the host side of dlp_batch_add_rows / Batch.add_rows (the symbol, its declaration and
binding, argument validation before any device call, the wrapper's checks of G and h) and the
numpy statement of the row rule, tests/rows_ref.py, against HiGHS on the stacked LP: the GPU
tests compare the kernel with that reference bit for bit, so it has to be right on its own."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.optimize import linprog

import oracle_py as O
import reopt_ref as R
import rhs_ref as RR
import rows_ref as AR
from conftest import ROOT

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

NAME = "dlp_batch_add_rows"


def test_symbol_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dlp.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(L.lib(), NAME)
    assert re.search(r"\b%s\s*\(" % NAME, header)
    sig = {s[0]: s for s in L.SIGNATURES}
    assert NAME in sig and sig[NAME][1] is C.c_int and len(sig[NAME][2]) == 9
    assert callable(dlp.Batch.add_rows)
    for m, n in ((5, 7), (37, 53), (64, 100), (65, 100)):
        assert AR.tableau_ld(m, n) == dlp.tableau_ld(m, n)


def _call(batch, r, G, sG, h, sh, dev, budget, out):
    return L.lib().dlp_batch_add_rows(batch, r, G, sG, h, sh, dev, budget, out)


def test_null_batch_is_an_argument_error():
    lib = L.lib()
    G, h = np.ones((2, 5)), np.ones(2)
    out = L.BatchOut()
    lib.dlp_batch_resolve(None, None, 0, 0, 10, None)   # (another function's name in dlp_last_error)
    assert NAME.encode() not in lib.dlp_last_error()
    assert _call(None, 2, G.ctypes.data, 0, h.ctypes.data, 0, 0, 10, C.byref(out)) == L.ERR_ARG
    assert NAME.encode() in lib.dlp_last_error()
    lib.dlp_batch_resolve(None, None, 0, 0, 10, None)
    assert _call(None, 0, None, 0, None, 0, 0, 10, None) == L.ERR_ARG
    assert NAME.encode() in lib.dlp_last_error()


@pytest.mark.parametrize("what,args", [
    ("r < 0", dict(r=-1)),
    ("NULL G", dict(G=None)),
    ("NULL h", dict(h=None)),
    ("short strideh", dict(sh=1)),
    ("negative strideG", dict(sG=-8)),
    ("flag 2", dict(dev=2)),
    ("flag -1", dict(dev=-1)),
    ("negative budget", dict(budget=-1)),
    ("negative log_cap", dict(log_cap=-1)),
])
def test_bad_scalars_are_argument_errors_before_any_device_call(what, args):
    """Every scalar check comes before the handle is used for anything but its shape: an
    all-zero block stands in for the handle (nlp = m = n = 0 and no live pointer in it: a check
    that let one of these through would find no LP to run).  A strideG below r * n needs a real
    n: tests/test_gpu_batch_add_rows.py."""
    lib = L.lib()
    fake = C.create_string_buffer(4096)
    G, h = np.ones((2, 4)), np.ones(2)
    a = dict(r=2, G=G.ctypes.data, sG=0, h=h.ctypes.data, sh=0, dev=0, budget=5, log_cap=0)
    a.update(args)
    out = L.BatchOut()
    out.log_cap = a["log_cap"]
    lib.dlp_batch_resolve(None, None, 0, 0, 10, None)
    rc = _call(C.cast(fake, C.c_void_p), a["r"], a["G"], a["sG"], a["h"], a["sh"], a["dev"], a["budget"],
               C.byref(out))
    assert rc == L.ERR_ARG, what
    assert NAME.encode() in lib.dlp_last_error()


class _Stub(dlp.Batch):
    """The wrapper's checks run before the native call: a 3 x (4 x 5) batch without a device
    behind it (the handle is a dummy that is never passed on)."""

    def __init__(self):
        self._h = C.c_void_p()
        self.nlp, self.m, self.n, self.device, self.max_pivots = 3, 4, 5, 0, 100

    def _handle(self):
        raise AssertionError("the native call was reached")


@pytest.mark.parametrize("G,h", [
    (np.ones((3, 2, 4)), np.ones((3, 2))),          # n
    (np.ones((2, 2, 5)), np.ones((2, 2))),          # nlp
    (np.ones((3, 2, 5)), np.ones((3, 3))),          # r of h
    (np.ones((3, 2, 5)), np.ones((2, 2))),          # nlp of h
    (np.ones((2, 5)), np.ones(3)),
    (np.ones((2, 5)), np.ones((2, 1))),
    (np.ones(5), np.ones(1)),                       # G needs its row dimension
    (np.ones((1, 3, 2, 5)), np.ones((3, 2))),
    (np.ones((0, 5)), np.ones(0)),                  # r = 0 is G=None, h=None
    (np.ones((2, 5)), np.float64(1.0)),
    (np.ones((2, 5), dtype=complex), np.ones(2)),
    (np.ones((2, 5)), np.array(["a", "b"])),
    (np.ones((2, 5), dtype=bool), np.ones(2)),
    (np.ones((2, 5)), None),
    (None, np.ones(2)),
], ids=lambda v: "None" if v is None else f"{v.dtype}{v.shape}")
def test_add_rows_rejects_bad_rows(G, h):
    s = _Stub()
    with pytest.raises(ValueError):
        s.add_rows(G, h)
    assert s.m == 4


def test_add_rows_rejects_a_negative_budget_and_a_closed_batch():
    with pytest.raises(ValueError):
        _Stub().add_rows(np.ones((2, 5)), np.ones(2), max_pivots=-1)
    with pytest.raises(ValueError):
        _Stub().add_rows(None, None, log_cap=-1)
    closed = dlp.Batch.__new__(dlp.Batch)
    closed._h = C.c_void_p()
    closed.nlp, closed.m, closed.n, closed.device, closed.max_pivots = 3, 4, 5, 0, 100
    for G, h in ((np.ones((2, 5)), np.ones(2)), (None, None)):
        with pytest.raises(ValueError, match="closed"):
            closed.add_rows(G, h)
    assert closed.m == 4
    closed.close()


# ---- the reference against HiGHS on the stacked LP (objective within 1e-9 * max(1, |obj|), the
# project's HiGHS bar)
def _highs(A, b, c):
    res = linprog(-c, A_ub=A, b_ub=b, bounds=(0, None), method="highs")
    return res.status, (-res.fun if res.status == 0 else None)


def _optimum(m, n, seed):
    A, b, c = O.gen_dense(m, n, seed)
    T, basis = R.oracle_tableau(A, b, c, 10 ** 6)
    x = np.zeros(n)
    for i, v in enumerate(basis):
        if v < n:
            x[v] = T[i, n + m]
    return A, b, c, T, basis, x


cuts = AR.cuts


def _check_ok(res, A2, b2, c):
    status, obj = _highs(A2, b2, c)
    assert status == 0 and res["status"] == RR.OK, (status, res["status"])
    assert abs(res["objective"] - obj) <= 1e-9 * max(1.0, abs(obj)), (res["objective"], obj)
    x = res["x"]
    assert (x >= -1e-9).all() and (A2 @ x <= b2 + 1e-7).all()
    assert abs(c @ x - obj) <= 1e-7 * max(1.0, abs(obj))


SHAPES = [(5, 7, 1), (5, 7, 3), (37, 53, 1), (37, 53, 4)]


@pytest.mark.parametrize("m,n,r", SHAPES)
def test_violated_cuts_match_highs(m, n, r):
    pivots = []
    for seed in range(3):
        A, b, c, T, basis, x = _optimum(m, n, 8100 + seed)
        G, h = cuts(x, n, r, 8150 + seed)
        assert (G @ x > h).any() and (G == 0.0).any()
        T2, basis2 = AR.add_rows(T, basis, n, G, h)
        # the layout: old rows and the objective row keep their bits, the new slacks are basic
        N, N2 = n + m, n + m + r
        assert T2[:m, :N].tobytes() == T[:m, :N].tobytes() and T2[m + r, :N].tobytes() == T[m, :N].tobytes()
        assert T2[:m, N2].tobytes() == T[:m, N].tobytes() and T2[m + r, N2] == T[m, N]
        assert not T2[:m, N:N2].any() and np.array_equal(T2[m:m + r, N:N2], np.eye(r))
        assert not T2[m:m + r][:, basis].any() and list(basis2[m:]) == list(range(N, N2))
        # a new row's RHS is its slack at x*: h - G x*
        np.testing.assert_allclose(T2[m:m + r, N2], h - G @ x, rtol=0, atol=1e-9 * max(1.0, np.abs(h).max()))
        res = AR.dual_phase(T2, basis2, n)
        _check_ok(res, np.vstack([A, G]), np.concatenate([b, h]), c)
        assert len(res["y"]) == m + r and len(res["basis"]) == m + r
        pivots.append(res["done"])
    assert min(pivots) >= 1, pivots


@pytest.mark.parametrize("m,n,r", SHAPES)
def test_a_slack_cut_needs_no_pivot(m, n, r):
    A, b, c, T, basis, x = _optimum(m, n, 8200 + m)
    G, _ = cuts(x, n, r, 8250)
    h = G @ x + 1.0
    res = AR.add_rows_and_solve(T, basis, n, G, h)
    assert res["status"] == RR.OK and res["done"] == 0
    assert list(res["basis"][:m]) == list(basis) and list(res["basis"][m:]) == list(range(n + m, n + m + r))
    _check_ok(res, np.vstack([A, G]), np.concatenate([b, h]), c)


@pytest.mark.parametrize("m,n,r", SHAPES)
def test_a_nonnegative_row_with_a_negative_h_is_infeasible(m, n, r):
    A, b, c, T, basis, x = _optimum(m, n, 8300 + m)
    G, h = cuts(x, n, r, 8350)
    h[r - 1] = -1.0
    assert (G >= 0.0).all()
    res = AR.add_rows_and_solve(T, basis, n, G, h)
    assert res["status"] == RR.INFEASIBLE
    assert _highs(np.vstack([A, G]), np.concatenate([b, h]), c)[0] == 2


@pytest.mark.parametrize("m,n,r", SHAPES)
def test_resolve_rhs_on_the_grown_tableau_matches_highs(m, n, r):
    """The grown record is a correct input to the RHS rule as it is: b2 has m + r entries."""
    A, b, c, T, basis, x = _optimum(m, n, 8400 + m)
    G, h = cuts(x, n, r, 8450)
    res = AR.add_rows_and_solve(T, basis, n, G, h)
    assert res["status"] == RR.OK
    b2 = np.concatenate([b, h]) * (1.0 + 0.05 * np.random.default_rng(8460).uniform(-1.0, 1.0, m + r))
    res2 = RR.resolve_rhs(res["T"], res["basis"], n, b2)
    _check_ok(res2, np.vstack([A, G]), b2, c)


def test_the_rule_holds_for_any_basis():
    """Stopped inside the primal solve (not dual feasible): the rows are still those of the
    stacked LP in that basis, and the dual phase is refused with the grown tableau kept."""
    m, n, r = 5, 7, 2
    A, b, c = O.gen_dense(m, n, 8500)
    T, basis = R.oracle_tableau(A, b, c, 1)
    G, _ = cuts(np.ones(n), n, r, 8550)
    h = G.sum(axis=1) + 100.0
    T2, basis2 = AR.add_rows(T, basis, n, G, h)
    res = AR.dual_phase(T2, basis2, n)
    assert res["status"] == RR.ERR_STATE and res["T"].tobytes() == T2.tobytes()
    # B^-1 [A I | b] of the stacked LP, row by row
    A2 = np.vstack([A, G])
    full = np.hstack([A2, np.eye(m + r), np.concatenate([b, h])[:, None]])
    B = full[:, basis2]
    want = np.linalg.solve(B, full)
    got = np.hstack([T2[:m + r, :n + m + r], T2[:m + r, [n + m + r]]])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))
