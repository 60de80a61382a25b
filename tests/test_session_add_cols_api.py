"""CPU: the host side of dlp_session_add_cols / Session.add_cols (the symbol, its declaration and
binding, the NULL-session refusal without a device, the wrapper's shape and dtype checks: these
fail without the feature) and the properties of the inputs tests/test_gpu_session_add_cols.py uses
(tests/add_cols_lp.py), on the C++ oracle and numpy alone: change the seed, not the condition.

Warm primal pivots of cols_ref.primal_phase after add_cols(new_cols(y*, k)) on the oracle's cold
tableau, Dantzig pricing ((m, n, k): pivots):
(5, 7, 1): 1, (5, 7, 2): 1, (5, 7, 4): 3, (37, 58, 1): 2, (37, 58, 5): 2, (37, 58, 6): 5,
(63, 70, 3): 8, (63, 70, 4): 5, (63, 70, 5): 12, (64, 66, 3): 10, (64, 66, 4): 10, (64, 66, 5): 10,
(65, 449, 3): 14, (65, 449, 4): 9, (65, 449, 5): 19, (300, 740, 3): 31
(Bland pricing: 65 x 449, k = 5: 41; 300 x 740, k = 3: 99.)  The degenerate family, k = 3, Dantzig /
Bland: 65 x 449: 20 / 76; 37 x 58: 11 / 26.  At 300 x 740: the counted columns 0, 0, 4, 1, 1, 2;
the column on the nonbasic slacks' rows 19, on the basic slacks' rows 0; the grouped columns 27."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import add_cols_lp as AC
import add_rows_lp as AL
import cols_ref as CR
import oracle_py as O
from conftest import ROOT

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

NAME = "dlp_session_add_cols"
MOST = 300          # "a few hundred numpy pivots" per GPU case


def _close(obj, ref):
    return abs(obj - ref) <= 1e-9 * (1.0 + abs(ref))


def test_symbol_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dlp.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(L.lib(), NAME)
    assert re.search(r"\b%s\s*\(" % NAME, header)
    sig = {s[0]: s for s in L.SIGNATURES}
    assert NAME in sig and sig[NAME][1] is C.c_int and len(sig[NAME][2]) == 6
    assert callable(dlp.Session.add_cols)


def test_null_session_is_an_argument_error_without_a_device():
    lib = L.lib()
    P, d = np.ones((5, 2)), np.ones(2)
    lib.dlp_session_set_defer(None, 1, 0, 0, None)   # (another function's name in dlp_last_error)
    assert NAME.encode() not in lib.dlp_last_error()
    assert lib.dlp_session_add_cols(None, 2, P.ctypes.data_as(L._DP), d.ctypes.data_as(L._DP), 5, None) == L.ERR_ARG
    assert NAME.encode() in lib.dlp_last_error()
    assert lib.dlp_session_add_cols(None, 0, None, None, 5, None) == L.ERR_ARG   # before "k == 0 touches nothing"


class _Stub(dlp.Session):
    """The wrapper's checks run before the native call: a 4 x 5 session without a device behind it
    (the NULL handle would come back as ERR_ARG if a call got through)."""

    def __init__(self):
        self._h = C.c_void_p()
        self.problem = type("P", (), dict(m=4, n=5))()

    def _info(self):
        raise AssertionError("the native call was reached and accepted")


@pytest.mark.parametrize("P,d", [
    (np.ones((5, 2)), np.ones(2)),                  # m
    (np.ones(5), 1.0),
    (np.ones((4, 2)), np.ones(3)),                  # k of d
    (np.ones((4, 2)), np.ones((2, 1))),
    (np.ones((4, 2)), np.float64(1.0)),             # a scalar d is one column's
    (np.ones((1, 4, 2)), np.ones(2)),
    (np.ones((4, 2), dtype=complex), np.ones(2)),
    (np.ones((4, 2)), np.array(["a", "b"])),
    (np.ones((4, 2), dtype=bool), np.ones(2)),
    (np.ones((4, 2)), None),
    (None, np.ones(2)),
], ids=lambda v: "None" if v is None else f"{np.asarray(v).dtype}{np.asarray(v).shape}")
def test_add_cols_rejects_bad_columns_before_the_native_call(P, d):
    s = _Stub()
    with pytest.raises(ValueError):
        s.add_cols(P, d)
    assert s.n == 5


@pytest.mark.parametrize("P,d", [(np.ones((4, 2)), np.ones(2)), (np.ones(4), 1.0), (np.ones(4), np.ones(1)),
                                 (np.ones((4, 1), dtype=np.int32), [2])], ids=["4x2", "m_scalar", "m_1", "int"])
def test_add_cols_hands_good_columns_on(P, d):
    """Accepted shapes reach the native call (which refuses the stub's NULL handle)."""
    s = _Stub()
    with pytest.raises(L.DLPError) as e:
        s.add_cols(P, d)
    assert e.value.status == L.ERR_ARG and s.n == 5


def test_live_shape_is_the_wrappers_shape():
    s = _Stub()
    assert (s.m, s.n) == (4, 5)
    s._live_n = 7                                    # as _info() reports after add_cols of two columns
    assert (s.m, s.n) == (4, 7)
    with pytest.raises(ValueError):
        s.set_objective(np.ones(5))
    with pytest.raises(L.DLPError):                  # n + k costs reach the native call
        s.set_objective(np.ones(7))
    with pytest.raises(ValueError):
        s.add_rows(np.ones((1, 5)), np.ones(1))
    with pytest.raises(L.DLPError):
        s.add_rows(np.ones((1, 7)), np.ones(1))


# ---- the inputs of the GPU tests, on the oracle and numpy alone

def _pivots_in_docstring():
    return {tuple(int(v) for v in g[:3]): int(g[3])
            for g in re.findall(r"\((\d+), (\d+), (\d+)\): (\d+)", __doc__)}


@pytest.mark.parametrize("m,n,k", AC.CASES)
def test_attractive_columns_pivot_and_end_optimal(m, n, k):
    T0, basis0, x, obj, _ = AC.cold(m, n)
    A, b, c = AC.lp(m, n)
    y = AC.duals(T0, basis0, n)
    P, d = AC.new_cols(y, k)
    assert (d > y @ P + 1e-9).any(), "no attractive column: change the seed"
    T2, basis2, ref = AC.reference(T0, basis0, n, P, d)
    assert T2.shape == (m + 1, CR.tableau_ld(m, n + k)) and len(basis2) == m
    assert ref["status"] == CR.OK and 1 <= ref["done"] <= MOST
    assert _pivots_in_docstring()[(m, n, k)] == ref["done"]
    stacked = O.solve_dense(np.hstack([A, P]), b, np.r_[c, d])
    assert stacked.status == CR.OK and _close(ref["objective"], stacked.objective)
    assert ref["objective"] > obj
    x2 = ref["x"]
    assert len(x2) == n + k and (np.hstack([A, P]) @ x2 <= b + 1e-7).all() and (x2 >= 0.0).all()


@pytest.mark.parametrize("m,n,k", AC.CASES)
def test_dull_columns_do_no_pivot(m, n, k):
    T0, basis0, x, obj, _ = AC.cold(m, n)
    _, _, ref = AC.reference(T0, basis0, n, *AC.dull_cols(AC.duals(T0, basis0, n), k))
    assert ref["status"] == CR.OK and ref["done"] == 0
    assert np.float64(ref["objective"]).tobytes() == np.float64(obj).tobytes()
    assert ref["x"][:n].tobytes() == x.tobytes() and not ref["x"][n:].any()


@pytest.mark.parametrize("m,n", AC.SHAPES)
def test_a_free_ray_is_unbounded(m, n):
    T0, basis0, _, _, _ = AC.cold(m, n)
    T2, _, ref = AC.reference(T0, basis0, n, *AC.ray(m))
    assert ref["status"] == CR.UNBOUNDED and ref["done"] == 0
    assert not T2[:m, n].any() and T2[m, n] == -1.0


def test_slack_sets_are_not_empty():
    for m, n in (AC.COUNT_SHAPE, (65, 449)):
        T0, basis0, _, _, _ = AC.cold(m, n)
        basic, nonbasic = AC.slack_rows(basis0, n, m)
        assert len(basic) >= 1 and len(nonbasic) >= 1 and len(basic) + len(nonbasic) == m


def test_counted_columns_have_their_counts():
    m, n = AC.COUNT_SHAPE
    T0, basis0, _, _, _ = AC.cold(m, n)
    y = AC.duals(T0, basis0, n)
    assert m >= max(AC.COUNTS)
    for count in AC.COUNTS:
        P, d = AC.counted(y, count)
        assert P.shape == (m, 1) and (P != 0.0).sum() == count and ((P < 0.0).sum() >= 1) == (count >= 1)
        T2, _, ref = AC.reference(T0, basis0, n, P, d)
        assert ref["status"] in (CR.OK, CR.UNBOUNDED) and ref["done"] <= MOST
        if count == 0:
            assert not T2[:m, n].any() and not np.signbit(T2[:m, n]).any() and T2[m, n] == -d[0]
    basic, nonbasic = AC.slack_rows(basis0, n, m)
    for (P, d), rows in ((AC.basic_only(y, basis0, n), basic), (AC.nonbasic_only(y, basis0, n), nonbasic)):
        assert np.array_equal(np.nonzero(P[:, 0])[0], rows)
        _, _, ref = AC.reference(T0, basis0, n, P, d)
        assert ref["status"] in (CR.OK, CR.UNBOUNDED) and ref["done"] <= MOST


def test_grouped_columns_skip_each_others_rows():
    m, n = AC.COUNT_SHAPE
    T0, basis0, _, _, _ = AC.cold(m, n)
    P, d = AC.grouped(AC.duals(T0, basis0, n))
    assert P.shape == (m, AC.CT)
    assert ((P[:, 0] != 0.0) != (P[:, 1] != 0.0)).all() and (P[:, 0] != 0.0).any() and (P[:, 1] != 0.0).any()
    neg0 = P[1::2, 2]
    assert (neg0 == 0.0).all() and np.signbit(neg0).all()
    assert (P[:, 3] < 0.0).any() and d[3] < 0.0
    _, _, ref = AC.reference(T0, basis0, n, P, d)
    assert ref["status"] in (CR.OK, CR.UNBOUNDED) and ref["done"] <= MOST


def test_degenerate_family_is_bounded_and_pivots():
    got = []
    for m, n, seed in AC.DEGENERATE:
        A, b, c = O.gen_dense(m, n, seed, degenerate=True)
        s = O.solve_dense(A, b, c)
        assert s.status == CR.OK and (b == 0.0).sum() >= m // 4
        T0, basis0 = AL.R.oracle_tableau(A, b, c, AL.BIG)
        P, d = AC.new_cols(AC.duals(T0, basis0, n), 3)
        for pricing in (0, 1):
            _, _, ref = AC.reference(T0, basis0, n, P, d, pricing=pricing)
            assert ref["status"] == CR.OK and 1 <= ref["done"] <= MOST
            stacked = O.solve_dense(np.hstack([A, P]), b, np.r_[c, d])
            assert _close(ref["objective"], stacked.objective)
            got.append(ref["done"])
    assert got == [20, 76, 11, 26]                   # (the docstring's)
