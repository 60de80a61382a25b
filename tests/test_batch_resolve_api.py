"""CPU: the host side of the resident batch (dlp_batch_* / dlp.Batch): the symbols and their
declarations, argument validation in the C ABI (which comes before any device call), the loud
failure without a GPU in the documented order, and the wrapper's checks of c."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

SYMBOLS = ["dlp_batch_create_dense", "dlp_batch_resolve", "dlp_batch_read", "dlp_batch_info", "dlp_batch_free"]


def test_symbols_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dlp.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {s[0] for s in L.SIGNATURES}
    for name in SYMBOLS:
        assert hasattr(L.lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in bound, name
    assert "typedef struct dlp_batch dlp_batch;" in header
    assert "Batch" in dlp.__all__ and callable(dlp.Batch)
    for method in ("resolve", "read", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(dlp.Batch, method))


def test_free_null_returns():
    L.lib().dlp_batch_free(None)
    L.lib().dlp_batch_free(C.c_void_p())


def _din(arrays, m, n, **kw):
    d = L.BatchDenseIn(*(v.ctypes.data for v in arrays), m * n, m, n, 0, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _create(nlp, m, n, din, out, handle, opt=None):
    return L.lib().dlp_batch_create_dense(nlp, m, n, C.byref(din) if din is not None else None, opt,
                                          C.byref(out) if out is not None else None,
                                          C.byref(handle) if handle is not None else None)


def test_create_rejects_bad_arguments():
    """DLP_ERR_ARG for bad sizes, strides and NULL inputs, before any device is looked for; the
    handle comes back NULL."""
    m, n, nlp = 4, 5, 3
    A, b, c = np.ones((nlp, m, n)), np.ones((nlp, m)), np.ones((nlp, n))
    out = L.BatchOut()
    h = C.c_void_p(1)
    din = lambda **kw: _din((A, b, c), m, n, **kw)   # noqa: E731
    assert _create(0, m, n, din(), out, h) == L.ERR_ARG and not h.value
    assert _create(nlp, 0, n, din(), out, h) == L.ERR_ARG
    assert _create(nlp, m, -1, din(), out, h) == L.ERR_ARG
    assert _create(65535 * 16 + 1, m, n, din(strideA=0, strideb=0, stridec=0), out, h) == L.ERR_ARG
    assert _create(nlp, m, n, None, out, h) == L.ERR_ARG
    assert _create(nlp, m, n, din(), out, None) == L.ERR_ARG
    for f in ("A", "b", "c"):
        assert _create(nlp, m, n, din(**{f: None}), out, h) == L.ERR_ARG
    assert _create(nlp, m, n, din(strideA=m * n - 1), out, h) == L.ERR_ARG
    assert _create(nlp, m, n, din(strideb=m - 1), out, h) == L.ERR_ARG
    assert _create(nlp, m, n, din(stridec=1), out, h) == L.ERR_ARG
    assert _create(nlp, m, n, din(strideA=-m * n), out, h) == L.ERR_ARG
    assert _create(nlp, m, n, din(device=2), out, h) == L.ERR_ARG
    bad_log = L.BatchOut()
    bad_log.log_cap = -1
    assert _create(nlp, m, n, din(), bad_log, h) == L.ERR_ARG
    assert b"dlp_batch_create_dense" in L.lib().dlp_last_error()
    assert not h.value


def test_calls_on_a_null_batch_are_argument_errors():
    lib = L.lib()
    c = np.ones(5)
    out = L.BatchOut()
    assert lib.dlp_batch_resolve(None, c.ctypes.data, 0, 0, 10, C.byref(out)) == L.ERR_ARG
    assert b"dlp_batch_resolve" in lib.dlp_last_error()
    assert lib.dlp_batch_resolve(None, None, 0, 0, 10, None) == L.ERR_ARG
    T, basis = np.zeros((5, 16)), np.zeros(4, np.int32)
    assert lib.dlp_batch_read(None, 0, T.ctypes.data_as(L._DP), basis.ctypes.data_as(C.POINTER(C.c_int32))) == L.ERR_ARG
    nlp = C.c_int64()
    assert lib.dlp_batch_info(None, C.byref(nlp), None, None, None, None) == L.ERR_ARG


def test_no_device_fails_loudly_in_the_documented_order():
    """Valid arguments without a GPU: DLP_ERR_NODEVICE, also for a shape too large for the LDS
    (the device check comes before the size check, as in dlp_batched_solve_dense), with and
    without an output struct; no handle is returned."""
    if dlp.device_count() > 0:
        pytest.skip("a HIP device is visible")
    for m, n in ((4, 5), (64, 128), (200, 200)):
        nlp = 3
        A, b, c = np.ones((nlp, m, n)), np.ones((nlp, m)), np.ones((nlp, n))
        for out in (L.BatchOut(), None):
            h = C.c_void_p(1)
            assert _create(nlp, m, n, _din((A, b, c), m, n), out, h) == L.ERR_NODEVICE
            assert not h.value
        for shared in (True, False):
            with pytest.raises(dlp.DLPError) as e:
                dlp.Batch(A[0] if shared else A, b, c[0] if shared else c)
            assert e.value.status == L.ERR_NODEVICE


@pytest.mark.parametrize("shapes", [
    ((3, 4, 5), (2, 4), (3, 5)),     # batch dimensions differ
    ((4, 5), (5,), (5,)),            # b is not m long
    ((4, 5), (4,), (4,)),            # c is not n long
    ((0, 4, 5), (0, 4), (0, 5)),     # an empty batch
])
def test_batch_inconsistent_shapes_raise(shapes):
    A, b, c = (np.ones(s) for s in shapes)
    with pytest.raises(ValueError):
        dlp.Batch(A, b, c)


class _Stub(dlp.Batch):
    """The wrapper's checks of c run before the native call: a 3 x (4 x 5) batch without a
    device behind it (the handle is a dummy that is never passed on)."""

    def __init__(self):
        self._h = C.c_void_p()
        self.nlp, self.m, self.n, self.device, self.max_pivots = 3, 4, 5, 0, 100

    def _handle(self):
        raise AssertionError("the native call was reached")


@pytest.mark.parametrize("c", [
    np.ones((3, 4)), np.ones((2, 5)), np.ones(4), np.ones((3, 5, 1)), np.ones((1, 3, 5)), np.float64(1.0),
    np.ones((3, 5), dtype=complex), np.array(["a"] * 5), np.ones(5, dtype=bool),
], ids=lambda c: f"{c.dtype}{c.shape}")
def test_resolve_rejects_bad_c(c):
    with pytest.raises(ValueError):
        _Stub().resolve(c)


def test_resolve_rejects_a_negative_budget_and_a_closed_batch():
    with pytest.raises(ValueError):
        _Stub().resolve(np.ones(5), max_pivots=-1)
    closed = dlp.Batch.__new__(dlp.Batch)
    closed._h = C.c_void_p()
    closed.nlp, closed.m, closed.n, closed.device, closed.max_pivots = 3, 4, 5, 0, 100
    with pytest.raises(ValueError):
        closed.resolve(np.ones(5))
    with pytest.raises(ValueError):
        closed.read(0)
    closed.close()
