"""CPU: the host side of dlp_batched_solve_dense / dlp.batched_solve_dense (the batch solve of
caller-supplied LPs): the symbol and its binding, argument validation in the wrapper and in
the C ABI (which comes before the device check), and the loud failure without a GPU."""
import ctypes as C

import numpy as np
import pytest

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L


def test_symbol_exported_and_bound():
    assert "dlp_batched_solve_dense" in {s[0] for s in L.SIGNATURES}
    assert hasattr(L.lib(), "dlp_batched_solve_dense")
    assert "batched_solve_dense" in dlp.__all__ and callable(dlp.batched_solve_dense)
    # the two argument structs mirror include/dlp.h
    assert C.sizeof(L.BatchDenseIn) == 56 and C.sizeof(L.BatchOut) == 72
    assert L.BatchDenseIn.device.offset == 48 and L.BatchOut.log_cap.offset == 40
    assert L.BatchOut.kernel_ms.offset == 64


def test_batch_result_six_positional_fields():
    z = np.zeros(1)
    r = dlp.BatchResult(z, z, z, None, None, 0.5)
    assert r.kernel_ms == 0.5 and r.x is None and r.y is None
    r = dlp.BatchResult(z, z, z, None, None, 0.5, z, z)
    assert r.x is z and r.y is z


@pytest.mark.parametrize("shapes", [
    ((3, 4, 5), (2, 4), (3, 5)),     # batch dimensions differ
    ((3, 4, 5), (3, 4), (2, 5)),
    ((4, 5), (5,), (5,)),            # b is not m long
    ((4, 5), (4,), (4,)),            # c is not n long
    ((3, 4, 5), (3, 5), (3, 5)),
    ((4,), (4,), (4,)),              # A has no columns
    ((2, 3, 4, 5), (4,), (5,)),
    ((4, 5), (1, 2, 4), (5,)),
    ((0, 4, 5), (0, 4), (0, 5)),     # an empty batch
    ((4, 0), (4,), (0,)),
])
def test_inconsistent_shapes_raise(shapes):
    A, b, c = (np.ones(s) for s in shapes)
    with pytest.raises(ValueError):
        dlp.batched_solve_dense(A, b, c)


def test_mixed_input_kinds_raise():
    class FakeTensor:
        def data_ptr(self):
            return 0
    with pytest.raises(ValueError):
        dlp.batched_solve_dense(FakeTensor(), np.ones(4), np.ones(5))


def _call(nlp, m, n, din, out, opt=None):
    return L.lib().dlp_batched_solve_dense(nlp, m, n, C.byref(din) if din is not None else None, opt,
                                           C.byref(out) if out is not None else None)


def test_c_abi_rejects_bad_arguments():
    """DLP_ERR_ARG for bad sizes, strides and NULL inputs, before any device is looked for."""
    m, n, nlp = 4, 5, 3
    A, b, c = np.ones((nlp, m, n)), np.ones((nlp, m)), np.ones((nlp, n))
    obj = np.zeros(nlp)
    out = L.BatchOut()
    out.objective = obj.ctypes.data_as(C.POINTER(C.c_double))

    def din(**kw):
        d = L.BatchDenseIn(A.ctypes.data, b.ctypes.data, c.ctypes.data, m * n, m, n, 0, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert _call(0, m, n, din(), out) == L.ERR_ARG
    assert _call(nlp, 0, n, din(), out) == L.ERR_ARG
    assert _call(nlp, m, -1, din(), out) == L.ERR_ARG
    assert _call(65535 * 16 + 1, m, n, din(strideA=0, strideb=0, stridec=0), out) == L.ERR_ARG
    assert _call(nlp, m, n, None, out) == L.ERR_ARG
    assert _call(nlp, m, n, din(), None) == L.ERR_ARG
    for f in ("A", "b", "c"):
        assert _call(nlp, m, n, din(**{f: None}), out) == L.ERR_ARG
    assert _call(nlp, m, n, din(strideA=m * n - 1), out) == L.ERR_ARG
    assert _call(nlp, m, n, din(strideb=m - 1), out) == L.ERR_ARG
    assert _call(nlp, m, n, din(stridec=1), out) == L.ERR_ARG
    assert _call(nlp, m, n, din(strideA=-m * n), out) == L.ERR_ARG
    assert _call(nlp, m, n, din(device=2), out) == L.ERR_ARG
    bad_log = L.BatchOut()
    bad_log.log_cap = -1
    assert _call(nlp, m, n, din(), bad_log) == L.ERR_ARG
    assert b"dlp_batched_solve_dense" in L.lib().dlp_last_error()


def test_no_device_fails_loudly():
    """Valid arguments without a GPU: DLP_ERR_NODEVICE (there is no CPU fallback), for the
    register-kernel shape, an LDS-kernel shape, shared arrays and a shape too large for the LDS
    alike (the device check comes before the size check)."""
    if dlp.device_count() > 0:
        pytest.skip("a HIP device is visible")
    for m, n in ((4, 5), (64, 128), (200, 200)):
        for batched in (True, False):
            A = np.ones((3, m, n) if batched else (m, n))
            with pytest.raises(dlp.DLPError) as e:
                dlp.batched_solve_dense(A, np.ones((3, m)), np.ones(n))
            assert e.value.status == L.ERR_NODEVICE
