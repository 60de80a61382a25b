"""CPU: the host side of dlp_batch_rhs_kernel / Batch.rhs_kernel, and the inputs
of tests/test_gpu_batch_rhs_reg.py held against the reference before any GPU sees them: what
the GPU file claims to exercise (dual pivots in the warm batches, the all-nonbasic and the
all-basic slack bases, exact ties in the row selection and across a wave boundary in the slot
selection) is checked here on the CPU oracle of the dual rule (oracle_resolve_rhs, the binding
tests/test_oracle_dual.py holds against tests/rhs_ref.py) and on rhs_ref itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_py as O
import rhs_ref as RR
import rhs_reg_inputs as I
from conftest import ROOT

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

NAME = "dlp_batch_rhs_kernel"


def test_symbol_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "dlp.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(L.lib(), NAME)
    assert re.search(r"\b%s\s*\(" % NAME, header)
    sig = {s[0]: s for s in L.SIGNATURES}
    assert NAME in sig and len(sig[NAME][2]) == 4
    assert callable(dlp.Batch.rhs_kernel)
    knobs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "DLP_BATCH_RHS_LDS" in knobs


def test_null_batch_is_an_argument_error():
    lib = L.lib()
    lib.dlp_batch_resolve(None, None, 0, 0, 10, None)   # (another function's name in dlp_last_error)
    assert lib.dlp_batch_rhs_kernel(None, None, None, None) == L.ERR_ARG
    assert NAME.encode() in lib.dlp_last_error()


def test_rhs_kernel_of_a_closed_batch_raises():
    closed = dlp.Batch.__new__(dlp.Batch)
    closed._h = C.c_void_p()
    closed.nlp, closed.m, closed.n, closed.device, closed.max_pivots = 3, 4, 5, 0, 100
    with pytest.raises(ValueError, match="closed"):
        closed.rhs_kernel()
    closed.close()


# ---- the warm batches: every LP ends DLP_OK, at least half of each batch pivots
@pytest.mark.parametrize("degen", [False, True], ids=["dense", "degenerate"])
@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("n", I.WARM_N)
def test_warm_batches_end_optimal_and_pivot(n, pricing, degen):
    colds = I.warm_cold(n, degen, pricing)
    for scale in I.SCALES:
        b2 = I.warm_b2(n, degen, scale)
        assert b2.shape == (I.NLP, I.M) and np.isfinite(b2).all()
        res = [O.resolve_rhs(T, basis, n, b2[k], pricing=pricing) for k, (T, basis, _) in enumerate(colds)]
        assert all(r["status"] == RR.OK for r in res), (scale, [r["status"] for r in res])
        done = [r["done"] for r in res]
        assert sum(d >= 1 for d in done) >= I.NLP // 2, (scale, done)
        assert max(done) <= 4096, done   # (the GPU file's log capacity)


def test_oracle_and_numpy_reference_agree_on_a_warm_case():
    """The CPU checks above run the C++ oracle of the dual rule, the GPU file numpy's rhs_ref:
    the same bits on one of the inputs (tests/test_oracle_dual.py holds the two together at
    large)."""
    n = 65
    T, basis, _ = I.warm_cold(n, True, 0)[0]
    bk = I.warm_b2(n, True, 0.3)[0]
    a, b = O.resolve_rhs(T, basis, n, bk), RR.resolve_rhs(T, basis, n, bk)
    assert a["status"] == b["status"] == RR.OK and a["done"] == b["done"] >= 2
    assert a["log"].tobytes() == b["log"].tobytes() and a["basis"].tobytes() == b["basis"].tobytes()
    assert np.float64(a["objective"]).tobytes() == np.float64(b["objective"]).tobytes()


# ---- the two extreme bases of the rebuild
def test_all_nonbasic_construction_reaches_its_basis():
    n = I.ALLNB_N
    b2 = I.all_nonbasic_b2()
    for k, lp in enumerate(I.all_nonbasic_lps()):
        T, basis, var = I.cold(*lp)
        assert (basis < n).all(), (k, basis)                       # every row's basic variable structural
        assert sorted(var[var >= n]) == list(range(n, n + I.M))    # every slack in a slot
        assert RR.resolve_rhs(T, basis, n, b2[k], max_pivots=0)["status"] in (RR.OK, RR.PIVOT_LIMIT)


def test_slack_basis_construction_stays_at_the_slack_basis():
    n = I.SLACK_N
    b2 = I.slack_basis_b2()
    status = []
    for k, (A, b, c) in enumerate(I.slack_basis_lps()):
        assert (c <= 0.0).all() and (b >= 0.0).all()
        T, basis, var = I.cold(A, b, c)
        assert basis.tolist() == list(range(n, n + I.M)) and var.tolist() == list(range(n))   # no pivot
        rhs = RR.fold_rhs(T, n, b2[k])
        assert rhs[:I.M].tobytes() == b2[k].tobytes()   # B^-1 = I: the rebuilt column is b itself
        assert (b2[k] < 0.0).any()
        r = O.resolve_rhs(T, basis, n, b2[k])
        assert r["done"] >= 1
        status.append(r["status"])
    assert RR.OK in status, status


# ---- exact ties, counted on the reference's trace
def test_tie_lps_tie_in_the_row_and_across_a_wave_in_the_slot_selection():
    lps, b2 = I.tie_lps()
    rows = slots = zero_ratio = 0
    for k, lp in enumerate(lps):
        T, basis, var = I.cold(*lp)
        r, s, last = I.count_ties(T, basis, var, I.TIE_N, b2[k])
        whole = O.resolve_rhs(T, basis, I.TIE_N, b2[k])
        assert whole["status"] == RR.OK
        # (one pivot per call with the continuation reaches the unbounded call's basis)
        assert last["basis"].tobytes() == whole["basis"].tobytes()
        rows, slots = rows + r, slots + s
        zero_ratio += int((whole["log"]["ratio"] == 0.0).sum())
    assert rows >= 1, "no exact tie in the leaving-row selection"
    assert slots >= 1, "no exact entering-slot tie between a slot < 64 and a slot >= 64"
    assert zero_ratio >= 1, "no pivot with r_q = 0: Bland mode is never entered"
