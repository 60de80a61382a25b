"""General LPs on every deferred block size, pass form and row band.

General LPs are the only sessions with nprice < N (the artificial columns are never priced) and
rows_elig < rows (the carried Phase II objective row is local row m': every pivot updates it, no
ratio test sees it).  The inputs (general_lp.DEFER_INPUTS, pinned on the CPU oracle by
tests/test_general_defer_inputs.py) put nprice on / beside a 512-column pricing tile and the
carried row on / beside a 128-lane ratio workgroup, so a chain or pass kernel instance that
drops either boundary changes the pivot sequence or the tableau.

The bar, with no tolerance anywhere: status, pivot count, phase1_pivots, every log field, x, y,
objective and basis equal O.solve_general bit for bit (_check), and where stated the whole
read-out tableau (carried row, artificial columns, objective row, padding) equals an eager
(defer = 1) session's at the same pivot count byte for byte; the eager session is held against
the oracle in the same test (_eager).

Tableau stops: 81 pivots (inside Phase I, mid-block at K = 64), phase1_pivots (right after the
drive-out and the carry-in: the objective row then equals the carried row), the end.  run(81)
must report exactly 81.  dlp_session_run "launches up to max_pivots": a window that holds the
Phase I optimum and a forced slot on a redundant row spend budget without a pivot, so the
second stop is reached by asking for the pivots still missing until none is (each call reports
at most what it was asked for, the count lands on phase1_pivots exactly), then by single units of
budget that must do no pivot until the carry-in has run, and the deferred session must report the
same (asked, done) sequence as the eager one."""
import functools

import numpy as np
import pytest

import oracle_py as O
from conftest import load_golden
from general_lp import DEFER_INPUTS, INF, defer_input, fixture_lp, lp_arrays

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in load_golden("general.json")}
MID = 81


def _same_log(got, ref):
    """Every field of every pivot; the message names the first differing pivot."""
    g, r = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    for k in range(min(len(g), len(r))):
        if g[k].tobytes() != r[k].tobytes():
            raise AssertionError(f"pivot {k}: gpu {g[k]} oracle {r[k]}")
    assert len(g) == len(r), f"gpu logged {len(g)} pivots, the oracle {len(r)} (equal up to the shorter)"


def _check(res, ref):
    """tests/test_gpu_general.py's bar: everything a result holds, bit for bit."""
    _same_log(res.pivot_log, ref.pivot_log)
    assert res.status == ref.status
    assert res.num_pivots == ref.num_pivots
    assert res.phase1_pivots == ref.phase1_pivots
    assert np.float64(res.objective).tobytes() == np.float64(ref.objective).tobytes()
    assert res.x.tobytes() == ref.x.tobytes()
    assert res.y.tobytes() == ref.y.tobytes()
    assert res.basis.tobytes() == ref.basis.tobytes()


@functools.lru_cache(maxsize=None)
def _input(label):
    """(lp, problem, (m', N, nprice)) of a generated input, or of a fixture of general.json."""
    lp = fixture_lp(defer_input(label) if label in DEFER_INPUTS else CASES[label])
    m_std, ncols, nprice, _ = O.general_std_dims(lp)
    return lp, dlp.Problem.general(*lp_arrays(lp)), (m_std, ncols, nprice)


@functools.lru_cache(maxsize=None)
def _ref(label, pricing=0):
    return O.solve_general(_input(label)[0], pricing=pricing)


def _same_tableau(got, want, label, what):
    """Byte equality; the message names the first differing (row, column) and what they are."""
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    m_std, N, nprice = _input(label)[2]
    i, j = (int(v) for v in np.argwhere(got.view(np.uint64) != want.view(np.uint64))[0])
    nbad = int((got.view(np.uint64) != want.view(np.uint64)).sum())
    carried = got.shape[0] == m_std + 2   # rows: m' constraint rows, the carried row, the objective row
    row = ("the carried row" if carried and i == m_std else
           "the objective row" if i == got.shape[0] - 1 else "a constraint row")
    col = ("priced (< nprice)" if j < nprice else "artificial (>= nprice)" if j < N else
           "the RHS" if j == N else "padding")
    raise AssertionError(f"{label} {what}: {nbad} tableau elements differ, first at row {i} ({row}), column {j} "
                         f"({col}; nprice {nprice}, N {N}): deferred {got[i, j]!r} eager {want[i, j]!r}")


def _run_stops(s, label, ref):
    """The three tableau stops (module docstring): ({stop: tableau}, [(asked, done), ...])."""
    out, sched = {}, []
    nprice = _input(label)[2][2]
    p1 = ref.phase1_pivots
    assert MID < p1
    st, done = s.run(MID)
    assert (st, done) == (L.RUNNING, MID)
    out[MID] = s.tableau()
    npiv = MID
    for _ in range(8):
        if npiv == p1:
            break
        st, done = s.run(p1 - npiv)
        assert st == L.RUNNING and 0 <= done <= p1 - npiv, (st, done, p1 - npiv)
        sched.append((p1 - npiv, done))
        npiv += done
    assert npiv == p1 == s.status()[1], (npiv, p1, sched)
    # What may still be missing does no pivot: the slot that finds the Phase I optimum (when no real
    # drive-out pivot follows it) and the forced slots of redundant rows at the end of the drive-out
    # list; the carry-in follows the last of them.  One unit of budget spends one such slot.
    T = s.tableau()
    for _ in range(1 + int((ref.basis >= nprice).sum())):   # (a redundant row keeps its artificial to the end)
        if T[-1].tobytes() == T[-2].tobytes():
            break
        st, done = s.run(1)
        assert (st, done) == (L.RUNNING, 0), (st, done, sched)
        sched.append((1, 0))
        T = s.tableau()
    out["phase1"] = T
    assert T[-1].tobytes() == T[-2].tobytes(), "the carry-in has not run at phase1_pivots"
    st, done = s.run(10 ** 6)
    assert st == ref.status and npiv + done == ref.num_pivots
    out["end"] = s.tableau()
    return out, sched


@functools.lru_cache(maxsize=None)
def _eager(label, pricing=0):
    """The eager session of the input: its tableau at the stops, itself exact against the oracle."""
    ref = _ref(label, pricing)
    with dlp.Session(_input(label)[1], defer=1, pricing=pricing) as e:
        assert e.get_defer_tuning()[2] == 1
        stops, sched = _run_stops(e, label, ref)
        _check(e.result(), ref)
    m_std = _input(label)[2][0]
    assert stops["end"].shape[0] == m_std + 2
    return stops, sched


def _solve(label, ref, tune=None, **opts):
    """One run to the end: the result against the oracle, the end tableau returned."""
    with dlp.Session(_input(label)[1], **opts) as s:
        if tune:
            tune(s)
        st, done = s.run(10 ** 6)
        _check(s.result(), ref)   # first: a wrong pivot is named before a wrong count
        assert st == ref.status and done == ref.num_pivots
        return s.tableau()


# ---- 1. block sizes ------------------------------------------------------------------------
@pytest.mark.parametrize("label,pricing", [("T0", 0), ("Tm", 0), ("Tp", 0), ("Rm", 0), ("Rp", 0),
                                           ("Tm", 1), ("Rp", 1)])
@pytest.mark.parametrize("K", [2, 3, 8, 16, 32, 64])
def test_block_sizes(K, label, pricing):
    """Every ratio / pivot-row template instance (K rounds up to 4 / 8 / 16 / 32 / 64) with
    nprice < N and the carried row, in both pricing modes."""
    ref = _ref(label, pricing)

    def tune(s):
        assert s.get_defer_tuning()[2] == K

    T = _solve(label, ref, tune, defer=K, pricing=pricing)
    _same_tableau(T, _eager(label, pricing)[0]["end"], label, f"K {K} pricing {pricing} end")


# ---- 2. pass forms ---------------------------------------------------------------------------
FORMS_32 = [0, 4, 6, 7, 10, 11, 14, 15, 16, 17, 20]   # 2 doubles per lane: at most 32 steps
FORMS_64 = [1, 2, 3, 5, 8, 9, 12, 13, 18, 19]
FORM_K = ([(f, K) for f in FORMS_32 for K in (16, 32)] + [(f, K) for f in FORMS_64 for K in (16, 64)] +
          [(f, K) for f in (21, 22, 23) for K in (64, 40)])   # K = 40: forms 21-23 run form 3's pass


@pytest.mark.parametrize("label", ["T0", "Rm"])
@pytest.mark.parametrize("form,K", FORM_K)
def test_pass_forms(form, K, label):
    """Every form dlp_session_set_defer_tuning accepts, at the K it is built for: the tableau at
    the three stops, then the result."""
    ref = _ref(label)
    want, want_sched = _eager(label)
    with dlp.Session(_input(label)[1], defer=K) as s:
        s.set_defer_tuning(0, form)
        assert s.get_defer_tuning() == (0, form, K)
        got, sched = _run_stops(s, label, ref)
        assert s.get_defer_tuning() == (0, form, K)
        _check(s.result(), ref)
    assert sched == want_sched
    for stop in (MID, "phase1", "end"):
        _same_tableau(got[stop], want[stop], label, f"form {form} K {K} stop {stop}")


def test_two_doubles_forms_refuse_more_than_32_steps():
    with dlp.Session(_input("S")[1], defer=64) as s:
        for form in FORMS_32:
            with pytest.raises(L.DLPError) as e:
                s.set_defer_tuning(0, form)
            assert e.value.status == L.ERR_ARG and "at most 32 steps" in str(e.value)


# ---- 3. row bands ----------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("label", ["T0", "Rp"])
@pytest.mark.parametrize("K,form", [(16, 3), (16, 4), (16, 23), (64, 3), (64, 21), (64, 23)])
@pytest.mark.parametrize("band", ["1", "2", "37", "m", "m+1", "m+2"])
def test_row_bands(band, K, form, label, nt):
    """rows_per_block around the carried row (local row m' of m' + 2): last in a band, alone with
    the objective row in a band, at both parities of a 2-row / 4-row group tail."""
    m_std = _input(label)[2][0]
    rb = {"1": 1, "2": 2, "37": 37, "m": m_std, "m+1": m_std + 1, "m+2": m_std + 2}[band]
    ref = _ref(label)

    def tune(s):
        s.set_defer_tuning(0, form)
        assert s.get_tuning()[1:] == (rb, nt) and s.get_defer_tuning() == (0, form, K)

    T = _solve(label, ref, tune, defer=K, rows_per_block=rb, nontemporal=nt)
    _same_tableau(T, _eager(label)[0]["end"], label, f"rows_per_block {rb} K {K} form {form} nt {nt} end")


# ---- 4. fused pivot --------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["Tm", "Rp"])
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_fused_pivot(K, fused, label):
    """Ratio test + selection + pivot row as one launch (pivot_defer_kernel<K>) or as two."""
    ref = _ref(label)
    T = _solve(label, ref, lambda s: s.set_fused_pivot(bool(fused)), defer=K)
    _same_tableau(T, _eager(label)[0]["end"], label, f"K {K} fused {fused} end")


# ---- 5. windows and slices -------------------------------------------------------------------
@pytest.mark.parametrize("label", ["S", "T0"])
@pytest.mark.parametrize("slice_", [4, 50])
@pytest.mark.parametrize("K", [8, 64])
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("ci", [3, 7, 64, 100])
def test_windows_and_slices(ci, graph, K, slice_, label):
    """The Phase I end, the drive-out pivots and the carry-in land in different calls, windows
    and places of a block."""
    ref = _ref(label)
    with dlp.Session(_input(label)[1], defer=K, check_interval=ci, use_graph=graph) as s:
        st, calls = L.RUNNING, 0
        while st == L.RUNNING:
            st, done = s.run(slice_)
            assert 0 <= done <= slice_
            calls += 1
            assert calls <= ref.num_pivots + 64, "the solve does not end"
        assert st == ref.status
        _check(s.result(), ref)


# ---- 6. fixtures at the untested K -----------------------------------------------------------
@pytest.mark.parametrize("name", ["basic_artificial_vars", "lpgen_2d_20x20_eq", "network_flow",
                                  "enzo_c_infeasible", "bounds_equal_but_infeasible", "enzo_c_unbounded"])
@pytest.mark.parametrize("K,form", [(2, -1), (32, -1), (64, -1), (64, 23)])
def test_fixtures(K, form, name):
    ref = _ref(name)
    with dlp.Session(_input(name)[1], defer=K) as s:
        if form >= 0:
            s.set_defer_tuning(0, form)
        assert s.get_defer_tuning()[2] == K
        st, _ = s.run(10 ** 6)
        res = s.result()
    assert st == ref.status
    _check(res, ref)
    if ref.status == L.INFEASIBLE:
        assert np.isnan(res.objective) and not res.y.any()


# ---- 7. no Phase I ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 64])
def test_no_phase1(K):
    """All-L rows with b >= 0 and x >= 0 (and a free row): no artificials, no carried row, and
    the pivots of the dense path."""
    A, b, c = O.gen_dense(64, 80, 9)
    dense = O.solve_dense(A, b, c)
    gpu_dense = dlp.solve(dlp.Problem.dense(A, b, c))
    _same_log(gpu_dense.pivot_log, dense.pivot_log)
    rl = np.full(65, -INF)
    rh = np.concatenate([b, [INF]])
    prob = dlp.Problem.general(np.vstack([A, np.ones(80)]), rl, rh, np.zeros(80), np.full(80, INF), c, 0.0,
                               L.MAXIMIZE)
    assert prob.std_dims() == (64, 144, 144, 0)
    with dlp.Session(prob, defer=K) as s:
        assert s.get_defer_tuning()[2] == K and s.rows == 64
        st, _ = s.run(10 ** 6)
        res = s.result()
    assert st == L.OK and res.phase1_pivots == 0
    _same_log(res.pivot_log, dense.pivot_log)
    assert res.objective == dense.objective and res.x.tobytes() == dense.x.tobytes()


# ---- 8. lookahead request --------------------------------------------------------------------
def test_lookahead_request_stays_off():
    """lookahead = 1 on a general session is silently off; the solve is exact (three tiles, the
    third unpriced)."""
    ref = _ref("W")
    with dlp.Session(_input("W")[1], defer=64, lookahead=1) as s:
        assert s.lookahead() is False and s.get_defer_tuning()[2] == 64
        st, _ = s.run(10 ** 6)
        assert s.lookahead() is False
        assert st == ref.status
        _check(s.result(), ref)


# ---- 9. the exchange kernels on one rank -----------------------------------------------------
@pytest.mark.parametrize("label", ["Tm", "Rp"])
@pytest.mark.parametrize("K,form", [(32, -1), (64, -1), (64, 21), (64, 23)])
@pytest.mark.parametrize("exchange", [L.XCHG_RCCL, L.XCHG_PEER], ids=["rccl", "peer"])
def test_exchange_one_rank(exchange, K, form, label):
    """commit_defer_kernel and the select path with nprice < N, on a 1-rank communicator."""
    ref = _ref(label)

    def tune(s):
        assert s.get_exchange() == exchange and s.get_defer_tuning()[2] == K
        if form >= 0:
            s.set_defer_tuning(0, form)

    T = _solve(label, ref, tune, rank=0, nranks=1, rccl_id=dlp.comm_unique_id(), exchange=exchange, defer=K)
    _same_tableau(T, _eager(label)[0]["end"], label, f"exchange {exchange} K {K} form {form} end")


# ---- 10. the one refusal that exists ---------------------------------------------------------
def test_host_driven_general_rank_is_eager():
    with pytest.raises(L.DLPError) as e:
        dlp.Session(_input("S")[1], rank=0, nranks=2, defer=16)
    assert e.value.status == L.ERR_ARG and "defer = 1" in str(e.value)
