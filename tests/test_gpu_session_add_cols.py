"""dlp_session_add_cols on the GPU: variables added to a live session on the eager
path and on every deferred path, then the primal phase on that path.

Reference: built from the session's own read-out before the call: tests/cols_ref.py's add_cols (the
column rule in numpy), then its primal_phase continuing from the widened tableau (one reference per
distinct read-out: sessions whose read-outs are byte-identical share it).  Bar (DESIGN.md §24's /
§26's, test_gpu_session_rhs_defer's _bar / _same_as): status, pivot count, basis, every log field,
x (n + k entries), y and the objective bit for bit; the nonbasic columns and the RHS byte for byte;
the whole read-out byte for byte on the full layout and equal as values on the condensed one.
Nothing may depend on K, the pass form, the row band, check_interval, use_graph or the budgets.

Inputs: tests/add_cols_lp.py; tests/test_session_add_cols_api.py holds their properties on the CPU
(pivot counts, statuses, the contributing-entry counts).  Every session has small_lp=-1."""
import functools
import hashlib

import numpy as np
import pytest

import add_cols_lp as AC
import add_rows_lp as AL
import cols_ref as CR
import dual_lp as D
import oracle_py as O
import reopt_ref as R
import rows_ref as AR

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

import test_gpu_session_rhs as S
import test_gpu_session_rhs_defer as SD

pytestmark = pytest.mark.gpu

BIG = AC.BIG
PATHS = {
    "eager": dict(defer=1),
    "k16f": dict(defer=16, condensed=-1),
    "k4c": dict(defer=4, condensed=1),
    "k16c": dict(defer=16, condensed=1),
    "k64c": dict(defer=64, condensed=1),
}
DEFERRED = [p for p in PATHS if p != "eager"]


def _open(prob, path, **more):
    opts = PATHS[path] if isinstance(path, str) else path
    return dlp.Session(prob, small_lp=-1, **opts, **more)


def _prob(m, n):
    return dlp.Problem.dense(*AC.lp(m, n))


def _round16(v):
    return (v + 15) // 16 * 16


_REFS = {}


def _ref(T2, basis2, n2, pricing=0, max_pivots=10 ** 6):
    """cols_ref.primal_phase on a widened read-out (read-only; computed once per distinct input)."""
    key = (hashlib.sha1(np.ascontiguousarray(T2).tobytes()).digest(), basis2.tobytes(), n2, pricing, max_pivots)
    if key not in _REFS:
        _REFS[key] = CR.primal_phase(T2, basis2, n2, pricing=pricing, max_pivots=max_pivots)
    return _REFS[key]


def _add(name, s, P, d):
    """add_cols on a session, the read-out right after it against cols_ref.add_cols on the read-out
    right before it, at the bar.  Returns (T0, basis0, T2, basis2)."""
    np0 = s.status()[1]
    T0, basis0 = s.tableau(), s.result().basis
    m, n = len(basis0), s.n
    P = np.asarray(P, dtype=np.float64).reshape(m, -1)
    k = P.shape[1]
    assert (s.m, s.rows, s.ncols) == (m, m, n + m), name
    cond = s.condensed
    T2, basis2 = CR.add_cols(T0, basis0, n, P, d)
    assert s.add_cols(P, d) >= 0.0, name
    n2, N2 = n + k, n + k + m
    assert s.status() == (L.RUNNING, np0), name
    assert (s.m, s.n, s.rows, s.ncols, s.ld) == (m, n2, m, N2, AR.tableau_ld(m, n2)), name
    assert s.storage() == ((_round16(n2 + 1), n2, True) if cond else (AR.tableau_ld(m, n2), N2, False)), name
    res = s.result()
    assert res.basis.tobytes() == basis2.tobytes(), name
    assert len(res.y) == m and len(res.x) == n2, name
    T1 = s.tableau()
    assert T1.shape == T2.shape, name
    new = T1[:, n:n2].view(np.int64) != T2[:, n:n2].view(np.int64)
    assert not new.any(), f"{name}: new columns differ from the rule at (row, column) {np.argwhere(new)[:8]}"
    assert SD._nonbasic_and_rhs(T1, basis2, N2) == SD._nonbasic_and_rhs(T2, basis2, N2), name
    assert np.array_equal(T1, T2), name
    if not cond:
        assert T1.tobytes() == T2.tobytes(), f"{name}: the full layout's read-out differs in some byte"
    assert s.read_rows(m, 1).tobytes() == T1[m:].tobytes(), name
    # x, y and the objective are read from the widened tableau as it stands
    x = np.zeros(n2)
    rows = np.nonzero(basis2 < n2)[0]
    x[basis2[rows]] = T2[rows, N2]
    assert res.x.tobytes() == x.tobytes() and np.array_equal(res.y, T2[m, n2:N2]), name
    assert np.float64(res.objective).tobytes() == T2[m, N2].tobytes(), name
    return T0, basis0, T2, basis2


def _cold(prob, path, **more):
    s = _open(prob, path, **more)
    assert s.run(BIG)[0] == L.OK
    return s


def _y(s):
    return s.result().y


def _finish(name, s, np0, T2, basis2, pricing=0):
    """run() to the end of the primal phase against the reference on the widened read-out."""
    n2 = s.n
    ref = _ref(T2, basis2, n2, pricing=pricing)
    st, done = s.run(BIG)
    assert done == ref["done"], (name, done, ref["done"])
    res = SD._bar(name, s, st, np0, ref, n2 + len(basis2))
    assert len(res.x) == n2 and s.run(BIG) == (st, 0), name
    return res, ref


def _phase(name, prob, path, cols, pricing=0, **more):
    """Cold solve on `path`, add_cols(cols(result)), the primal phase to its end, against the
    reference on the session's own read-out.  Returns (blob, final tableau, reference)."""
    with _cold(prob, path, pricing=pricing, **more) as s:
        np0 = s.status()[1]
        P, d = cols(s.result())
        _, _, T2, basis2 = _add(name, s, P, d)
        assert not s.lookahead(), name
        assert s.get_defer_tuning()[2] == (PATHS[path] if isinstance(path, str) else path)["defer"], name
        res, ref = _finish(name, s, np0, T2, basis2, pricing)
        return S._blob(res), s.tableau(), ref


# ---- 1. the columns alone

@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("m,n,k", AC.CASES)
def test_columns_alone(m, n, k, path):
    with _cold(_prob(m, n), path) as s:
        _add(f"{m}x{n} k {k} {path}", s, *AC.new_cols(_y(s), k))


@pytest.mark.parametrize("path", ["eager", "k16f", "k16c"])
def test_contributing_entry_counts(path):
    """Columns with exactly 0, 1, T - 1, T, T + 1, 2 T + 1 nonzero p_l (T: the fold's list tile), one
    session per count; then nonzeros only on the rows whose slack is basic (condensed: unit terms
    only) and only on those whose slack is nonbasic."""
    m, n = AC.COUNT_SHAPE
    prob = _prob(m, n)
    makers = [(f"count {c}", lambda res, c=c: AC.counted(res.y, c)) for c in AC.COUNTS]
    makers += [("basic only", lambda res: AC.basic_only(res.y, res.basis, n)),
               ("nonbasic only", lambda res: AC.nonbasic_only(res.y, res.basis, n))]
    for what, make in makers:
        with _cold(prob, path) as s:
            np0 = s.status()[1]
            P, d = make(s.result())
            _, _, T2, basis2 = _add(f"{what} {path}", s, P, d)
            if what == "count 0":
                col = s.tableau()[:, n]
                assert not col[:m].any() and not np.signbit(col[:m]).any() and col[m] == -d[0]
            _finish(f"{what} {path}", s, np0, T2, basis2)


@pytest.mark.parametrize("path", ["eager", "k16f", "k64c"])
def test_column_group(path):
    """One group of CT columns: column 1 zero exactly where column 0 is not, -0.0 entries, negative
    entries and a negative cost."""
    m, n = AC.COUNT_SHAPE
    with _cold(_prob(m, n), path) as s:
        np0 = s.status()[1]
        _, _, T2, basis2 = _add(f"group {path}", s, *AC.grouped(_y(s)))
        _finish(f"group {path}", s, np0, T2, basis2)


def test_no_columns_touches_nothing():
    m, n = 63, 70
    with _cold(_prob(m, n), "k16c") as s:
        before, T0 = S._blob(s.result()), s.tableau().tobytes()
        assert L.lib().dlp_session_add_cols(s._h, 0, None, None, m, None) == L.OK
        assert s.add_cols(np.zeros((m, 0)), np.zeros(0)) == 0.0
        assert s.status()[0] == L.OK and S._blob(s.result()) == before and s.tableau().tobytes() == T0
        assert s.n == n and s.run(BIG) == (L.OK, 0)


# ---- 2. the primal phase: the eager route against the reference, every deferred path against it

@functools.lru_cache(maxsize=None)
def _eager(m, n, k, pricing=0):
    blob, T, ref = _phase(f"eager {m}x{n} k {k} pricing {pricing}", _prob(m, n), "eager",
                          lambda res: AC.new_cols(res.y, k), pricing=pricing)
    assert blob[0] == L.OK and ref["done"] >= 1
    return blob, T


@pytest.mark.parametrize("m,n,k", AC.CASES)
def test_primal_phase_eager_every_case(m, n, k):
    _eager(m, n, k)


# (Bland pricing at 65 x 449 only: its 99 numpy pivots at 300 x 740 take longer than a test should)
@pytest.mark.parametrize("path", DEFERRED)
@pytest.mark.parametrize("m,n,k,pricing", [(65, 449, 5, 0), (65, 449, 5, 1), (300, 740, 3, 0)])
def test_primal_phase_every_path(m, n, k, pricing, path):
    name = f"{m}x{n} k {k} {path} pricing {pricing}"
    blob, T, ref = _phase(name, _prob(m, n), path, lambda res: AC.new_cols(res.y, k), pricing=pricing)
    eb, eT = _eager(m, n, k, pricing)
    assert blob == eb and np.array_equal(T, eT), name
    if not PATHS[path]["condensed"] == 1:
        assert T.tobytes() == eT.tobytes(), "the full layout's read-out differs from the eager session's"


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("path", ["eager", "k16f", "k16c", "k64c"])
@pytest.mark.parametrize("m,n,seed", AC.DEGENERATE)
def test_primal_phase_degenerate_family(m, n, seed, path, pricing):
    A, b, c = O.gen_dense(m, n, seed, degenerate=True)
    blob, T, ref = _phase(f"degenerate {m}x{n} {path} pricing {pricing}", dlp.Problem.dense(A, b, c), path,
                          lambda res: AC.new_cols(res.y, 3), pricing=pricing)
    assert blob[0] == L.OK and ref["done"] >= 1


@pytest.mark.parametrize("path", list(PATHS))
def test_dull_columns_do_no_pivot(path):
    m, n, k = 65, 449, 5
    blob, T, ref = _phase(f"dull {path}", _prob(m, n), path, lambda res: AC.dull_cols(res.y, k))
    assert blob[0] == L.OK and ref["done"] == 0


@pytest.mark.parametrize("path", list(PATHS))
def test_a_free_ray_is_unbounded(path):
    m, n = 65, 449
    blob, T, ref = _phase(f"ray {path}", _prob(m, n), path, lambda res: AC.ray(m))
    assert blob[0] == L.UNBOUNDED and ref["done"] == 0


# ---- 3. independence: budgets, windows, graphs, pass forms, row bands

IND = (300, 740, 3)


@pytest.mark.parametrize("budget", [1, 7])
@pytest.mark.parametrize("path", ["k16c", "k64c"])
def test_budgets(path, budget):
    m, n, k = IND
    eb, eT = _eager(m, n, k)
    with _cold(_prob(m, n), path) as s:
        np0 = s.status()[1]
        s.add_cols(*AC.new_cols(_y(s), k))
        calls = 0
        while True:
            st, done = s.run(budget)
            calls += 1
            assert done <= budget and calls < 500
            if st != L.RUNNING:
                break
        assert st == L.OK
        SD._same_as(f"{path} budget {budget}", s, eb, eT, n + k + m)


@pytest.mark.parametrize("path,more,form", [
    ("k16c", dict(check_interval=5), None), ("k16c", dict(check_interval=5, use_graph=1), None),
    ("k64c", dict(check_interval=64, use_graph=1), None), ("k64c", dict(check_interval=64, use_graph=0), None),
    ("eager", dict(check_interval=5, use_graph=1), None),
    ("k16c", dict(rows_per_block=4), None), ("k64c", dict(rows_per_block=64), 3), ("k64c", {}, 21),
    ("k64c", {}, 23), ("k16c", {}, 4), ("k16f", {}, 3),
], ids=lambda v: str(v).replace(" ", ""))
def test_windows_graphs_forms_and_bands(path, more, form):
    m, n, k = IND
    eb, eT = _eager(m, n, k)
    with _open(_prob(m, n), path, **more) as s:
        if form is not None:
            s.set_defer_tuning(0, form)
        assert s.run(BIG)[0] == L.OK
        s.add_cols(*AC.new_cols(_y(s), k))
        if form is not None:
            assert s.defer_form() == form
        assert s.run(BIG)[0] == L.OK
        SD._same_as(f"{path} {more} form {form}", s, eb, eT, n + k + m)


# ---- 4. states

@pytest.mark.parametrize("path,budget", [("eager", 7), ("k16f", 7), ("k4c", 7), ("k16c", 21), ("k64c", 21)])
def test_stopped_inside_the_cold_solve(path, budget):
    """A session stopped by a budget inside its cold solve (not a multiple of K), widened, continued."""
    m, n, k = 65, 449, 3
    with _open(_prob(m, n), path) as s:
        assert s.run(budget) == (L.RUNNING, budget)
        P, d = AC.new_cols(AC.duals(*AC.cold(m, n)[:2], n), k)
        _, _, T2, basis2 = _add(f"mid-solve {path}", s, P, d)
        res, ref = _finish(f"mid-solve {path}", s, budget, T2, basis2)
        assert res.status == L.OK and ref["done"] >= 1
        A, b, c = AC.lp(m, n)
        stacked = O.solve_dense(np.hstack([A, P]), b, np.r_[c, d])
        assert S._close(res.objective, stacked.objective)


def _stepped(prob, path, np_cold, steps):
    """A session whose last `steps` pivots of the cold solve went through the step API: the tableau
    is optimal, the status still RUNNING, and a block of `steps` steps is open."""
    s = _open(prob, path)
    assert s.run(np_cold - steps) == (L.RUNNING, np_cold - steps)
    for _ in range(steps):
        cand = s.step_candidate()
        s.step_update(s.step_select(cand))
    return s


@pytest.mark.parametrize("path", ["k16c", "k16f", "k64c"])
def test_open_step_block_is_applied_first(path):
    m, n, k = 65, 449, 3
    prob = _prob(m, n)
    with _cold(prob, path) as s:
        np_cold = s.status()[1]
        P, d = AC.new_cols(_y(s), k)
    with _stepped(prob, path, np_cold, 3) as a:      # the read-out of this twin applies its block
        T0, basis0 = a.tableau(), a.result().basis
        assert a.status()[1] == np_cold
    T2, basis2 = CR.add_cols(T0, basis0, n, P, d)
    with _stepped(prob, path, np_cold, 3) as s:      # this one is not read before the call
        assert s.add_cols(P, d) >= 0.0
        N2 = n + k + m
        assert s.status() == (L.RUNNING, np_cold) and s.n == n + k
        T1 = s.tableau()
        assert s.result().basis.tobytes() == basis2.tobytes()
        assert SD._nonbasic_and_rhs(T1, basis2, N2) == SD._nonbasic_and_rhs(T2, basis2, N2)
        assert np.array_equal(T1, T2)
        if not s.condensed:
            assert T1.tobytes() == T2.tobytes()
        res, ref = _finish(f"open block {path}", s, np_cold, T2, basis2)
        assert res.status == L.OK and ref["done"] >= 1


def test_lookahead_session():
    m, n, k = IND
    want = None
    for la in (0, 1):
        with _cold(_prob(m, n), dict(defer=16, condensed=1, lookahead=la)) as s:
            assert s.lookahead() == bool(la)
            np0 = s.status()[1]
            _, _, T2, basis2 = _add(f"lookahead {la}", s, *AC.new_cols(_y(s), k))
            assert not s.lookahead()
            res, _ = _finish(f"lookahead {la}", s, np0, T2, basis2)
            assert res.status == L.OK
            if la:
                s.set_defer(16, 1, 1)
                assert s.lookahead() and s.condensed
            c2 = np.r_[R.make_c2(AC.lp(m, n)[2], D.DENSE_SEED[(m, n)], scale=0.02, holes=False), np.full(k, 0.5)]
            s.set_objective(c2)
            assert s.run(BIG)[0] == L.OK
            got = S._blob(s.result()), s.tableau()
            if want is None:
                want = got
            assert got[0] == want[0] and np.array_equal(got[1], want[1]), "the primal continuation differs"


@pytest.mark.parametrize("path", ["eager", "k16c"])
def test_unbounded_session_is_accepted(path):
    m, n = 65, 449
    with _cold(_prob(m, n), path) as s:
        s.add_cols(*AC.ray(m))
        assert s.run(BIG) == (L.UNBOUNDED, 0)
        np0 = s.status()[1]
        _, _, T2, basis2 = _add(f"after unbounded {path}", s, *AC.new_cols(_y(s), 2))
        res, ref = _finish(f"after unbounded {path}", s, np0, T2, basis2)
        assert res.status == L.UNBOUNDED == ref["status"]      # the ray is still there


# ---- 5. sequences, each step at the bar

@pytest.mark.parametrize("path", ["eager", "k16c", "k64c", "k16f"])
def test_life_after(path):
    """add_cols twice (k1 = 2, k2 = 3), set_objective of n + 5 costs, set_rhs (in place on the deferred
    paths), add_rows with G of n + 5 columns and its dual run, set_defer eager <-> condensed, add_cols
    after add_rows: each stage against the references on the read-out."""
    m, n = 65, 449
    A, b, c = AC.lp(m, n)
    seed = D.DENSE_SEED[(m, n)]
    with _cold(_prob(m, n), path) as s:
        P, d = AC.new_cols(_y(s), 5)
        for part, lo, hi in (("first", 0, 2), ("second", 2, 5)):
            np0 = s.status()[1]
            _, _, T2, basis2 = _add(f"{part} {path}", s, P[:, lo:hi], d[lo:hi])
            res, ref = _finish(f"{part} {path}", s, np0, T2, basis2)
            assert res.status == L.OK
        n2, N2 = n + 5, n + 5 + m
        assert (s.m, s.n) == (m, n2)
        A2 = np.hstack([A, P])
        # a new objective of n + 5 costs: a primal phase on the widened session
        c2 = np.r_[R.make_c2(c, seed, scale=0.02, holes=False), d * 0.98]
        S._raises(lambda: L.check(L.lib().dlp_session_set_objective(s._h, c2.ctypes.data_as(L._DP), n, None), "n"),
                  L.ERR_ARG)
        T0, basis0 = s.tableau(), s.result().basis
        s.set_objective(c2)
        zref = R.objective_row(T0[:m], basis0, c2)
        zrow = s.read_rows(m, 1)[0]
        bad = np.nonzero(zrow.view(np.int64) != zref.view(np.int64))[0]
        assert len(bad) == 0, f"{path}: objective row differs at columns {bad[:8]}"
        np0 = s.status()[1]
        T0 = s.tableau()
        ref = _ref(T0, basis0, n2)
        st, done = s.run(BIG)
        SD._bar(f"set_objective {path}", s, st, np0, ref, N2)
        assert st == L.OK and S._close(s.result().objective, O.solve_dense(A2, b, c2).objective)
        # new right-hand sides
        b2 = b * (1.0 + 0.2 * np.random.default_rng(seed + 2).uniform(-1.0, 1.0, m))
        np0 = s.status()[1]
        T0, basis0 = s.tableau(), s.result().basis
        ref = O.resolve_rhs(T0, basis0, n2, b2)
        s.set_rhs(b2, in_place=path != "eager")
        st, done = s.run(BIG)
        assert st == L.OK and done == ref["done"]
        SD._bar(f"set_rhs {path}", s, st, np0, ref, N2)
        # rows with n + 5 columns, and the dual run
        G, h = AR.cuts(s.result().x, n2, 2, 7811, depth=0.1)
        np0 = s.status()[1]
        T0, basis0 = s.tableau(), s.result().basis
        T3, basis3 = AR.add_rows(T0, basis0, n2, G, h)
        s.add_rows(G, h)
        assert (s.m, s.n, s.ncols) == (m + 2, n2, N2 + 2)
        ref = O.resolve_rhs(T3, basis3, n2, np.zeros(m + 2), continued=False)
        st, done = s.run(BIG)
        assert st == L.OK and done == ref["done"] >= 1
        SD._bar(f"add_rows {path}", s, st, np0, ref, N2 + 2)
        # the storage switch on the widened session
        T1, blob = s.tableau(), S._blob(s.result())
        if path == "eager":
            s.set_defer(16, 1)
            assert s.condensed and np.array_equal(s.tableau(), T1) and S._blob(s.result()) == blob
            s.set_defer(1)
            # (as values: the eager dual pivots leave signed zeros in basic columns, the expansion +0.0)
            basis1 = s.result().basis
            assert not s.condensed and np.array_equal(s.tableau(), T1)
            assert SD._nonbasic_and_rhs(s.tableau(), basis1, N2 + 2) == SD._nonbasic_and_rhs(T1, basis1, N2 + 2)
        else:
            s.set_defer(1)
            assert not s.condensed and np.array_equal(s.tableau(), T1) and S._blob(s.result()) == blob
            s.set_defer(**PATHS[path])
            assert np.array_equal(s.tableau(), T1)
        assert s.storage()[1] == (n2 if s.condensed else N2 + 2) and s.run(BIG) == (L.OK, 0)
        # columns after rows: P has m + 2 rows
        np0 = s.status()[1]
        P3, d3 = CR.columns(_y(s), 2, 7720, depth=0.1)
        _, _, T4, basis4 = _add(f"after add_rows {path}", s, P3, d3)
        res, ref = _finish(f"after add_rows {path}", s, np0, T4, basis4)
        assert res.status == L.OK and len(res.x) == n2 + 2 and len(res.y) == m + 2
        stacked = O.solve_dense(np.hstack([np.vstack([A2, G]), P3]), np.r_[b2, h], np.r_[c2, d3])
        assert stacked.status == 0 and S._close(res.objective, stacked.objective)


# ---- 6. refusals

def _unchanged(s, call, status, word=None):
    storage = s.storage()
    shape = (s.m, s.n, s.rows, s.ld, s.ncols)
    S._unchanged(s, call, status, word)
    assert s.storage() == storage and (s.m, s.n, s.rows, s.ld, s.ncols) == shape


def test_refusals_leave_the_session_unchanged():
    m, n = 63, 70
    A, b, c = AC.lp(m, n)
    prob = dlp.Problem.dense(A, b, c)
    P, d = AC.new_cols(np.ones(m), 2)
    lib = L.lib()
    gen = dlp.Problem.general(A, np.full(m, -np.inf), b, 0.0, np.inf, -c)
    with dlp.Session(gen) as s:
        s.run(BIG)
        S._unchanged(s, lambda: s.add_cols(P, d), L.ERR_UNSUPPORTED, "general", tableau=False)
    with dlp.Session(prob, rank=0, nranks=2) as s:
        S._raises(lambda: L.check(lib.dlp_session_add_cols(s._h, 2, P.ctypes.data_as(L._DP), d.ctypes.data_as(L._DP),
                                                           m, None), "ranks"), L.ERR_UNSUPPORTED)
        assert "single-GPU" in L.last_error()
    with dlp.Session(prob, small_lp=1) as s:
        assert s.small_lp() and s.run(BIG)[0] == L.OK
        _unchanged(s, lambda: s.add_cols(P, d), L.ERR_UNSUPPORTED, "small_lp = -1")
    b2 = b * (1.0 + 0.2 * np.random.default_rng(5).uniform(-1.0, 1.0, m))
    for path in ("k16c", "k16f", "eager"):
        with _cold(prob, path) as s:
            pp, dp = P.ctypes.data_as(L._DP), d.ctypes.data_as(L._DP)
            for what, args in (("k < 0", (-1, pp, dp, m)), ("NULL P", (2, None, dp, m)), ("NULL d", (2, pp, None, m)),
                               ("m - 1", (2, pp, dp, m - 1)), ("m + 1", (2, pp, dp, m + 1)),
                               # n + k and N + k beyond creation's int32 limit (checked before P is read)
                               ("k = 2^31", (2 ** 31, pp, dp, m)), ("N + k + 1 = 2^31", (2 ** 31 - 1 - n - m, pp, dp, m))):
                _unchanged(s, lambda: L.check(lib.dlp_session_add_cols(s._h, *args, None), what), L.ERR_ARG,
                           "dlp_session_add_cols")
            for bad in (np.nan, np.inf, -np.inf):
                Pb = P.copy()
                Pb[17, 1] = bad
                _unchanged(s, lambda: s.add_cols(Pb, d), L.ERR_ARG, "P[17][1]")
                db = d.copy()
                db[1] = bad
                _unchanged(s, lambda: s.add_cols(P, db), L.ERR_ARG, "d[1]")
            assert s.run(BIG) == (L.OK, 0)
            # a pending dual phase: the RHS has negative entries
            s.set_rhs(b2, in_place=path != "eager")
            la = s.lookahead()
            _unchanged(s, lambda: s.add_cols(P, d), L.ERR_STATE, "dual phase")
            assert s.lookahead() == la
            assert s.run(BIG)[0] == L.OK             # and it goes on as if nothing had been asked
            s.add_cols(P, d)                         # accepted once the dual phase has ended OK
            assert s.n == n + 2 and s.run(BIG)[0] == L.OK
    with _cold(prob, "k16c") as s:                   # a dual phase that ended INFEASIBLE
        s.add_rows(*AL.infeasible_row(n))
        assert s.run(BIG)[0] == L.INFEASIBLE
        Pi = np.vstack([P, np.ones((1, 2))])
        _unchanged(s, lambda: s.add_cols(Pi, d), L.ERR_STATE, "infeasible")
    with _cold(prob, "k16c") as s:
        cand = s.step_candidate()                # a caller-driven step in progress (optimal: a void one)
        _unchanged(s, lambda: s.add_cols(P, d), L.ERR_STATE, "step")
        s.step_update(s.step_select(cand))
        s.add_cols(P, d)                         # accepted once the step is finished
        assert s.n == n + 2 and s.run(BIG)[0] == L.OK
