"""dlp_session_add_rows on the GPU: constraint rows added to a live session on the
eager path and on every deferred path, then the dual phase on that path.

Reference: built from the session's own read-out before the call: tests/rows_ref.py's add_rows (the
row rule in numpy), then the C++ dual oracle continuing from the grown tableau
(tests/add_rows_lp.py's reference).  Bar (DESIGN.md §24's, test_gpu_session_rhs_defer's _bar /
_same_as): status, pivot count, basis, every log field, x, y and the objective bit for bit; the
nonbasic columns and the RHS byte for byte; the whole read-out byte for byte on the full layout and
equal as values on the condensed one.  Nothing may depend on K, the pass form, the row band,
check_interval, use_graph or the budgets.

Inputs: tests/add_rows_lp.py; tests/test_session_add_rows_api.py holds their properties on the CPU
oracle (pivot counts, statuses, the contributing-row counts).  Every session has small_lp=-1."""
import functools

import numpy as np
import pytest

import add_rows_lp as AL
import dual_lp as D
import oracle_py as O
import reopt_ref as R
import rhs_ref as RR
import rows_ref as AR

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

import test_gpu_session_rhs as S
import test_gpu_session_rhs_defer as SD

pytestmark = pytest.mark.gpu

BIG = AL.BIG
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
    return dlp.Problem.dense(*AL.lp(m, n))


def _round16(v):
    return (v + 15) // 16 * 16


def _add(name, s, n, G, h):
    """add_rows on a session, the read-out right after it against rows_ref.add_rows on the read-out
    right before it, at the bar.  Returns (T0, basis0, T2, basis2)."""
    G = np.asarray(G, dtype=np.float64).reshape(-1, n)
    r = G.shape[0]
    np0 = s.status()[1]
    T0, basis0 = s.tableau(), s.result().basis
    m = len(basis0)
    assert (s.m, s.n, s.rows) == (m, n, m), name
    cond = s.condensed
    T2, basis2 = AR.add_rows(T0, basis0, n, G, h)
    assert s.add_rows(G, h) >= 0.0, name
    N2 = n + m + r
    assert s.status() == (L.RUNNING, np0), name
    assert (s.m, s.n, s.rows, s.ncols, s.ld) == (m + r, n, m + r, N2, AR.tableau_ld(m + r, n)), name
    assert s.storage() == ((_round16(n + 1), n, True) if cond else (AR.tableau_ld(m + r, n), N2, False)), name
    res = s.result()
    assert res.basis.tobytes() == basis2.tobytes(), name
    assert len(res.y) == m + r and len(res.x) == n, name
    T1 = s.tableau()
    assert T1.shape == T2.shape, name
    new = T1[m:m + r].view(np.int64) != T2[m:m + r].view(np.int64)
    assert not new.any(), f"{name}: new rows differ from the rule at (row, column) {np.argwhere(new)[:8]}"
    assert SD._nonbasic_and_rhs(T1, basis2, N2) == SD._nonbasic_and_rhs(T2, basis2, N2), name
    assert np.array_equal(T1, T2), name
    if not cond:
        assert T1.tobytes() == T2.tobytes(), f"{name}: the full layout's read-out differs in some byte"
    assert s.read_rows(m, r + 1).tobytes() == T1[m:].tobytes(), name
    # x, y and the objective are read from the grown tableau as it stands
    x = np.zeros(n)
    rows = np.nonzero(basis2 < n)[0]
    x[basis2[rows]] = T2[rows, N2]
    assert res.x.tobytes() == x.tobytes() and np.array_equal(res.y, T2[m + r, n:N2]), name
    assert np.float64(res.objective).tobytes() == T2[m + r, N2].tobytes(), name
    return T0, basis0, T2, basis2


def _ref(T2, basis2, n, pricing=0, max_pivots=BIG):
    return O.resolve_rhs(T2, basis2, n, np.zeros(len(basis2)), continued=False, pricing=pricing,
                         max_pivots=max_pivots)


def _cold(prob, path, **more):
    s = _open(prob, path, **more)
    assert s.run(BIG)[0] == L.OK
    return s


def _phase(name, prob, path, n, rows, pricing=0, **more):
    """Cold solve on `path`, add_rows(rows(x*)), the dual phase to its end, against the oracle on the
    session's own read-out.  Returns (blob, final tableau, reference)."""
    with _cold(prob, path, pricing=pricing, **more) as s:
        np0 = s.status()[1]
        G, h = rows(s.result())
        _, _, T2, basis2 = _add(name, s, n, G, h)
        ref = _ref(T2, basis2, n, pricing=pricing)
        assert not s.lookahead(), name
        assert s.get_defer_tuning()[2] == (PATHS[path] if isinstance(path, str) else path)["defer"], name
        st, done = s.run(BIG)
        assert done == ref["done"], (name, done, ref["done"])
        res = SD._bar(name, s, st, np0, ref, len(basis2) + n)
        assert s.run(BIG) == (st, 0), name
        return S._blob(res), s.tableau(), ref


# ---- 1. the rows alone

@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("m,n,r", AL.CASES)
def test_rows_alone(m, n, r, path):
    with _cold(_prob(m, n), path) as s:
        x = s.result().x
        _add(f"{m}x{n} r {r} {path}", s, n, *AL.cut_rows(x, n, r))


@pytest.mark.parametrize("path", ["eager", "k16f", "k16c"])
def test_contributing_row_counts(path):
    """Rows with exactly R = 0, 1, B - 1, B, B + 1, 2 B + 1 contributing old rows (B: the fold's
    batch), one session per count."""
    m, n = AL.COUNT_SHAPE
    prob = _prob(m, n)
    for R_ in AL.COUNTS:
        with _cold(prob, path) as s:
            res = s.result()
            G, h = AL.counted(res.basis, res.x, n, R_)
            _add(f"R {R_} {path}", s, n, G, h)
            st, done = s.run(BIG)
            assert st == L.OK and (done >= 1) == (R_ > 0), (R_, st, done)


@pytest.mark.parametrize("path", ["eager", "k16f", "k64c"])
@pytest.mark.parametrize("r", [AL.RT - 1, AL.RT, AL.RT + 1])
def test_row_groups(r, path):
    """One group short of a row, full, and a second group of one row; rows whose coefficients are
    zero (+0.0 and -0.0) where another row of the group has nonzeros."""
    m, n = AL.COUNT_SHAPE
    with _cold(_prob(m, n), path) as s:
        res = s.result()
        _add(f"group r {r} {path}", s, n, *AL.grouped(res.basis, res.x, n, r))
        assert s.run(BIG)[0] == L.OK


def test_no_rows_touches_nothing():
    m, n = 63, 70
    with _cold(_prob(m, n), "k16c") as s:
        before, T0 = S._blob(s.result()), s.tableau().tobytes()
        assert L.lib().dlp_session_add_rows(s._h, 0, None, None, n, None) == L.OK
        assert s.add_rows(np.zeros((0, n)), np.zeros(0)) == 0.0
        assert s.status()[0] == L.OK and S._blob(s.result()) == before and s.tableau().tobytes() == T0
        assert s.m == m and s.run(BIG) == (L.OK, 0)


# ---- 2. the dual phase: the eager route against the oracle, every deferred path against it

@functools.lru_cache(maxsize=None)
def _eager(m, n, r, pricing=0):
    blob, T, ref = _phase(f"eager {m}x{n} r {r} pricing {pricing}", _prob(m, n), "eager", n,
                          lambda res: AL.cut_rows(res.x, n, r), pricing=pricing)
    assert blob[0] == L.OK and ref["done"] >= 1
    return blob, T


@pytest.mark.parametrize("m,n,r", AL.CASES)
def test_dual_phase_eager_every_case(m, n, r):
    _eager(m, n, r)


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("path", DEFERRED)
@pytest.mark.parametrize("m,n,r", [(65, 449, 5), (300, 740, 3)])
def test_dual_phase_every_path(m, n, r, path, pricing):
    name = f"{m}x{n} r {r} {path} pricing {pricing}"
    blob, T, ref = _phase(name, _prob(m, n), path, n, lambda res: AL.cut_rows(res.x, n, r), pricing=pricing)
    eb, eT = _eager(m, n, r, pricing)
    assert blob == eb and np.array_equal(T, eT), name
    if not PATHS[path]["condensed"] == 1:
        assert T.tobytes() == eT.tobytes(), "the full layout's read-out differs from the eager session's"


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("path", ["eager", "k16f", "k16c", "k64c"])
@pytest.mark.parametrize("m,n,seed", AL.DEGENERATE)
def test_dual_phase_degenerate_family(m, n, seed, path, pricing):
    A, b, c = O.gen_dense(m, n, seed, degenerate=True)
    blob, T, ref = _phase(f"degenerate {m}x{n} {path} pricing {pricing}", dlp.Problem.dense(A, b, c), path, n,
                          lambda res: AL.cut_rows(res.x, n, 3), pricing=pricing)
    assert blob[0] == L.OK and ref["done"] >= 1


@pytest.mark.parametrize("path", list(PATHS))
def test_slack_cut_does_no_pivot(path):
    m, n, r = 65, 449, 5
    blob, T, ref = _phase(f"slack {path}", _prob(m, n), path, n, lambda res: AL.slack_rows(res.x, n, r))
    assert blob[0] == L.OK and ref["done"] == 0


@pytest.mark.parametrize("path", ["eager", "k16c"])
def test_infeasible_cut_and_a_second_call_after_it(path):
    m, n = AL.INFEASIBLE_SHAPE
    with _cold(_prob(m, n), path) as s:
        np0 = s.status()[1]
        x = s.result().x
        _, _, T2, basis2 = _add(f"infeasible {path}", s, n, *AL.infeasible_row(n))
        ref = _ref(T2, basis2, n)
        assert ref["status"] == RR.INFEASIBLE and ref["done"] >= 1
        st, done = s.run(BIG)
        assert (st, done) == (L.INFEASIBLE, ref["done"])
        SD._bar(f"infeasible {path}", s, st, np0, ref, n + m + 1)
        assert s.run(BIG) == (L.INFEASIBLE, 0)
        np1 = s.status()[1]
        _, _, T3, basis3 = _add(f"after infeasible {path}", s, n, *AL.cut_rows(x, n, 2))
        ref = _ref(T3, basis3, n)
        st, done = s.run(BIG)
        assert (st, done) == (L.INFEASIBLE, ref["done"])
        SD._bar(f"still infeasible {path}", s, st, np1, ref, n + m + 3)


# ---- 3. independence: budgets, windows, graphs, pass forms, row bands

IND = (300, 740, 3)


@pytest.mark.parametrize("budget", [1, 7])
@pytest.mark.parametrize("path", ["k16c", "k64c"])
def test_budgets(path, budget):
    m, n, r = IND
    eb, eT = _eager(m, n, r)
    with _cold(_prob(m, n), path) as s:
        np0 = s.status()[1]
        s.add_rows(*AL.cut_rows(s.result().x, n, r))
        calls = 0
        while True:
            st, done = s.run(budget)
            calls += 1
            assert done <= budget and calls < 500
            if st != L.RUNNING:
                break
        assert st == L.OK
        if budget == 1:
            assert calls == s.status()[1] - np0          # OK comes with the last pivot
        SD._same_as(f"{path} budget {budget}", s, eb, eT, n + m + r)


@pytest.mark.parametrize("path,more,form", [
    ("k16c", dict(check_interval=5), None), ("k16c", dict(check_interval=5, use_graph=1), None),
    ("k64c", dict(check_interval=64, use_graph=1), None), ("k64c", dict(check_interval=64, use_graph=0), None),
    ("eager", dict(check_interval=5, use_graph=1), None),
    ("k16c", dict(rows_per_block=4), None), ("k64c", dict(rows_per_block=64), 3), ("k64c", {}, 21),
    ("k64c", {}, 23), ("k16c", {}, 4), ("k16f", {}, 3),
], ids=lambda v: str(v).replace(" ", ""))
def test_windows_graphs_forms_and_bands(path, more, form):
    m, n, r = IND
    eb, eT = _eager(m, n, r)
    with _open(_prob(m, n), path, **more) as s:
        if form is not None:
            s.set_defer_tuning(0, form)
        assert s.run(BIG)[0] == L.OK
        s.add_rows(*AL.cut_rows(s.result().x, n, r))
        if form is not None:
            assert s.defer_form() == form
        assert s.run(BIG)[0] == L.OK
        SD._same_as(f"{path} {more} form {form}", s, eb, eT, n + m + r)


# ---- 4. life after

@pytest.mark.parametrize("path", ["eager", "k16c", "k64c"])
def test_life_after(path):
    """add_rows twice (1, then 2 rows), set_rhs of m + 3 entries in place, set_objective and a primal
    run: each stage against the oracle chain on the read-out."""
    m, n = 65, 449
    A, b, c = AL.lp(m, n)
    seed = D.DENSE_SEED[(m, n)]
    with _cold(_prob(m, n), path) as s:
        x = s.result().x
        G, h = AL.cut_rows(x, n, 3)
        for part, lo, hi in (("first", 0, 1), ("second", 1, 3)):
            np0 = s.status()[1]
            _, _, T2, basis2 = _add(f"{part} {path}", s, n, G[lo:hi], h[lo:hi])
            ref = _ref(T2, basis2, n)
            st, done = s.run(BIG)
            assert st == L.OK and done == ref["done"]
            SD._bar(f"{part} {path}", s, st, np0, ref, n + m + hi)
        m2 = m + 3
        N2 = n + m2
        assert s.m == m2
        # new right-hand sides for all m + 3 rows
        b3 = np.r_[b, h] * (1.0 + 0.2 * np.random.default_rng(seed + 2).uniform(-1.0, 1.0, m2))
        S._raises(lambda: L.check(L.lib().dlp_session_set_rhs_in_place(s._h, b3.ctypes.data_as(L._DP), m, None), "m"),
                  L.ERR_ARG)
        np0 = s.status()[1]
        T0, basis0 = s.tableau(), s.result().basis
        ref = O.resolve_rhs(T0, basis0, n, b3)
        s.set_rhs(b3, in_place=True)
        st, done = s.run(BIG)
        assert st == L.OK and done == ref["done"]
        SD._bar(f"set_rhs {path}", s, st, np0, ref, N2)
        # a new objective: a primal phase on the grown session
        c2 = R.make_c2(c, seed, scale=0.02, holes=False)
        T0, basis0 = s.tableau(), s.result().basis
        s.set_objective(c2)
        zref = R.objective_row(T0[:m2], basis0, c2)
        zrow = s.read_rows(m2, 1)[0]
        bad = np.nonzero(zrow.view(np.int64) != zref.view(np.int64))[0]
        assert len(bad) == 0, f"{path}: objective row differs at columns {bad[:8]}"
        st, done = s.run(BIG)
        assert st == L.OK and done >= 1
        res = s.result()
        stacked = O.solve_dense(np.vstack([A, G]), b3, c2)
        assert stacked.status == RR.OK and S._close(res.objective, stacked.objective)
        assert (np.vstack([A, G]) @ res.x <= b3 + 1e-7).all()


def test_life_after_is_the_same_on_every_path():
    """The whole chain of test_life_after, blob and tableau of each deferred path against the eager
    session's after every stage; then set_defer eager <-> condensed on the grown session."""
    m, n = 65, 449
    A, b, c = AL.lp(m, n)
    seed = D.DENSE_SEED[(m, n)]
    c2 = R.make_c2(c, seed, scale=0.02, holes=False)
    want = None
    for path in ("eager", "k16c", "k64c", "k16f"):
        got = []
        with _cold(_prob(m, n), path) as s:
            x = s.result().x
            G, h = AL.cut_rows(x, n, 3)
            b3 = np.r_[b, h] * (1.0 + 0.2 * np.random.default_rng(seed + 2).uniform(-1.0, 1.0, m + 3))
            for change in (lambda: s.add_rows(G[:1], h[:1]), lambda: s.add_rows(G[1:], h[1:]),
                           lambda: s.set_rhs(b3, in_place=True), lambda: s.set_objective(c2)):
                change()
                assert s.run(BIG)[0] == L.OK
                got.append((S._blob(s.result()), s.tableau()))
            if want is None:
                want = got
            for k, ((gb, gT), (wb, wT)) in enumerate(zip(got, want)):
                assert gb == wb and np.array_equal(gT, wT), f"{path}: stage {k} differs from the eager session"
            T1 = s.tableau()
            blob = S._blob(s.result())
            if path == "eager":
                s.set_defer(16, 1)
                assert s.condensed and np.array_equal(s.tableau(), T1) and S._blob(s.result()) == blob
                s.set_defer(1)
                assert not s.condensed and s.tableau().tobytes() == T1.tobytes()
            else:
                s.set_defer(1)
                assert not s.condensed and np.array_equal(s.tableau(), T1) and S._blob(s.result()) == blob
                s.set_defer(**PATHS[path])
                assert np.array_equal(s.tableau(), T1)
            assert s.storage()[1] == (n if s.condensed else n + m + 3)
            assert s.run(BIG) == (L.OK, 0)
            s.set_objective(c)                       # and a primal run on the path it came back to
            assert s.run(BIG)[0] == L.OK
            got.append((S._blob(s.result()), s.tableau()))
            assert got[-1][0] == want[-1][0] and np.array_equal(got[-1][1], want[-1][1]), path


def test_lookahead_session():
    m, n, r = IND
    c2 = R.make_c2(AL.lp(m, n)[2], D.DENSE_SEED[(m, n)], scale=0.02, holes=False)
    want = None
    for la in (0, 1):
        with _cold(_prob(m, n), dict(defer=16, condensed=1, lookahead=la)) as s:
            assert s.lookahead() == bool(la)
            np0 = s.status()[1]
            _, _, T2, basis2 = _add(f"lookahead {la}", s, n, *AL.cut_rows(s.result().x, n, r))
            assert not s.lookahead()
            st, done = s.run(BIG)
            SD._bar(f"lookahead {la}", s, st, np0, _ref(T2, basis2, n), n + m + r)
            assert st == L.OK
            if la:
                s.set_defer(16, 1, 1)
                assert s.lookahead() and s.condensed
            s.set_objective(c2)
            assert s.run(BIG)[0] == L.OK
            got = S._blob(s.result()), s.tableau()
            if want is None:
                want = got
            assert got[0] == want[0] and np.array_equal(got[1], want[1]), "the primal continuation differs"


# ---- 5. mid-phase

@pytest.mark.parametrize("path", ["eager", "k16c", "k64c"])
def test_add_rows_inside_a_pending_dual_phase(path):
    m, n, r = IND
    with _cold(_prob(m, n), path) as s:
        x = s.result().x
        s.add_rows(*AL.cut_rows(x, n, r))
        assert s.run(10) == (L.RUNNING, 10)              # stopped by the budget, mid-block at K = 16 / 64
        np0 = s.status()[1]
        G, h = AL.cut_rows(x, n, 2)
        _, _, T2, basis2 = _add(f"mid-phase {path}", s, n, G, h)
        ref = _ref(T2, basis2, n)
        st, done = s.run(BIG)
        assert st == L.OK and done == ref["done"] >= 1
        SD._bar(f"mid-phase {path}", s, st, np0, ref, n + m + r + 2)


# ---- 5b. a block the step API left open; more rows than one fold launch holds

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
    m, n, r = 65, 449, 3
    prob = _prob(m, n)
    with _cold(prob, path) as s:
        np_cold = s.status()[1]
        G, h = AL.cut_rows(s.result().x, n, r)
    with _stepped(prob, path, np_cold, 3) as a:      # the read-out of this one applies its block
        T0, basis0 = a.tableau(), a.result().basis
        assert a.status()[1] == np_cold
    T2, basis2 = AR.add_rows(T0, basis0, n, G, h)
    with _stepped(prob, path, np_cold, 3) as s:      # this one is not read before the call
        assert s.add_rows(G, h) >= 0.0
        N2 = n + m + r
        assert s.status() == (L.RUNNING, np_cold) and s.m == m + r
        T1 = s.tableau()
        assert s.result().basis.tobytes() == basis2.tobytes()
        assert SD._nonbasic_and_rhs(T1, basis2, N2) == SD._nonbasic_and_rhs(T2, basis2, N2)
        assert np.array_equal(T1, T2)
        if not s.condensed:
            assert T1.tobytes() == T2.tobytes()
        ref = _ref(T2, basis2, n)
        st, done = s.run(BIG)
        assert st == L.OK and done == ref["done"] >= 1
        SD._bar(f"open block {path}", s, st, np_cold, ref, N2)


def test_more_rows_than_one_fold_launch():
    """r = 4 x 65,535 + 1: the fold's row groups fill one launch's grid and one group of a second.
    The full layout of such an LP is too wide to read out whole; rows on both sides of the launch
    boundary are read one by one and held against the rule for that row alone."""
    m, n = 5, 7
    r = 4 * 65535 + 1
    with _cold(_prob(m, n), "k4c") as s:
        res0 = s.result()
        T0, basis0 = s.tableau(), res0.basis
        rng = np.random.default_rng(7990)
        G = rng.uniform(0.0, 1.0, (r, n)) * (rng.uniform(size=(r, n)) >= 0.3)
        h = 2.0 * (G @ res0.x) + 1.0                 # slack rows: no pivot
        assert s.add_rows(G, h) >= 0.0
        N, N2 = n + m, n + m + r
        assert (s.m, s.rows, s.ncols) == (m + r, m + r, N2) and s.storage() == (16, n, True)
        assert s.status() == (L.RUNNING, res0.num_pivots)
        for t in (0, 1, 4 * 65535 - 1, 4 * 65535):
            T2, _ = AR.add_rows(T0, basis0, n, G[t:t + 1], h[t:t + 1])
            row = s.read_rows(m + t, 1)[0]
            assert row[:N].tobytes() == T2[m, :N].tobytes(), t
            assert row[N2].tobytes() == T2[m, N + 1].tobytes(), t
            assert row[N + t] == 1.0 and np.count_nonzero(row[N:N2]) == 1, t
        assert s.run(BIG) == (L.OK, 0)
        res = s.result()
        assert np.float64(res.objective).tobytes() == np.float64(res0.objective).tobytes()
        assert res.x.tobytes() == res0.x.tobytes() and len(res.y) == m + r
        assert res.basis[m:].tobytes() == np.arange(N, N2, dtype=np.int32).tobytes()


# ---- 6. refusals

def _unchanged(s, call, status, word=None):
    storage = s.storage()
    shape = (s.m, s.rows, s.ld, s.ncols)
    S._unchanged(s, call, status, word)
    assert s.storage() == storage and (s.m, s.rows, s.ld, s.ncols) == shape


def test_refusals_leave_the_session_unchanged():
    m, n = 63, 70
    A, b, c = AL.lp(m, n)
    prob = dlp.Problem.dense(A, b, c)
    G, h = AL.cut_rows(np.ones(n), n, 2)
    lib = L.lib()
    gen = dlp.Problem.general(A, np.full(m, -np.inf), b, 0.0, np.inf, -c)
    with dlp.Session(gen) as s:
        s.run(BIG)
        S._unchanged(s, lambda: s.add_rows(G, h), L.ERR_UNSUPPORTED, "general", tableau=False)
    with dlp.Session(prob, rank=0, nranks=2) as s:
        S._unchanged(s, lambda: s.add_rows(G, h), L.ERR_UNSUPPORTED, "single-GPU", tableau=False)
    with dlp.Session(prob, small_lp=1) as s:
        assert s.small_lp() and s.run(BIG)[0] == L.OK
        _unchanged(s, lambda: s.add_rows(G, h), L.ERR_UNSUPPORTED, "small_lp = -1")
    for path in ("k16c", "k16f", dict(defer=16, condensed=1, lookahead=1), "eager"):
        with _open(prob, path) as s:                 # stopped inside the primal solve
            assert s.run(7) == (L.RUNNING, 7)
            la = s.lookahead()
            _unchanged(s, lambda: s.add_rows(G, h), L.ERR_STATE, "dual feasible")
            assert s.lookahead() == la
            assert s.run(BIG)[0] == L.OK             # and it goes on as if nothing had been asked
            gp, hp = G.ctypes.data_as(L._DP), h.ctypes.data_as(L._DP)
            for what, args in (("r < 0", (-1, gp, hp, n)), ("NULL G", (2, None, hp, n)), ("NULL h", (2, gp, None, n)),
                               ("n - 1", (2, gp, hp, n - 1)), ("n + 1", (2, gp, hp, n + 1)),
                               # m + r and N + r beyond creation's int32 limit (checked before G is read)
                               ("r = 2^31", (2 ** 31, gp, hp, n)), ("N + r + 1 = 2^31", (2 ** 31 - 1 - n - m, gp, hp, n))):
                _unchanged(s, lambda: L.check(lib.dlp_session_add_rows(s._h, *args, None), what), L.ERR_ARG,
                           "dlp_session_add_rows")
            for bad in (np.nan, np.inf, -np.inf):
                Gb = G.copy()
                Gb[1, 17] = bad
                _unchanged(s, lambda: s.add_rows(Gb, h), L.ERR_ARG, "G[1][17]")
                hb = h.copy()
                hb[1] = bad
                _unchanged(s, lambda: s.add_rows(G, hb), L.ERR_ARG, "h[1]")
            assert s.run(BIG) == (L.OK, 0)
    with _open(prob, "k16c") as s:
        assert s.run(BIG)[0] == L.OK
        cand = s.step_candidate()                # a caller-driven step in progress (optimal: a void one)
        _unchanged(s, lambda: s.add_rows(G, h), L.ERR_STATE, "step")
        s.step_update(s.step_select(cand))
        s.add_rows(G, h)                         # accepted once the step is finished
        assert s.m == m + 2 and s.run(BIG)[0] in (L.OK, L.INFEASIBLE)
