"""dlp_session_set_rhs on the GPU: the rebuilt RHS column and every dual pivot against the numpy
reference of the rule (tests/rhs_ref.py) on the session's own tableau, bit for bit in status,
pivot count, basis and log, equal as values in x, y and the tableau (a negative pivot leaves -0
where the reference keeps +0 in basic columns of the pivot row); the eager path, its graph
windows and the one-launch small-LP path against each other; the session state around the dual
phase (budgets, pivot limit, infeasible, back to a primal phase, refusals).

The inputs are checked on the CPU by tests/test_session_rhs_api.py: at rng seed = LP seed every
dense shape pivots at least once and ends optimal (no seed had to be skipped); the cone LPs
contain no zero ratio as generated, so the variant with c[::2] = 0 is part of the set."""
import functools

import numpy as np
import pytest

import oracle_py as O
import reopt_ref as R
import rhs_ref as RR

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 1), (40, 50, 2), (96, 160, 5)]
# (m, n, seed, variant): variant 1 zeroes every other cost, which makes z_s == 0 and the ratio 0
CONES = [(m, n, seed, v) for (m, n) in ((5, 7), (37, 53)) for seed in range(4) for v in (0, 1)]

PATHS = [
    ("eager", dict(defer=1, small_lp=-1)),
    ("eager_graph5", dict(defer=1, small_lp=-1, use_graph=1, check_interval=5)),
    ("small_lp", dict(small_lp=1)),
]
BIG = 10 ** 6


@functools.lru_cache(maxsize=None)
def dense_lp(m, n, seed):
    A, b, c = O.gen_dense(m, n, seed)
    b2 = b * (1.0 + 0.3 * np.random.default_rng(seed).uniform(-1.0, 1.0, m))
    return A, b, c, b2


@functools.lru_cache(maxsize=None)
def cone_lp(m, n, seed, variant):
    """tests/test_batch_rhs_api.py's mixed-sign LPs: A in [-1, 1), c <= 0, two entries of b pushed
    negative."""
    rng = np.random.default_rng(6300 + 10 * m + seed)
    A = rng.uniform(-1.0, 1.0, (m, n))
    b = A @ rng.uniform(0.0, 1.0, n) + rng.uniform(0.0, 1.0, m)
    b[rng.choice(m, 2, replace=False)] -= (0.5, 4.0)[seed % 2] * (1 + seed)
    c = -rng.uniform(0.0, 1.0, n)
    if variant:
        c[::2] = 0.0
    return A, b, c


_REFS = {}


def _ref(T0, basis0, n, b2, **kw):
    """The reference on a session's tableau, computed once per distinct input (the paths hand in
    the same bytes)."""
    key = (T0.tobytes(), basis0.tobytes(), n, np.asarray(b2).tobytes(), tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = RR.resolve_rhs(T0, basis0, n, b2, **kw)
    return _REFS[key]


def _open(prob, name, opts, **more):
    s = dlp.Session(prob, **opts, **more)
    if name == "small_lp":
        assert s.small_lp()
    return s


def _blob(r):
    return (r.status, r.num_pivots, np.float64(r.objective).tobytes(), r.x.tobytes(), r.y.tobytes(),
            r.basis.tobytes(), np.ascontiguousarray(r.pivot_log).tobytes())


def _close(obj, ref):
    return abs(obj - ref) <= 1e-9 * (1.0 + abs(ref))


def _raises(call, status):
    with pytest.raises(L.DLPError) as ei:
        call()
    assert ei.value.status == status, ei.value


def _bar(name, s, st, np0, ref):
    """The bar of every dual phase: status, pivot count, basis and the new log entries bit for
    bit; x, y and the tableau equal as values."""
    res = s.result()
    want = RR.PIVOT_LIMIT if ref["status"] == RR.PIVOT_LIMIT else ref["status"]
    assert res.status == want, (name, res.status, ref["status"])
    if st is not None:
        assert st == (L.RUNNING if want == RR.PIVOT_LIMIT else want), (name, st)
    assert res.num_pivots - np0 == ref["done"], (name, res.num_pivots - np0, ref["done"])
    assert res.basis.tobytes() == ref["basis"].tobytes(), name
    new = np.ascontiguousarray(res.pivot_log[np0:])
    assert len(new) == len(ref["log"]), name
    for f in ("q", "p", "leaving", "ratio", "objective"):
        got, exp = np.ascontiguousarray(new[f]), np.ascontiguousarray(ref["log"][f])
        bad = np.nonzero(got.view(np.int32 if got.dtype.itemsize == 4 else np.int64) !=
                         exp.view(np.int32 if exp.dtype.itemsize == 4 else np.int64))[0]
        assert len(bad) == 0, f"{name}: log field {f} differs at dual pivots {bad[:8]}: " \
                              f"{got[bad[:8]]} vs {exp[bad[:8]]}"
    assert np.float64(res.objective).tobytes() == np.float64(ref["objective"]).tobytes(), name
    assert np.array_equal(res.x, ref["x"]) and np.array_equal(res.y, ref["y"]), name
    assert np.array_equal(s.tableau(), ref["T"]), name
    return res


@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_rebuild_alone(m, n, seed):
    """Case 1: set_rhs writes exactly the reference's RHS column and nothing else; with the
    creation b the session is optimal again without a pivot."""
    A, b, c, b2 = dense_lp(m, n, seed)
    prob = dlp.Problem.dense(A, b, c)
    N = n + m
    for name, opts in PATHS:
        with _open(prob, name, opts) as s:
            assert s.run(BIG)[0] == L.OK
            cold = s.result()
            T0 = s.tableau()
            ms = s.set_rhs(b2)
            assert ms >= 0.0
            assert s.status() == (L.RUNNING, cold.num_pivots), name
            T1 = s.tableau()
            want = RR.fold_rhs(T0, n, b2)
            bad = np.nonzero(T1[:, N].view(np.int64) != want.view(np.int64))[0]
            assert len(bad) == 0, f"{name}: RHS differs at rows {bad[:8]}: {T1[bad[:8], N]} vs {want[bad[:8]]}"
            T1[:, N] = T0[:, N]
            assert T1.tobytes() == T0.tobytes(), f"{name}: an entry outside the RHS column changed"
            assert s.result().basis.tobytes() == cold.basis.tobytes(), name
            s.set_rhs(b)
            assert s.run(BIG) == (L.OK, 0), name
            assert _close(s.result().objective, cold.objective), name


@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_dual_phase_to_the_end(m, n, seed):
    """Case 2."""
    A, b, c, b2 = dense_lp(m, n, seed)
    prob = dlp.Problem.dense(A, b, c)
    cold2 = O.solve_dense(A, b2, c)
    base = None
    for name, opts in PATHS:
        with _open(prob, name, opts) as s:
            assert s.run(BIG)[0] == L.OK
            np0 = s.status()[1]
            T0, basis0 = s.tableau(), s.result().basis
            ref = _ref(T0, basis0, n, b2)
            s.set_rhs(b2)
            st, done = s.run(BIG)
            assert done == ref["done"], name
            res = _bar(name, s, st, np0, ref)
            print(f"{m}x{n} {name}: {np0} cold + {done} dual pivots, objective {res.objective!r} "
                  f"(oracle cold on b2: {cold2.objective!r}, {cold2.num_pivots} pivots)")
            assert st == L.OK and (done >= 1 or m == 5), name
            assert _close(res.objective, cold2.objective), name
            assert s.run(BIG) == (L.OK, 0), name
        if base is None:
            base = res
        else:
            assert _blob(res) == _blob(base), f"{name} differs from the eager path"


def test_budgets():
    """Case 3: budgets of any size give the pivots of one unbounded call, and max_pivots counts
    across the cold solve and the dual phase."""
    m, n, seed = 40, 50, 2
    A, b, c, b2 = dense_lp(m, n, seed)
    prob = dlp.Problem.dense(A, b, c)
    base = None
    for name, opts in PATHS:
        for budget in (1, 7, BIG):
            with _open(prob, name, opts) as s:
                assert s.run(BIG)[0] == L.OK
                np0 = s.status()[1]
                s.set_rhs(b2)
                calls = 0
                while True:
                    st, done = s.run(budget)
                    calls += 1
                    assert done <= budget and calls < 200
                    if st != L.RUNNING:
                        break
                res = s.result()
            assert st == L.OK and res.num_pivots > np0, (name, budget)
            if budget == 1:
                assert calls == res.num_pivots - np0, (name, calls)   # OK comes with the last pivot
            if base is None:
                base = res
            else:
                assert _blob(res) == _blob(base), f"{name}, budget {budget}: differs from run(1) on the eager path"
    assert base.num_pivots - np0 > 5     # (np0: the cold solve's pivots, the same on every path)
    for name, opts in PATHS:
        with _open(prob, name, opts, max_pivots=np0 + 5) as s:
            assert s.run(BIG)[0] == L.OK
            T0, basis0 = s.tableau(), s.result().basis
            s.set_rhs(b2)
            st, done = s.run(BIG)
            assert (st, done) == (L.PIVOT_LIMIT, 5), (name, st, done)
            _bar(name, s, None, np0, _ref(T0, basis0, n, b2, max_pivots=5))
            assert s.run(10) == (L.PIVOT_LIMIT, 0), name


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("m,n", [(5, 7), (37, 53)])
def test_cold_dual_from_the_slack_basis(m, n, pricing):
    """Case 4: cone LPs with c <= 0 are optimal at the slack basis for |b|; set_rhs(b) with its
    negative entries then runs the whole dual simplex from there, Bland mode included."""
    seen_ok = seen_zero = False
    for (mm, nn, seed, variant) in CONES:
        if (mm, nn) != (m, n):
            continue
        A, b, c = cone_lp(m, n, seed, variant)
        prob = dlp.Problem.dense(A, np.abs(b), c)
        base = None
        for name, opts in PATHS:
            with _open(prob, name, opts, pricing=pricing) as s:
                assert s.run(BIG) == (L.OK, 0), name
                T0, basis0 = s.tableau(), s.result().basis
                ref = _ref(T0, basis0, n, b, pricing=pricing)
                s.set_rhs(b)
                st, done = s.run(BIG)
                res = _bar(f"{name} seed {seed} variant {variant}", s, st, 0, ref)
                assert st in (L.OK, L.INFEASIBLE) and done > 0
            if base is None:
                base = res
            else:
                assert _blob(res) == _blob(base), name
        seen_ok |= st == L.OK
        seen_zero |= pricing == 0 and bool((res.pivot_log["ratio"][:-1] == 0.0).any())
    assert seen_ok
    assert seen_zero or pricing == 1


def test_infeasible_and_back():
    """Case 5."""
    A, b, c = O.gen_dense(37, 53, 6500)
    b2 = b.copy()
    b2[3] = -1.0
    prob = dlp.Problem.dense(A, b, c)
    for name, opts in PATHS:
        with _open(prob, name, opts) as s:
            assert s.run(BIG)[0] == L.OK
            cold = s.result()
            T0 = s.tableau()
            ref = _ref(T0, cold.basis, 53, b2)
            assert ref["status"] == RR.INFEASIBLE
            s.set_rhs(b2)
            st, _ = s.run(BIG)
            assert st == L.INFEASIBLE, name
            _bar(name, s, st, cold.num_pivots, ref)
            assert s.run(BIG) == (L.INFEASIBLE, 0), name
            before, Tb = _blob(s.result()), s.tableau().tobytes()
            _raises(lambda: s.set_objective(c), L.ERR_STATE)
            _raises(lambda: s.step_candidate(), L.ERR_STATE)
            assert _blob(s.result()) == before and s.tableau().tobytes() == Tb, name
            s.set_rhs(b)
            st, _ = s.run(BIG)
            assert st == L.OK and _close(s.result().objective, cold.objective), name


def test_after_ok_the_session_is_ordinary():
    """Case 6."""
    m, n, seed = 40, 50, 2
    A, b, c, b2 = dense_lp(m, n, seed)
    c2 = R.make_c2(c, seed, scale=0.02, holes=False)
    ref2 = O.solve_dense(A, b2, c2)
    b3 = b * (1.0 + 0.3 * np.random.default_rng(seed + 1).uniform(-1.0, 1.0, m))
    ref3 = O.solve_dense(A, b3, c2)
    assert ref2.status == ref3.status == L.OK
    prob = dlp.Problem.dense(A, b, c)
    for name, opts in (PATHS[0], PATHS[2]):
        with _open(prob, name, opts) as s:
            assert s.run(BIG)[0] == L.OK
            s.set_rhs(b2)
            assert s.run(BIG)[0] == L.OK
            s.set_objective(c2)
            assert s.status()[0] == L.RUNNING
            st, _ = s.run(BIG)
            assert st == L.OK and _close(s.result().objective, ref2.objective), name
            np0 = s.status()[1]
            T0, basis0 = s.tableau(), s.result().basis
            s.set_rhs(b3)                       # a second change of b, on the new objective
            st, _ = s.run(BIG)
            res = _bar(name, s, st, np0, _ref(T0, basis0, n, b3))
            assert st == L.OK and _close(res.objective, ref3.objective), name
            assert res.num_pivots == len(res.pivot_log)


def _unchanged(s, call, status, word=None, tableau=True):
    before, T0 = _blob(s.result()), s.tableau().tobytes() if tableau else None
    _raises(call, status)
    if word:
        assert word in L.last_error(), L.last_error()
    assert _blob(s.result()) == before
    assert not tableau or s.tableau().tobytes() == T0


def test_refusals_leave_the_session_unchanged():
    """Case 7."""
    m, n, seed = 40, 50, 2
    A, b, c, b2 = dense_lp(m, n, seed)
    prob = dlp.Problem.dense(A, b, c)
    for name, opts in (PATHS[0], PATHS[2]):
        with _open(prob, name, opts) as s:
            assert s.run(BIG)[0] == L.OK
            for bad in (np.nan, np.inf, -np.inf):
                bb = b2.copy()
                bb[17] = bad
                _unchanged(s, lambda: s.set_rhs(bb), L.ERR_ARG)
            before, T0 = _blob(s.result()), s.tableau().tobytes()
            assert L.lib().dlp_session_set_rhs(s._h, b2.ctypes.data_as(L._DP), m - 1, None) == L.ERR_ARG
            assert L.lib().dlp_session_set_rhs(s._h, None, m, None) == L.ERR_ARG
            assert _blob(s.result()) == before and s.tableau().tobytes() == T0
            cand = s.step_candidate()           # a caller-driven step in progress
            _unchanged(s, lambda: s.set_rhs(b2), L.ERR_STATE, "step")
            s.step_update(s.step_select(cand))
            s.set_rhs(b2)                       # between steps it is allowed again
            assert s.run(1)[0] == L.RUNNING     # a pending dual phase
            _unchanged(s, lambda: s.step_candidate(), L.ERR_STATE)
            _unchanged(s, lambda: s.set_objective(c), L.ERR_STATE)
            assert s.run(BIG)[0] == L.OK
        with _open(prob, name, opts) as s:      # stopped inside the primal solve
            assert s.run(5) == (L.RUNNING, 5)
            _unchanged(s, lambda: s.set_rhs(b2), L.ERR_STATE, "dual feasible")
        Au = np.array([[-1.0, 1.0], [1.0, -2.0]])   # tests/test_gpu_reopt.py's unbounded LP
        with _open(dlp.Problem.dense(Au, np.array([1.0, 2.0]), np.array([1.0, 1.0])), name, opts) as s:
            assert s.run(1000)[0] == L.UNBOUNDED
            _unchanged(s, lambda: s.set_rhs(np.array([2.0, 1.0])), L.ERR_STATE, "dual feasible")
    gen = dlp.Problem.general(A, np.full(m, -np.inf), b, 0.0, np.inf, -c)
    with dlp.Session(gen) as s:
        s.run(BIG)
        _unchanged(s, lambda: s.set_rhs(b2), L.ERR_UNSUPPORTED, "general", tableau=False)
    with dlp.Session(prob, rank=0, nranks=2) as s:
        _unchanged(s, lambda: s.set_rhs(b2), L.ERR_UNSUPPORTED, tableau=False)
    for opts in (dict(defer=4, condensed=1), dict(defer=16, condensed=-1), dict(defer=16, lookahead=1)):
        with dlp.Session(prob, **opts) as s:
            assert s.run(BIG)[0] == L.OK
            _unchanged(s, lambda: s.set_rhs(b2), L.ERR_UNSUPPORTED, "defer")
            assert s.run(BIG) == (L.OK, 0)


def test_timed_sessions_do_the_same_pivots():
    """The per-pivot event paths (timing = 1: the update, 2: every phase) record a dual pivot as
    they record a primal one: the same pivots, one sample per pivot."""
    m, n, seed = 40, 50, 2
    A, b, c, b2 = dense_lp(m, n, seed)
    prob = dlp.Problem.dense(A, b, c)
    base = None
    for timing in (0, 1, 2):
        with dlp.Session(prob, defer=1, small_lp=-1, timing=timing, check_interval=7) as s:
            assert s.run(BIG)[0] == L.OK
            s.set_rhs(b2)
            assert s.run(BIG)[0] == L.OK
            res = s.result()
            tm, nsamples = s.timings()
        if timing:
            assert nsamples == res.num_pivots and tm[L.PHASE_UPDATE] > 0.0, (timing, nsamples)
        if base is None:
            base = res
        else:
            assert _blob(res) == _blob(base), timing


def test_random_and_adalloc_problems():
    """Case 8."""
    m, n, seed = 40, 50, 2
    A, b, c, b2 = dense_lp(m, n, seed)
    blobs = []
    for prob in (dlp.Problem.dense(A, b, c), dlp.Problem.random(m, n, seed)):
        with dlp.Session(prob, defer=1, small_lp=-1) as s:
            assert s.run(BIG)[0] == L.OK
            s.set_rhs(b2)
            assert s.run(BIG)[0] == L.OK
            blobs.append(_blob(s.result()))
    assert blobs[0] == blobs[1]
    M, bb, cc = O.adalloc_lp(100, 100, 0.1, 0.25)
    bn = bb.copy()
    bn[:100] *= 1.0 + 0.1 * np.random.default_rng(4).uniform(-1.0, 1.0, 100)   # the budgets
    ref = O.solve_dense(M, bn, cc)
    with dlp.Session(dlp.Problem.adalloc(100, 100, 1, 0.1, 0.25), small_lp=1) as s:
        assert s.run(BIG)[0] == L.OK
        np0 = s.status()[1]
        T0, basis0 = s.tableau(), s.result().basis
        s.set_rhs(bn)
        st, done = s.run(BIG)
        res = s.result()
        # the full bar (m = 200: rhs_ref.py is too slow here; the C++ dual oracle is pinned to it
        # bit for bit by tests/test_oracle_dual.py)
        _bar("adalloc 100x100", s, st, np0, O.resolve_rhs(T0, basis0, M.shape[1], bn))
    print(f"adalloc 100x100: {np0} cold + {done} dual pivots (oracle cold on the new budgets: {ref.num_pivots})")
    assert st == ref.status == L.OK and res.status == L.OK
    assert _close(res.objective, ref.objective)
