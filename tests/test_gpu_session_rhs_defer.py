"""dlp_session_set_rhs_in_place on the GPU: the dual phase of a deferred session,
in blocks of K on the session's own storage path, against the route that existed before it (an eager
session's dlp_session_set_rhs) and the C++ dual oracle run on the session's own read-out.

Bar (include/dlp.h, dlp_session_set_rhs_in_place): status, pivot count, basis, every log entry, x,
y and the objective bit for bit; the nonbasic columns and the RHS of the final tableau byte for
byte; the whole tableau equal as values (np.array_equal: the condensed layout's read-out gives +0
in a basic variable's column where the full layout may hold a -0).  Nothing may depend on K, the
pass form, the row band, check_interval, use_graph or the budgets.

Inputs: tests/dual_lp.py; tests/test_session_rhs_in_place_api.py counts, on the CPU oracle, the
restarts and repeated pivot rows these inputs put inside a block.  Every session has small_lp=-1."""
import functools

import numpy as np
import pytest

import dual_lp as D
import oracle_py as O
import reopt_ref as R
import rhs_ref as RR

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

import test_gpu_session_rhs as S
import test_gpu_session_rhs_wide as W

pytestmark = pytest.mark.gpu

BIG = D.BIG
P = {
    "k4c": dict(defer=4, condensed=1),
    "k16f": dict(defer=16, condensed=-1),
    "k16c": dict(defer=16, condensed=1),
    "k64c": dict(defer=64, condensed=1),
    "k16c_la": dict(defer=16, condensed=1, lookahead=1),
}
EAGER = dict(defer=1)


def _open(prob, path, **more):
    opts = P[path] if isinstance(path, str) else path
    return dlp.Session(prob, small_lp=-1, **opts, **more)


def _nonbasic_and_rhs(T, basis, N):
    """The bytes of the nonbasic columns and the RHS column of a read-out."""
    keep = np.ones(N + 1, bool)
    keep[np.asarray(basis)] = False
    return np.ascontiguousarray(T[:, :N + 1][:, keep]).tobytes()


def _bar(name, s, st, np0, ref, N):
    """The whole bar against a reference dict (the oracle's)."""
    res = S._bar(name, s, st, np0, ref)
    assert res.x.tobytes() == ref["x"].tobytes() and res.y.tobytes() == ref["y"].tobytes(), name
    assert _nonbasic_and_rhs(s.tableau(), res.basis, N) == _nonbasic_and_rhs(ref["T"], ref["basis"], N), \
        f"{name}: a nonbasic column or the RHS differs from the reference in some byte"
    return res


def _same_as(name, s, blob, T, N):
    """The whole bar against an eager session's (blob, tableau)."""
    res = s.result()
    assert S._blob(res) == blob, f"{name}: differs from the eager session"
    Ts = s.tableau()
    assert _nonbasic_and_rhs(Ts, res.basis, N) == _nonbasic_and_rhs(T, res.basis, N), name
    assert np.array_equal(Ts, T), name
    if not s.condensed:
        assert Ts.tobytes() == T.tobytes(), f"{name}: the full layout's read-out differs in some byte"


def _phase(name, prob, path, n, b2, pricing=0, **more):
    """Cold solve on `path`, set_rhs(in_place), the dual phase to its end, against the oracle on the
    session's own read-out.  Returns (blob, final tableau, reference)."""
    N = n + prob.m
    with _open(prob, path, pricing=pricing, **more) as s:
        assert s.run(BIG)[0] == L.OK, name
        np0 = s.status()[1]
        T0, basis0 = s.tableau(), s.result().basis
        ref = W._ref(T0, basis0, n, b2, pricing=pricing)
        want_la = isinstance(path, str) and P[path].get("lookahead") == 1
        assert s.lookahead() == want_la, name
        assert s.set_rhs(b2, in_place=True) >= 0.0
        assert not s.lookahead(), name
        assert s.status() == (L.RUNNING, np0), name
        assert s.get_defer_tuning()[2] == (P[path] if isinstance(path, str) else path)["defer"], name
        st, done = s.run(BIG)
        assert done == ref["done"], (name, done, ref["done"])
        res = _bar(name, s, st, np0, ref, N)
        assert s.run(BIG) == (st, 0), name
        return S._blob(res), s.tableau(), ref


# ---- 1. the rebuild alone

@pytest.mark.parametrize("path", ["k16f", "k16c", "k64c"])
@pytest.mark.parametrize("m,n", [(63, 70), (64, 66), (65, 449), (300, 740)])
def test_rebuild_alone(m, n, path):
    A, b, c, b2 = D.dense_lp(m, n)
    N = n + m
    with _open(dlp.Problem.dense(A, b, c), path) as s:
        assert s.run(BIG)[0] == L.OK
        cold = s.result()
        T0 = s.tableau()
        assert s.set_rhs(b2, in_place=True) >= 0.0
        assert s.status() == (L.RUNNING, cold.num_pivots)
        T1 = s.tableau()
        for what, want in (("rhs_ref.fold_rhs", RR.fold_rhs(T0, n, b2)),
                           ("the oracle", W._ref(T0, cold.basis, n, b2, max_pivots=0)["T"][:, N])):
            bad = np.nonzero(T1[:, N].view(np.int64) != want.view(np.int64))[0]
            assert len(bad) == 0, f"RHS differs from {what} at rows {bad[:8]}: {T1[bad[:8], N]} vs {want[bad[:8]]}"
        T1[:, N] = T0[:, N]
        assert T1.tobytes() == T0.tobytes(), "an entry outside the RHS column changed"
        assert s.result().basis.tobytes() == cold.basis.tobytes()
        s.set_rhs(b, in_place=True)              # the creation b: optimal again without a pivot
        assert s.run(BIG) == (L.OK, 0)
        assert S._close(s.result().objective, cold.objective)


# ---- 2. the dual phase against the oracle and the eager session

@functools.lru_cache(maxsize=None)
def _eager_dense(m, n):
    A, b, c, b2 = D.dense_lp(m, n)
    with _open(dlp.Problem.dense(A, b, c), EAGER) as s:
        assert s.run(BIG)[0] == L.OK
        s.set_rhs(b2)
        assert s.run(BIG)[0] == L.OK
        return S._blob(s.result()), s.tableau()


@pytest.mark.parametrize("m,n", list(D.SHAPES))
def test_dual_phase_dense_every_shape(m, n):
    A, b, c, b2 = D.dense_lp(m, n)
    blob, T, ref = _phase(f"dense {m}x{n} k16c", dlp.Problem.dense(A, b, c), "k16c", n, b2)
    assert blob[0] == L.OK and ref["done"] >= 10
    eb, eT = _eager_dense(m, n)
    assert blob == eb and np.array_equal(T, eT)


@pytest.mark.parametrize("path", list(P))
@pytest.mark.parametrize("m,n", [(65, 449), (300, 740)])
def test_dual_phase_every_path(m, n, path):
    A, b, c, b2 = D.dense_lp(m, n)
    blob, T, ref = _phase(f"dense {m}x{n} {path}", dlp.Problem.dense(A, b, c), path, n, b2)
    eb, eT = _eager_dense(m, n)
    assert blob == eb and np.array_equal(T, eT)
    if P[path]["condensed"] != 1:
        assert T.tobytes() == eT.tobytes(), "the full layout's read-out differs from the eager session's"


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("path", ["k16c", "k64c"])
@pytest.mark.parametrize("m,n", [(65, 449), (257, 260), (300, 740)])
def test_dual_phase_cone(m, n, path, pricing):
    A, b, c = D.cone_lp(m, n)
    blob, T, ref = _phase(f"cone {m}x{n} {path} pricing {pricing}", dlp.Problem.dense(A, np.abs(b), c), path, n, b,
                          pricing=pricing)
    assert blob[0] in (L.OK, L.INFEASIBLE) and ref["done"] >= 10


@functools.lru_cache(maxsize=None)
def _eager_tied(name, pricing):
    A, b, c = D.tied_lp(name)
    with _open(dlp.Problem.dense(A, np.abs(b), c), EAGER, pricing=pricing) as s:
        assert s.run(BIG)[0] == L.OK
        s.set_rhs(b)
        assert s.run(BIG)[0] == L.OK
        return S._blob(s.result()), s.tableau()


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("path", ["k16c", "k64c"])
@pytest.mark.parametrize("name", ["dup_rows", "dup_cols"])
def test_dual_phase_tied(name, path, pricing):
    """Exact ties between row workgroups and between column workgroups (on the condensed layout
    between slots: the smaller variable index wins), against an eager session holding the same LP."""
    A, b, c = D.tied_lp(name)
    m, n = A.shape
    eb, eT = _eager_tied(name, pricing)
    with _open(dlp.Problem.dense(A, np.abs(b), c), path, pricing=pricing) as s:
        assert s.run(BIG)[0] == L.OK
        s.set_rhs(b, in_place=True)
        st, done = s.run(BIG)
        assert st == L.OK and done >= 10
        _same_as(f"{name} {path} pricing {pricing}", s, eb, eT, n + m)


# ---- 3. blocks cut in every way

CUT = (300, 740)


@functools.lru_cache(maxsize=None)
def _cut_base(path):
    m, n = CUT
    A, b, c, b2 = D.dense_lp(m, n)
    blob, T, ref = _phase(f"cut base {path}", dlp.Problem.dense(A, b, c), path, n, b2)
    assert blob[0] == L.OK and ref["done"] > 800
    return blob, T.tobytes()


@pytest.mark.parametrize("budget", [1, 7, 37, 100])
@pytest.mark.parametrize("path", ["k16c", "k64c"])
def test_budgets(path, budget):
    m, n = CUT
    A, b, c, b2 = D.dense_lp(m, n)
    blob, Tb = _cut_base(path)
    with _open(dlp.Problem.dense(A, b, c), path) as s:
        assert s.run(BIG)[0] == L.OK
        np0 = s.status()[1]
        s.set_rhs(b2, in_place=True)
        calls = 0
        while True:
            st, done = s.run(budget)
            calls += 1
            assert done <= budget and calls < 2000
            if st != L.RUNNING:
                break
        assert st == L.OK
        if budget == 1:
            assert calls == s.status()[1] - np0          # OK comes with the last pivot
        assert S._blob(s.result()) == blob, f"{path}, budget {budget}: differs from one unbounded call"
        assert s.tableau().tobytes() == Tb, f"{path}, budget {budget}: final tableau differs"


@pytest.mark.parametrize("more", [dict(check_interval=5), dict(check_interval=5, use_graph=1),
                                  dict(check_interval=64, use_graph=0), dict(check_interval=64, use_graph=1)],
                         ids=["ci5", "ci5_graph", "ci64", "ci64_graph"])
@pytest.mark.parametrize("path", ["k16c", "k64c"])
def test_windows(path, more):
    """Windows shorter than K (check_interval 5), of K = 64 and 4 K = 16 blocks, captured or not."""
    m, n = CUT
    A, b, c, b2 = D.dense_lp(m, n)
    blob, Tb = _cut_base(path)
    got, T, _ = _phase(f"{path} {more}", dlp.Problem.dense(A, b, c), path, n, b2, **more)
    assert got == blob and T.tobytes() == Tb


@pytest.mark.parametrize("path", ["k16c", "k64c"])
def test_pivot_limit(path):
    m, n = CUT
    A, b, c, b2 = D.dense_lp(m, n)
    prob = dlp.Problem.dense(A, b, c)
    with _open(prob, path) as s:
        assert s.run(BIG)[0] == L.OK
        np0 = s.status()[1]                                      # the cold solve's pivots
    with _open(prob, path, max_pivots=np0 + 37) as s:
        assert s.run(BIG)[0] == L.OK
        T0, basis0 = s.tableau(), s.result().basis
        s.set_rhs(b2, in_place=True)
        assert s.run(20) == (L.RUNNING, 20)                      # resumes from an applied block
        assert s.run(BIG) == (L.PIVOT_LIMIT, 17)
        _bar(f"{path} pivot limit", s, None, np0, W._ref(T0, basis0, n, b2, max_pivots=37), n + m)
        assert s.run(10) == (L.PIVOT_LIMIT, 0)


@pytest.mark.parametrize("path", ["k16c", "k64c"])
def test_timed_sessions_do_the_same_pivots(path):
    """The per-pivot event paths (timing = 1: the pass, 2: every phase) record a deferred dual pivot
    as they record a deferred primal one: the same pivots, one sample per pivot."""
    m, n = 65, 449
    A, b, c, b2 = D.dense_lp(m, n)
    eb, eT = _eager_dense(m, n)
    for timing in (1, 2):
        with _open(dlp.Problem.dense(A, b, c), path, timing=timing, check_interval=7) as s:
            assert s.run(BIG)[0] == L.OK
            s.set_rhs(b2, in_place=True)
            assert s.run(BIG)[0] == L.OK
            _same_as(f"{path} timing {timing}", s, eb, eT, n + m)
            tm, nsamples = s.timings()
            assert nsamples == s.status()[1] and tm[L.PHASE_UPDATE] > 0.0, (timing, nsamples)


# ---- 4. infeasible and back

def test_infeasible_and_back():
    m, n = 65, 449
    A, b, c, b2 = D.dense_lp(m, n)
    N = n + m
    bad = b2.copy()
    bad[3] = -1.0            # A > 0: row 3 cannot hold; the oracle needs 163 dual pivots to see it
    c2 = R.make_c2(c, D.DENSE_SEED[(m, n)], scale=0.02, holes=False)
    prob = dlp.Problem.dense(A, b, c)
    with _open(prob, EAGER) as e:
        assert e.run(BIG)[0] == L.OK
        e.set_rhs(bad)
        assert e.run(BIG)[0] == L.INFEASIBLE
        e_bad = S._blob(e.result()), e.tableau()
        e.set_rhs(b2)
        assert e.run(BIG)[0] == L.OK
        e_ok = S._blob(e.result()), e.tableau()
    with _open(prob, "k16c") as s:
        assert s.run(BIG)[0] == L.OK
        np0 = s.status()[1]
        T0, basis0 = s.tableau(), s.result().basis
        ref = W._ref(T0, basis0, n, bad)
        assert ref["status"] == RR.INFEASIBLE and ref["done"] % 16 != 0 and ref["done"] > 16
        s.set_rhs(bad, in_place=True)
        st, done = s.run(BIG)
        assert (st, done) == (L.INFEASIBLE, ref["done"])
        _bar("infeasible", s, st, np0, ref, N)
        _same_as("infeasible", s, *e_bad, N)
        assert s.run(BIG) == (L.INFEASIBLE, 0)
        S._unchanged(s, lambda: s.set_objective(c2), L.ERR_STATE, "dual")
        S._unchanged(s, lambda: s.set_defer(1), L.ERR_STATE, "dual")
        S._unchanged(s, lambda: s.step_candidate(), L.ERR_STATE)
        s.set_rhs(b2, in_place=True)             # the block arrays are consistent: the next phase runs on them
        assert s.run(BIG)[0] == L.OK
        _same_as("feasible again", s, *e_ok, N)


# ---- 5. after the phase the session is an ordinary optimal deferred session

@pytest.mark.parametrize("path", ["k16c", "k64c"])
def test_after_the_phase(path):
    m, n = 65, 449
    A, b, c, b2 = D.dense_lp(m, n)
    N = n + m
    seed = D.DENSE_SEED[(m, n)]
    c2 = R.make_c2(c, seed, scale=0.02, holes=False)
    b3 = b * (1.0 + 0.3 * np.random.default_rng(seed + 1).uniform(-1.0, 1.0, m))
    prob = dlp.Problem.dense(A, b, c)
    want = []
    with _open(prob, EAGER) as e:
        assert e.run(BIG)[0] == L.OK
        for change, v in ((e.set_rhs, b2), (e.set_objective, c2), (e.set_rhs, b3), (e.set_objective, c)):
            change(v)
            assert e.run(BIG)[0] == L.OK
            want.append((S._blob(e.result()), e.tableau()))
    with _open(prob, path) as s:
        assert s.run(BIG)[0] == L.OK
        K = P[path]["defer"]
        s.set_rhs(b2, in_place=True)
        assert s.run(BIG)[0] == L.OK
        _same_as("rhs b2", s, *want[0], N)
        s.set_objective(c2)                      # a primal phase on the deferred path
        assert s.status()[0] == L.RUNNING
        assert s.run(BIG)[0] == L.OK and s.get_defer_tuning()[2] == K and s.condensed
        _same_as("objective c2", s, *want[1], N)
        s.set_rhs(b3, in_place=True)             # a second dual phase, on the new objective
        assert s.run(BIG)[0] == L.OK
        _same_as("rhs b3", s, *want[2], N)
        T1 = s.tableau()
        s.set_defer(1)                           # to eager and back
        assert not s.condensed and np.array_equal(s.tableau(), T1)
        s.set_defer(**P[path])
        assert s.condensed and s.tableau().tobytes() == T1.tobytes()
        assert s.run(BIG) == (L.OK, 0)
        s.set_objective(c)
        assert s.run(BIG)[0] == L.OK
        _same_as("objective c", s, *want[3], N)


# ---- 6. a session with lookahead on

def test_lookahead_session():
    m, n = 300, 740
    A, b, c, b2 = D.dense_lp(m, n)
    N = n + m
    c2 = R.make_c2(c, D.DENSE_SEED[(m, n)], scale=0.02, holes=False)
    prob = dlp.Problem.dense(A, b, c)
    with _open(prob, EAGER) as e:
        assert e.run(BIG)[0] == L.OK
        e.set_rhs(b2)
        assert e.run(BIG)[0] == L.OK
        e.set_objective(c2)
        assert e.run(BIG)[0] == L.OK
        want = S._blob(e.result()), e.tableau()
    with _open(prob, "k16c_la") as s:
        assert s.lookahead()
        assert s.run(BIG)[0] == L.OK
        np0 = s.status()[1]
        T0, basis0 = s.tableau(), s.result().basis
        s.set_rhs(b2, in_place=True)
        assert not s.lookahead()
        st, done = s.run(BIG)
        _bar("k16c_la", s, st, np0, W._ref(T0, basis0, n, b2), N)
        assert st == L.OK
        s.set_defer(16, 1, 1)
        assert s.lookahead() and s.condensed
        s.set_objective(c2)
        assert s.run(BIG)[0] == L.OK
        _same_as("lookahead restored, primal re-optimisation", s, *want, N)


# ---- 7. pass forms and row bands

@pytest.mark.parametrize("K,form,rb", [(64, 3, 0), (64, 21, 0), (64, 22, 0), (64, 23, 0), (16, 3, 0), (16, 4, 0),
                                       (16, 3, 4), (16, 3, 64), (64, 3, 4), (64, 3, 64)])
def test_pass_forms_and_bands(K, form, rb):
    m, n = 65, 449
    A, b, c, b2 = D.dense_lp(m, n)
    eb, eT = _eager_dense(m, n)
    more = dict(rows_per_block=rb) if rb else {}
    with _open(dlp.Problem.dense(A, b, c), dict(defer=K, condensed=1), **more) as s:
        s.set_defer_tuning(0, form)
        assert s.run(BIG)[0] == L.OK
        s.set_rhs(b2, in_place=True)
        assert s.defer_form() == form
        assert s.run(BIG)[0] == L.OK
        _same_as(f"K {K} form {form} rows_per_block {rb}", s, eb, eT, n + m)


# ---- 8. refusals, and the paths on which the call is dlp_session_set_rhs itself

def test_refusals_leave_the_session_unchanged():
    m, n = 63, 70
    A, b, c, b2 = D.dense_lp(m, n)
    prob = dlp.Problem.dense(A, b, c)
    gen = dlp.Problem.general(A, np.full(m, -np.inf), b, 0.0, np.inf, -c)
    with dlp.Session(gen) as s:
        s.run(BIG)
        S._unchanged(s, lambda: s.set_rhs(b2, in_place=True), L.ERR_UNSUPPORTED, "general", tableau=False)
    with dlp.Session(prob, rank=0, nranks=2) as s:
        S._unchanged(s, lambda: s.set_rhs(b2, in_place=True), L.ERR_UNSUPPORTED, "single-GPU", tableau=False)
    for path in ("k16c", "k16f", "k16c_la", EAGER):
        with _open(prob, path) as s:             # stopped inside the primal solve
            assert s.run(7) == (L.RUNNING, 7)
            la = s.lookahead()
            S._unchanged(s, lambda: s.set_rhs(b2, in_place=True), L.ERR_STATE, "dual feasible")
            assert s.lookahead() == la
            before, T0 = S._blob(s.result()), s.tableau().tobytes()
            assert L.lib().dlp_session_set_rhs_in_place(s._h, None, m, None) == L.ERR_ARG
            assert L.lib().dlp_session_set_rhs_in_place(s._h, b2.ctypes.data_as(L._DP), m - 1, None) == L.ERR_ARG
            bb = b2.copy()
            bb[17] = np.nan
            S._unchanged(s, lambda: s.set_rhs(bb, in_place=True), L.ERR_ARG)
            assert S._blob(s.result()) == before and s.tableau().tobytes() == T0
            assert s.run(BIG)[0] == L.OK         # and it goes on as if nothing had been asked
    with _open(prob, "k16c") as s:
        assert s.run(BIG)[0] == L.OK
        cand = s.step_candidate()                # a caller-driven step in progress (optimal: a void one)
        S._unchanged(s, lambda: s.set_rhs(b2, in_place=True), L.ERR_STATE, "step")
        s.step_update(s.step_select(cand))
        s.set_rhs(b2, in_place=True)
        assert s.run(1)[0] == L.RUNNING          # a pending dual phase
        S._unchanged(s, lambda: s.step_candidate(), L.ERR_STATE)
        S._unchanged(s, lambda: s.set_defer(1), L.ERR_STATE, "dual")
        S._unchanged(s, lambda: s.set_rhs(b2), L.ERR_UNSUPPORTED, "defer")   # the old call keeps its refusal
        assert s.run(BIG)[0] == L.OK


@pytest.mark.parametrize("name,opts", S.PATHS, ids=[p[0] for p in S.PATHS])
def test_eager_and_small_lp_sessions_are_set_rhs_itself(name, opts):
    m, n, seed = S.SHAPES[1]
    A, b, c, b2 = S.dense_lp(m, n, seed)
    prob = dlp.Problem.dense(A, b, c)
    out = []
    for in_place in (False, True):
        with S._open(prob, name, opts) as s:
            assert s.run(BIG)[0] == L.OK
            s.set_rhs(b2, in_place=in_place)
            T1 = s.tableau().tobytes()
            assert s.run(3)[0] == L.RUNNING
            st, _ = s.run(BIG)
            assert st == L.OK
            out.append((T1, S._blob(s.result()), s.tableau().tobytes()))
    assert out[0] == out[1]
