"""dlp_session_set_rhs on the GPU past the first workgroup of its three kernels (dlp_dual.hip):
the shapes of tests/dual_lp.py, each on a boundary of rhs_rebuild_kernel (64 stored rows per
wave, 64-column tiles), dual_row_kernel (256 rows per workgroup) or dual_col_kernel (512 columns
per workgroup, 2 per lane), and its two LPs whose exact ties straddle the workgroups, so that the
winner comes out of the last workgroup's reduction of the partials.

Reference: the C++ dual oracle (oracle/oracle_dual.inc, pinned bit for bit to tests/rhs_ref.py by
tests/test_oracle_dual.py) run on the session's own tableau and basis.  Bar: test_gpu_session_rhs's
_bar (status, pivot count, basis, every log field and the objective bit for bit; x, y and the
tableau equal as values), and equal blobs on the eager path, its graph windows of 5 and the
small-LP path.  tests/test_dual_inputs.py holds the inputs' properties (pivot counts, tie counts)
on the CPU."""
import functools

import numpy as np
import pytest

import dual_lp as D
import oracle_py as O

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

import test_gpu_session_rhs as G

pytestmark = pytest.mark.gpu

BIG = G.BIG
SHAPES = list(D.SHAPES)
_REFS = {}


def _ref(T0, basis0, n, b2, **kw):
    """The oracle on a session's tableau, once per distinct input (the paths hand in the same bytes)."""
    key = (T0.tobytes(), basis0.tobytes(), n, np.asarray(b2).tobytes(), tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = O.resolve_rhs(T0, basis0, n, b2, **kw)
    return _REFS[key]


def _sessions(prob, what, **more):
    """(name, session) over G.PATHS; the small-LP path is left out by name where the shape does
    not get it."""
    for name, opts in G.PATHS:
        with dlp.Session(prob, **opts, **more) as s:
            if name == "small_lp" and not s.small_lp():
                print(f"{what}: path small_lp left out (the session did not take the one-launch path)")
                continue
            yield name, s


def _phase(prob, what, n, b2, pricing=0, np_cold=None, **more):
    """Cold solve, set_rhs(b2), the dual phase to the end on every path: each against the oracle,
    all with one blob.  Returns (result, reference)."""
    base = ref = None
    names = []
    for name, s in _sessions(prob, what, pricing=pricing, **more):
        assert s.run(BIG)[0] == L.OK, (what, name)
        np0 = s.status()[1]
        assert np_cold is None or np0 == np_cold, (what, name, np0)
        T0, basis0 = s.tableau(), s.result().basis
        ref = _ref(T0, basis0, n, b2, pricing=pricing)
        s.set_rhs(b2)
        st, done = s.run(BIG)
        assert done == ref["done"], (what, name, done, ref["done"])
        res = G._bar(f"{what} {name}", s, st, np0, ref)
        assert s.run(BIG) == (st, 0), (what, name)
        names.append(name)
        if base is None:
            base = res
        else:
            assert G._blob(res) == G._blob(base), f"{what}: {name} differs from the eager path"
    assert names[:2] == ["eager", "eager_graph5"], names
    print(f"{what}: paths {names}, {ref['done']} dual pivots, status {ref['status']}")
    return base, ref


@pytest.mark.parametrize("m,n", SHAPES)
def test_rebuild_alone(m, n):
    """set_rhs writes the oracle's RHS column bit for bit, the objective entry included, and
    changes no other byte; the session is RUNNING with the cold solve's pivot count."""
    A, b, c, b2 = D.dense_lp(m, n)
    prob = dlp.Problem.dense(A, b, c)
    N = n + m
    for name, s in _sessions(prob, f"{m}x{n}"):
        assert s.run(BIG)[0] == L.OK
        cold = s.result()
        T0 = s.tableau()
        want = _ref(T0, cold.basis, n, b2, max_pivots=0)["T"][:, N]
        assert s.set_rhs(b2) >= 0.0
        assert s.status() == (L.RUNNING, cold.num_pivots), name
        T1 = s.tableau()
        bad = np.nonzero(T1[:, N].view(np.int64) != want.view(np.int64))[0]
        assert len(bad) == 0, f"{name}: RHS differs at rows {bad[:8]}: {T1[bad[:8], N]} vs {want[bad[:8]]}"
        T1[:, N] = T0[:, N]
        assert T1.tobytes() == T0.tobytes(), f"{name}: an entry outside the RHS column changed"
        assert s.result().basis.tobytes() == cold.basis.tobytes(), name


@pytest.mark.parametrize("m,n", SHAPES)
def test_dual_phase_dense(m, n):
    A, b, c, b2 = D.dense_lp(m, n)
    res, ref = _phase(dlp.Problem.dense(A, b, c), f"dense {m}x{n}", n, b2)
    assert res.status == L.OK and ref["done"] >= 10
    cold2 = O.solve_dense(A, b2, c)
    assert G._close(res.objective, cold2.objective)


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_dual_phase_cone(m, n, pricing):
    """The whole dual simplex from the slack basis; with m > 256 both row workgroups hold
    eligible rows."""
    A, b, c = D.cone_lp(m, n)
    res, ref = _phase(dlp.Problem.dense(A, np.abs(b), c), f"cone {m}x{n} pricing {pricing}", n, b,
                      pricing=pricing, np_cold=0)
    assert res.status in (L.OK, L.INFEASIBLE) and ref["done"] >= 10


@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("name", ["dup_rows", "dup_cols"])
def test_dual_phase_tied(name, pricing):
    """Exact ties between row workgroups (dup_rows: 12 with Dantzig pricing, 6 of them won by the
    higher workgroup's row) and between column workgroups (dup_cols: 843, 228 of them over all
    three): tests/test_dual_inputs.py counts them on the oracle's trace."""
    A, b, c = D.tied_lp(name)
    cold = len(range(0, D.TIED[name][1]["pairs"], 2)) if name == "dup_rows" else 0
    res, ref = _phase(dlp.Problem.dense(A, np.abs(b), c), f"{name} pricing {pricing}", A.shape[1], b,
                      pricing=pricing, np_cold=cold)
    assert res.status == L.OK and ref["done"] >= 10


def test_budgets_on_the_widest_shape():
    """run(1) repeated and run(7) repeated give the pivots of one unbounded call: the ticket of
    the hand-off is re-armed between launches and, on the graph path, inside a window."""
    A, b, c = D.tied_lp("dup_rows")
    n = A.shape[1]
    prob = dlp.Problem.dense(A, np.abs(b), c)
    base = None
    for budget in (BIG, 1, 7):
        for name, s in _sessions(prob, f"dup_rows budget {budget}"):
            assert s.run(BIG)[0] == L.OK
            np0 = s.status()[1]
            T0, basis0 = s.tableau(), s.result().basis
            s.set_rhs(b)
            calls = 0
            while True:
                st, done = s.run(budget)
                calls += 1
                assert done <= budget and calls < 2000
                if st != L.RUNNING:
                    break
            res = G._bar(f"{name} budget {budget}", s, st, np0, _ref(T0, basis0, n, b))
            assert st == L.OK
            if budget == 1:
                assert calls == res.num_pivots - np0, (name, calls)   # OK comes with the last pivot
            if base is None:
                base = res
            else:
                assert G._blob(res) == G._blob(base), f"{name}, budget {budget}: differs from one unbounded call"
    assert base.num_pivots > 100


@pytest.mark.parametrize("m,n", [(128, 385), (257, 260)])
def test_row_stride(m, n):
    """ld_align 16, 128 and 512: the RHS column sits at r * ld + N, not at the row end; the same
    blobs."""
    A, b, c, b2 = D.dense_lp(m, n)
    prob = dlp.Problem.dense(A, b, c)
    N = n + m
    base = None
    lds = set()
    for align in (16, 128, 512):
        for name, opts in G.PATHS[:2]:
            with dlp.Session(prob, **opts, ld_align=align) as s:
                assert s.ld % align == 0 and s.ld >= N + 1
                lds.add(s.ld)
                assert s.run(BIG)[0] == L.OK
                np0 = s.status()[1]
                T0, basis0 = s.tableau(), s.result().basis
                assert T0.shape == (m + 1, s.ld)
                s.set_rhs(b2)
                T1 = s.tableau()
                want = _ref(T0, basis0, n, b2, max_pivots=0)["T"]
                assert T1[:, N].tobytes() == want[:, N].tobytes(), (align, name)
                assert not T1[:, N + 1:].any(), (align, name)           # the padding stays +0.0
                st, _ = s.run(BIG)
                res = G._bar(f"ld_align {align} {name}", s, st, np0, _ref(T0, basis0, n, b2))
                assert not s.tableau()[:, N + 1:].any(), (align, name)
            if base is None:
                base = res
            else:
                assert G._blob(res) == G._blob(base), (align, name)
    assert len(lds) == 3        # three different strides (N + 1 = 514 / 518: 528, 640, 1024)


@functools.lru_cache(maxsize=None)
def _tuning_case():
    m, n, seed = G.SHAPES[-1]
    A, b, c, b2 = G.dense_lp(m, n, seed)
    with dlp.Session(dlp.Problem.dense(A, b, c), defer=1, small_lp=-1) as s:
        assert s.run(BIG)[0] == L.OK
        np0 = s.status()[1]
        T0, basis0 = s.tableau(), s.result().basis
        s.set_rhs(b2)
        st, _ = s.run(BIG)
        res = G._bar("default tuning", s, st, np0, _ref(T0, basis0, n, b2))
    assert st == L.OK and res.num_pivots - np0 >= 10
    return G._blob(res)


@pytest.mark.parametrize("variant", range(L.lib().dlp_update_variants()))
def test_update_variants_in_the_dual_phase(variant):
    """Every rank-1 update variant, rows_per_block 4 and 8, nontemporal 0 and 1, through a dual
    phase (a negative pivot) at 96 x 160: one blob."""
    m, n, seed = G.SHAPES[-1]
    A, b, c, b2 = G.dense_lp(m, n, seed)
    prob = dlp.Problem.dense(A, b, c)
    base = _tuning_case()
    for rb in (4, 8):
        for nt in (0, 1):
            with dlp.Session(prob, defer=1, small_lp=-1, update_variant=variant, rows_per_block=rb,
                             nontemporal=nt) as s:
                assert s.run(BIG)[0] == L.OK
                s.set_rhs(b2)
                assert s.run(BIG)[0] == L.OK
                assert G._blob(s.result()) == base, (variant, rb, nt)


@pytest.mark.parametrize("m,n", [pytest.param(64, 130, id="register"), pytest.param(37, 53, id="lds")])
def test_session_against_batch(m, n):
    """dlp.h promises the session "the batch's rule bit for bit": the same LP and the same b2
    through Batch.resolve_rhs and through Session.set_rhs + run."""
    seed = 7700 + m
    A, b, c = O.gen_dense(m, n, seed)
    b2 = b * (1.0 + 0.3 * np.random.default_rng(seed).uniform(-1.0, 1.0, m))
    cap = 4096
    with dlp.Batch(A[None], b[None], c[None], want_basis=True, log_cap=cap) as bt:
        assert bt.info()["register_kernel"] == (m == 64)
        assert bt.result.status[0] == L.OK
        cold_pivots = int(bt.result.num_pivots[0])
        br = bt.resolve_rhs(b2[None], want_basis=True, log_cap=cap)
    done = int(br.num_pivots[0])
    assert br.status[0] == L.OK and 1 <= done <= cap
    for name, s in _sessions(dlp.Problem.dense(A, b, c), f"{m}x{n}"):
        assert s.run(BIG)[0] == L.OK
        np0 = s.status()[1]
        assert np0 == cold_pivots, name
        s.set_rhs(b2)
        st, sdone = s.run(BIG)
        res = s.result()
        assert (st, sdone) == (int(br.status[0]), done), name
        assert res.basis.tobytes() == br.basis[0].tobytes(), name
        assert np.float64(res.objective).tobytes() == np.float64(br.objective[0]).tobytes(), name
        got, want = np.ascontiguousarray(res.pivot_log[np0:]), np.ascontiguousarray(br.logs[0][:done])
        for i in range(done):
            assert got[i].tobytes() == want[i].tobytes(), f"{name} dual pivot {i}: session {got[i]} batch {want[i]}"
        assert np.array_equal(res.x, br.x[0]) and np.array_equal(res.y, br.y[0]), name
