"""dlp_session_set_defer on the GPU: a live session moved between the eager full layout and the
deferred paths keeps everything the rule can see.  The tableau read out before and after a switch
is the same bytes (the device expand against the host read-out's rule, the pack against both), the
session reports the new path, every later pivot is the pivot an unconverted eager session does
(result blob and final tableau bit for bit), the round trip cold-deferred -> eager dual phase ->
deferred re-optimisation gives the eager session's results, and every refusal leaves the session
as it was.

Inputs: tests/dual_lp.py's dense LPs at the shapes that cross the kernels' boundaries (64 stored
rows, the 512-column tile of the full and of the condensed layout, a 256-row band); tests/
test_set_defer_api.py checks on the CPU oracle that every stop lies inside the cold solve."""
import functools

import numpy as np
import pytest

import oracle_py as O
import reopt_ref as R

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

import dual_lp as D
import test_gpu_session_rhs as S

pytestmark = pytest.mark.gpu

BIG = 10 ** 6
# the set of paths: set_defer's arguments, and creation's options
P = {
    "eager": dict(defer=1),
    "k4c": dict(defer=4, condensed=1),
    "k16f": dict(defer=16, condensed=-1),
    "k16c_la": dict(defer=16, condensed=1, lookahead=1),
    "k64c": dict(defer=64, condensed=1),
}
# stops 7 and 37 end inside a block at K = 16 and K = 64, stop 100 36 steps into the second K = 64 block
STOPS = {(63, 70): (7, 29), (65, 449): (7, 37, 100), (257, 260): (7, 37, 100), (300, 740): (7, 37, 100)}
K16C = dict(defer=16, condensed=1)   # tests 2-4: the plain condensed path
FULL_MATRIX = (65, 449)
CHAIN_SHAPE, CHAIN_STOP = (300, 740), 100
PAIRS_ALL = [(a, b) for a in P for b in P if a != b]
PAIRS_EAGER = [(a, b) for (a, b) in PAIRS_ALL if "eager" in (a, b)]


def _open(prob, path, **more):
    return dlp.Session(prob, small_lp=-1, **P[path], **more)


def _prob(m, n):
    A, b, c, b2 = D.dense_lp(m, n)
    return dlp.Problem.dense(A, b, c)


@functools.lru_cache(maxsize=None)
def _eager_ref(m, n, **more):
    """(result blob, final tableau bytes) of an unconverted eager session, once per shape."""
    with _open(_prob(m, n), "eager", **dict(more)) as s:
        assert s.run(BIG)[0] == L.OK
        return S._blob(s.result()), s.tableau().tobytes()


def _reports(s, path):
    want = P[path] if isinstance(path, str) else path
    K = want["defer"]
    assert s.get_defer_tuning()[2] == K, (path, s.get_defer_tuning())
    assert s.storage()[2] == (K > 1 and want.get("condensed", 0) == 1), (path, s.storage())
    assert s.condensed == s.storage()[2]
    assert s.lookahead() == (K > 1 and want.get("lookahead", -1) == 1), path
    assert (s.get_defer_tuning()[1] >= 0) == (K > 1), path
    n, m = s.problem.n, s.problem.m
    assert s.storage()[1] == (n if s.condensed else n + m), path


def _switch(s, to):
    """set_defer(to) between two read-outs that must be the same bytes; returns the kernel ms."""
    T0 = s.tableau()
    st0 = s.status()
    ms = s.set_defer(**P[to])
    assert ms >= 0.0
    T1 = s.tableau()
    assert T1.tobytes() == T0.tobytes(), f"-> {to}: the tableau read out changed"
    assert s.status() == st0, to
    _reports(s, to)
    return ms


def _continuation(m, n, frm, to, stop, **more):
    ref_blob, ref_T = _eager_ref(m, n, **more)
    with _open(_prob(m, n), frm, **more) as s:
        _reports(s, frm)
        assert s.run(stop) == (L.RUNNING, stop), (frm, stop)
        _switch(s, to)
        st, done = s.run(BIG)
        assert st == L.OK and done == ref_blob[1] - stop, (frm, to, stop, st, done)
        assert S._blob(s.result()) == ref_blob, f"{m}x{n} {frm} -> {to} at {stop}: differs from the eager session"
        assert s.tableau().tobytes() == ref_T, f"{m}x{n} {frm} -> {to} at {stop}: final tableau differs"
        assert s.run(BIG) == (L.OK, 0)


# ---- 1. primal continuation across a switch

@pytest.mark.parametrize("frm,to", PAIRS_ALL, ids=[f"{a}-{b}" for a, b in PAIRS_ALL])
def test_continuation_every_pair(frm, to):
    m, n = FULL_MATRIX
    for stop in STOPS[(m, n)]:
        _continuation(m, n, frm, to, stop)


@pytest.mark.parametrize("frm,to", PAIRS_EAGER, ids=[f"{a}-{b}" for a, b in PAIRS_EAGER])
@pytest.mark.parametrize("m,n", [s for s in sorted(STOPS) if s != FULL_MATRIX])
def test_continuation_eager_pairs(m, n, frm, to):
    for stop in STOPS[(m, n)]:
        _continuation(m, n, frm, to, stop)


def test_chain_through_every_path():
    m, n = CHAIN_SHAPE
    ref_blob, ref_T = _eager_ref(m, n)
    with _open(_prob(m, n), "eager") as s:
        assert s.run(37) == (L.RUNNING, 37)
        for to in ("k4c", "k16f", "k16c_la", "k64c", "eager", "k64c", "k16f"):
            _switch(s, to)
            assert s.run(CHAIN_STOP) == (L.RUNNING, CHAIN_STOP), to
        assert s.run(BIG)[0] == L.OK
        assert S._blob(s.result()) == ref_blob
        assert s.tableau().tobytes() == ref_T


# ---- 2. expand and pack alone

@pytest.mark.parametrize("ld_align", [0, 16, 128])
@pytest.mark.parametrize("m,n", sorted(STOPS))
def test_expand_and_pack_alone(m, n, ld_align):
    N = n + m
    strides = set()
    with dlp.Session(_prob(m, n), small_lp=-1, ld_align=ld_align, **K16C) as s:
        stop = STOPS[(m, n)][1]                  # 37 (29 at 63 x 70, whose cold solve has 33 pivots)
        assert s.run(stop) == (L.RUNNING, stop)
        host = s.tableau()                       # the host read-out of the condensed tableau
        strides.add(s.storage()[0])
        ms = s.set_defer(1)
        assert ms > 0.0 and not s.condensed and s.storage()[1] == N
        strides.add(s.storage()[0])
        assert s.storage()[0] == s.ld == host.shape[1]
        if ld_align:
            assert s.storage()[0] % ld_align == 0
        dev = s.tableau()                        # the device expand, copied out as stored
        assert dev.tobytes() == host.tobytes(), "cond_expand differs from the host read-out"
        assert not dev[:, N + 1:].view(np.int64).any(), "padding is not +0.0"
        assert s.set_defer(1) == 0.0             # the path it runs
        ms = s.set_defer(16, condensed=1)
        assert ms > 0.0 and s.condensed and s.storage()[1] == n
        assert s.tableau().tobytes() == host.tobytes(), "cond_pack differs"
        strides.add(s.storage()[0])
        print(f"{m}x{n} ld_align {ld_align}: stored strides {sorted(strides)}, kernel {ms:.4f} ms")


# ---- 3. the round trip the feature is for

@pytest.mark.parametrize("m,n", [(65, 449), (300, 740)])
def test_round_trip_dual_phase_and_back(m, n):
    A, b, c, b2 = D.dense_lp(m, n)
    c2 = R.make_c2(c, D.DENSE_SEED[(m, n)], scale=0.02, holes=False)
    prob = dlp.Problem.dense(A, b, c)
    with _open(prob, "eager") as e:              # a session created eager does the same
        assert e.run(BIG)[0] == L.OK
        e.set_rhs(b2)
        assert e.run(BIG)[0] == L.OK
        dual_blob = S._blob(e.result())
        e.set_objective(c2)
        assert e.run(BIG)[0] == L.OK
        end_blob, end_T = S._blob(e.result()), e.tableau()
    with dlp.Session(prob, small_lp=-1, defer=16, condensed=1) as s:
        assert s.run(BIG)[0] == L.OK
        S._unchanged(s, lambda: s.set_rhs(b2), L.ERR_UNSUPPORTED, "defer")
        np0 = s.status()[1]
        _switch(s, "eager")
        assert s.run(BIG) == (L.OK, 0)
        T0, basis0 = s.tableau(), s.result().basis
        ref = O.resolve_rhs(T0, basis0, n, b2)
        s.set_rhs(b2)
        st, done = s.run(BIG)
        assert st == L.OK and done >= 10
        S._bar(f"{m}x{n} round trip", s, st, np0, ref)
        assert S._blob(s.result()) == dual_blob
        T1 = s.tableau()
        s.set_defer(**K16C)
        _reports(s, K16C)
        assert np.array_equal(s.tableau(), T1)   # (values: the dual phase left -0 in basic columns)
        assert s.run(BIG) == (L.OK, 0)
        s.set_objective(c2)
        assert s.run(BIG)[0] == L.OK
        assert S._blob(s.result()) == end_blob
        assert np.array_equal(s.tableau(), end_T)


# ---- 4. graph windows

@pytest.mark.parametrize("frm,to", [("eager", "k16c"), ("k16c", "eager")])
def test_graph_windows_are_dropped(frm, to):
    m, n = 257, 260
    more = dict(use_graph=1, check_interval=5)
    ref_blob, ref_T = _eager_ref(m, n)
    opts = {"eager": P["eager"], "k16c": K16C}
    for stop in STOPS[(m, n)]:
        with dlp.Session(_prob(m, n), small_lp=-1, **opts[frm], **more) as s:
            assert s.run(stop) == (L.RUNNING, stop)
            T0 = s.tableau()
            s.set_defer(**opts[to])
            assert s.tableau().tobytes() == T0.tobytes()
            assert s.get_defer_tuning()[2] == opts[to]["defer"] and s.condensed == (to == "k16c")
            assert s.run(BIG)[0] == L.OK
            assert S._blob(s.result()) == ref_blob, (frm, to, stop)
            assert s.tableau().tobytes() == ref_T, (frm, to, stop)


# ---- 5. refusals

def _c_call(s, defer, condensed, lookahead):
    def call():
        L.check(L.lib().dlp_session_set_defer(s._h, defer, condensed, lookahead, None), "dlp_session_set_defer")
    return call


def test_refusals_leave_the_session_unchanged():
    m, n = 63, 70
    A, b, c, b2 = D.dense_lp(m, n)
    prob = dlp.Problem.dense(A, b, c)
    gen = dlp.Problem.general(A, np.full(m, -np.inf), b, 0.0, np.inf, -c)
    with dlp.Session(gen) as s:
        s.run(BIG)
        S._unchanged(s, lambda: s.set_defer(16), L.ERR_UNSUPPORTED, "general", tableau=False)
    with dlp.Session(prob, rank=0, nranks=2) as s:
        S._unchanged(s, lambda: s.set_defer(16), L.ERR_UNSUPPORTED, "single-GPU", tableau=False)
    with dlp.Session(prob, small_lp=1) as s:
        assert s.small_lp()
        assert s.run(7) == (L.RUNNING, 7)
        S._unchanged(s, lambda: s.set_defer(16), L.ERR_UNSUPPORTED, "small-LP")
        S._unchanged(s, lambda: s.set_defer(1), L.ERR_UNSUPPORTED, "small-LP")
    for path in ("eager", "k16f", "k4c"):
        with _open(prob, path) as s:
            assert s.run(7) == (L.RUNNING, 7)
            for bad in ((65, 0, -1), (-1, 0, -1), (16, 2, -1), (16, -2, -1), (16, 1, 2), (16, 1, -2)):
                S._unchanged(s, _c_call(s, *bad), L.ERR_ARG)
            cand = s.step_candidate()               # a caller-driven step in progress
            S._unchanged(s, lambda: s.set_defer(1 if path != "eager" else 16), L.ERR_STATE, "step")
            s.step_update(s.step_select(cand))
            _switch(s, "k16f" if path != "k16f" else "eager")   # between steps it is allowed
    with _open(prob, "eager") as s:
        assert s.run(BIG)[0] == L.OK
        s.set_rhs(b2)
        assert s.run(1)[0] == L.RUNNING             # a pending dual phase
        S._unchanged(s, lambda: s.set_defer(16, condensed=1), L.ERR_STATE, "dual")
        assert s.run(BIG)[0] == L.OK                # ended DLP_OK: accepted again
        T1 = s.tableau()
        assert s.set_defer(16, condensed=1) > 0.0
        assert np.array_equal(s.tableau(), T1)
        assert s.run(BIG) == (L.OK, 0)
    with _open(prob, "eager", update_variant=4) as s:   # a 1024-column rank-1 variant
        assert s.run(7) == (L.RUNNING, 7)
        S._unchanged(s, lambda: s.set_defer(16), L.ERR_ARG, "512-column")
        S._unchanged(s, _c_call(s, 65, 2, 2), L.ERR_ARG)


def test_noop_and_optimal_sessions():
    m, n = 63, 70
    prob = _prob(m, n)
    for path in P:
        with _open(prob, path) as s:
            assert s.run(29) == (L.RUNNING, 29)
            before, T0 = S._blob(s.result()), s.tableau().tobytes()
            assert s.set_defer(**P[path]) == 0.0    # the path it runs: nothing touched
            assert S._blob(s.result()) == before and s.tableau().tobytes() == T0
            _reports(s, path)
            assert s.run(BIG)[0] == L.OK
            blob = S._blob(s.result())
            for to in P:                            # an optimal session stays optimal
                if to != path:
                    _switch(s, to)
                    assert s.run(BIG) == (L.OK, 0), (path, to)
                    assert S._blob(s.result()) == blob, (path, to)
            assert blob == _eager_ref(m, n)[0]
