"""GPU parity on the structured LPs of tests/structured_lp.py: exact Dantzig ties (also where the
condensed slot order differs from the variable order), exact ratio ties at a nonzero ratio,
values exactly at the tolerances, subnormal and huge b, signed zeros.

Every comparison is with the oracle (O.solve_dense, reopt_ref.oracle_tableau) and bit for bit:
the pivot log (q, p, leaving, r_p, objective), objective, x, y, the basis, and the whole tableau
at a mid-solve stop that is neither 0 nor a multiple of a block size, and at the end.  The batch
compares x and y with np.array_equal, its documented bar.  That the cases hold the ties they are
here for is asserted on the CPU (tests/test_structured_ref.py).

One exemption, on condensed sessions only: the sign of a zero in a basic column of a read-out
(_same_tableau).  What these LPs caught when they were added: the batched register kernel
skipped the elimination of rows 32..63 whenever row 31 of the entering column was +-0 (sparse
LPs: wrong optima); a deferred pass after an unbounded step, and the lookahead's pass of an empty
block, turned -0.0 entries into +0.0."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
import reopt_ref as R
import structured_lp as S
from conftest import ROOT

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

pytestmark = pytest.mark.gpu

# the option sets of tests/test_gpu_reopt.py::PATHS: name, session options, driven through the
# step API
PATHS = [
    ("eager", dict(defer=1, small_lp=-1), False),
    ("eager_graph5", dict(defer=1, small_lp=-1, use_graph=1, check_interval=5), False),
    ("small_lp", dict(small_lp=1), False),
    ("d4_cond", dict(defer=4, condensed=1), False),
    ("d4_full", dict(defer=4, condensed=-1), False),
    ("d16_cond", dict(defer=16, condensed=1), False),
    ("d16_full", dict(defer=16, condensed=-1), False),
    ("d4_cond_steps", dict(defer=4, condensed=1), True),
    ("d16_full_steps", dict(defer=16, condensed=-1), True),
    ("eager_steps", dict(defer=1, small_lp=-1), True),
    ("d16_la", dict(defer=16, lookahead=1), False),
    ("d16_la_full", dict(defer=16, lookahead=1, condensed=-1), False),
    ("d64_la", dict(defer=64, lookahead=1), False),
]
LOG_CAP = 1024


def _lp(name):
    return S.edge_case(name)[:3] if name in S.EDGE_NAMES else S.session_lp(name)


@functools.lru_cache(maxsize=None)
def _ref(name, pricing=0):
    return O.solve_dense(*_lp(name), pricing=pricing, nthreads=1)


def _oracle_tableau(A, b, c, k, pricing=0):
    """reopt_ref.oracle_tableau, for either pricing."""
    if pricing == 0:
        return R.oracle_tableau(A, b, c, k)
    m, n = A.shape
    e = O.OracleEngine(A, b, c, 0, 1, 0, m, pricing=pricing)
    try:
        for _ in range(k):
            cand = e.step_candidate()
            if e.state != 4:
                break
            bits = e.step_select(cand)
            if e.state != 4:
                break
            e.step_update(bits)
        T = np.zeros((m + 1, e.ld))
        O.lib().oracle_slice_tableau(e.h, O._d(T))
        return T, R.basis_from_log(m, n, e.log())
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def _ref_tableau(name, k, pricing=0):
    T, basis = _oracle_tableau(*_lp(name), k, pricing)
    T.setflags(write=False)
    return T, basis


def _stop(num_pivots):
    """An odd pivot count about half way (no multiple of a block size 4, 16 or 64)."""
    return (num_pivots // 2) | 1 if num_pivots >= 2 else num_pivots


def _same_log(got, ref, tag):
    assert len(got) == len(ref), (tag, len(got), len(ref))
    g, r = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if g.tobytes() != r.tobytes():
        for k in range(len(r)):
            if g[k].tobytes() != r[k].tobytes():
                raise AssertionError(f"{tag}: pivot {k}: gpu {g[k]} oracle {r[k]}")


def _same_result(res, ref, tag):
    assert res.status == ref.status, (tag, res.status, ref.status)
    _same_log(res.pivot_log, ref.pivot_log, tag)
    assert res.num_pivots == ref.num_pivots, tag
    assert np.float64(res.objective).tobytes() == np.float64(ref.objective).tobytes(), \
        (tag, res.objective, ref.objective)
    for what, a, r in (("x", res.x, ref.x), ("y", res.y, ref.y)):
        bad = np.flatnonzero(S.bits(a) != S.bits(r))
        assert len(bad) == 0, f"{tag}: {what} differs at {bad[:8]}: {a[bad[:8]]} vs {r[bad[:8]]}"
    assert res.basis.tobytes() == ref.basis.tobytes(), tag


def _same_tableau(T, Tref, basis, tag, condensed=False):
    """Bit for bit.  A condensed session's read-out rebuilds the basic columns as unit vectors,
    where the full tableau may keep a -0.0 the rule left untouched (include/dlp.h,
    dlp_options.condensed): those columns are compared as values."""
    assert T.shape == Tref.shape, (tag, T.shape, Tref.shape)
    bad = S.tableau_diff(T, Tref)
    if condensed and len(bad):
        assert np.array_equal(T[:, basis], Tref[:, basis]), f"{tag}: a basic column differs in value"
        bad = bad[~np.isin(bad[:, 1], basis)]
    if len(bad):
        in_basic = np.isin(bad[:, 1], basis)
        zero = (T[bad[:, 0], bad[:, 1]] == 0.0) & (Tref[bad[:, 0], bad[:, 1]] == 0.0)
        i, j = bad[0]
        raise AssertionError(
            f"{tag}: {len(bad)} entries differ ({int((in_basic & zero).sum())} are the sign of a zero in "
            f"a basic column, {int((~in_basic & zero).sum())} the sign of a zero elsewhere); first at "
            f"({i}, {j}): gpu {T[i, j]!r} oracle {Tref[i, j]!r}")


def _steps(s, k):
    for _ in range(k):
        s.step_update(s.step_select(s.step_candidate()))


def _session_paths(name, pricing=0):
    """Every path: k pivots, the whole tableau and the state against the oracle's; then to the
    end, the result and the final tableau against the oracle's."""
    A, b, c = _lp(name)
    m, n = A.shape
    ref = _ref(name, pricing)
    k = _stop(ref.num_pivots)
    Tk, basis_k = _ref_tableau(name, k, pricing)
    Tend, basis_end = _ref_tableau(name, ref.num_pivots, pricing)
    assert basis_end.tobytes() == ref.basis.tobytes()
    prob = dlp.Problem.dense(A, b, c)
    for pname, opts, steps in PATHS:
        if pname == "d64_la" and m != 300:
            continue
        tag = f"{name} pricing {pricing} {pname}"
        with dlp.Session(prob, pricing=pricing, **opts) as s:
            assert s.lookahead() == (opts.get("lookahead") == 1), tag
            if pname == "small_lp":
                assert s.small_lp(), tag
            if "condensed" in opts:
                assert s.condensed == (opts["condensed"] == 1), tag
            if steps:
                _steps(s, k)
            else:
                s.run(k)
            mid = s.result()
            assert mid.num_pivots == k, (tag, mid.num_pivots, k)
            _same_log(mid.pivot_log, ref.pivot_log[:k], tag)
            assert mid.basis.tobytes() == basis_k.tobytes(), tag
            _same_tableau(s.tableau(), Tk, basis_k, f"{tag} after {k} pivots", s.condensed)
            st, _ = s.run(10 ** 6)
            assert st == ref.status, (tag, st, ref.status)
            _same_result(s.result(), ref, tag)
            _same_tableau(s.tableau(), Tend, basis_end, f"{tag} at the end", s.condensed)
    print(f"{name} pricing {pricing}: {ref.num_pivots} pivots, stop at {k}, status {ref.status}, "
          f"objective {ref.objective!r}")


# ---- sessions
@pytest.mark.parametrize("name", list(S.SESSION_INTERVAL) + list(S.DUP))
def test_session_paths_tied_lps(name):
    _session_paths(name)


@pytest.mark.parametrize("name", S.EDGE_NAMES)
def test_session_paths_edge_cases(name):
    _session_paths(name)
    exp, ref = S.edge_case(name)[3], _ref(name)
    assert ref.status == exp["status"] and ref.num_pivots == exp.get("num_pivots", ref.num_pivots)


def test_session_paths_bland_always():
    _session_paths("iv300x520_s0", pricing=1)


# ---- row-block ranks on one GPU, the host doing the exchanges
@pytest.mark.parametrize("P,K", [(2, 0), (3, 0), (8, 0), (8, 16)])   # K = 0: the default (eager)
def test_rank_sessions_one_gpu(P, K):
    name = "iv300x520_s0"
    A, b, c = _lp(name)
    m, n = A.shape
    ref = _ref(name)
    k0 = _stop(ref.num_pivots)
    Tk, basis_k = _ref_tableau(name, k0)
    Tend, _ = _ref_tableau(name, ref.num_pivots)
    prob = dlp.Problem.dense(A, b, c)
    sess = [dlp.Session(prob, rank=r, nranks=P, **(dict(defer=K) if K else {})) for r in range(P)]
    try:
        assert all(s.update_stats()[2] == (K or 1) for s in sess)
        assert sum(s.rows for s in sess) == m
        if P == 8:   # ratio ties whose rows lie on different ranks
            first = np.array([s.row_first for s in sess[1:]])
            ties = S.tie_stats(A, b, c).ratio_tie_rows
            assert sum(len(set(np.searchsorted(first, rows, side="right"))) > 1 for rows in ties) >= 3

        def stacked():
            tabs = [s.tableau() for s in sess]
            assert all(t[-1].tobytes() == tabs[0][-1].tobytes() for t in tabs)
            return np.concatenate([t[:-1] for t in tabs] + [tabs[0][-1:]])

        status = L.RUNNING
        for it in range(10_000):
            if it == k0:
                _same_tableau(stacked(), Tk, basis_k, f"P = {P} after {k0} pivots", sess[0].condensed)
            cands = np.concatenate([s.step_candidate() for s in sess])
            st, _ = sess[0].status()
            if st != L.RUNNING:
                status = st
                break
            sends = [s.step_select(cands) for s in sess]
            prow = np.max(np.stack(sends), axis=0)
            for s in sess:
                s.step_update(prow)
        assert status == L.OK
        results = [s.result() for s in sess]
        for r in results:
            _same_log(r.pivot_log, ref.pivot_log, f"P = {P}")
            assert np.float64(r.objective).tobytes() == np.float64(ref.objective).tobytes()
            assert r.y.tobytes() == ref.y.tobytes()
        x = np.sum([r.x for r in results], axis=0)   # each basic row lives on one rank
        assert x.tobytes() == ref.x.tobytes()
        _same_result(dlp.Session.merged_result(sess[::-1]), ref, f"P = {P} merged")
        _same_tableau(stacked(), Tend, ref.basis, f"P = {P} at the end", sess[0].condensed)
    finally:
        for s in sess:
            s.close()


# ---- the small-LP launch on 16 and 64 workgroups.  The knob is read once per process, so each
# setting runs in a child process, which compares with the oracle itself.
CLUSTER_SCRIPT = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import oracle_py as O
import reopt_ref as R
import structured_lp as S
import distributedlpsolver_amd as dlp

name, k = sys.argv[2], int(sys.argv[3])
A, b, c = S.session_lp(name)
ref = O.solve_dense(A, b, c, nthreads=1)
Tk, basis_k = R.oracle_tableau(A, b, c, k)
Tend, _ = R.oracle_tableau(A, b, c, ref.num_pivots)
same = lambda a, r: np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(r).tobytes()
out = {}
with dlp.Session(dlp.Problem.dense(A, b, c), small_lp=1) as s:
    out["small_lp"] = s.small_lp()
    s.run(k)
    mid = s.result()
    out["mid pivots"] = mid.num_pivots == k
    out["mid basis"] = same(mid.basis, basis_k)
    out["mid tableau"] = len(S.tableau_diff(s.tableau(), Tk)) == 0
    st, _ = s.run(10 ** 6)
    r = s.result()
    out["end tableau"] = len(S.tableau_diff(s.tableau(), Tend)) == 0
out["status"] = bool(st == ref.status == 0 and r.status == 0)
out["pivots"] = r.num_pivots == ref.num_pivots
out["log"] = same(r.pivot_log, ref.pivot_log)
out["objective"] = same(np.float64(r.objective), np.float64(ref.objective))
out["x"], out["y"], out["basis"] = same(r.x, ref.x), same(r.y, ref.y), same(r.basis, ref.basis)
print(json.dumps(out))
"""


@pytest.mark.parametrize("wg", ["16", "64"])   # slices of 52 / 13 columns fit the LDS
def test_small_lp_launch_workgroups(wg):
    name = "iv300x520_s0"
    env = dict(os.environ)
    env["DLP_CLUSTER_WG"] = wg
    p = subprocess.run([sys.executable, "-c", CLUSTER_SCRIPT, ROOT, name, str(_stop(_ref(name).num_pivots))],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(out) == 12 and all(out.values()), out


# ---- the batch: six LPs per call, every LP against the oracle
def _batch_same_lp(res, k, ref, tag):
    assert res.status[k] == ref.status, (tag, k, res.status[k], ref.status)
    assert res.num_pivots[k] == ref.num_pivots, (tag, k, res.num_pivots[k], ref.num_pivots)
    assert np.float64(res.objective[k]).tobytes() == np.float64(ref.objective).tobytes(), \
        (tag, k, res.objective[k], ref.objective)
    assert res.basis[k].tobytes() == ref.basis.tobytes(), (tag, k)
    assert ref.num_pivots <= LOG_CAP
    _same_log(res.logs[k][:ref.num_pivots], ref.pivot_log, f"{tag} LP {k}")
    assert np.array_equal(res.x[k], ref.x), (tag, k, np.flatnonzero(res.x[k] != ref.x)[:8])
    assert np.array_equal(res.y[k], ref.y), (tag, k, np.flatnonzero(res.y[k] != ref.y)[:8])


def _batch(lps, register, tag):
    m, n = lps[0][0].shape
    assert dlp.batched_occupancy(m, n)["register_kernel"] == register, tag
    res = dlp.batched_solve_dense(np.stack([p[0] for p in lps]), np.stack([p[1] for p in lps]),
                                  np.stack([p[2] for p in lps]), want_basis=True, log_cap=LOG_CAP)
    refs = [O.solve_dense(*p, nthreads=1) for p in lps]
    for k, ref in enumerate(refs):
        _batch_same_lp(res, k, ref, tag)
    return refs


@pytest.mark.parametrize("m,n", list(S.BATCH_REGISTER) + list(S.BATCH_LDS))
def test_batch_interval(m, n):
    refs = _batch([S.batch_lp(m, n, k) for k in range(S.NLP)], (m, n) in S.BATCH_REGISTER, f"interval {m}x{n}")
    assert all(r.status == L.OK for r in refs)


@pytest.mark.parametrize("m,n", list(S.BATCH_DUP))
def test_batch_dup(m, n):
    refs = _batch([S.batch_dup_lp(m, n, k) for k in range(S.NLP)], m == 64, f"dup {m}x{n}")
    assert all(r.status == L.OK for r in refs)


@pytest.mark.parametrize("m,n", [S.EDGE_SMALL, S.EDGE_BIG])
def test_batch_edge_cases_among_ordinary_lps(m, n):
    lps = [S.edge_case(name)[:3] for name in S.EDGE_NAMES if name.endswith(f"_{m}x{n}")]
    assert len(lps) == 9
    lps[2:2] = [O.gen_dense(m, n, 31)]
    lps.append(O.gen_dense(m, n, 32))
    refs = _batch(lps, m == 64, f"edge cases {m}x{n}")
    assert {r.status for r in refs} == {L.OK, L.UNBOUNDED}


# ---- warm re-solve with a tied objective
def test_warm_resolve_tied_objective():
    name, k = "iv300x520_s0", 70
    A, b, c = _lp(name)
    m, n = A.shape
    N = n + m
    c2 = np.random.default_rng(77).integers(1, 3, n).astype(np.float64)
    ref2 = O.solve_dense(A, b, c2, nthreads=1)
    prob = dlp.Problem.dense(A, b, c)
    base = None
    for pname, opts, _ in [p for p in PATHS if p[0] in ("eager", "small_lp", "d4_cond", "d16_cond", "d16_full",
                                                        "d16_la", "d64_la")]:
        with dlp.Session(prob, **opts) as s:
            s.run(k)
            T0, basis0 = s.tableau(), s.result().basis
            s.set_objective(c2)
            assert s.status() == (L.RUNNING, k), pname
            T1 = s.tableau()
            assert T1[:m].tobytes() == T0[:m].tobytes(), f"{pname}: a constraint row changed"
            zref = R.objective_row(T0[:m], basis0, c2)
            bad = np.flatnonzero(S.bits(T1[m]) != S.bits(zref))
            assert len(bad) == 0, f"{pname}: objective row differs at columns {bad[:8]}: " \
                                  f"{T1[m][bad[:8]]} vs {zref[bad[:8]]}"
            z = zref[:N]
            assert z.min() < -1e-9 and (z == z.min()).sum() > 1   # tied again
            want_status, want_more = R.simplex_continue(T1[:, :N + 1].copy(), basis0, n)
            st, more = s.run(10 ** 6)
            res = s.result()
        assert st == want_status == L.OK and res.status == L.OK, pname
        assert more == want_more and res.num_pivots == k + more, (pname, more, want_more)
        assert res.pivot_log[k]["q"] == int(np.argmin(z)), pname
        assert res.objective == ref2.objective, (pname, res.objective, ref2.objective)   # exact arithmetic
        blob = (res.status, res.num_pivots, np.float64(res.objective).tobytes(), res.x.tobytes(), res.y.tobytes(),
                res.basis.tobytes(), np.ascontiguousarray(res.pivot_log).tobytes())
        if base is None:
            base = blob
        else:
            assert blob == base, f"{pname} differs from the eager path"
    assert ref2.status == L.OK
