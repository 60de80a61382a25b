"""GPU: the resident batch (dlp.Batch / dlp_batch_*): thousands of small LPs kept on the device
and re-optimised from each LP's basis after new objectives.

Reference for the warm continuation: the single-LP eager session
``Session(Problem.dense(A_k, b_k, c_k), defer=1, small_lp=-1)`` driven through the same
sequence (run, set_objective, run); that path is itself pinned to tests/reopt_ref.py and the
oracle by tests/test_gpu_reopt.py.  Where a cold solve suffices the reference is the CPU oracle.

Bar, as in tests/test_gpu_batched_dense.py: status, pivot count, basis, objective and every
pivot-log entry are bit-identical; x, y and tableau read-outs are equal as values
(np.array_equal: the sign of a zero is exempt, the condensed tableau's own exemption)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
import reopt_ref as R
import test_gpu_batched_dense as BD
from conftest import ROOT

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

pytestmark = pytest.mark.gpu

LOG_CAP = BD.LOG_CAP
NLP = 6
BIG = 10 ** 6
EAGER = dict(defer=1, small_lp=-1)
KW = dict(want_basis=True, log_cap=LOG_CAP)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _lps(m, n, seed, degen=False, nlp=NLP):
    return [BD._gen(m, n, seed + k, degen) for k in range(nlp)]


@functools.lru_cache(maxsize=None)
def _c2(m, n, seed, degen, k, rnd=0):
    c2 = R.make_c2(BD._gen(m, n, seed + k, degen)[2], 31 * rnd + seed + k)
    c2.setflags(write=False)
    return c2


def _stop(m, n, seed, degen, pricing=0, nlp=NLP):
    """A pivot budget that stops every LP of the batch strictly inside its cold solve where it
    has one of at least two pivots: half the shortest oracle solve, at least 1."""
    return max(1, min(BD._gen_ref(m, n, seed + k, degen, pricing).num_pivots for k in range(nlp)) // 2)


class _Sess:
    """The reference: one eager session per LP, snapshotted after every run."""

    def __init__(self, A, b, c, **opts):
        self.s = dlp.Session(dlp.Problem.dense(A, b, c), **EAGER, **opts)
        self.np0 = 0

    def run(self, budget):
        st, done = self.s.run(budget)
        res = self.s.result()
        assert res.num_pivots == self.np0 + done
        snap = dict(status=L.PIVOT_LIMIT if st == L.RUNNING else st, done=done, objective=res.objective,
                    x=res.x, y=res.y, basis=res.basis, log=res.pivot_log[self.np0:])
        self.np0 = res.num_pivots
        return snap

    def set(self, c):
        self.s.set_objective(c)

    def tableau(self):
        return self.s.tableau()

    def close(self):
        self.s.close()


def _same_run(res, k, snap, what=""):
    """LP k of one batch call against the session's run of the same step."""
    tag = f"{what} LP {k}"
    assert res.status[k] == snap["status"], (tag, res.status[k], snap["status"])
    assert res.num_pivots[k] == snap["done"], (tag, res.num_pivots[k], snap["done"])
    assert np.float64(res.objective[k]).tobytes() == np.float64(snap["objective"]).tobytes(), \
        (tag, res.objective[k], snap["objective"])
    np.testing.assert_array_equal(res.basis[k], snap["basis"], err_msg=tag)
    cnt = min(snap["done"], LOG_CAP)
    got, want = np.ascontiguousarray(res.logs[k][:cnt]), np.ascontiguousarray(snap["log"][:cnt])
    if got.tobytes() != want.tobytes():
        for i in range(cnt):
            assert got[i].tobytes() == want[i].tobytes(), f"{tag} pivot {i}: batch {got[i]} session {want[i]}"
    assert np.array_equal(res.x[k], snap["x"]), (tag, np.flatnonzero(res.x[k] != snap["x"])[:8])
    assert np.array_equal(res.y[k], snap["y"]), (tag, np.flatnonzero(res.y[k] != snap["y"])[:8])


def _is_rejected(res, k, m, n, basis=None):
    assert res.status[k] == L.ERR_ARG and res.num_pivots[k] == 0, (k, res.status[k])
    assert np.isnan(res.objective[k]) and np.isnan(res.x[k]).all() and np.isnan(res.y[k]).all(), k
    np.testing.assert_array_equal(res.basis[k], n + np.arange(m) if basis is None else basis)


# ---- 1. the rule in isolation
@pytest.mark.parametrize("m,n", [(64, 130), (37, 53)], ids=["register", "lds"])
def test_objective_rows_follow_the_rule(m, n):
    seed = 3100 + n
    lps = _lps(m, n, seed)
    k = _stop(m, n, seed, False)
    assert 0 < k < min(BD._gen_ref(m, n, seed + j).num_pivots for j in range(NLP))
    N = n + m
    with dlp.Batch(*BD._stack(lps), max_pivots=k, **KW) as bt:
        assert bt.info() == dict(nlp=NLP, m=m, n=n, register_kernel=m == 64,
                                 device_bytes=bt.info()["device_bytes"]) and bt.info()["device_bytes"] > 0
        assert (bt.result.status == L.PIVOT_LIMIT).all() and (bt.result.num_pivots == k).all()
        before = [bt.read(j) for j in range(NLP)]
        c2 = np.stack([_c2(m, n, seed, False, j) for j in range(NLP)])
        assert (c2[:, ::7] == 0.0).all() and (c2[:, 11] < 0.0).all()   # skipped rows, a -0.0 start
        res = bt.resolve(c2, max_pivots=0, **KW)
        assert (res.status == L.PIVOT_LIMIT).all() and (res.num_pivots == 0).all()
        for j in range(NLP):
            T0, basis0 = before[j]
            T1, basis1 = bt.read(j)
            assert T0.shape == (m + 1, dlp.tableau_ld(m, n))
            assert basis1.tobytes() == basis0.tobytes() == bt.result.basis[j].tobytes(), j
            assert T1[:m].tobytes() == T0[:m].tobytes(), f"LP {j}: a constraint row changed"
            # the full layout: basic columns exact unit vectors with objective entry +0.0, padding +0.0
            assert np.array_equal(T1[:m, basis1], np.eye(m)) and not _bits(T1[m, basis1]).any()
            assert not _bits(T1[:, N + 1:]).any()
            zref = R.objective_row(T0[:m], basis0, c2[j])
            bad = np.nonzero(_bits(T1[m]) != _bits(zref))[0]
            assert len(bad) == 0, f"LP {j}: objective row differs at columns {bad[:8]}: " \
                                  f"{T1[m][bad[:8]]} vs {zref[bad[:8]]}"
            assert np.float64(res.objective[j]).tobytes() == np.float64(T1[m, N]).tobytes()


# ---- 2. warm re-solve against the eager session, from the optimum and from a stop at k pivots
def _warm(m, n, seed, degen, pricing, stop):
    lps = _lps(m, n, seed, degen)
    k = _stop(m, n, seed, degen, pricing) if stop else BIG
    c2 = np.stack([_c2(m, n, seed, degen, j) for j in range(NLP)])
    with dlp.Batch(*BD._stack(lps), max_pivots=k, pricing=pricing, **KW) as bt:
        assert bt.info()["register_kernel"] == dlp.batched_occupancy(m, n)["register_kernel"]
        r1 = bt.resolve(c2, max_pivots=BIG, **KW)
        tabs = [bt.read(j)[0] for j in range(NLP)]
        r0 = bt.result
    for j, (A, b, c) in enumerate(lps):
        s = _Sess(A, b, c, pricing=pricing)
        try:
            _same_run(r0, j, s.run(k), "cold")
            s.set(c2[j])
            _same_run(r1, j, s.run(BIG), "warm")
            assert np.array_equal(tabs[j], s.tableau()), f"LP {j}: tableau"
        finally:
            s.close()
    return r0, r1


REG_N = [1, 64, 65, 128, 130, 192]           # 1, 2, 3 waves per LP, exact boundaries, idle last waves
LDS_SHAPES = [(1, 1), (5, 7), (37, 53), (65, 30), (64, 200)]
ONE_ROW_GROUP = (6, 300)                     # n + 1 past the 256-lane workgroup: one row group


def _lds_bytes(m, n):
    return 8 * ((m + 1) * (n + 1) + (m + 1) + (n + 1)) + 4 * (n + m + 8) + 8 * 2 + 16


def _cases(shapes, one_pivot):
    """shape x family x (from the optimum, from a stop); a one-pivot LP has no pivot count
    strictly inside its solve, so its shape runs from the optimum only."""
    return [pytest.param(sh, degen, stop, id=f"{sh}-{'degenerate' if degen else 'dense'}-"
                                             f"{'stopped' if stop else 'optimum'}")
            for sh in shapes for degen in (False, True) for stop in (False, True)
            if not (stop and sh == one_pivot)]


@pytest.mark.parametrize("n,degen,stop", _cases(REG_N, 1))
def test_warm_resolve_register_kernel(n, degen, stop):
    assert dlp.batched_occupancy(64, n)["register_kernel"]
    _warm(64, n, 3300 + n, degen, 0, stop)


@pytest.mark.parametrize("shape,degen,stop", _cases(LDS_SHAPES + [ONE_ROW_GROUP], (1, 1)))
def test_warm_resolve_lds_kernel(shape, degen, stop):
    m, n = shape
    assert not dlp.batched_occupancy(m, n)["register_kernel"]
    if (m, n) == ONE_ROW_GROUP:
        assert _lds_bytes(m, n) <= 40 * 1024 and n + 1 > 256   # 256 lanes, and it fits 160 KiB
    assert _lds_bytes(m, n) <= 160 * 1024
    _warm(m, n, 3500 + m + n, degen, 0, stop)


@pytest.mark.parametrize("m,n", [(64, 130), (37, 53)], ids=["register", "lds"])
def test_warm_resolve_bland(m, n):
    """DLP_PRICING_BLAND on one shape per kernel (the default mode runs everywhere above): the
    Bland state is reset to Bland, not to Dantzig."""
    r0, r1 = _warm(m, n, 3700 + n, m != 64, 1, True)   # (degenerate where Bland's solve stays short)
    assert (r1.status == L.OK).all() and r1.num_pivots.all()


# ---- 3. the loop itself: three re-solves in a row
@pytest.mark.parametrize("m,n", [(64, 100), (37, 53)], ids=["register", "lds"])
def test_three_resolves_in_a_row(m, n):
    seed = 3900 + n
    lps = _lps(m, n, seed)
    rounds = [np.stack([_c2(m, n, seed, False, j, 1) for j in range(NLP)]),
              np.array(_c2(m, n, seed, False, 0, 2)),                        # one (n,) c for all: stride 0
              np.stack([_c2(m, n, seed, False, j, 3) for j in range(NLP)])]
    with dlp.Batch(*BD._stack(lps), **KW) as bt:
        res = [bt.result] + [bt.resolve(c, **KW) for c in rounds]
    assert sum(int(r.num_pivots.sum()) for r in res[1:]) > 0
    for j, (A, b, c) in enumerate(lps):
        s = _Sess(A, b, c)
        try:
            _same_run(res[0], j, s.run(BIG), "cold")
            for t, c in enumerate(rounds):
                s.set(c if c.ndim == 1 else c[j])
                _same_run(res[t + 1], j, s.run(BIG), f"round {t}")
        finally:
            s.close()


# A device-tensor c gives the bytes of the host-array call.  In a child process: torch brings
# its own HIP runtime, which has to be the one the process loads first (see
# tests/test_gpu_batched_dense.py).
DEVICE_SCRIPT = r"""
import json, sys
import torch
torch.cuda.init()
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import oracle_py as O
import reopt_ref as R
import distributedlpsolver_amd as dlp

KW = dict(want_basis=True, log_cap=512)

def same(r1, r2):
    ok = all(getattr(r1, f).tobytes() == getattr(r2, f).tobytes()
             for f in ("status", "num_pivots", "objective", "basis", "x", "y"))
    return ok and all(r1.logs[k][:r1.num_pivots[k]].tobytes() == r2.logs[k][:r1.num_pivots[k]].tobytes()
                      for k in range(len(r1.status)))

def raises(f, *args):
    try:
        f(*args)
    except ValueError:
        return True
    return False

out = {}
for m, n in ((64, 100), (37, 53)):
    lps = [O.gen_dense(m, n, 4100 + k) for k in range(6)]
    A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
    c1 = np.stack([R.make_c2(c[k], 50 + k) for k in range(6)])
    c2 = R.make_c2(c[0], 60)
    c3 = np.stack([R.make_c2(c[k], 70 + k) for k in range(6)])
    c3[4, 3] = np.nan   # the kernel's check sees device inputs too
    with dlp.Batch(A, b, c, **KW) as host, dlp.Batch(*(torch.from_numpy(v).to("cuda:0") for v in (A, b, c)), **KW) as dev:
        ok = same(host.result, dev.result)
        for cc in (c1, c2, c3):
            tc = torch.from_numpy(cc).to("cuda:0")
            rh, rd = host.resolve(cc, **KW), dev.resolve(tc, **KW)
            ok = ok and same(rh, rd) and int(rh.num_pivots.sum()) > 0
            ok = ok and all(host.read(k)[0].tobytes() == dev.read(k)[0].tobytes() for k in range(6))
        out[f"{m}x{n} device c"] = bool(ok)
        out[f"{m}x{n} nan seen"] = bool(rd.status[4] == -1 and (np.delete(rd.status, 4) == 0).all())
        view = torch.from_numpy(np.ascontiguousarray(c1.T)).to("cuda:0").T   # has to be made contiguous
        out[f"{m}x{n} view"] = (not view.is_contiguous()) and same(host.resolve(c1, **KW), dev.resolve(view, **KW))
        out[f"{m}x{n} float32 raises"] = raises(dev.resolve, tc.float())
        out[f"{m}x{n} cpu tensor raises"] = raises(dev.resolve, tc.cpu())
print(json.dumps(out))
"""


def test_device_c_gives_the_host_bytes():
    p = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT, ROOT], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(out) == 10 and all(out.values()), out


# ---- 4. before any pivot: the oracle's cold solve of c2
@pytest.mark.parametrize("m,n", [(64, 100), (37, 53)], ids=["register", "lds"])
def test_before_any_pivot_equals_the_cold_solve(m, n):
    seed = 4300 + n
    lps = _lps(m, n, seed)
    c2 = np.stack([_c2(m, n, seed, False, j) for j in range(NLP)])
    with dlp.Batch(*BD._stack(lps), max_pivots=0, **KW) as bt:
        assert (bt.result.status == L.PIVOT_LIMIT).all() and not bt.result.num_pivots.any()
        res = bt.resolve(c2, max_pivots=BIG, **KW)
    for j, (A, b, c) in enumerate(lps):
        BD._same_lp(res, j, BD._ref(A, b, c2[j]))


# ---- 5. resume without a new objective: the uninterrupted cold solve
@pytest.mark.parametrize("m,n", [(64, 100), (37, 53)], ids=["register", "lds"])
def test_resume_continues_the_cold_solve(m, n):
    seed = 4500 + n
    lps = _lps(m, n, seed, True)
    k = _stop(m, n, seed, True)
    refs = [BD._gen_ref(m, n, seed + j, True) for j in range(NLP)]
    assert any(r.num_pivots > k for r in refs)
    # some LP enters Bland mode at or before the stop and leaves the stop in it, or the saved flag is not exercised
    assert any(r.num_pivots > k and r.pivot_log[k - 1]["ratio"] == 0.0 for r in refs)
    with dlp.Batch(*BD._stack(lps), max_pivots=k, **KW) as bt:
        r0 = bt.result
        r1 = bt.resolve(None, max_pivots=BIG, **KW)
        r2 = bt.resolve(None, max_pivots=BIG, **KW)
    for j, ref in enumerate(refs):
        assert r0.num_pivots[j] + r1.num_pivots[j] == ref.num_pivots, j
        assert r1.status[j] == ref.status == L.OK
        log = np.concatenate([r0.logs[j][:r0.num_pivots[j]], r1.logs[j][:r1.num_pivots[j]]])
        assert log.tobytes() == np.ascontiguousarray(ref.pivot_log).tobytes(), j
        assert np.float64(r1.objective[j]).tobytes() == np.float64(ref.objective).tobytes()
        np.testing.assert_array_equal(r1.basis[j], ref.basis)
        assert np.array_equal(r1.x[j], ref.x) and np.array_equal(r1.y[j], ref.y)
    assert (r2.status == L.OK).all() and not r2.num_pivots.any()
    for f in ("objective", "basis", "x", "y"):
        assert getattr(r2, f).tobytes() == getattr(r1, f).tobytes(), f


# ---- 6. one batch with every status
@pytest.mark.parametrize("m,n", [(64, 100), (37, 53)], ids=["register", "lds"])
def test_every_status_in_one_batch(m, n):
    seed = 4700 + m
    lps, kinds = BD._mixed_batch(m, n, seed)
    nlp = len(lps)
    rejected = [j for j, kd in enumerate(kinds) if kd in ("negative b", "nan b")]
    unb = kinds.index("unbounded")
    nan_lp, inf_lp = nlp - 1, kinds.index("degenerate")   # a normal and a degenerate LP get a bad c_k
    ca = np.stack([R.make_c2(lp[2], seed + 10 + j) for j, lp in enumerate(lps)])
    ca[unb] = -np.abs(lps[unb][2])   # bounds the unbounded LP
    bad = ca.copy()
    bad[nan_lp, n // 3] = np.nan
    bad[inf_lp, 0] = -np.inf
    cb = np.stack([R.make_c2(lp[2], seed + 30 + j) for j, lp in enumerate(lps)])
    with dlp.Batch(*BD._stack(lps), **KW) as bt:
        r0 = bt.result
        before = {j: bt.read(j) for j in (nan_lp, inf_lp)}
        ra = bt.resolve(bad, **KW)
        for j in (nan_lp, inf_lp):   # this call only, nothing stored
            _is_rejected(ra, j, m, n, basis=r0.basis[j])
            T, basis = bt.read(j)
            assert T.tobytes() == before[j][0].tobytes() and basis.tobytes() == before[j][1].tobytes()
        rb = bt.resolve(cb, **KW)
        rn = bt.resolve(None, **KW)
    assert r0.status[unb] == L.UNBOUNDED and ra.status[unb] == L.OK
    for j, (A, b, c) in enumerate(lps):
        if j in rejected:
            for r in (r0, ra, rb, rn):
                _is_rejected(r, j, m, n)
            continue
        s = _Sess(A, b, c)
        try:
            _same_run(r0, j, s.run(BIG), "cold")
            if j not in (nan_lp, inf_lp):   # (their sessions never see the bad call)
                s.set(ca[j])
                _same_run(ra, j, s.run(BIG), "round a")
            s.set(cb[j])
            snap = s.run(BIG)
            _same_run(rb, j, snap, "round b")
        finally:
            s.close()
        assert rn.status[j] == rb.status[j] and rn.num_pivots[j] == 0
        assert rn.objective[j].tobytes() == rb.objective[j].tobytes() and rn.x[j].tobytes() == rb.x[j].tobytes()
    assert {int(v) for v in r0.status} == {L.OK, L.UNBOUNDED, L.ERR_ARG}


# ---- 7. m = 64 through the LDS kernel gives the register kernel's bytes
KNOB_SCRIPT = r"""
import hashlib, json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import oracle_py as O
import reopt_ref as R
import distributedlpsolver_amd as dlp

def h(*arrays):
    d = hashlib.sha256()
    for a in arrays:
        d.update(np.ascontiguousarray(a).tobytes())
    return d.hexdigest()

def digest(r):
    logs = [r.logs[k][:r.num_pivots[k]] for k in range(len(r.status))]
    return h(r.status, r.num_pivots, r.objective, r.basis, r.x, r.y, *logs)

m, n, seed, nlp = 64, 100, 4900, 6
KW = dict(want_basis=True, log_cap=512)
lps = [O.gen_dense(m, n, seed + k, k % 2 == 1) for k in range(nlp)]
A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
c2 = np.stack([R.make_c2(c[k], seed + k) for k in range(nlp)])
out = {}
for name, k in (("optimum", 10 ** 6), ("stopped", int(sys.argv[2]))):
    with dlp.Batch(A, b, c, max_pivots=k, **KW) as bt:
        out["register_kernel"] = bt.info()["register_kernel"]
        r1 = bt.resolve(c2, max_pivots=10 ** 6, **KW)
        out[name] = [digest(bt.result), digest(r1), h(*(bt.read(j)[0] + 0.0 for j in range(nlp))),
                     int(bt.result.num_pivots.sum()), int(r1.num_pivots.sum())]
print(json.dumps(out))
"""


def test_m64_through_the_lds_kernel():
    """(read() + 0.0 in the digest: the sign of a zero is the condensed tableau's exemption, and
    the two kernels build the entering slot's zeros by different instructions.)"""
    k = max(1, min(O.solve_dense(*O.gen_dense(64, 100, 4900 + j, j % 2 == 1), nthreads=1).num_pivots
                   for j in range(6)) // 2)

    def run(env):
        e = dict(os.environ)
        e.pop("DLP_BATCH_LDS", None)
        e.update(env)
        p = subprocess.run([sys.executable, "-c", KNOB_SCRIPT, ROOT, str(k)], env=e, capture_output=True,
                           text=True, timeout=240)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads(p.stdout.strip().splitlines()[-1])

    reg, lds = run({}), run({"DLP_BATCH_LDS": "1"})
    assert reg.pop("register_kernel") is True and lds.pop("register_kernel") is False
    assert reg["optimum"][3] > 0 and reg["optimum"][4] > 0 and reg["stopped"][3] == 6 * k
    assert reg == lds


# ---- 8. the one-shot path is untouched
@pytest.mark.parametrize("m,n", [(64, 128), (37, 53)], ids=["register", "lds"])
def test_one_shot_path_gives_the_batch_bytes(m, n):
    lps, _ = BD._mixed_batch(m, n, 5100 + m)
    arrays = BD._stack(lps)
    one = dlp.batched_solve_dense(*arrays, **KW)
    with dlp.Batch(*arrays, **KW) as bt:
        BD._same_bytes(one, bt.result)
        assert bt.info()["device_bytes"] >= 8 * len(lps) * (m + 1) * (n + 1)
        BD._same_bytes(one, dlp.batched_solve_dense(*arrays, **KW))   # beside a live resident batch
        # the state belongs to the handle: releasing the cached contexts leaves it alone
        assert dlp.release_cached_memory(0) > 0
        again = bt.resolve(None, **KW)
        assert not again.num_pivots.any() and again.status.tobytes() == one.status.tobytes()
        for f in ("objective", "basis", "x", "y"):
            assert getattr(again, f).tobytes() == getattr(one, f).tobytes(), f
    BD._same_bytes(one, dlp.batched_solve_dense(*arrays, **KW))


# ---- call-level errors are found before anything is enqueued and leave the batch unchanged
def test_call_level_errors_leave_the_batch_unchanged():
    m, n = 37, 53
    lps = _lps(m, n, 5300)
    c2 = np.stack([_c2(m, n, 5300, False, j) for j in range(NLP)])
    lib = L.lib()
    with dlp.Batch(*BD._stack(lps), max_pivots=5, **KW) as bt:
        before = [bt.read(j) for j in range(NLP)]
        out, bad_log = L.BatchOut(), L.BatchOut()
        bad_log.log_cap = -1
        ptr = c2.ctypes.data
        assert lib.dlp_batch_resolve(bt._h, ptr, n - 1, 0, 10, C.byref(out)) == L.ERR_ARG     # 0 < stride < n
        assert lib.dlp_batch_resolve(bt._h, ptr, -n, 0, 10, C.byref(out)) == L.ERR_ARG
        assert lib.dlp_batch_resolve(bt._h, ptr, n, 2, 10, C.byref(out)) == L.ERR_ARG         # c_is_device
        assert lib.dlp_batch_resolve(bt._h, ptr, n, 0, -1, C.byref(out)) == L.ERR_ARG         # max_pivots
        assert lib.dlp_batch_resolve(bt._h, None, 0, 0, -1, None) == L.ERR_ARG
        assert lib.dlp_batch_resolve(bt._h, ptr, n, 0, 10, C.byref(bad_log)) == L.ERR_ARG
        assert b"dlp_batch_resolve" in lib.dlp_last_error()
        T = np.zeros((m + 1, dlp.tableau_ld(m, n)))
        for k in (-1, NLP):
            assert lib.dlp_batch_read(bt._h, k, T.ctypes.data_as(L._DP), None) == L.ERR_ARG
        for j in range(NLP):
            T1, basis1 = bt.read(j)
            assert T1.tobytes() == before[j][0].tobytes() and basis1.tobytes() == before[j][1].tobytes()
        assert lib.dlp_batch_resolve(bt._h, ptr, n, 0, BIG, None) == L.OK    # out may be NULL
        res = bt.resolve(None, **KW)
        assert (res.status == L.OK).all() and not res.num_pivots.any()
    for j, (A, b, c) in enumerate(lps):
        ref = BD._ref(A, b, c2[j])
        assert abs(res.objective[j] - ref.objective) <= 1e-9 * (1.0 + abs(ref.objective))
