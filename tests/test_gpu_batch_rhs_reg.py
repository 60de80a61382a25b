"""GPU: dlp_batch_resolve_rhs at m = 64 on the register-resident kernel's dual instantiation
(batched_reg_kernel<64, NW, RhsIn>), and dlp_batch_rhs_kernel.

The bar is tests/test_gpu_batch_rhs.py's, through its helpers: status, pivot count, basis, every
log entry and the objective bit for bit, x, y and the read-out tableau equal as values, against
tests/rhs_ref.py run from the batch's own read-out before the call.  The inputs come from
tests/rhs_reg_inputs.py; tests/test_batch_rhs_reg_api.py holds them against the reference on the
CPU (that they pivot, reach the bases they are built for, and tie where they should)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rhs_ref as RR
import rhs_reg_inputs as I
import test_gpu_batch_resolve as BR
import test_gpu_batch_rhs as TR
from conftest import ROOT
from test_gpu_batch_rhs import _rhs_step, _same_ref

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

pytestmark = pytest.mark.gpu

M, NLP, BIG, KW = I.M, I.NLP, TR.BIG, TR.KW
assert NLP == TR.NLP


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- 1. which kernel the dual call runs, and its residency
@pytest.mark.parametrize("m,n,reg", [(64, 64, True), (64, 128, True), (64, 192, True), (64, 193, False),
                                     (37, 53, False)])
def test_rhs_kernel_reports_the_dual_call_s_kernel(m, n, reg):
    rng = np.random.default_rng(n)
    A, b, c = rng.uniform(0.0, 1.0, (2, m, n)), rng.uniform(1.0, 2.0, (2, m)), rng.uniform(0.0, 1.0, (2, n))
    with dlp.Batch(A, b, c, max_pivots=3) as bt:
        k = bt.rhs_kernel()
        info = bt.info()
    occ = dlp.batched_occupancy(m, n)
    print(f"{m}x{n}: rhs_kernel {k}, batched_occupancy {occ}")
    assert k["register_kernel"] is reg
    assert info["register_kernel"] is reg   # (the kernel of creation: the same rule of shapes)
    assert k["threads_per_lp"] == occ["threads_per_lp"]
    if reg:   # the dual instantiation keeps the primal kernels' residency
        assert k["lps_per_cu"] == occ["lps_per_cu"] >= 1
        assert k["threads_per_lp"] == 64 * ((n + 63) // 64)
    else:
        assert k["lps_per_cu"] >= 1


# ---- 2. warm dual re-solves on the wave boundaries
@pytest.mark.parametrize("scale", I.SCALES, ids=["2pct", "30pct"])
@pytest.mark.parametrize("degen", [False, True], ids=["dense", "degenerate"])
@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("n", I.WARM_N)
def test_warm_dual_resolve_on_the_wave_boundaries(n, pricing, degen, scale):
    A, b, c = I.stack(I.warm_lps(n, degen))
    b2 = I.warm_b2(n, degen, scale)
    with dlp.Batch(A, b, c, pricing=pricing, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        assert bt.rhs_kernel()["register_kernel"] is True
        res, refs = _rhs_step(bt, b2, f"64x{n}", pricing=pricing)
        after = bt.resolve(None, **KW)   # after DLP_OK: as after any optimal solve
    done = [r["done"] for r in refs]
    assert (res.status == L.OK).all() and sum(d >= 1 for d in done) >= NLP // 2, (res.status, done)
    assert (after.status == L.OK).all() and not after.num_pivots.any()
    assert after.objective.tobytes() == res.objective.tobytes() and after.x.tobytes() == res.x.tobytes()


# ---- 3. the rebuild alone
def _rebuild_alone(bt, b2, what):
    """max_pivots = 0: the RHS column and the objective entry bit for bit against the fold of
    the read-out before the call, nothing else touched, the status by the eligibility test."""
    n, N = bt.n, bt.n + M
    before = [bt.read(k) for k in range(NLP)]
    res = bt.resolve_rhs(b2, max_pivots=0, **KW)
    assert not res.num_pivots.any()
    for k, (T0, basis0) in enumerate(before):
        T1, basis1 = bt.read(k)
        rhs = RR.fold_rhs(T0, n, b2[k])
        bad = np.nonzero(_bits(T1[:, N]) != _bits(rhs))[0]
        assert len(bad) == 0, f"{what} LP {k}: RHS differs at rows {bad[:8]}: {T1[bad[:8], N]} vs {rhs[bad[:8]]}"
        keep = np.arange(T0.shape[1]) != N
        assert T1[:, keep].tobytes() == T0[:, keep].tobytes(), f"{what} LP {k}: an entry outside the RHS column changed"
        assert basis1.tobytes() == basis0.tobytes() == res.basis[k].tobytes()
        assert np.float64(res.objective[k]).tobytes() == np.float64(rhs[M]).tobytes()
        want = L.PIVOT_LIMIT if len(RR.eligible_rows(rhs[:M])) else L.OK
        assert res.status[k] == want, (what, k, res.status[k], want)
    return before, res


def test_rebuild_alone_on_a_mixed_basis():
    n = 129
    A, b, c = I.stack(I.warm_lps(n, False))
    with dlp.Batch(A, b, c, **KW) as bt:
        assert bt.rhs_kernel()["register_kernel"] is True
        before, res = _rebuild_alone(bt, I.warm_b2(n, False, 0.3), "mixed")
        slacks = [int((basis >= n).sum()) for _, basis in before]
        assert all(0 < s < M for s in slacks), slacks   # basic and nonbasic slacks in every LP
        assert L.PIVOT_LIMIT in set(res.status)


def test_rebuild_alone_with_every_slack_nonbasic():
    n = I.ALLNB_N
    A, b, c = I.stack(I.all_nonbasic_lps())
    b2 = I.all_nonbasic_b2()
    with dlp.Batch(A, b, c, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        assert (bt.result.basis < n).all()   # every row's basic variable structural
        _rebuild_alone(bt, b2, "all nonbasic")
        _rhs_step(bt, b2, "all nonbasic")


def test_rebuild_alone_at_the_slack_basis_then_the_dual_run():
    n = I.SLACK_N
    A, b, c = I.stack(I.slack_basis_lps())
    b2 = I.slack_basis_b2()
    with dlp.Batch(A, b, c, **KW) as bt:
        assert (bt.result.status == L.OK).all() and not bt.result.num_pivots.any()
        assert (bt.result.basis == n + np.arange(M)).all()
        before, res = _rebuild_alone(bt, b2, "slack basis")
        for k in range(NLP):   # B^-1 = I: the column is b itself
            assert bt.read(k)[0][:M, n + M].tobytes() == b2[k].tobytes()
        assert (res.status == L.PIVOT_LIMIT).all()
        # the pending LPs handed the same b go on from the column as it stands
        run, refs = _rhs_step(bt, b2, "from the slack basis", continued=[False] * NLP)
        assert all(r["done"] >= 1 for r in refs) and L.OK in set(run.status)
        assert set(run.status) <= {L.OK, L.INFEASIBLE}


# ---- 4. exact ties
def test_exact_ties():
    lps, b2 = I.tie_lps()
    with dlp.Batch(*I.stack(lps), **KW) as bt:
        assert (bt.result.status == L.OK).all()
        assert bt.rhs_kernel()["register_kernel"] is True
        res, refs = _rhs_step(bt, b2, "ties")
    assert (res.status == L.OK).all()
    assert any((r["log"]["ratio"] == 0.0).any() for r in refs)
    # one pivot per call: a phase the budget stopped in Bland mode goes on in it, and the steps
    # end in the basis of the one unbounded call
    in_bland = False
    with dlp.Batch(*I.stack(lps), **KW) as bt:
        cont = [None] * NLP
        for t in range(max(r["done"] for r in refs) + 2):
            step, srefs = _rhs_step(bt, b2, f"ties step {t}", max_pivots=1, continued=cont)
            cont = [r["bland"] if r["status"] == L.PIVOT_LIMIT else None for r in srefs]
            in_bland = in_bland or any(c is True for c in cont)
            if (step.status == L.OK).all():
                break
        assert (step.status == L.OK).all() and in_bland
        assert step.basis.tobytes() == res.basis.tobytes()


# ---- 5. budgets
def _budget_inputs():
    n = 65
    A, b, c = I.stack(I.warm_lps(n, False))
    return n, A, b, c, I.warm_b2(n, False, 0.3)


def test_budgets_give_the_unbounded_call_s_bits():
    """Budgets 0, 1 and 7, repeated with the same b until DLP_OK, give the concatenated log, the
    basis, objective, x and y bits of one unbounded call."""
    n, A, b, c, b2 = _budget_inputs()
    with dlp.Batch(A, b, c, **KW) as bt:
        whole = bt.resolve_rhs(b2, **KW)
        T_whole = [bt.read(k)[0] + 0.0 for k in range(NLP)]
    assert (whole.status == L.OK).all() and whole.num_pivots.max() >= 9
    with dlp.Batch(A, b, c, **KW) as bt:
        logs = [[] for _ in range(NLP)]
        final = {}
        for t, budget in enumerate([0, 1, 7] * (int(whole.num_pivots.max()) // 8 + 2)):
            r = bt.resolve_rhs(b2, max_pivots=budget, **KW)
            assert (r.num_pivots <= budget).all()
            for k in range(NLP):
                if k not in final:
                    logs[k].append(r.logs[k][:r.num_pivots[k]])
                    if r.status[k] == L.OK:   # (a later call rebuilds its column: read it now)
                        final[k] = (r.objective[k], r.basis[k].copy(), r.x[k].copy(), r.y[k].copy(),
                                    bt.read(k)[0] + 0.0)
            if len(final) == NLP:
                break
        assert len(final) == NLP
        for k in range(NLP):
            got, want = np.concatenate(logs[k]), whole.logs[k][:whole.num_pivots[k]]
            assert got.tobytes() == want.tobytes(), k
            assert np.float64(final[k][0]).tobytes() == np.float64(whole.objective[k]).tobytes(), k
            assert final[k][1].tobytes() == whole.basis[k].tobytes(), k
            assert final[k][2].tobytes() == whole.x[k].tobytes() and final[k][3].tobytes() == whole.y[k].tobytes(), k
            assert final[k][4].tobytes() == T_whole[k].tobytes(), k


def test_another_b_on_a_pending_lp_takes_the_rebuild():
    n, A, b, c, b2 = _budget_inputs()
    with dlp.Batch(A, b, c, **KW) as bt:
        r = bt.resolve_rhs(b2, max_pivots=1, **KW)
        assert (r.status == L.PIVOT_LIMIT).any()
        b3 = b2.copy()
        b3[:, M - 1] = np.nextafter(b3[:, M - 1], np.inf)   # one entry, one bit
        _, refs = _rhs_step(bt, b3, "another b", max_pivots=1)   # (continued = None: the reference rebuilds)
        # the same b3 again: what that call left pending goes on without a rebuild
        cont = [ref["bland"] if ref["status"] == L.PIVOT_LIMIT else None for ref in refs]
        assert any(c is not None for c in cont)
        fin, _ = _rhs_step(bt, b3, "another b, all of it", continued=cont)
        assert (fin.status == L.OK).all()


def test_log_cap_smaller_than_the_pivot_count():
    n, A, b, c, b2 = _budget_inputs()
    with dlp.Batch(A, b, c, **KW) as bt:
        whole = bt.resolve_rhs(b2, **KW)
    cap = 3
    assert whole.num_pivots.min() > cap
    with dlp.Batch(A, b, c, **KW) as bt:
        r = bt.resolve_rhs(b2, want_basis=True, log_cap=cap)
    for f in ("status", "num_pivots", "objective", "basis", "x", "y"):
        assert getattr(r, f).tobytes() == getattr(whole, f).tobytes(), f
    for k in range(NLP):
        assert r.logs[k][:cap].tobytes() == whole.logs[k][:cap].tobytes(), k


# ---- 6. every outcome in one batch
@pytest.mark.parametrize("how", ["host", "stride0", "device"])
def test_every_outcome_in_one_batch(how):
    """[rejected at creation, a NaN in b_k, an inf in b_k, stopped inside its primal solve,
    optimal, infeasible]; then the infeasible LP back, a pending LP before resolve, and
    resolve(c2) between two dual calls.  stride0: one shared b (LP 5's, which the others take
    too); device: b as a tensor on the batch's device, in a child process of its own."""
    if how == "device":
        p = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT, ROOT], capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stderr[-2000:]
        out = json.loads(p.stdout.strip().splitlines()[-1])
        assert len(out) == 4 and all(out.values()), out
        return
    m, n = M, 100
    seed = 7900 + m
    lps, budget = TR._outcome_batch(m, n, seed)
    A, b, c = TR.BD._stack(lps)
    b2 = TR.perturbed(b, seed)
    b2[1, m // 3] = np.nan
    b2[2, 0] = -np.inf
    b2[5, 3] = -1.0
    c2 = np.stack([BR._c2(m, n, seed, False, j) for j in range(NLP)])
    with dlp.Batch(A, b, c, max_pivots=budget, **KW) as bt:
        r0 = bt.result
        assert bt.rhs_kernel()["register_kernel"] is True
        assert list(r0.status) == [L.ERR_ARG, L.OK, L.OK, L.PIVOT_LIMIT, L.OK, L.OK]
        if how == "stride0":
            # LP 5's b for all: LP 0 rejected at creation, LP 3 not dual feasible, the others run
            res, refs = _rhs_step(bt, b2[5], "outcomes, one b")
            assert list(res.status[[0, 3]]) == [L.ERR_ARG, L.ERR_STATE]
            assert set(res.status[[1, 2, 4, 5]]) <= {L.OK, L.INFEASIBLE} and res.status[5] == L.INFEASIBLE
            bad = b2[5].copy()
            bad[7] = np.nan
            res, _ = _rhs_step(bt, bad, "outcomes, one b with a NaN")   # every record's bytes stay
            assert list(res.status) == [L.ERR_ARG] * NLP   # (the finite test comes before the dual-feasibility one)
            return
        res, refs = _rhs_step(bt, b2, "outcomes")   # (refused LPs: the state's bytes are compared)
        assert list(res.status) == [L.ERR_ARG, L.ERR_ARG, L.ERR_ARG, L.ERR_STATE, L.OK, L.INFEASIBLE]
        for j in (1, 2, 3):
            np.testing.assert_array_equal(res.basis[j], r0.basis[j])
        # infeasible, then feasible again
        back, _ = _rhs_step(bt, b, "back")
        assert list(back.status) == [L.ERR_ARG, L.OK, L.OK, L.ERR_STATE, L.OK, L.OK]
        # pending, then resolve: DLP_ERR_STATE, the record untouched
        b3 = TR.perturbed(b, seed + 1, 0.3)
        pend = bt.resolve_rhs(b3, max_pivots=1, **KW)
        pending = np.nonzero(pend.status == L.PIVOT_LIMIT)[0]
        assert len(pending) > 0
        before = [bt.read(k) for k in pending]
        for cc in (c2, None):
            rp = bt.resolve(cc, max_pivots=BIG, **KW)
            for (T0, basis0), k in zip(before, pending):
                assert rp.status[k] == L.ERR_STATE and rp.num_pivots[k] == 0 and np.isnan(rp.objective[k])
                T1, basis1 = bt.read(k)
                assert T1.tobytes() == T0.tobytes() and basis1.tobytes() == basis0.tobytes()
        # (resolve(c2) has finished LP 3's primal solve: it is dual feasible now)
        fin, _ = _rhs_step(bt, b, "finish")
        assert list(fin.status) == [L.ERR_ARG] + [L.OK] * 5
        # DLP_OK, then resolve(c2), then resolve_rhs again
        rc = bt.resolve(c2, max_pivots=BIG, **KW)
        assert (rc.status[1:] == L.OK).all() and rc.num_pivots.sum() > 0
        again, refs = _rhs_step(bt, b3, "after resolve(c2)")
        assert (again.status[1:] == L.OK).all() and sum(r["done"] for r in refs if r) > 0


DEVICE_SCRIPT = r"""
import json, sys
import torch
torch.cuda.init()
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import oracle_py as O
import distributedlpsolver_amd as dlp

KW = dict(want_basis=True, log_cap=512)

def same(r1, r2):
    ok = all(getattr(r1, f).tobytes() == getattr(r2, f).tobytes()
             for f in ("status", "num_pivots", "objective", "basis", "x", "y"))
    return ok and all(r1.logs[k][:r1.num_pivots[k]].tobytes() == r2.logs[k][:r1.num_pivots[k]].tobytes()
                      for k in range(len(r1.status)))

m, n = 64, 129
lps = [O.gen_dense(m, n, 9800 + k) for k in range(6)]
A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
b = b.copy()
b[0, m - 1] = -1.0                       # rejected at creation
rng = np.random.default_rng(m)
b2 = b * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, b.shape))
b2[1, 5] = np.nan                         # the kernel's check sees device inputs too
b2[2, 3] = -1.0                           # infeasible (A >= 0)
out = {}
with dlp.Batch(A, b, c, **KW) as host, dlp.Batch(*(torch.from_numpy(v).to("cuda:0") for v in (A, b, c)), **KW) as dev:
    ok = same(host.result, dev.result) and dev.rhs_kernel()["register_kernel"]
    for bb in (b2, b2[3], b):
        rh, rd = host.resolve_rhs(bb, **KW), dev.resolve_rhs(torch.from_numpy(np.ascontiguousarray(bb)).to("cuda:0"), **KW)
        ok = ok and same(rh, rd)
        ok = ok and all(host.read(k)[0].tobytes() == dev.read(k)[0].tobytes() for k in range(6))
        if bb is b2:
            out["outcomes"] = [int(s) for s in rd.status] == [-1, -1, 1, 0, 0, 0]
            out["pivots"] = int(rd.num_pivots.sum()) > 0
    out["device b"] = bool(ok)
    out["back"] = [int(s) for s in rd.status] == [-1, 0, 0, 0, 0, 0]
print(json.dumps(out))
"""


# ---- 7. the register instantiation against the LDS one, on the same inputs
KNOB_SCRIPT = r"""
import hashlib, json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import oracle_py as O
import distributedlpsolver_amd as dlp

def h(*arrays):
    d = hashlib.sha256()
    for a in arrays:
        d.update(np.ascontiguousarray(a).tobytes())
    return d.hexdigest()

def digest(r):
    logs = [r.logs[k][:r.num_pivots[k]] for k in range(len(r.status))]
    return h(r.status, r.num_pivots, r.objective, r.basis, r.x, r.y, *logs)

m, n, seed, nlp = 64, 100, 9900, 6
KW = dict(want_basis=True, log_cap=512)
lps = [O.gen_dense(m, n, seed + k, k % 2 == 1) for k in range(nlp)]
A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
b2 = b * (1.0 + 0.3 * np.random.default_rng(seed).uniform(-1.0, 1.0, b.shape))
b3 = b2.copy()
b3[:, 5] = -0.25
b3[1, 9] = np.nan
out = {}
with dlp.Batch(A, b, c, **KW) as bt:
    out["created_by_register_kernel"] = bt.info()["register_kernel"]
    out["rhs_register_kernel"] = bt.rhs_kernel()["register_kernel"]
    reads = []
    runs = [bt.result]
    for bb, budget in ((b2, 0), (b2, 1), (b2, 7), (b2, 10 ** 6), (b3, 10 ** 6), (b, 10 ** 6)):
        runs.append(bt.resolve_rhs(bb, max_pivots=budget, **KW))
        reads.append(h(*(bt.read(j)[0] + 0.0 for j in range(nlp)), *(bt.read(j)[1] for j in range(nlp))))
    out["runs"] = [digest(r) for r in runs] + reads
    out["pivots"] = [int(r.num_pivots.sum()) for r in runs]
    out["statuses"] = [sorted(set(int(s) for s in r.status)) for r in runs]
print(json.dumps(out))
"""


def test_m64_register_and_lds_dual_kernels_agree():
    """One child with DLP_BATCH_RHS_LDS=1 (the dual call alone through the LDS kernel) and one
    without: the digests of every output and read-out are equal.  (read() + 0.0 in the digest:
    the sign of a zero is the condensed tableau's exemption.)"""
    def run(env):
        e = dict(os.environ)
        e.pop("DLP_BATCH_LDS", None)
        e.pop("DLP_BATCH_RHS_LDS", None)
        e.update(env)
        p = subprocess.run([sys.executable, "-c", KNOB_SCRIPT, ROOT], env=e, capture_output=True, text=True,
                           timeout=240)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads(p.stdout.strip().splitlines()[-1])

    reg, lds = run({}), run({"DLP_BATCH_RHS_LDS": "1"})
    assert reg.pop("created_by_register_kernel") is True and lds.pop("created_by_register_kernel") is True
    assert reg.pop("rhs_register_kernel") is True and lds.pop("rhs_register_kernel") is False
    assert reg["pivots"][2] > 0 and reg["pivots"][4] > 0 and reg["pivots"][6] > 0
    assert 1 in reg["statuses"][5] and -1 in reg["statuses"][5]   # infeasible and refused LPs among them
    assert reg == lds
