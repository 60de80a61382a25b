"""GPU: dlp_batch_add_cols / Batch.add_cols, k structural variables added to every resident LP and
the batch re-solved warm by the primal simplex (include/dlp.h).

Reference: tests/cols_ref.py (the column rule and the primal phase in numpy, held against the C++
oracle's pivot log and against HiGHS by tests/test_batch_add_cols_api.py) applied to
``bt.read(j)`` taken before the call.

Bar, as in tests/test_gpu_batch_add_rows.py: status, pivot count, basis, objective and every
pivot-log entry are bit-identical; x, y and the read-out afterwards are equal as values.  With
max_pivots = 0 the whole read-out is compared byte for byte: the new columns are the rule's bits,
the old columns, the RHS and the basis (renamed) are the bytes they were.

Shapes: 64 x 100 + 4 (a register batch that stays one; this call itself runs the LDS kernel),
64 x 190 + 3 (leaves the register kernel), 37 x 53 + 1 / 2 / 3 (both parities of the record's
int tail n + m + 2, more work items than one pass of the workgroup at + 3 ... + 4), 5 x 7 + 2."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

import cols_ref as CR
import reopt_ref as R
import rows_ref as AR
import test_gpu_batch_add_rows as BA
import test_gpu_batch_resolve as BR
import test_gpu_batch_rhs as BH
import test_gpu_batched_dense as BD
from conftest import ROOT

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

pytestmark = pytest.mark.gpu

LOG_CAP = BD.LOG_CAP
NLP = 6
BIG = 10 ** 6
KW = dict(want_basis=True, log_cap=LOG_CAP)
# (m, n, k)
SHAPES = [pytest.param(64, 100, 4, id="64x100+4"), pytest.param(37, 53, 3, id="37x53+3"),
          pytest.param(5, 7, 2, id="5x7+2")]
RULE_ONLY = [pytest.param(64, 190, 3, id="64x190+3"), pytest.param(37, 53, 1, id="37x53+1"),
             pytest.param(37, 53, 2, id="37x53+2")]


def _reg_rule(m, n):
    return m == 64 and n <= 192


def _cols_of(P, d, j):
    return (P if P.ndim == 2 else P[j]), (d if d.ndim == 1 else d[j])


def _columns(bt, k, seed, depth=0.1):
    """Per-LP columns priced at each LP's duals as the batch stands (cols_ref.columns)."""
    P, d = zip(*(CR.columns(CR.duals(*bt.read(j), bt.n), k, seed + j, depth) for j in range(bt.nlp)))
    return np.stack(P), np.stack(d)


def _is_refused(res, j, basis):
    assert res.status[j] == L.ERR_STATE and res.num_pivots[j] == 0, (j, res.status[j])
    assert np.isnan(res.objective[j]) and np.isnan(res.x[j]).all() and np.isnan(res.y[j]).all(), j
    np.testing.assert_array_equal(res.basis[j], basis)


def _cols_step(bt, P, d, what="", max_pivots=BIG, pricing=0, refused=()):
    """One add_cols call on the whole batch, every LP checked against the reference from its
    read-out before the call, the read-out afterwards included.  refused: the LPs whose stored
    status is infeasible or pending (the read-out does not show it): ERR_STATE, the record by the
    rule.  Returns (result, references, widened tableaus by the rule)."""
    n0, m = bt.n, bt.m
    before = [bt.read(j) for j in range(bt.nlp)]
    res = bt.add_cols(P, d, max_pivots=max_pivots, **KW)
    k = P.shape[-1]
    n = n0 + k
    assert bt.n == n and bt.m == m and res.x.shape == (bt.nlp, n) and res.y.shape == (bt.nlp, m)
    assert res.basis.shape == (bt.nlp, m)
    refs, wide = [], []
    for j, (T0, basis0) in enumerate(before):
        T2, basis2 = CR.add_cols(T0, basis0, n0, *_cols_of(P, d, j))
        tag = f"{what} LP {j}"
        T1, basis1 = bt.read(j)
        assert T1.shape == T2.shape, tag
        ref = None
        if bt.result.status[j] == L.ERR_ARG:   # rejected at creation: in every call, the slack basis
            BR._is_rejected(res, j, m, n)
        elif j in refused:
            _is_refused(res, j, basis2)
        else:
            ref = CR.primal_phase(T2, basis2, n, max_pivots=max_pivots, pricing=pricing)
            BH._same_ref(res, j, ref, what)
        if ref is None:   # the record of the new shape, by the rule, no pivot
            assert T1.tobytes() == T2.tobytes(), f"{tag}: the widened record is not the rule's"
            assert basis1.tobytes() == basis2.tobytes(), tag
        else:
            assert np.array_equal(T1, ref["T"]), f"{tag}: tableau"
            assert basis1.tobytes() == ref["basis"].tobytes(), tag
        refs.append(ref)
        wide.append((T2, basis2))
    return res, refs, wide


# ---- 1. the rule alone
def _rule_alone(bt, m, n, k, seed, info0):
    P, d = _columns(bt, k, seed)
    P[1], d[1] = CR.columns(CR.duals(*bt.read(1), n), k, seed + 1, depth=-0.1)   # LP 1: nothing prices out
    before = [bt.read(j) for j in range(NLP)]
    res = bt.add_cols(P, d, max_pivots=0, **KW)
    assert not res.num_pivots.any() and bt.n == n + k and bt.m == m
    info = bt.info()
    assert (info["nlp"], info["m"], info["n"]) == (NLP, m, n + k)
    assert info["device_bytes"] >= info0["device_bytes"] + 8 * NLP * k * (m + 2)
    assert info["register_kernel"] == _reg_rule(m, n + k) == bt.rhs_kernel()["register_kernel"]
    N, N2 = n + m, n + k + m
    for j in range(NLP):
        T0, basis0 = before[j]
        T2, basis2 = CR.add_cols(T0, basis0, n, P[j], d[j])
        T1, basis1 = bt.read(j)
        assert T1.shape == (m + 1, dlp.tableau_ld(m, n + k))
        new = np.nonzero(BH._bits(T1[:, n:n + k]) != BH._bits(T2[:, n:n + k]))
        assert len(new[0]) == 0, f"LP {j}: new columns differ at {list(zip(*new))[:8]}"
        assert T1[:, :n].tobytes() == T0[:, :n].tobytes() and T1[:, n + k:N2].tobytes() == T0[:, n:N].tobytes(), j
        assert T1[:, N2].tobytes() == T0[:, N].tobytes(), f"LP {j}: the RHS or the objective value changed"
        assert T1.tobytes() == T2.tobytes(), j
        assert basis1.tobytes() == basis2.tobytes() == res.basis[j].tobytes(), j
        assert list(basis1) == [v + k if v >= n else v for v in basis0]
        assert res.status[j] == L.PIVOT_LIMIT   # accepted: running, whatever it was; no budget
        assert np.float64(res.objective[j]).tobytes() == np.float64(T0[m, N]).tobytes()
    return P, d


@pytest.mark.parametrize("m,n,k", SHAPES + RULE_ONLY)
def test_new_columns_follow_the_rule(m, n, k):
    seed = 11600 + 7 * n + k
    A, b, c = BD._stack(BH._lps(m, n, seed))
    with dlp.Batch(A, b, c, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        info0 = bt.info()
        assert info0["register_kernel"] == _reg_rule(m, n)
        P, d = _rule_alone(bt, m, n, k, seed, info0)
        # the budget was the only stop: resolve(None) goes on, LP 1 has nothing to do
        fin = bt.resolve(None, **KW)
        assert (fin.status == L.OK).all() and fin.num_pivots[1] == 0 and fin.num_pivots.sum() > 0
        cold = dlp.batched_solve_dense(np.concatenate([A, P], axis=2), b, np.concatenate([c, d], axis=1))
        for j in range(NLP):
            assert abs(fin.objective[j] - cold.objective[j]) <= 1e-9 * max(1.0, abs(cold.objective[j])), j


def test_new_columns_on_a_batch_stopped_inside_its_cold_solve():
    """Not optimal and not dual feasible: the rule holds for any basis, and the primal phase is
    the continuation of the cold solve on the wider LP."""
    m, n, k, seed = 37, 53, 2, 11700
    A, b, c = BD._stack(BH._lps(m, n, seed))
    with dlp.Batch(A, b, c, max_pivots=BR._stop(m, n, seed, False), **KW) as bt:
        assert (bt.result.status == L.PIVOT_LIMIT).all()
        assert all((bt.read(j)[0][m, :n + m] < -1e-9).any() for j in range(NLP))
        P, d = _rule_alone(bt, m, n, k, seed, bt.info())
        fin = bt.resolve(None, max_pivots=BIG, **KW)
        assert (fin.status == L.OK).all()
        cold = dlp.batched_solve_dense(np.concatenate([A, P], axis=2), b, np.concatenate([c, d], axis=1))
        for j in range(NLP):
            assert abs(fin.objective[j] - cold.objective[j]) <= 1e-9 * max(1.0, abs(cold.objective[j])), j


def test_new_columns_after_added_rows():
    m, n, k, seed = 37, 53, 2, 11800
    A, b, c = BD._stack(BH._lps(m, n, seed))
    with dlp.Batch(A, b, c, **KW) as bt:
        G, h = BA._cuts(bt.result.x, n, 1, seed)
        assert (bt.add_rows(G, h, **KW).status == L.OK).all() and bt.m == m + 1
        P, d = _rule_alone(bt, m + 1, n, k, seed, bt.info())
        fin = bt.resolve(None, **KW)
        assert (fin.status == L.OK).all()
        cold = dlp.batched_solve_dense(np.concatenate([np.concatenate([A, G], axis=1), P], axis=2),
                                       np.concatenate([b, h], axis=1), np.concatenate([c, d], axis=1))
        for j in range(NLP):
            assert abs(fin.objective[j] - cold.objective[j]) <= 1e-9 * max(1.0, abs(cold.objective[j])), j


# ---- 2. the full phase
@pytest.mark.parametrize("degen", [False, True], ids=["dense", "degenerate"])
@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_warm_resolve_after_added_columns(m, n, k, pricing, degen):
    seed = 11900 + 11 * n + 2 * k + degen
    A, b, c = BD._stack(BH._lps(m, n, seed, degen))
    with dlp.Batch(A, b, c, pricing=pricing, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        P, d = _columns(bt, k, seed)
        res, refs, _ = _cols_step(bt, P, d, "warm", pricing=pricing)
        after = bt.resolve(None, **KW)   # after DLP_OK: as after any optimal solve
        assert bt.info()["register_kernel"] == _reg_rule(m, n + k)
    assert (res.status == L.OK).all(), res.status
    done = [ref["done"] for ref in refs]
    assert sum(v >= 1 for v in done) >= (1 if degen else NLP // 2), done
    assert (after.status == L.OK).all() and not after.num_pivots.any()
    assert after.objective.tobytes() == res.objective.tobytes() and after.x.tobytes() == res.x.tobytes()
    cold = dlp.batched_solve_dense(np.concatenate([A, P], axis=2), b, np.concatenate([c, d], axis=1), pricing=pricing)
    assert (cold.status == L.OK).all()
    for j in range(NLP):
        assert abs(res.objective[j] - cold.objective[j]) <= 1e-9 * max(1.0, abs(cold.objective[j])), j


# ---- 3. the budget: 1 pivot, then resolve(None) calls
@pytest.mark.parametrize("m,n,k", SHAPES[:2])
def test_budget_steps_give_the_unbounded_call_bits(m, n, k):
    seed = 12100 + n
    A, b, c = BD._stack(BH._lps(m, n, seed))
    with dlp.Batch(A, b, c, **KW) as bt:
        P, d = _columns(bt, k, seed, depth=0.3)
        whole = bt.add_cols(P, d, **KW)
    assert (whole.status == L.OK).all() and whole.num_pivots.max() >= 2
    logs = [[] for _ in range(NLP)]
    final = {}
    with dlp.Batch(A, b, c, **KW) as bt:
        step, refs, _ = _cols_step(bt, P, d, "step 0", max_pivots=1)
        for t in range(int(whole.num_pivots.max()) + 2):
            assert set(step.status) <= {L.OK, L.PIVOT_LIMIT} and (step.num_pivots <= 1).all()
            for j in range(NLP):
                if j not in final:
                    logs[j].append(step.logs[j][:step.num_pivots[j]])
                    if step.status[j] == L.OK:
                        final[j] = (step.objective[j], step.basis[j].copy(), step.x[j].copy(), step.y[j].copy())
            if len(final) == NLP:
                break
            # resolve(None) continues a stopped LP with its stored Bland state; a finished one does nothing
            before = [bt.read(j) for j in range(NLP)]
            step = bt.resolve(None, max_pivots=1, **KW)
            for j in range(NLP):
                budget = 0 if refs[j]["status"] == L.OK else 1
                refs[j] = dict(CR.primal_phase(*before[j], bt.n, max_pivots=budget, bland=refs[j]["bland"]),
                               **({"status": L.OK} if budget == 0 else {}))
                BH._same_ref(step, j, refs[j], f"step {t + 1}")
        assert len(final) == NLP and t >= 2 and bt.n == n + k
    for j in range(NLP):
        got, want = np.concatenate(logs[j]), whole.logs[j][:whole.num_pivots[j]]
        assert got.tobytes() == want.tobytes(), j
        assert np.float64(final[j][0]).tobytes() == np.float64(whole.objective[j]).tobytes(), j
        assert final[j][1].tobytes() == whole.basis[j].tobytes(), j
        assert final[j][2].tobytes() == whole.x[j].tobytes() and final[j][3].tobytes() == whole.y[j].tobytes(), j


# ---- 4. input forms: one (m, k) / (k,) for all LPs, padded strides, device tensors
@pytest.mark.parametrize("m,n,k", SHAPES[:2])
def test_shared_columns_equal_tiled_columns(m, n, k):
    seed = 12300 + n
    A, b, c = BD._stack(BH._lps(m, n, seed))
    with dlp.Batch(A, b, c, **KW) as one, dlp.Batch(A, b, c, **KW) as tiled:
        P = CR.columns(one.result.y[0], k, seed)[0]
        d = 1.05 * (one.result.y @ P).max(axis=0)      # attractive in every LP
        r1 = one.add_cols(P, d, **KW)
        r2 = tiled.add_cols(np.tile(P, (NLP, 1, 1)), np.tile(d, (NLP, 1)), **KW)
        BD._same_bytes(r1, r2)
        assert r1.num_pivots.all() and (r1.status == L.OK).all()
        for j in range(NLP):
            assert one.read(j)[0].tobytes() == tiled.read(j)[0].tobytes()
        # mixed: per-LP P with one d for all
        r3 = one.add_cols(np.tile(P, (NLP, 1, 1)), d + 0.01, **KW)
        r4 = tiled.add_cols(P, np.tile(d + 0.01, (NLP, 1)), **KW)
        BD._same_bytes(r3, r4)
        assert one.n == tiled.n == n + 2 * k


def test_padded_strides_and_call_level_errors():
    m, n, k = 37, 53, 2
    A, b, c = BD._stack(BH._lps(m, n, 12400))
    lib = L.lib()
    with dlp.Batch(A, b, c, **KW) as bt:
        P, d = _columns(bt, k, 12400)
        before = [bt.read(j) for j in range(NLP)]
        info0 = bt.info()
        out, bad_log = L.BatchOut(), L.BatchOut()
        bad_log.log_cap = -1
        pP, pd = P.ctypes.data, d.ctypes.data
        call = lambda *a: lib.dlp_batch_add_cols(bt._h, *a)
        lib.dlp_batch_resolve(None, None, 0, 0, 10, None)   # (another name in dlp_last_error)
        assert call(k, pP, m * k - 1, pd, k, 0, 10, C.byref(out)) == L.ERR_ARG      # 0 < strideP < m * k
        assert b"dlp_batch_add_cols" in lib.dlp_last_error()
        assert call(k, pP, m * k, pd, k - 1, 0, 10, C.byref(out)) == L.ERR_ARG      # 0 < strided < k
        assert call(k, pP, -m * k, pd, k, 0, 10, C.byref(out)) == L.ERR_ARG
        assert call(k, pP, m * k, pd, k, 2, 10, C.byref(out)) == L.ERR_ARG          # cols_are_device
        assert call(k, pP, m * k, pd, k, 0, -1, C.byref(out)) == L.ERR_ARG          # max_pivots
        assert call(k, None, m * k, pd, k, 0, 10, C.byref(out)) == L.ERR_ARG
        assert call(k, pP, m * k, None, k, 0, 10, C.byref(out)) == L.ERR_ARG
        assert call(-1, pP, m * k, pd, k, 0, 10, C.byref(out)) == L.ERR_ARG
        assert call(k, pP, m * k, pd, k, 0, 10, C.byref(bad_log)) == L.ERR_ARG
        assert call(10 ** 6, pP, 0, pd, 0, 0, 10, C.byref(out)) == L.ERR_UNSUPPORTED
        assert bt.info() == info0
        for j in range(NLP):
            T1, basis1 = bt.read(j)
            assert T1.tobytes() == before[j][0].tobytes() and basis1.tobytes() == before[j][1].tobytes()
        # k = 0 is resolve(None), out may be NULL
        assert call(0, None, 0, None, 0, 0, BIG, None) == L.OK and bt.info() == info0
        zero, same = bt.add_cols(None, None, **KW), bt.resolve(None, **KW)
        BD._same_bytes(zero, same)
        assert (zero.status == L.OK).all() and not zero.num_pivots.any() and bt.n == n
        # padded strides: LP j's columns at P + j * strideP
        Pp, dp = np.zeros((NLP, m * k + 5)), np.zeros((NLP, k + 3))
        Pp[:, :m * k], dp[:, :k] = P.reshape(NLP, -1), d
        with dlp.Batch(A, b, c, **KW) as twin:
            want = twin.add_cols(P, d, **KW)
        o, result = dlp.solver._batch_outputs(NLP, m, n + k, True, True, True, LOG_CAP)
        assert call(k, Pp.ctypes.data, m * k + 5, dp.ctypes.data, k + 3, 0, BIG, C.byref(o)) == L.OK
        bt.n += k
        BD._same_bytes(result(), want)
        assert want.num_pivots.sum() > 0


# (in a child process: torch brings its own HIP runtime, see tests/test_gpu_batched_dense.py)
DEVICE_SCRIPT = r"""
import json, sys
import torch
torch.cuda.init()
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import oracle_py as O
import cols_ref as CR
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

dev0 = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")
out = {}
for m, n, k in ((64, 100, 4), (37, 53, 3)):
    lps = [O.gen_dense(m, n, 12500 + j) for j in range(6)]
    A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
    with dlp.Batch(A, b, c, **KW) as host, dlp.Batch(*(dev0(v) for v in (A, b, c)), **KW) as dev:
        ok = same(host.result, dev.result)
        P, d = (np.stack(v) for v in zip(*(CR.columns(host.result.y[j], k, 12550 + j) for j in range(6))))
        rh, rd = host.add_cols(P, d, **KW), dev.add_cols(dev0(P), dev0(d), **KW)
        ok = ok and same(rh, rd) and int(rh.num_pivots.sum()) > 0 and host.n == dev.n == n + k
        ok = ok and all(host.read(j)[0].tobytes() == dev.read(j)[0].tobytes() for j in range(6))
        out[f"{m}x{n} device columns"] = bool(ok)
        P1, d1 = P[0], 1.05 * (rh.y @ P[0]).max(axis=0)             # shared columns, the second growth
        view = dev0(P1.T).T                                           # has to be made contiguous
        rh, rd = host.add_cols(P1, d1, **KW), dev.add_cols(view, dev0(d1), **KW)
        out[f"{m}x{n} shared view"] = (not view.is_contiguous()) and same(rh, rd) and host.n == dev.n == n + 2 * k
        c2 = np.concatenate([c, d, np.tile(d1, (6, 1))], axis=1) * 0.9  # and the later calls take n + 2k entries
        out[f"{m}x{n} resolve"] = same(host.resolve(c2, **KW), dev.resolve(dev0(c2), **KW))
        bad = dev0(P)
        bad[4, 3, 0] = float("nan")                                  # the kernel's check sees device inputs too
        try:
            dev.add_cols(bad, dev0(d), **KW)
            seen = False
        except dlp.DLPError as e:
            seen = e.status == -1 and "LP 4" in str(e)
        out[f"{m}x{n} nan seen"] = seen and dev.n == n + 2 * k and \
            all(host.read(j)[0].tobytes() == dev.read(j)[0].tobytes() for j in range(6))
        out[f"{m}x{n} float32 raises"] = raises(dev.add_cols, dev0(P).float(), dev0(d))
        out[f"{m}x{n} cpu tensor raises"] = raises(dev.add_cols, dev0(P).cpu(), dev0(d))
        out[f"{m}x{n} mixed raises"] = raises(dev.add_cols, dev0(P), d)
print(json.dumps(out))
"""


def test_device_columns_give_the_host_bytes():
    p = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT, ROOT], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(out) == 14 and all(out.values()), out


# ---- 5. per-LP outcomes in one batch
def _outcome_batch(m, n, seed):
    """[rejected at creation, pending dual, infeasible, unbounded, stopped inside its primal solve,
    optimal], the creation budget that stops LP 4 alone, and the right-hand sides whose one-pivot
    dual call leaves LP 1 pending and LP 2 infeasible (the others keep their b)."""
    cand = sorted(range(8), key=lambda j: BD._gen_ref(m, n, seed + j).num_pivots)
    counts = [BD._gen_ref(m, n, seed + j).num_pivots for j in cand]
    assert counts[-1] > counts[1] + 1   # the longest solve is stopped, the two shortest finish
    order = [cand[2], cand[0], cand[3], cand[4], cand[-1], cand[1]]
    lps = [tuple(v.copy() for v in BD._gen(m, n, seed + j)) for j in order]
    lps[0][1][m - 1] = -1.0
    lps[2][2][:] = -np.abs(lps[2][2])            # no cost is positive: optimal on the slack basis, x = 0
    lps[3][0][:, 5] = -lps[3][0][:, 5]           # a column without a positive entry, the largest cost: a ray
    lps[3][2][5] = 10.0
    assert BD._ref(*lps[2]).num_pivots == 0
    ray = BD._ref(*lps[3])
    assert ray.status == L.UNBOUNDED and ray.num_pivots == 0
    budget = counts[1] + 1   # (one more: optimality is seen by the pricing after the last pivot)
    b2 = np.stack([lp[1] for lp in lps]).copy()
    b2[1] = BH.perturbed(b2[1], seed, 0.3)
    b2[2, 3] = -1.0                              # row 3 is A >= 0 with the slack basis: no entering slot
    return lps, budget, b2


@pytest.mark.parametrize("m,n,k", [(64, 100, 4), (37, 53, 3)], ids=["64x100+4", "37x53+3"])
def test_every_outcome_in_one_batch(m, n, k):
    seed = 12600 + m
    lps, budget, b2 = _outcome_batch(m, n, seed)
    A, b, c = BD._stack(lps)
    with dlp.Batch(A, b, c, max_pivots=budget, **KW) as bt:
        assert list(bt.result.status) == [L.ERR_ARG, L.OK, L.OK, L.UNBOUNDED, L.PIVOT_LIMIT, L.OK]
        r1, refs1 = BH._rhs_step(bt, b2, "one dual pivot", max_pivots=1)
        assert list(r1.status) == [L.ERR_ARG, L.PIVOT_LIMIT, L.INFEASIBLE, L.ERR_STATE, L.ERR_STATE, L.OK]
        P, d = _columns(bt, k, seed)
        P[1], d[1] = CR.columns(CR.duals(*bt.read(1), n), k, seed + 1, depth=-0.1)   # LP 1 stays dual feasible
        P[2], d[2] = CR.columns(np.ones(m), k, seed + 2, depth=-0.1)                 # and LP 2 (d < 0 <= its z)
        d[2] = -np.abs(d[2]) - 1.0
        last = [bt.read(j) for j in (1, 2)]
        res, refs, wide = _cols_step(bt, P, d, "outcomes", refused=(1, 2))
        assert [int(s) for s in res.status[:3]] == [L.ERR_ARG, L.ERR_STATE, L.ERR_STATE]
        assert res.status[3] == refs[3]["status"] == L.UNBOUNDED
        assert res.status[4] == L.OK and refs[4]["done"] > 0 and res.status[5] == L.OK
        for (T0, _), j in zip(last, (1, 2)):    # the refused LPs: the RHS (negative entries) as it stood
            assert wide[j][0][:, n + k + m].tobytes() == T0[:, n + m].tobytes() and (T0[:m, n + m] < -1e-9).any()
        # the primal call refuses them as before; the stored status, Bland state and last b_k stayed:
        # the very b2 continues LP 1's dual phase without a rebuild, LP 2 is infeasible again
        rp = bt.resolve(None, **KW)
        assert [int(s) for s in rp.status] == [L.ERR_ARG, L.ERR_STATE, L.ERR_STATE, L.UNBOUNDED, L.OK, L.OK]
        assert not rp.num_pivots.any()
        cont = [None, refs1[1]["bland"], None, None, None, None]
        r2, refs2 = BH._rhs_step(bt, b2, "the dual phase goes on", continued=cont)
        assert list(r2.status) == [L.ERR_ARG, L.OK, L.INFEASIBLE, L.ERR_STATE, L.OK, L.OK]
        assert r2.num_pivots[1] >= 1 and r2.x.shape == (NLP, n + k)
        # the call after an infeasible LP: refused again; the original b brings it back on the wider LP
        P2, d2 = _columns(bt, 1, seed + 20)
        _cols_step(bt, P2, d2, "after infeasible", refused=(2,))
        b3 = b2.copy()
        b3[2] = b[2]
        r3, _ = BH._rhs_step(bt, b3, "back")
        assert r3.status[2] == L.OK and bt.n == n + k + 1


# ---- 6. a column that is not finite fails the whole call
@pytest.mark.parametrize("where,value,first", [
    (("P", 4, 0, 1), np.nan, 4), (("d", 2, 0), np.inf, 2), (("P", 5, -1, -1), -np.inf, 1), (("d", 0, -1), np.nan, 0),
], ids=["nan in P", "inf in d", "-inf in P, nan in d before it", "nan in d of LP 0"])
@pytest.mark.parametrize("m,n,k", SHAPES[:2])
def test_a_column_that_is_not_finite_fails_the_whole_call(m, n, k, where, value, first):
    seed = 12700 + n
    A, b, c = BD._stack(BH._lps(m, n, seed))
    c2 = np.stack([R.make_c2(c[j], seed + j, holes=False) for j in range(NLP)])
    with dlp.Batch(A, b, c, **KW) as bt, dlp.Batch(A, b, c, **KW) as twin:
        P, d = _columns(bt, k, seed)
        bad = {"P": P.copy(), "d": d.copy()}
        bad[where[0]][where[1:]] = value
        if first != where[1]:
            bad["d"][first, 0] = np.nan
        before = [bt.read(j) for j in range(NLP)]
        info0 = bt.info()
        with pytest.raises(dlp.DLPError) as e:
            bt.add_cols(bad["P"], bad["d"], **KW)
        assert e.value.status == L.ERR_ARG and f"LP {first}:" in str(e.value) and "dlp_batch_add_cols" in str(e.value)
        assert bt.n == n and bt.info() == info0
        for j in range(NLP):
            T1, basis1 = bt.read(j)
            assert T1.tobytes() == before[j][0].tobytes() and basis1.tobytes() == before[j][1].tobytes()
        r1, r2 = bt.resolve(c2, **KW), twin.resolve(c2, **KW)
        BD._same_bytes(r1, r2)
        assert r1.num_pivots.sum() > 0
        assert bt.info() == twin.info()
        # and the call still works afterwards
        BD._same_bytes(bt.add_cols(P, d, **KW), twin.add_cols(P, d, **KW))


def test_the_output_arrays_of_a_failed_call_are_untouched():
    m, n, k = 37, 53, 2
    A, b, c = BD._stack(BH._lps(m, n, 12800))
    lib = L.lib()
    with dlp.Batch(A, b, c, **KW) as bt:
        P, d = _columns(bt, k, 12800)
        P[3, 7, 1] = np.nan
        obj = np.full(NLP, 7.0)
        st = np.full(NLP, 77, np.int32)
        npv = np.full(NLP, 777, np.int64)
        basis = np.full((NLP, m), 7777, np.int32)
        x, y = np.full((NLP, n + k), 7.5), np.full((NLP, m), 7.25)
        ms = C.c_double(-1.0)
        out = L.BatchOut(obj.ctypes.data_as(C.POINTER(C.c_double)), st.ctypes.data_as(C.POINTER(C.c_int32)),
                         npv.ctypes.data_as(C.POINTER(C.c_int64)), basis.ctypes.data_as(C.POINTER(C.c_int32)), None, 0,
                         x.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double)), C.pointer(ms))
        rc = lib.dlp_batch_add_cols(bt._h, k, P.ctypes.data, m * k, d.ctypes.data, k, 0, BIG, C.byref(out))
        assert rc == L.ERR_ARG and b"LP 3" in lib.dlp_last_error()
        assert (obj == 7.0).all() and (st == 77).all() and (npv == 777).all() and (basis == 7777).all()
        assert (x == 7.5).all() and (y == 7.25).all() and ms.value == -1.0


# ---- 7. a shape that fits at n + k and not at n + k + 1
def _lds_bytes(m, n):
    return 8 * ((m + 1) * (n + 1) + (m + 1) + (n + 1)) + 4 * (n + m + 8) + 16 + 16


def test_growth_past_the_lds_is_unsupported():
    m, n, nlp = 40, 400, 2
    kmax = max(k for k in range(1, 400) if _lds_bytes(m, n + k) <= 160 * 1024)
    assert _lds_bytes(m, n + kmax) <= 160 * 1024 < _lds_bytes(m, n + kmax + 1) and 8 <= kmax < 399
    A, b, c = BD._stack(BH._lps(m, n, 12900, nlp=nlp))
    with dlp.Batch(A, b, c, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        # three of the columns price out, the others do not (the numpy reference pays per pivot)
        P, d = _columns(bt, kmax + 1, 12900, depth=-0.1)
        P3, d3 = _columns(bt, 3, 12950, depth=0.05)
        P[:, :, 5:8], d[:, 5:8] = P3, d3
        before = [bt.read(j) for j in range(nlp)]
        info0 = bt.info()
        with pytest.raises(dlp.DLPError) as e:
            bt.add_cols(P, d, **KW)
        assert e.value.status == L.ERR_UNSUPPORTED and bt.n == n and bt.info() == info0
        for j in range(nlp):
            T1, basis1 = bt.read(j)
            assert T1.tobytes() == before[j][0].tobytes() and basis1.tobytes() == before[j][1].tobytes()
        # kmax of them fit: the largest tableau the launch takes
        Pk, dk = np.ascontiguousarray(P[:, :, :kmax]), np.ascontiguousarray(d[:, :kmax])
        res = bt.add_cols(Pk, dk, **KW)
        assert (res.status == L.OK).all() and res.num_pivots.all() and bt.n == n + kmax
        for j in range(nlp):
            ref = CR.add_cols_and_solve(*before[j], n, Pk[j], dk[j])
            assert res.num_pivots[j] == ref["done"]
            assert np.float64(res.objective[j]).tobytes() == np.float64(ref["objective"]).tobytes()
            assert res.basis[j].tobytes() == ref["basis"].tobytes()
            assert np.array_equal(bt.read(j)[0], ref["T"])
        with pytest.raises(dlp.DLPError) as e:
            bt.add_cols(Pk[:, :, :1], dk[:, :1], **KW)
        assert e.value.status == L.ERR_UNSUPPORTED and bt.n == n + kmax


# ---- 8. twice, then new objectives, right-hand sides and rows on the widened batch
@pytest.mark.parametrize("m,n", [(64, 100), (64, 188), (37, 53), (5, 7)], ids=["64x100", "64x188", "37x53", "5x7"])
def test_add_cols_twice_then_the_other_calls(m, n):
    """n -> n + 1 -> n + 4, then resolve(c2) with an (n + 4)-vector against the numpy primal rule,
    resolve_rhs against rhs_ref and add_rows against rows_ref, on whichever kernel the widened
    shape takes (64 x 100 stays on the register kernel throughout; 64 x 188 is on it at 189 and
    192 columns, its limit; the row growth leaves it)."""
    seed = 13000 + n
    lps = BH._lps(m, n, seed)
    A, b, c = BD._stack(lps)
    with dlp.Batch(A, b, c, **KW) as bt:
        P1, d1 = _columns(bt, 1, seed)
        r1, _, _ = _cols_step(bt, P1, d1, "first")
        assert (r1.status == L.OK).all() and bt.n == n + 1
        assert bt.info()["register_kernel"] == _reg_rule(m, n + 1) == bt.rhs_kernel()["register_kernel"]
        P2, d2 = _columns(bt, 3, seed + 3)
        r2, _, _ = _cols_step(bt, P2, d2, "second")
        assert (r2.status == L.OK).all() and bt.n == n + 4 and (r1.num_pivots + r2.num_pivots).sum() > 0
        assert bt.info()["register_kernel"] == _reg_rule(m, n + 4) == bt.rhs_kernel()["register_kernel"]
        wide = [(np.concatenate([A[j], P1[j], P2[j]], axis=1), b[j], np.concatenate([c[j], d1[j], d2[j]]))
                for j in range(NLP)]
        c2 = BA._resolve_c2(bt, wide, seed + 6)
        b3 = BH.perturbed(b, seed + 4)
        r3, _ = BH._rhs_step(bt, b3, "rhs on n + 4")
        assert (r3.status == L.OK).all() and (r3.num_pivots.sum() > 0 or m == 5)   # (5 x 7: 2 % moves no basis)
        G, h = BA._cuts(r3.x, n + 4, 1, seed + 7)
        r4, _, _ = BA._add_step(bt, G, h, "rows on n + 4")
        assert (r4.status == L.OK).all() and bt.m == m + 1 and bt.n == n + 4
    A4 = np.stack([np.vstack([w[0], G[j]]) for j, w in enumerate(wide)])
    cold = dlp.batched_solve_dense(A4, np.concatenate([b3, h], axis=1), c2)
    for j in range(NLP):
        assert cold.status[j] == L.OK
        assert abs(r4.objective[j] - cold.objective[j]) <= 1e-9 * max(1.0, abs(cold.objective[j])), j
