"""GPU: dlp_batch_add_rows / Batch.add_rows, r constraint rows added to every resident LP and the
batch re-solved warm by the dual simplex (include/dlp.h).

Reference: tests/rows_ref.py (the row rule in numpy, held against HiGHS by
tests/test_batch_add_rows_api.py) applied to ``bt.read(k)`` taken before the call, then
tests/rhs_ref.py's dual phase on the grown tableau.

Bar, as in tests/test_gpu_batch_rhs.py: status, pivot count, basis, objective and every
pivot-log entry are bit-identical; x, y and the read-out afterwards are equal as values.  With
max_pivots = 0 the whole read-out is compared byte for byte: the new rows are the rule's bits,
the old rows and the objective row are the bytes they were.

Shapes: 64 x 100 (created on the register kernel, grown to 65 rows: more than a wave's lanes),
63 x 100 + 1 (gains the register kernel), 37 x 53 (r = 3 and 4: the staging holds two new rows at
a time, so two passes, the second a full or a half one), 5 x 7; r = 1 and r = 2 at one shape flip
the parity of n + m + r (the record's int tail, the scratch alignment)."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest
from scipy.optimize import linprog

import reopt_ref as R
import rhs_ref as RR
import rows_ref as AR
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
# (m, n, r)
SHAPES = [pytest.param(64, 100, 1, id="64x100+1"), pytest.param(63, 100, 1, id="63x100+1"),
          pytest.param(37, 53, 3, id="37x53+3"), pytest.param(5, 7, 2, id="5x7+2")]
PARITY = [pytest.param(37, 53, 1, id="37x53+1"), pytest.param(37, 53, 2, id="37x53+2"),
          pytest.param(37, 53, 4, id="37x53+4"), pytest.param(5, 7, 1, id="5x7+1")]


def _reg_rule(m, n):
    return m == 64 and n <= 192


def _rows_of(G, h, k):
    if G is None:
        return None, None
    return (G if G.ndim == 2 else G[k]), (h if h.ndim == 1 else h[k])


def _cuts(bt_x, n, r, seed, depth=0.1):
    """Per-LP violated cuts at each LP's x* (NaN for a rejected LP: cut at 0 there)."""
    G, h = zip(*(AR.cuts(np.nan_to_num(x), n, r, seed + k, depth) for k, x in enumerate(bt_x)))
    return np.stack(G), np.stack(h)


def _add_step(bt, G, h, what="", max_pivots=BIG, pricing=0, continued=None):
    """One add_rows call on the whole batch, every LP checked against the reference from its
    read-out before the call, the read-out afterwards included.  continued[k]: None, or the
    Bland state LP k's pending dual phase was left in (an r = 0 call continues it).  Returns
    (result, references, grown tableaus by the rule)."""
    n, m0 = bt.n, bt.m
    before = [bt.read(k) for k in range(bt.nlp)]
    res = bt.add_rows(G, h, max_pivots=max_pivots, **KW)
    r = 0 if G is None else G.shape[-2]
    assert bt.m == m0 + r and res.basis.shape == (bt.nlp, m0 + r) and res.y.shape == (bt.nlp, m0 + r)
    refs, grown = [], []
    for k, (T0, basis0) in enumerate(before):
        Gk, hk = _rows_of(G, h, k)
        if r:
            T2, basis2 = AR.add_rows(T0, basis0, n, Gk, hk)
        else:
            T2, basis2 = T0, basis0
        tag = f"{what} LP {k}"
        T1, basis1 = bt.read(k)
        assert T1.shape == T2.shape, tag
        if bt.result.status[k] == L.ERR_ARG:   # rejected at creation: in every call, the slack basis
            BR._is_rejected(res, k, bt.m, n)
            ref = None
        else:
            cont = continued[k] if continued and continued[k] is not None else False
            ref = AR.dual_phase(T2, basis2, n, continued=cont, max_pivots=max_pivots, pricing=pricing)
            BH._same_ref(res, k, ref, what)
        if ref is None or ref["status"] < 0:   # the record of the new shape, by the rule, no pivot
            assert T1.tobytes() == T2.tobytes(), f"{tag}: the grown record is not the rule's"
            assert basis1.tobytes() == basis2.tobytes(), tag
        else:
            assert np.array_equal(T1, ref["T"]), f"{tag}: tableau"
            assert basis1.tobytes() == ref["basis"].tobytes(), tag
        refs.append(ref)
        grown.append((T2, basis2))
    return res, refs, grown


# ---- 1. the rule alone
@pytest.mark.parametrize("m,n,r", SHAPES + PARITY)
def test_new_rows_follow_the_rule(m, n, r):
    seed = 9100 + 7 * n + r
    A, b, c = BD._stack(BH._lps(m, n, seed))
    N2 = n + m + r
    with dlp.Batch(A, b, c, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        info0 = bt.info()
        assert info0["register_kernel"] == _reg_rule(m, n)
        G, h = _cuts(bt.result.x, n, r, seed)
        h[1] = np.einsum("rj,j->r", G[1], bt.result.x[1]) + 1.0   # LP 1: slack cuts, nothing to do
        before = [bt.read(k) for k in range(NLP)]
        res = bt.add_rows(G, h, max_pivots=0, **KW)
        assert not res.num_pivots.any() and bt.m == m + r
        info = bt.info()
        assert (info["nlp"], info["m"], info["n"]) == (NLP, m + r, n)
        assert info["device_bytes"] >= info0["device_bytes"] + 8 * NLP * r * (n + 2)
        assert info["register_kernel"] == _reg_rule(m + r, n) == bt.rhs_kernel()["register_kernel"]
        statuses = set()
        for k in range(NLP):
            T0, basis0 = before[k]
            T2, basis2 = AR.add_rows(T0, basis0, n, G[k], h[k])
            T1, basis1 = bt.read(k)
            new = np.nonzero(BH._bits(T1[m:m + r]) != BH._bits(T2[m:m + r]))
            assert len(new[0]) == 0, f"LP {k}: new rows differ at {list(zip(*new))[:8]}"
            assert T1.tobytes() == T2.tobytes(), f"LP {k}: an old row, the objective row or a basic column changed"
            assert basis1.tobytes() == basis2.tobytes() == res.basis[k].tobytes(), k
            assert list(basis1[m:]) == list(range(n + m, N2))
            want = L.PIVOT_LIMIT if len(RR.eligible_rows(T2[:m + r, N2])) else L.OK
            assert res.status[k] == want, (k, res.status[k], want)
            assert np.float64(res.objective[k]).tobytes() == np.float64(T0[m, n + m]).tobytes()
            statuses.add(int(res.status[k]))
        assert statuses == {L.OK, L.PIVOT_LIMIT} and res.status[1] == L.OK


# ---- 2. the full phase
@pytest.mark.parametrize("degen", [False, True], ids=["dense", "degenerate"])
@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("m,n,r", SHAPES)
def test_warm_resolve_after_added_rows(m, n, r, pricing, degen):
    seed = 9300 + 11 * n + 2 * r + degen
    A, b, c = BD._stack(BH._lps(m, n, seed, degen))
    with dlp.Batch(A, b, c, pricing=pricing, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        G, h = _cuts(bt.result.x, n, r, seed)
        res, refs, _ = _add_step(bt, G, h, "warm", pricing=pricing)
        after = bt.resolve(None, **KW)   # after DLP_OK: as after any optimal solve
        assert bt.info()["register_kernel"] == _reg_rule(m + r, n)
    assert (res.status == L.OK).all(), res.status
    done = [ref["done"] for ref in refs]
    assert sum(d >= 1 for d in done) >= NLP // 2, done
    assert (after.status == L.OK).all() and not after.num_pivots.any()
    assert after.objective.tobytes() == res.objective.tobytes() and after.x.tobytes() == res.x.tobytes()
    A2, b2 = np.concatenate([A, G], axis=1), np.concatenate([b, h], axis=1)
    if (b2 >= 0.0).all():
        cold = dlp.batched_solve_dense(A2, b2, c, pricing=pricing)
        assert (cold.status == L.OK).all()
        for k in range(NLP):
            assert abs(res.objective[k] - cold.objective[k]) <= 1e-9 * max(1.0, abs(cold.objective[k])), k


# ---- 3. the budget: 1 pivot, then r = 0 calls
@pytest.mark.parametrize("m,n,r", SHAPES[:3])
def test_budget_steps_give_the_unbounded_call_bits(m, n, r):
    seed = 9500 + n
    A, b, c = BD._stack(BH._lps(m, n, seed))
    with dlp.Batch(A, b, c, **KW) as bt:
        G, h = _cuts(bt.result.x, n, r, seed, depth=0.3)
        whole = bt.add_rows(G, h, **KW)
    assert (whole.status == L.OK).all() and whole.num_pivots.max() >= 2
    logs = [[] for _ in range(NLP)]
    final = {}
    with dlp.Batch(A, b, c, **KW) as bt:
        cont = [None] * NLP
        for t in range(4 * int(whole.num_pivots.max()) + 2):
            step, refs, _ = _add_step(bt, G if t == 0 else None, h if t == 0 else None, f"step {t}", max_pivots=1,
                                      continued=cont)
            cont = [ref["bland"] if ref["status"] == L.PIVOT_LIMIT else None for ref in refs]
            assert set(step.status) <= {L.OK, L.PIVOT_LIMIT} and (step.num_pivots <= 1).all()
            for k in range(NLP):
                if k not in final:
                    logs[k].append(step.logs[k][:step.num_pivots[k]])
                    if step.status[k] == L.OK:
                        final[k] = (step.objective[k], step.basis[k].copy(), step.x[k].copy(), step.y[k].copy())
            if len(final) == NLP:
                break
        assert len(final) == NLP and t >= 2 and bt.m == m + r
    for k in range(NLP):
        got, want = np.concatenate(logs[k]), whole.logs[k][:whole.num_pivots[k]]
        assert got.tobytes() == want.tobytes(), k
        assert np.float64(final[k][0]).tobytes() == np.float64(whole.objective[k]).tobytes(), k
        assert final[k][1].tobytes() == whole.basis[k].tobytes(), k
        assert final[k][2].tobytes() == whole.x[k].tobytes() and final[k][3].tobytes() == whole.y[k].tobytes(), k


# ---- 4. one (r, n) / (r,) for all LPs
@pytest.mark.parametrize("m,n,r", [SHAPES[0], SHAPES[2]])
def test_shared_rows_equal_tiled_rows(m, n, r):
    seed = 9700 + n
    A, b, c = BD._stack(BH._lps(m, n, seed))
    with dlp.Batch(A, b, c, **KW) as one, dlp.Batch(A, b, c, **KW) as tiled:
        G = AR.cuts(one.result.x[0], n, r, seed)[0]
        h = 0.95 * (one.result.x @ G.T).min(axis=0)
        r1 = one.add_rows(G, h, **KW)
        r2 = tiled.add_rows(np.tile(G, (NLP, 1, 1)), np.tile(h, (NLP, 1)), **KW)
        BD._same_bytes(r1, r2)
        assert r1.num_pivots.all() and (r1.status == L.OK).all()
        for k in range(NLP):
            assert one.read(k)[0].tobytes() == tiled.read(k)[0].tobytes()
        # mixed: per-LP G with one h for all
        r3 = one.add_rows(np.tile(G, (NLP, 1, 1)), h - 0.01, **KW)
        r4 = tiled.add_rows(G, np.tile(h - 0.01, (NLP, 1)), **KW)
        BD._same_bytes(r3, r4)
        assert one.m == tiled.m == m + 2 * r


# ---- 5. device tensors give the bytes of the host-array call (in a child process: torch brings
# its own HIP runtime, see tests/test_gpu_batched_dense.py)
DEVICE_SCRIPT = r"""
import json, sys
import torch
torch.cuda.init()
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import oracle_py as O
import rows_ref as AR
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
for m, n, r in ((64, 100, 1), (37, 53, 3)):
    lps = [O.gen_dense(m, n, 9800 + k) for k in range(6)]
    A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
    with dlp.Batch(A, b, c, **KW) as host, dlp.Batch(*(dev0(v) for v in (A, b, c)), **KW) as dev:
        ok = same(host.result, dev.result)
        G, h = (np.stack(v) for v in zip(*(AR.cuts(host.result.x[k], n, r, 9850 + k) for k in range(6))))
        rh, rd = host.add_rows(G, h, **KW), dev.add_rows(dev0(G), dev0(h), **KW)
        ok = ok and same(rh, rd) and int(rh.num_pivots.sum()) > 0 and host.m == dev.m == m + r
        ok = ok and all(host.read(k)[0].tobytes() == dev.read(k)[0].tobytes() for k in range(6))
        out[f"{m}x{n} device rows"] = bool(ok)
        G1, h1 = G[0], 0.9 * (rh.x @ G[0].T).min(axis=0)            # shared rows, the second growth
        view = dev0(G1.T).T                                           # has to be made contiguous
        rh, rd = host.add_rows(G1, h1, **KW), dev.add_rows(view, dev0(h1), **KW)
        out[f"{m}x{n} shared view"] = (not view.is_contiguous() or r == 1) and same(rh, rd) and host.m == dev.m == m + 2 * r
        bad = dev0(G)
        bad[4, 0, 3] = float("nan")                                  # the kernel's check sees device inputs too
        try:
            dev.add_rows(bad, dev0(h), **KW)
            seen = False
        except dlp.DLPError as e:
            seen = e.status == -1 and "LP 4" in str(e)
        out[f"{m}x{n} nan seen"] = seen and dev.m == m + 2 * r and \
            all(host.read(k)[0].tobytes() == dev.read(k)[0].tobytes() for k in range(6))
        out[f"{m}x{n} float32 raises"] = raises(dev.add_rows, dev0(G).float(), dev0(h))
        out[f"{m}x{n} cpu tensor raises"] = raises(dev.add_rows, dev0(G).cpu(), dev0(h))
        out[f"{m}x{n} mixed raises"] = raises(dev.add_rows, dev0(G), h)
print(json.dumps(out))
"""


def test_device_rows_give_the_host_bytes():
    p = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT, ROOT], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(out) == 12 and all(out.values()), out


# ---- 6. per-LP outcomes in one batch
def _highs_obj(A, b, c):
    res = linprog(-c, A_ub=A, b_ub=b, bounds=(0, None), method="highs")
    assert res.status == 0
    return -res.fun


@pytest.mark.parametrize("m,n", [(63, 100), (37, 53)], ids=["63x100", "37x53"])
def test_every_outcome_in_one_batch(m, n):
    """[rejected at creation, optimal x 2, stopped inside its primal solve, optimal x 2].  Cuts no
    feasible x violates (h = G ub + 1 with ub_j = min_i b_i / A_ij): the stopped LP reports
    ERR_STATE, its rows follow the rule, its stored status stays, and resolve(None) finishes
    it on the larger LP.  Then a cut its vertex violates: the record is stored pending and both
    resolve calls refuse it."""
    seed = 9900 + m
    r = 2
    lps, budget = BH._outcome_batch(m, n, seed)
    A, b, c = BD._stack(lps)
    rng = np.random.default_rng(seed)
    G = rng.uniform(0.0, 1.0, (NLP, r, n)) * (rng.uniform(size=(NLP, r, n)) >= 0.3)
    with np.errstate(divide="ignore"):
        ub = np.where(A > 0.0, np.abs(b)[:, :, None] / A, np.inf).min(axis=1)
    assert np.isfinite(ub).all()
    h = np.einsum("krj,kj->kr", G, ub) + 1.0
    with dlp.Batch(A, b, c, max_pivots=budget, **KW) as bt:
        assert list(bt.result.status) == [L.ERR_ARG, L.OK, L.OK, L.PIVOT_LIMIT, L.OK, L.OK]
        res, refs, _ = _add_step(bt, G, h, "outcomes")
        assert list(res.status) == [L.ERR_ARG, L.OK, L.OK, L.ERR_STATE, L.OK, L.OK]
        assert not res.num_pivots.any()
        np.testing.assert_array_equal(res.basis[3][:m], bt.result.basis[3])
        fin = bt.resolve(None, max_pivots=BIG, **KW)
        assert list(fin.status) == [L.ERR_ARG] + [L.OK] * 5 and fin.num_pivots[3] > 0
        assert fin.basis.shape == (NLP, m + r)
        for k in range(1, NLP):
            obj = _highs_obj(np.vstack([A[k], G[k]]), np.concatenate([b[k], h[k]]), c[k])
            assert abs(fin.objective[k] - obj) <= 1e-9 * max(1.0, abs(obj)), (k, fin.objective[k], obj)
        # an r = 0 call: nothing to do, the rejected LP stays rejected
        again, _, _ = _add_step(bt, None, None, "r = 0")
        assert list(again.status) == [L.ERR_ARG] + [L.OK] * 5 and not again.num_pivots.any()
    with dlp.Batch(A, b, c, max_pivots=budget, **KW) as bt:
        h2 = h.copy()
        h2[3, 1] = -1.0
        res, refs, grown = _add_step(bt, G, h2, "stopped and cut")
        assert res.status[3] == L.ERR_STATE and grown[3][0][m + 1, n + m + r] <= -1.0
        T3, basis3 = bt.read(3)
        b2 = np.concatenate([b, h2], axis=1)
        for rp in (bt.resolve(None, max_pivots=BIG, **KW), bt.resolve_rhs(b2, **KW)):
            assert rp.status[3] == L.ERR_STATE and rp.num_pivots[3] == 0 and np.isnan(rp.objective[3])
            np.testing.assert_array_equal(rp.basis[3], basis3)
            T, basis = bt.read(3)
            assert T.tobytes() == T3.tobytes() and basis.tobytes() == basis3.tobytes()
            BR._is_rejected(rp, 0, m + r, n)
            assert (np.delete(rp.status, [0, 3]) == L.OK).all()


# ---- 7. the infeasible cut
@pytest.mark.parametrize("m,n,r", SHAPES)
def test_a_nonnegative_row_with_a_negative_h_is_infeasible(m, n, r):
    seed = 10100 + n
    A, b, c = BD._stack(BH._lps(m, n, seed))
    with dlp.Batch(A, b, c, **KW) as bt:
        G, h = _cuts(bt.result.x, n, r, seed)
        h[:, r - 1] = -1.0
        assert (G >= 0.0).all()
        res, refs, _ = _add_step(bt, G, h, "infeasible")
        assert (res.status == L.INFEASIBLE).all()
        # an LP left infeasible is accepted again: the rows are added, the dual phase runs
        G2, _ = _cuts(bt.result.x, n, 1, seed + 50)
        res2, refs2, _ = _add_step(bt, G2, G2.sum(axis=2) + 100.0, "infeasible again")
        assert (res2.status == L.INFEASIBLE).all() and bt.m == m + r + 1
        rp = bt.resolve(None, **KW)   # the primal rule refuses it
        assert (rp.status == L.ERR_STATE).all()


# ---- 8. a row that is not finite fails the whole call
@pytest.mark.parametrize("where,value,first", [
    (("G", 4, 0, 3), np.nan, 4), (("h", 2, 0), np.inf, 2), (("G", 5, -1, -1), -np.inf, 1), (("h", 0, -1), np.nan, 0),
], ids=["nan in G", "inf in h", "-inf in G, nan in h before it", "nan in h of LP 0"])
@pytest.mark.parametrize("m,n,r", [SHAPES[0], SHAPES[2]])
def test_a_row_that_is_not_finite_fails_the_whole_call(m, n, r, where, value, first):
    seed = 10300 + n
    A, b, c = BD._stack(BH._lps(m, n, seed))
    b2 = BH.perturbed(b, seed)
    with dlp.Batch(A, b, c, **KW) as bt, dlp.Batch(A, b, c, **KW) as twin:
        G, h = _cuts(bt.result.x, n, r, seed)
        bad = {"G": G.copy(), "h": h.copy()}
        bad[where[0]][where[1:]] = value
        if first != where[1]:
            bad["h"][first, 0] = np.nan
        before = [bt.read(k) for k in range(NLP)]
        info0 = bt.info()
        with pytest.raises(dlp.DLPError) as e:
            bt.add_rows(bad["G"], bad["h"], **KW)
        assert e.value.status == L.ERR_ARG and f"LP {first}:" in str(e.value) and "dlp_batch_add_rows" in str(e.value)
        assert bt.m == m and bt.info() == info0
        for k in range(NLP):
            T1, basis1 = bt.read(k)
            assert T1.tobytes() == before[k][0].tobytes() and basis1.tobytes() == before[k][1].tobytes()
        r1, r2 = bt.resolve_rhs(b2, **KW), twin.resolve_rhs(b2, **KW)
        BD._same_bytes(r1, r2)
        assert r1.num_pivots.sum() > 0
        assert bt.info() == twin.info()
        # and the call still works afterwards
        BD._same_bytes(bt.add_rows(G, h, **KW), twin.add_rows(G, h, **KW))


def test_the_output_arrays_of_a_failed_call_are_untouched():
    m, n, r = 37, 53, 2
    A, b, c = BD._stack(BH._lps(m, n, 10400))
    lib = L.lib()
    with dlp.Batch(A, b, c, **KW) as bt:
        G, h = _cuts(bt.result.x, n, r, 10400)
        G[3, 1, 7] = np.nan
        obj = np.full(NLP, 7.0)
        st = np.full(NLP, 77, np.int32)
        npv = np.full(NLP, 777, np.int64)
        basis = np.full((NLP, m + r), 7777, np.int32)
        x, y = np.full((NLP, n), 7.5), np.full((NLP, m + r), 7.25)
        ms = C.c_double(-1.0)
        out = L.BatchOut(obj.ctypes.data_as(C.POINTER(C.c_double)), st.ctypes.data_as(C.POINTER(C.c_int32)),
                         npv.ctypes.data_as(C.POINTER(C.c_int64)), basis.ctypes.data_as(C.POINTER(C.c_int32)), None, 0,
                         x.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double)), C.pointer(ms))
        rc = lib.dlp_batch_add_rows(bt._h, r, G.ctypes.data, r * n, h.ctypes.data, r, 0, BIG, C.byref(out))
        assert rc == L.ERR_ARG and b"LP 3" in lib.dlp_last_error()
        assert (obj == 7.0).all() and (st == 77).all() and (npv == 777).all() and (basis == 7777).all()
        assert (x == 7.5).all() and (y == 7.25).all() and ms.value == -1.0


# ---- 9. a shape that fits at m and not at m + r; the other call-level errors
def _lds_bytes(m, n):
    return 8 * ((m + 1) * (n + 1) + (m + 1) + (n + 1)) + 4 * (n + m + 8) + 16 + 16


def test_growth_past_the_lds_is_unsupported():
    m, n, nlp = 40, 400, 2
    assert _lds_bytes(m + 8, n) <= 160 * 1024 < _lds_bytes(m + 9, n)
    A, b, c = BD._stack(BH._lps(m, n, 10500, nlp=nlp))
    rng = np.random.default_rng(10500)
    with dlp.Batch(A, b, c, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        G9 = rng.uniform(0.0, 1.0, (nlp, 9, n))
        h9 = 0.95 * np.einsum("krj,kj->kr", G9, bt.result.x)
        before = [bt.read(k) for k in range(nlp)]
        info0 = bt.info()
        with pytest.raises(dlp.DLPError) as e:
            bt.add_rows(G9, h9, **KW)
        assert e.value.status == L.ERR_UNSUPPORTED and bt.m == m and bt.info() == info0
        for k in range(nlp):
            T1, basis1 = bt.read(k)
            assert T1.tobytes() == before[k][0].tobytes() and basis1.tobytes() == before[k][1].tobytes()
        # eight of them fit: the largest tableau the launch takes, all its rows in one pass
        before = [bt.read(k) for k in range(nlp)]
        res = bt.add_rows(G9[:, :8], h9[:, :8], **KW)
        assert (res.status == L.OK).all() and res.num_pivots.all() and bt.m == m + 8
        for k in range(nlp):
            ref = AR.add_rows_and_solve(*before[k], n, G9[k, :8], h9[k, :8])
            assert res.num_pivots[k] == ref["done"]
            assert np.float64(res.objective[k]).tobytes() == np.float64(ref["objective"]).tobytes()
            assert res.basis[k].tobytes() == ref["basis"].tobytes()
            assert np.array_equal(bt.read(k)[0], ref["T"])
        with pytest.raises(dlp.DLPError) as e:
            bt.add_rows(G9[:, :1], h9[:, :1], **KW)
        assert e.value.status == L.ERR_UNSUPPORTED and bt.m == m + 8


def test_call_level_errors_leave_the_batch_unchanged():
    m, n, r = 37, 53, 2
    A, b, c = BD._stack(BH._lps(m, n, 10600))
    lib = L.lib()
    with dlp.Batch(A, b, c, **KW) as bt:
        G, h = _cuts(bt.result.x, n, r, 10600)
        before = [bt.read(k) for k in range(NLP)]
        info0 = bt.info()
        out, bad_log = L.BatchOut(), L.BatchOut()
        bad_log.log_cap = -1
        pG, ph = G.ctypes.data, h.ctypes.data
        call = lambda *a: lib.dlp_batch_add_rows(bt._h, *a)
        lib.dlp_batch_resolve(None, None, 0, 0, 10, None)   # (another name in dlp_last_error)
        assert call(r, pG, r * n - 1, ph, r, 0, 10, C.byref(out)) == L.ERR_ARG      # 0 < strideG < r * n
        assert b"dlp_batch_add_rows" in lib.dlp_last_error()
        assert call(r, pG, r * n, ph, r - 1, 0, 10, C.byref(out)) == L.ERR_ARG      # 0 < strideh < r
        assert call(r, pG, -r * n, ph, r, 0, 10, C.byref(out)) == L.ERR_ARG
        assert call(r, pG, r * n, ph, r, 2, 10, C.byref(out)) == L.ERR_ARG          # rows_are_device
        assert call(r, pG, r * n, ph, r, 0, -1, C.byref(out)) == L.ERR_ARG          # max_pivots
        assert call(r, None, r * n, ph, r, 0, 10, C.byref(out)) == L.ERR_ARG
        assert call(r, pG, r * n, None, r, 0, 10, C.byref(out)) == L.ERR_ARG
        assert call(-1, pG, r * n, ph, r, 0, 10, C.byref(out)) == L.ERR_ARG
        assert call(r, pG, r * n, ph, r, 0, 10, C.byref(bad_log)) == L.ERR_ARG
        assert bt.info() == info0
        for k in range(NLP):
            T1, basis1 = bt.read(k)
            assert T1.tobytes() == before[k][0].tobytes() and basis1.tobytes() == before[k][1].tobytes()
        assert call(0, None, 0, None, 0, 0, BIG, None) == L.OK                      # r = 0, out may be NULL
        assert bt.info() == info0
        # padded strides: LP k's rows at G + k * strideG
        Gp, hp = np.zeros((NLP, r * n + 5)), np.zeros((NLP, r + 3))
        Gp[:, :r * n], hp[:, :r] = G.reshape(NLP, -1), h
        with dlp.Batch(A, b, c, **KW) as twin:
            want = twin.add_rows(G, h, **KW)
        o, result = dlp.solver._batch_outputs(NLP, m + r, n, True, True, True, LOG_CAP)
        assert call(r, Gp.ctypes.data, r * n + 5, hp.ctypes.data, r + 3, 0, BIG, C.byref(o)) == L.OK
        bt.m += r
        BD._same_bytes(result(), want)


# ---- 10. twice, then new right-hand sides and new objectives on the grown batch
@pytest.mark.parametrize("m,n", [(64, 100), (63, 100), (37, 53), (5, 7)], ids=["64x100", "63x100", "37x53", "5x7"])
def test_add_rows_twice_then_the_other_calls(m, n):
    """m -> m + 1 -> m + 3, then resolve_rhs with an (m + 3)-vector against rhs_ref and resolve(c2)
    against the numpy primal rule, on whichever kernel the grown shape takes (63 x 100 gains the
    register kernel at 64 rows and leaves it again at 66; 64 x 100 leaves it at 65)."""
    seed = 10700 + n
    lps = BH._lps(m, n, seed)
    A, b, c = BD._stack(lps)
    with dlp.Batch(A, b, c, **KW) as bt:
        G1, h1 = _cuts(bt.result.x, n, 1, seed)
        r1, _, _ = _add_step(bt, G1, h1, "first")
        assert (r1.status == L.OK).all() and bt.m == m + 1
        assert bt.info()["register_kernel"] == _reg_rule(m + 1, n) == bt.rhs_kernel()["register_kernel"]
        if m + 1 == 64:   # the grown record on the register kernel: both resolve calls, then back
            bmid = BH.perturbed(np.concatenate([b, h1], axis=1), seed + 1)
            rr, refs = BH._rhs_step(bt, bmid, "register rhs")
            assert (rr.status == L.OK).all() and rr.num_pivots.sum() > 0
            c = _resolve_c2(bt, lps, seed + 2)
        G2, h2 = _cuts(bt.resolve(None, **KW).x, n, 2, seed + 3)
        r2, _, _ = _add_step(bt, G2, h2, "second")
        assert (r2.status == L.OK).all() and bt.m == m + 3 and r2.num_pivots.sum() > 0
        assert bt.info()["register_kernel"] == _reg_rule(m + 3, n) == bt.rhs_kernel()["register_kernel"]
        b3 = BH.perturbed(np.concatenate([b, h1, h2], axis=1), seed + 4)
        r3, refs3 = BH._rhs_step(bt, b3, "rhs on m + 3")
        assert (r3.status == L.OK).all() and r3.num_pivots.sum() > 0
        # one pivot per call on the grown batch: the continuation through the new `last` record
        b4 = BH.perturbed(b3, seed + 5, 0.1)
        cont = [None] * NLP
        for t in range(3):
            r4, refs4 = BH._rhs_step(bt, b4, f"rhs step {t}", max_pivots=1, continued=cont)
            cont = [ref["bland"] if ref["status"] == L.PIVOT_LIMIT else None for ref in refs4]
        _resolve_c2(bt, lps, seed + 6, pending=[k for k in range(NLP) if cont[k] is not None])
    cold = dlp.batched_solve_dense(np.concatenate([A, G1, G2], axis=1), b3, c)   # (c: as it stood at r3)
    for k in range(NLP):
        if cold.status[k] == L.OK:
            assert abs(r3.objective[k] - cold.objective[k]) <= 1e-9 * max(1.0, abs(cold.objective[k])), k


def _resolve_c2(bt, lps, seed, pending=()):
    """resolve(c2) on the batch as it stands against test_gpu_batch_rhs.primal_continue from the
    read-out before it (a pending LP is refused)."""
    n = bt.n
    c2 = np.stack([R.make_c2(lp[2], seed + k, holes=False) for k, lp in enumerate(lps)])
    before = [bt.read(k) for k in range(NLP)]
    res = bt.resolve(c2, **KW)
    for k, (T0, basis0) in enumerate(before):
        if k in pending:
            assert res.status[k] == L.ERR_STATE
            continue
        status, basis, log, obj, _ = BH.primal_continue(T0, basis0, n, c2[k])
        got = [(int(e["q"]), int(e["p"]), int(e["leaving"])) for e in res.logs[k][:res.num_pivots[k]]]
        assert res.status[k] == status and got == log, (k, res.status[k], status, got[:4], log[:4])
        assert np.float64(res.objective[k]).tobytes() == np.float64(obj).tobytes(), (k, res.objective[k], obj)
        np.testing.assert_array_equal(res.basis[k], basis, err_msg=f"resolve(c2) LP {k}")
    return c2
