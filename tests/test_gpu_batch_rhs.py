"""GPU: dlp_batch_resolve_rhs / Batch.resolve_rhs, the resident batch re-solved by the dual
simplex after new right-hand sides (include/dlp.h).

Reference: tests/rhs_ref.py (the rule in numpy with a real fma, itself held against HiGHS by
tests/test_batch_rhs_api.py) applied to ``bt.read(k)`` taken before the call.

Bar, as in tests/test_gpu_batch_resolve.py: status, pivot count, basis, objective and every
pivot-log entry are bit-identical; x, y and the tableau read-out afterwards are equal as values
(np.array_equal: the sign of a zero is exempt, the condensed tableau's own exemption)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import reopt_ref as R
import rhs_ref as RR
import test_gpu_batch_resolve as BR
import test_gpu_batched_dense as BD
from conftest import ROOT

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

pytestmark = pytest.mark.gpu

LOG_CAP = BD.LOG_CAP
NLP = 6
BIG = 10 ** 6
KW = dict(want_basis=True, log_cap=LOG_CAP)
KERNELS = [pytest.param(64, 100, id="register"), pytest.param(37, 53, id="lds")]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _lps(m, n, seed, degen=False, nlp=NLP):
    return [BD._gen(m, n, seed + k, degen) for k in range(nlp)]


def perturbed(b, seed, scale=0.02):
    """b * (1 + scale * u), u ~ U(-1, 1) seeded."""
    return np.ascontiguousarray(b * (1.0 + scale * np.random.default_rng(seed).uniform(-1.0, 1.0, b.shape)))


def _same_ref(res, k, ref, what=""):
    """LP k of one resolve_rhs call against the reference's run from the state before it."""
    tag = f"{what} LP {k}"
    assert res.status[k] == ref["status"], (tag, res.status[k], ref["status"])
    assert res.num_pivots[k] == ref["done"], (tag, res.num_pivots[k], ref["done"])
    np.testing.assert_array_equal(res.basis[k], ref["basis"], err_msg=tag)
    if ref["status"] < 0:
        assert np.isnan(res.objective[k]) and np.isnan(res.x[k]).all() and np.isnan(res.y[k]).all(), tag
        return
    assert np.float64(res.objective[k]).tobytes() == np.float64(ref["objective"]).tobytes(), \
        (tag, res.objective[k], ref["objective"])
    cnt = min(ref["done"], LOG_CAP)
    got, want = np.ascontiguousarray(res.logs[k][:cnt]), np.ascontiguousarray(ref["log"][:cnt])
    if got.tobytes() != want.tobytes():
        for i in range(cnt):
            assert got[i].tobytes() == want[i].tobytes(), f"{tag} pivot {i}: batch {got[i]} reference {want[i]}"
    assert np.array_equal(res.x[k], ref["x"]), (tag, np.flatnonzero(res.x[k] != ref["x"])[:8])
    assert np.array_equal(res.y[k], ref["y"]), (tag, np.flatnonzero(res.y[k] != ref["y"])[:8])


def _rhs_step(bt, b2, what="", max_pivots=BIG, pricing=0, continued=None):
    """One resolve_rhs call on the whole batch, every LP checked against the reference from
    its read-out before the call, the read-out afterwards included (a refused LP: the same
    bytes).  continued[k]: None, or the Bland state LP k's pending dual phase was left in by the
    previous call with this very b2 (the continuation of dlp.h).  Returns (result, references)."""
    n = bt.n
    before = [bt.read(k) for k in range(bt.nlp)]
    res = bt.resolve_rhs(b2, max_pivots=max_pivots, **KW)
    refs = []
    for k, (T0, basis0) in enumerate(before):
        bk = b2 if b2.ndim == 1 else b2[k]
        rejected = bt.result.status[k] == L.ERR_ARG
        if rejected:   # at creation: in every later call, the slack basis
            BR._is_rejected(res, k, bt.m, n)
            ref = None
        else:
            ref = RR.resolve_rhs(T0, basis0, n, bk, max_pivots=max_pivots, pricing=pricing,
                                 continued=continued[k] if continued else None)
            _same_ref(res, k, ref, what)
        T1, basis1 = bt.read(k)
        if ref is None or ref["status"] < 0:
            assert T1.tobytes() == T0.tobytes() and basis1.tobytes() == basis0.tobytes(), f"{what} LP {k}: state"
        else:
            assert np.array_equal(T1, ref["T"]), f"{what} LP {k}: tableau"
            assert basis1.tobytes() == ref["basis"].tobytes()
        refs.append(ref)
    return res, refs


# ---- 1. the rule alone
@pytest.mark.parametrize("m,n", [pytest.param(64, 130, id="register"), pytest.param(37, 53, id="lds"),
                                 pytest.param(5, 7, id="5x7")])
def test_rhs_column_follows_the_rule(m, n):
    seed = 7100 + n
    lps = _lps(m, n, seed)
    N = n + m
    A, b, c = BD._stack(lps)
    b2 = perturbed(b, seed, 0.3)
    with dlp.Batch(A, b, c, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        before = [bt.read(j) for j in range(NLP)]
        res = bt.resolve_rhs(b2, max_pivots=0, **KW)
        assert not res.num_pivots.any()
        assert bt.info()["register_kernel"] == (m == 64)
        statuses = set()
        for j in range(NLP):
            T0, basis0 = before[j]
            T1, basis1 = bt.read(j)
            assert basis1.tobytes() == basis0.tobytes() == res.basis[j].tobytes(), j
            rhs = RR.fold_rhs(T0, n, b2[j])
            bad = np.nonzero(_bits(T1[:, N]) != _bits(rhs))[0]
            assert len(bad) == 0, f"LP {j}: RHS differs at rows {bad[:8]}: {T1[bad[:8], N]} vs {rhs[bad[:8]]}"
            keep = np.arange(T0.shape[1]) != N
            assert T1[:, keep].tobytes() == T0[:, keep].tobytes(), f"LP {j}: an entry outside the RHS column changed"
            assert np.float64(res.objective[j]).tobytes() == np.float64(rhs[m]).tobytes()
            want = L.PIVOT_LIMIT if len(RR.eligible_rows(rhs[:m])) else L.OK
            assert res.status[j] == want, (j, res.status[j], want)
            statuses.add(int(res.status[j]))
        assert L.PIVOT_LIMIT in statuses   # (30 % moves some basis at every shape)
        # the b of creation: the optimum's status again, no pivot (pending LPs are accepted again)
        again = bt.resolve_rhs(b, max_pivots=0, **KW)
        assert (again.status == L.OK).all() and not again.num_pivots.any()
        assert again.basis.tobytes() == bt.result.basis.tobytes()
        for j in range(NLP):
            assert abs(again.objective[j] - bt.result.objective[j]) <= 1e-9 * max(1.0, abs(bt.result.objective[j]))
        one = bt.resolve_rhs(b[0], max_pivots=0, **KW)   # one (m,) b for all: stride 0
        for j in range(NLP):
            rhs = RR.fold_rhs(before[j][0], n, b[0])
            assert np.float64(one.objective[j]).tobytes() == np.float64(rhs[m]).tobytes(), j


# ---- 2. warm dual re-solve from the optimum
WARM_SEEDS = {(64, 100, False): 7300, (64, 100, True): 7320, (37, 53, False): 7340, (37, 53, True): 7360}


@pytest.mark.parametrize("degen", [False, True], ids=["dense", "degenerate"])
@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("m,n", KERNELS)
def test_warm_dual_resolve(m, n, pricing, degen):
    seed = WARM_SEEDS[m, n, degen]
    A, b, c = BD._stack(_lps(m, n, seed, degen))
    b2 = perturbed(b, seed)
    with dlp.Batch(A, b, c, pricing=pricing, **KW) as bt:
        assert (bt.result.status == L.OK).all()
        res, refs = _rhs_step(bt, b2, "warm", pricing=pricing)
        after = bt.resolve(None, **KW)   # after DLP_OK: as after any optimal solve
    done = [r["done"] for r in refs]
    assert sum(d >= 1 for d in done) >= NLP // 2 and max(done) >= 2, done
    assert (res.status == L.OK).all()
    assert (after.status == L.OK).all() and not after.num_pivots.any()
    assert after.objective.tobytes() == res.objective.tobytes() and after.x.tobytes() == res.x.tobytes()
    assert (b2 >= 0.0).all()
    cold = dlp.batched_solve_dense(A, b2, c, pricing=pricing)
    assert (cold.status == L.OK).all()
    for j in range(NLP):
        assert abs(res.objective[j] - cold.objective[j]) <= 1e-9 * max(1.0, abs(cold.objective[j])), j


# ---- 3. negative right-hand sides
def negative_b_batch(m, n, seed):
    """Five degenerate-family LPs with b_i made negative on three cone rows (entries of both
    signs: such a row can still be satisfied), by more from LP to LP, and one dense-family LP
    (A >= 0) with b_3 = -1."""
    lps = _lps(m, n, seed, True, NLP - 1) + [BD._gen(m, n, seed + NLP - 1, False)]
    b2 = np.stack([lp[1] for lp in lps]).copy()
    rng = np.random.default_rng(seed)
    for k, mag in enumerate((0.3, 1.0, 3.0, 10.0, 30.0)):
        cone = (lps[k][0] < 0.0).any(axis=1)
        b2[k, rng.choice(np.nonzero(cone)[0], 3, replace=False)] = -mag * rng.uniform(0.5, 1.0, 3)
    b2[NLP - 1, 3] = -1.0
    return lps, b2


NEG_SEEDS = {(64, 100): 7500, (37, 53): 7502}


@pytest.mark.parametrize("m,n", KERNELS)
def test_negative_b(m, n):
    lps, b2 = negative_b_batch(m, n, NEG_SEEDS[m, n])
    assert (lps[-1][0] >= 0.0).all()
    with dlp.Batch(*BD._stack(lps), **KW) as bt:
        assert (bt.result.status == L.OK).all()
        res, refs = _rhs_step(bt, b2, "negative b")
    assert res.status[NLP - 1] == L.INFEASIBLE
    seen = {int(s) for s in res.status[:NLP - 1]}
    assert seen == {L.OK, L.INFEASIBLE}, res.status
    assert sum(r["status"] == L.OK and r["done"] >= 2 for r in refs) >= 2


# ---- 4. exact ties
def integer_lps(m, n, seed, nlp=NLP):
    """Small-integer LPs (A in {0, 1, 2}, c in {1, 2}, integer b and b2).  The second half of the
    columns copies the first with the same cost and 5 % of the entries one smaller: where such
    a column differs from its basic twin only in rows that are not tight, its z is exactly 0 and
    its entry in the slack's row negative, so the dual ratio is 0 once b2 makes that row
    leave.  The last m // 8 pairs of adjacent rows are twins (the same row of A, b and b2):
    while both slacks are basic the two rows hold the same bits and their rebuilt RHS entries
    are equal exactly (the own slack's term is the only one between l = i and l = i + 1), so the
    row selection ties whenever a twin pair is the most negative."""
    rng = np.random.default_rng(seed)
    lps, b2 = [], []
    h = n // 2
    for _ in range(nlp):
        A = rng.integers(0, 3, (m, n)).astype(np.float64)
        c = rng.integers(1, 3, n).astype(np.float64)
        dec = rng.uniform(size=(m, h)) < 0.05
        A[:, h:2 * h], c[h:2 * h] = np.maximum(A[:, :h] - dec, 0.0), c[:h]
        b = rng.integers(4, 12, m).astype(np.float64)
        bk = np.maximum(b + rng.integers(-3, 2, m), 0.0)
        for i in range(m - 2 * (m // 8), m, 2):   # the last m // 8 pairs of rows: twins
            A[i + 1], b[i + 1], bk[i + 1] = A[i], b[i], bk[i]
        lps.append((A, b, c))
        b2.append(bk)
    return lps, np.stack(b2)


TIE_SEEDS = {(64, 100): 7700, (37, 53): 7720}


def _row_tie(read, bk, ref, n):
    """Does some Dantzig-mode pivot of the reference's run choose among rows that share the most
    negative RHS exactly?  Replays the run one pivot at a time."""
    T, basis = read
    cont = None
    for t in range(ref["done"]):
        if not cont:   # (in Bland mode the row is chosen by the basic variable alone)
            rhs = RR.fold_rhs(T, n, bk)[:-1] if t == 0 else T[:-1, n + len(basis)]
            if (rhs == rhs.min()).sum() >= 2 and rhs.min() < -1e-9:
                return True
        r = RR.resolve_rhs(T, basis, n, bk, max_pivots=1, continued=cont)
        T, basis, cont = r["T"], r["basis"], r["bland"]
    return False


@pytest.mark.parametrize("m,n", KERNELS)
def test_exact_ties(m, n):
    lps, b2 = integer_lps(m, n, TIE_SEEDS[m, n])
    with dlp.Batch(*BD._stack(lps), **KW) as bt:
        assert (bt.result.status == L.OK).all()
        reads = [bt.read(k) for k in range(NLP)]
        res, refs = _rhs_step(bt, b2, "ties")
    assert any((r["log"]["ratio"] == 0.0).any() for r in refs), "no pivot with r_q = 0: Bland mode is not entered"
    assert any(r["done"] >= 2 for r in refs)
    # a tie in the row selection: some pivot's leaving row shares the most negative RHS
    assert any(_row_tie(bt_read, b2[k], r, n) for k, (bt_read, r) in enumerate(zip(reads, refs))), \
        "no tie in the row selection"


def test_exact_ties_continue_in_bland_mode():
    """One pivot per call on the tie LPs: a phase the budget stopped in Bland mode goes on in it
    (the continuation of dlp.h), and ends in the basis of one unbounded call."""
    m, n = 37, 53
    lps, b2 = integer_lps(m, n, TIE_SEEDS[m, n])
    with dlp.Batch(*BD._stack(lps), **KW) as bt:
        res, refs = _rhs_step(bt, b2, "ties")
    in_bland = False
    with dlp.Batch(*BD._stack(lps), **KW) as bt:
        cont = [None] * NLP
        for t in range(max(r["done"] for r in refs) + 2):
            step, srefs = _rhs_step(bt, b2, f"ties step {t}", max_pivots=1, continued=cont)
            cont = [r["bland"] if r["status"] == L.PIVOT_LIMIT else None for r in srefs]
            in_bland = in_bland or any(c is True for c in cont)
            if (step.status == L.OK).all():
                break
        assert (step.status == L.OK).all() and in_bland
        assert step.basis.tobytes() == res.basis.tobytes()


# ---- 5. every outcome in one batch
@functools.lru_cache(maxsize=None)
def _outcome_batch(m, n, seed):
    """[rejected at creation, a NaN in b_k, an inf in b_k, stopped inside its primal solve,
    optimal, infeasible] and the creation budget that stops LP 3 alone."""
    cand = sorted(range(8), key=lambda k: BD._gen_ref(m, n, seed + k).num_pivots)
    counts = [BD._gen_ref(m, n, seed + k).num_pivots for k in cand]
    assert counts[-1] > counts[4] + 1   # the longest solve is stopped, the five shortest finish
    order = [cand[0], cand[1], cand[2], cand[-1], cand[3], cand[4]]
    lps = [tuple(v.copy() for v in BD._gen(m, n, seed + k)) for k in order]
    lps[0][1][m - 1] = -1.0
    return lps, counts[4] + 1   # (one more: optimality is seen by the pricing after the last pivot)


@pytest.mark.parametrize("m,n", KERNELS)
def test_every_outcome_in_one_batch(m, n):
    seed = 7900 + m
    lps, budget = _outcome_batch(m, n, seed)
    A, b, c = BD._stack(lps)
    b2 = perturbed(b, seed)
    b2[1, m // 3] = np.nan
    b2[2, 0] = -np.inf
    b2[5, 3] = -1.0
    c2 = np.stack([BR._c2(m, n, seed, False, j) for j in range(NLP)])
    with dlp.Batch(A, b, c, max_pivots=budget, **KW) as bt:
        r0 = bt.result
        assert list(r0.status) == [L.ERR_ARG, L.OK, L.OK, L.PIVOT_LIMIT, L.OK, L.OK]
        res, refs = _rhs_step(bt, b2, "outcomes")   # (refused LPs: the state's bytes are compared)
        assert list(res.status) == [L.ERR_ARG, L.ERR_ARG, L.ERR_ARG, L.ERR_STATE, L.OK, L.INFEASIBLE]
        for j in (1, 2, 3):
            np.testing.assert_array_equal(res.basis[j], r0.basis[j])
        # the primal calls refuse the infeasible LP and leave it untouched
        T5, basis5 = bt.read(5)
        for cc in (c2, None):
            rp = bt.resolve(cc, max_pivots=BIG, **KW)
            assert rp.status[5] == L.ERR_STATE and rp.num_pivots[5] == 0
            assert np.isnan(rp.objective[5]) and np.isnan(rp.x[5]).all() and np.isnan(rp.y[5]).all()
            np.testing.assert_array_equal(rp.basis[5], basis5)
            T, basis = bt.read(5)
            assert T.tobytes() == T5.tobytes() and basis.tobytes() == basis5.tobytes()
            BR._is_rejected(rp, 0, m, n)
            assert (rp.status[1:5] == L.OK).all()
        # the original b brings it back
        back, refs = _rhs_step(bt, b, "back")
        assert list(back.status) == [L.ERR_ARG] + [L.OK] * 5
        fin = bt.resolve(None, **KW)
        assert list(fin.status) == [L.ERR_ARG] + [L.OK] * 5 and not fin.num_pivots.any()
        assert fin.objective[1:].tobytes() == back.objective[1:].tobytes()


# ---- 6. the budget
def _budget_batch(m, n):
    seed = WARM_SEEDS[m, n, False]
    A, b, c = BD._stack(_lps(m, n, seed))
    return A, b, c, perturbed(b, seed)


@pytest.mark.parametrize("m,n", KERNELS)
def test_budget_steps_follow_the_reference(m, n):
    """One dual pivot per call until DLP_OK: every call equals the reference from the state
    before it and the steps reach the unbounded call's basis; in between, the primal rule
    refuses a pending LP and leaves it as it is."""
    A, b, c, b2 = _budget_batch(m, n)
    with dlp.Batch(A, b, c, **KW) as bt:
        whole, _ = _rhs_step(bt, b2, "whole")
    assert whole.num_pivots.max() >= 2
    with dlp.Batch(A, b, c, **KW) as bt:
        cont = [None] * NLP
        for t in range(4 * int(whole.num_pivots.max()) + 2):
            r, refs = _rhs_step(bt, b2, f"step {t}", max_pivots=1, continued=cont)
            cont = [ref["bland"] if ref["status"] == L.PIVOT_LIMIT else None for ref in refs]
            assert set(r.status) <= {L.OK, L.PIVOT_LIMIT}
            # (an LP whose one pivot made it optimal reports DLP_OK: that test comes before the budget's)
            assert (r.num_pivots <= 1).all() and (r.num_pivots[r.status == L.PIVOT_LIMIT] == 1).all()
            if (r.status == L.OK).all():
                break
        assert t >= 2 and (r.status == L.OK).all()
        assert r.basis.tobytes() == whole.basis.tobytes()
    c2 = np.stack([BR._c2(m, n, 0, False, j) for j in range(NLP)])
    with dlp.Batch(A, b, c, **KW) as bt:
        r = bt.resolve_rhs(b2, max_pivots=1, **KW)
        pending = np.nonzero(r.status == L.PIVOT_LIMIT)[0]
        assert len(pending) > 0
        before = [bt.read(k) for k in pending]
        for cc in (c2, None):
            rp = bt.resolve(cc, max_pivots=BIG, **KW)
            for (T0, basis0), k in zip(before, pending):
                assert rp.status[k] == L.ERR_STATE and rp.num_pivots[k] == 0 and np.isnan(rp.objective[k])
                np.testing.assert_array_equal(rp.basis[k], basis0)
                T1, basis1 = bt.read(k)
                assert T1.tobytes() == T0.tobytes() and basis1.tobytes() == basis0.tobytes()
        fin = bt.resolve_rhs(b2, **KW)   # more budget finishes them
        assert (fin.status == L.OK).all() and fin.num_pivots[pending].all()
    # a pending LP handed another b takes the rebuild and the reset, not the continuation
    with dlp.Batch(A, b, c, **KW) as bt:
        r = bt.resolve_rhs(b2, max_pivots=1, **KW)
        assert (r.status == L.PIVOT_LIMIT).any()
        b3 = b2.copy()
        b3[:, 0] = np.nextafter(b3[:, 0], np.inf)
        _rhs_step(bt, b3, "another b", max_pivots=1)


@pytest.mark.parametrize("m,n", KERNELS)
def test_budget_steps_give_the_unbounded_call_bits(m, n):
    """``max_pivots=1`` repeated until DLP_OK gives the same concatenated log, final basis and
    objective bits as one unbounded call."""
    A, b, c, b2 = _budget_batch(m, n)
    with dlp.Batch(A, b, c, **KW) as bt:
        whole = bt.resolve_rhs(b2, **KW)
    logs = [[] for _ in range(NLP)]
    final = {}   # LP -> (objective, basis, x, y) of the call that first reported DLP_OK
    with dlp.Batch(A, b, c, **KW) as bt:
        for t in range(4 * int(whole.num_pivots.max()) + 2):
            r = bt.resolve_rhs(b2, max_pivots=1, **KW)
            for k in range(NLP):
                if k not in final:
                    logs[k].append(r.logs[k][:r.num_pivots[k]])
                    if r.status[k] == L.OK:
                        final[k] = (r.objective[k], r.basis[k].copy(), r.x[k].copy(), r.y[k].copy())
            if len(final) == NLP:
                break
    assert len(final) == NLP and t >= 2
    for k in range(NLP):
        got, want = np.concatenate(logs[k]), whole.logs[k][:whole.num_pivots[k]]
        print(f"LP {k}: {len(got)} pivots in steps, {len(want)} in one call, objective {final[k][0]!r} vs "
              f"{whole.objective[k]!r}")
    for k in range(NLP):
        got, want = np.concatenate(logs[k]), whole.logs[k][:whole.num_pivots[k]]
        assert got.tobytes() == want.tobytes(), k
        assert np.float64(final[k][0]).tobytes() == np.float64(whole.objective[k]).tobytes(), k
        assert final[k][1].tobytes() == whole.basis[k].tobytes(), k
        assert final[k][2].tobytes() == whole.x[k].tobytes() and final[k][3].tobytes() == whole.y[k].tobytes(), k


# ---- 7. objectives and right-hand sides in turn
def primal_continue(T, basis, n, c, tol_dj=1e-9, tol_piv=1e-9):
    """dlp_batch_resolve(c) on one LP in numpy, from the full layout Batch.read returns (not
    modified): the objective row by reopt_ref.objective_row, then the primal rule (Dantzig, ties
    to the smallest variable; Bland after a zero ratio; ratio ties to the smallest basic
    variable) with rhs_ref's update (division for the pivot row, a real fma elsewhere).
    Returns (status, basis, [(q, p, leaving), ...], objective, T afterwards)."""
    T = np.array(T, dtype=np.float64)
    basis = np.array(basis, dtype=np.int32)
    m = len(basis)
    N = n + m
    T[m] = R.objective_row(T[:m], basis, c)
    isbasic = np.zeros(N, bool)
    isbasic[basis] = True
    bland, log = False, []
    while True:
        z = np.where(isbasic, 0.0, T[m, :N])
        neg = np.nonzero(z < -tol_dj)[0]
        if len(neg) == 0:
            return L.OK, basis, log, T[m, N], T
        q = int(neg[0]) if bland else int(np.argmin(z))
        elig = np.nonzero(T[:m, q] > tol_piv)[0]
        if len(elig) == 0:
            return L.UNBOUNDED, basis, log, T[m, N], T
        ratio = np.maximum(T[elig, N], 0.0) / T[elig, q]
        ties = elig[ratio == ratio.min()]
        p = int(ties[np.argmin(basis[ties])])
        bland = bool(ratio.min() == 0.0)
        leaving = int(basis[p])
        colq = T[:, q].copy()
        cols = np.concatenate([np.nonzero(~isbasic)[0], [leaving, N]])
        cols = cols[cols != q]
        prow = T[p, cols] / T[p, q]
        rows = np.nonzero(colq != 0.0)[0]
        T[np.ix_(rows, cols)] = RR.fma(-colq[rows, None], prow[None, :], T[np.ix_(rows, cols)])
        T[p, cols] = prow
        T[:, q] = 0.0
        T[p, q] = 1.0
        basis[p] = q
        isbasic[q], isbasic[leaving] = True, False
        log.append((q, p, leaving))


@pytest.mark.parametrize("m,n", KERNELS)
def test_mixed_sequence(m, n):
    """resolve(c2), resolve_rhs(b2), resolve(c3), resolve_rhs(b).  The first step against the
    eager session, the dual steps against rhs_ref bit for bit.  No single-LP path follows a
    session through a change of b, so resolve(c3) is held to primal_continue from the read-out
    before it (status, pivot count, every pivot's q, p and leaving variable, the basis and the
    objective's bits; run from the slack basis it gives the CPU oracle's pivots and bits), to the
    cold solve of (A, b2, c3) at the project's HiGHS bar, and its state is the input of the last
    reference run."""
    seed = 8100 + n
    lps = _lps(m, n, seed)
    A, b, c = BD._stack(lps)
    b2 = perturbed(b, seed)
    c2 = np.stack([R.make_c2(lp[2], seed + 10 + j, holes=False) for j, lp in enumerate(lps)])
    c3 = np.stack([R.make_c2(lp[2], seed + 20 + j, holes=False) for j, lp in enumerate(lps)])
    with dlp.Batch(A, b, c, **KW) as bt:
        r0 = bt.result
        r1 = bt.resolve(c2, **KW)
        r2, refs2 = _rhs_step(bt, b2, "rhs 1")
        before3 = [bt.read(k) for k in range(NLP)]
        r3 = bt.resolve(c3, **KW)
        r4, refs4 = _rhs_step(bt, b, "rhs 2")
    for j, (Aj, bj, cj) in enumerate(lps):
        s = BR._Sess(Aj, bj, cj)
        try:
            BR._same_run(r0, j, s.run(BIG), "cold")
            s.set(c2[j])
            BR._same_run(r1, j, s.run(BIG), "resolve(c2)")
        finally:
            s.close()
    for j, (T0, basis0) in enumerate(before3):
        status, basis3, log3, obj3, _ = primal_continue(T0, basis0, n, c3[j])
        got = [(int(e["q"]), int(e["p"]), int(e["leaving"])) for e in r3.logs[j][:r3.num_pivots[j]]]
        print(f"resolve(c3) LP {j}: {r3.num_pivots[j]} pivots, reference {len(log3)}; objective "
              f"{r3.objective[j]!r}, reference {obj3!r}")
        assert r3.status[j] == status and r3.num_pivots[j] == len(log3) <= LOG_CAP, (j, r3.status[j], status)
        assert got == log3, (j, got, log3)
        assert np.float64(r3.objective[j]).tobytes() == np.float64(obj3).tobytes(), (j, r3.objective[j], obj3)
        np.testing.assert_array_equal(r3.basis[j], basis3, err_msg=f"resolve(c3) LP {j}")
    assert (r2.status == L.OK).all() and (r3.status == L.OK).all() and (r4.status == L.OK).all()
    assert r2.num_pivots.sum() > 0 and r3.num_pivots.sum() > 0 and r4.num_pivots.sum() > 0
    for res, bb, cc in ((r2, b2, c2), (r3, b2, c3), (r4, b, c3)):
        cold = dlp.batched_solve_dense(A, bb, cc)
        assert (cold.status == L.OK).all()
        for j in range(NLP):
            assert abs(res.objective[j] - cold.objective[j]) <= 1e-9 * max(1.0, abs(cold.objective[j])), j


# ---- 8. m = 64: a batch the LDS kernel created gives the register-created batch's bytes
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

m, n, seed, nlp = 64, 100, 8300, 6
KW = dict(want_basis=True, log_cap=512)
lps = [O.gen_dense(m, n, seed + k, k % 2 == 1) for k in range(nlp)]
A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
b2 = b * (1.0 + 0.02 * np.random.default_rng(seed).uniform(-1.0, 1.0, b.shape))
b3 = b2.copy()
b3[:, 5] = -0.25
out = {}
with dlp.Batch(A, b, c, **KW) as bt:
    out["register_kernel"] = bt.info()["register_kernel"]
    r1 = bt.resolve_rhs(b2, max_pivots=1, **KW)
    r2 = bt.resolve_rhs(b2, **KW)
    r3 = bt.resolve_rhs(b3, **KW)
    out["still"] = bt.info()["register_kernel"]
    out["runs"] = [digest(bt.result), digest(r1), digest(r2), digest(r3), h(*(bt.read(j)[0] + 0.0 for j in range(nlp))),
                   int(r1.num_pivots.sum()), int(r2.num_pivots.sum()), int(r3.num_pivots.sum()),
                   sorted(set(int(s) for s in r3.status))]
print(json.dumps(out))
"""


def test_m64_through_both_kernels():
    """(read() + 0.0 in the digest: the sign of a zero is the condensed tableau's exemption.)"""
    def run(env):
        e = dict(os.environ)
        e.pop("DLP_BATCH_LDS", None)
        e.update(env)
        p = subprocess.run([sys.executable, "-c", KNOB_SCRIPT, ROOT], env=e, capture_output=True, text=True,
                           timeout=240)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads(p.stdout.strip().splitlines()[-1])

    reg, lds = run({}), run({"DLP_BATCH_LDS": "1"})
    assert reg.pop("register_kernel") is True and lds.pop("register_kernel") is False
    assert reg.pop("still") is True and lds.pop("still") is False
    assert reg["runs"][5] > 0 and reg["runs"][6] > 0 and reg["runs"][7] > 0
    assert reg == lds


# ---- 9. a device-tensor b gives the bytes of the host-array call (in a child process: torch
# brings its own HIP runtime, see tests/test_gpu_batched_dense.py)
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

def raises(f, *args):
    try:
        f(*args)
    except ValueError:
        return True
    return False

out = {}
for m, n in ((64, 100), (37, 53)):
    lps = [O.gen_dense(m, n, 8500 + k) for k in range(6)]
    A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
    rng = np.random.default_rng(m)
    b1 = b * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, b.shape))
    b2 = b[0] * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, m))
    b3 = b * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, b.shape))
    b3[4, 3] = np.nan   # the kernel's check sees device inputs too
    with dlp.Batch(A, b, c, **KW) as host, dlp.Batch(*(torch.from_numpy(v).to("cuda:0") for v in (A, b, c)), **KW) as dev:
        ok = same(host.result, dev.result)
        for bb in (b1, b2, b3):
            tb = torch.from_numpy(bb).to("cuda:0")
            rh, rd = host.resolve_rhs(bb, **KW), dev.resolve_rhs(tb, **KW)
            ok = ok and same(rh, rd) and int(rh.num_pivots.sum()) > 0
            ok = ok and all(host.read(k)[0].tobytes() == dev.read(k)[0].tobytes() for k in range(6))
        out[f"{m}x{n} device b"] = bool(ok)
        out[f"{m}x{n} nan seen"] = bool(rd.status[4] == -1 and (np.delete(rd.status, 4) >= 0).all())
        view = torch.from_numpy(np.ascontiguousarray(b1.T)).to("cuda:0").T   # has to be made contiguous
        out[f"{m}x{n} view"] = (not view.is_contiguous()) and same(host.resolve_rhs(b1, **KW), dev.resolve_rhs(view, **KW))
        out[f"{m}x{n} float32 raises"] = raises(dev.resolve_rhs, tb.float())
        out[f"{m}x{n} cpu tensor raises"] = raises(dev.resolve_rhs, tb.cpu())
print(json.dumps(out))
"""


def test_device_b_gives_the_host_bytes():
    p = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT, ROOT], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(out) == 10 and all(out.values()), out


# ---- 10. call-level errors are found before anything is enqueued and leave the batch unchanged
def test_call_level_errors_leave_the_batch_unchanged():
    m, n = 37, 53
    lps = _lps(m, n, 8700)
    A, b, c = BD._stack(lps)
    b2 = perturbed(b, 8700)
    lib = L.lib()
    with dlp.Batch(A, b, c, **KW) as bt:
        prev = bt.resolve(None, **KW)
        before = [bt.read(j) for j in range(NLP)]
        out, bad_log = L.BatchOut(), L.BatchOut()
        bad_log.log_cap = -1
        ptr = b2.ctypes.data
        lib.dlp_batch_resolve(None, None, 0, 0, 10, None)   # (another name in dlp_last_error)
        assert lib.dlp_batch_resolve_rhs(bt._h, ptr, m - 1, 0, 10, C.byref(out)) == L.ERR_ARG    # 0 < stride < m
        assert b"dlp_batch_resolve_rhs" in lib.dlp_last_error()
        assert lib.dlp_batch_resolve_rhs(bt._h, ptr, -m, 0, 10, C.byref(out)) == L.ERR_ARG
        assert lib.dlp_batch_resolve_rhs(bt._h, ptr, m, 2, 10, C.byref(out)) == L.ERR_ARG        # b_is_device
        assert lib.dlp_batch_resolve_rhs(bt._h, ptr, m, -1, 10, C.byref(out)) == L.ERR_ARG
        assert lib.dlp_batch_resolve_rhs(bt._h, ptr, m, 0, -1, C.byref(out)) == L.ERR_ARG        # max_pivots
        assert lib.dlp_batch_resolve_rhs(bt._h, None, m, 0, 10, C.byref(out)) == L.ERR_ARG       # b is required
        assert lib.dlp_batch_resolve_rhs(bt._h, ptr, m, 0, 10, C.byref(bad_log)) == L.ERR_ARG
        for j in range(NLP):
            T1, basis1 = bt.read(j)
            assert T1.tobytes() == before[j][0].tobytes() and basis1.tobytes() == before[j][1].tobytes()
        res = bt.resolve(None, **KW)
        for f in ("status", "num_pivots", "objective", "basis", "x", "y"):
            assert getattr(res, f).tobytes() == getattr(prev, f).tobytes(), f
        assert lib.dlp_batch_resolve_rhs(bt._h, ptr, m, 0, BIG, None) == L.OK    # out may be NULL
        fin = bt.resolve_rhs(b2, **KW)
        assert (fin.status == L.OK).all() and not fin.num_pivots.any()
