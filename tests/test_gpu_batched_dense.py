"""GPU: dlp.batched_solve_dense (dlp_batched_solve_dense), the batch solve of caller-supplied
LPs, against the CPU oracle, one LP at a time.

Bar: status, pivot count, objective, basis and the pivot-log prefix are bit-identical to
O.solve_dense(..., nthreads=1); x and y are equal as values (np.array_equal: the sign of a
zero is exempt, the batch kernels keep the condensed tableau, which holds the full tableau's
bits up to the sign of a zero)."""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
from conftest import ROOT

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

pytestmark = pytest.mark.gpu

LOG_CAP = 4096


@functools.lru_cache(maxsize=None)
def _gen(m, n, seed, degen=False):
    A, b, c = O.gen_dense(m, n, seed, degen)
    for v in (A, b, c):
        v.setflags(write=False)   # shared between tests: copy before changing
    return A, b, c


def _ref(A, b, c, **o):
    return O.solve_dense(A, b, c, nthreads=1, log_cap=LOG_CAP, **o)


@functools.lru_cache(maxsize=None)
def _gen_ref(m, n, seed, degen=False, pricing=0, max_pivots=1_000_000):
    return _ref(*_gen(m, n, seed, degen), pricing=pricing, max_pivots=max_pivots)


def _same_lp(res, k, ref):
    """LP k of the batch result against its oracle solution."""
    assert res.status[k] == ref.status, (k, res.status[k], ref.status)
    assert res.num_pivots[k] == ref.num_pivots, (k, res.num_pivots[k], ref.num_pivots)
    assert np.float64(res.objective[k]).tobytes() == np.float64(ref.objective).tobytes(), k
    if res.basis is not None:
        np.testing.assert_array_equal(res.basis[k], ref.basis)
    if res.logs is not None:
        cnt = min(ref.num_pivots, LOG_CAP)
        got, want = np.ascontiguousarray(res.logs[k][:cnt]), np.ascontiguousarray(ref.pivot_log[:cnt])
        if got.tobytes() != want.tobytes():
            for i in range(cnt):
                assert got[i].tobytes() == want[i].tobytes(), f"LP {k} pivot {i}: gpu {got[i]} oracle {want[i]}"
    if res.x is not None:
        assert np.array_equal(res.x[k], ref.x), (k, np.flatnonzero(res.x[k] != ref.x)[:8])
    if res.y is not None:
        assert np.array_equal(res.y[k], ref.y), (k, np.flatnonzero(res.y[k] != ref.y)[:8])


def _stack(lps):
    return (np.stack([p[0] for p in lps]), np.stack([p[1] for p in lps]), np.stack([p[2] for p in lps]))


def _solve(A, b, c, **kw):
    kw.setdefault("want_basis", True)
    kw.setdefault("log_cap", LOG_CAP)
    return dlp.batched_solve_dense(A, b, c, **kw)


def _same_bytes(r1, r2, logs=True):
    assert r1.status.tobytes() == r2.status.tobytes()
    assert r1.num_pivots.tobytes() == r2.num_pivots.tobytes()
    assert r1.objective.tobytes() == r2.objective.tobytes()
    assert r1.basis.tobytes() == r2.basis.tobytes()
    if logs:
        for k in range(len(r1.status)):   # (entries past an LP's pivot count are not written)
            cnt = min(int(r1.num_pivots[k]), LOG_CAP)
            assert r1.logs[k][:cnt].tobytes() == r2.logs[k][:cnt].tobytes(), k
    for a, b in ((r1.x, r2.x), (r1.y, r2.y)):
        if a is not None and b is not None:
            assert a.tobytes() == b.tobytes()


# ---- every LP against the oracle: the register kernel (m = 64; 1, 2, 3 waves per LP, partly idle
# last waves and exact wave boundaries) and the LDS kernel ((65, 30) just off the register path,
# (64, 200) m = 64 with four waves' worth of columns)
@pytest.mark.parametrize("degen", [False, True], ids=["dense", "degenerate"])
@pytest.mark.parametrize("n", [1, 32, 64, 65, 100, 128, 191, 192])
def test_register_kernel_shapes(n, degen):
    nlp, m, seed = 6, 64, 700 + n
    assert dlp.batched_occupancy(m, n)["register_kernel"]
    lps = [_gen(m, n, seed + k, degen) for k in range(nlp)]
    res = _solve(*_stack(lps))
    assert res.x.shape == (nlp, n) and res.y.shape == (nlp, m)
    for k in range(nlp):
        _same_lp(res, k, _gen_ref(m, n, seed + k, degen))


@pytest.mark.parametrize("degen", [False, True], ids=["dense", "degenerate"])
@pytest.mark.parametrize("m,n", [(1, 1), (5, 7), (37, 53), (40, 60), (65, 30), (64, 200)])
def test_lds_kernel_shapes(m, n, degen):
    nlp, seed = 6, 900 + m + n
    assert not dlp.batched_occupancy(m, n)["register_kernel"]
    lps = [_gen(m, n, seed + k, degen) for k in range(nlp)]
    res = _solve(*_stack(lps))
    for k in range(nlp):
        _same_lp(res, k, _gen_ref(m, n, seed + k, degen))


# ---- one batch with every status, invalid LPs between valid ones
def _mixed_batch(m, n, seed):
    lps, kinds = [], []

    def add(kind, A, b, c):
        lps.append((A, b, c))
        kinds.append(kind)

    add("normal", *_gen(m, n, seed))
    A, b, c = (v.copy() for v in _gen(m, n, seed + 1))
    b[m - 1] = -1.0
    add("negative b", A, b, c)
    A, b, c = (v.copy() for v in _gen(m, n, seed + 2))
    j = n // 2
    A[:, j] = -A[:, j]
    A[0, j] = 0.0
    c[j] = 0.5 * c.min() + 1e-3   # priced after other columns: unbounded after some pivots
    add("unbounded", A, b, c)
    A, b, c = (v.copy() for v in _gen(m, n, seed + 3))
    b[0] = np.nan
    add("nan b", A, b, c)
    A, b, c = (v.copy() for v in _gen(m, n, seed + 4))
    c = -c
    c[0] = 0.0
    add("c <= 0", A, b, c)
    add("degenerate", *_gen(m, n, seed + 5, True))
    A, b, c = (v.copy() for v in _gen(m, n, seed + 6))
    b[:] = 0.0
    add("b = 0", A, b, c)
    add("normal", *_gen(m, n, seed + 7))
    return lps, kinds


@pytest.mark.parametrize("m,n", [(64, 100), (37, 53)])
def test_mixed_statuses_in_one_batch(m, n):
    lps, kinds = _mixed_batch(m, n, 1200 + m)
    res = _solve(*_stack(lps))
    seen = set()
    for k, (kind, lp) in enumerate(zip(kinds, lps)):
        if kind in ("negative b", "nan b"):
            assert res.status[k] == L.ERR_ARG and res.num_pivots[k] == 0
            assert np.isnan(res.objective[k])
            assert np.isnan(res.x[k]).all() and np.isnan(res.y[k]).all()
            np.testing.assert_array_equal(res.basis[k], n + np.arange(m))
            continue
        ref = _ref(*lp)
        seen.add(ref.status)
        _same_lp(res, k, ref)
        if kind == "unbounded":
            assert ref.status == L.UNBOUNDED
        elif kind == "c <= 0":
            assert ref.status == L.OK and ref.num_pivots == 0
            assert not res.x[k].any() and res.objective[k] == 0.0
        else:
            assert ref.status == L.OK
    assert seen == {L.OK, L.UNBOUNDED}


# ---- the pivot limit (x, y and the objective of the tableau as it stands) and Bland's rule
@pytest.mark.parametrize("pricing", [0, 1], ids=["dantzig", "bland"])
@pytest.mark.parametrize("max_pivots", [10, 1_000_000])
@pytest.mark.parametrize("m,n", [(64, 100), (37, 53)])
def test_pivot_limit_and_bland(m, n, max_pivots, pricing):
    nlp, seed = 4, 1500
    lps = [_gen(m, n, seed + k, k % 2 == 1) for k in range(nlp)]
    res = _solve(*_stack(lps), max_pivots=max_pivots, pricing=pricing)
    for k in range(nlp):
        ref = _gen_ref(m, n, seed + k, k % 2 == 1, pricing, max_pivots)
        _same_lp(res, k, ref)
    if max_pivots == 10:
        assert (res.status == L.PIVOT_LIMIT).all() and (res.num_pivots == 10).all()


# ---- shared arrays (stride 0) give the bytes of explicitly replicated ones
@pytest.mark.parametrize("m,n", [(64, 100), (37, 53)])
def test_broadcasting(m, n):
    nlp, seed = 5, 1700
    A, b, c = _stack([_gen(m, n, seed + k) for k in range(nlp)])
    rep = lambda v: np.ascontiguousarray(np.broadcast_to(v, (nlp,) + v.shape))   # noqa: E731
    # shared A, per-LP b and c
    r1 = _solve(A[0], b, c)
    _same_bytes(r1, _solve(rep(A[0]), b, c))
    for k in range(nlp):
        _same_lp(r1, k, _ref(A[0], b[k], c[k]))
    # shared A and b, per-LP c
    r2 = _solve(A[1], b[1], c)
    _same_bytes(r2, _solve(rep(A[1]), rep(b[1]), c))
    for k in range(nlp):
        _same_lp(r2, k, _ref(A[1], b[1], c[k]))
    # nothing batched: one LP
    r3 = _solve(A[2], b[2], c[2])
    assert r3.status.shape == (1,) and r3.x.shape == (1, n)
    _same_lp(r3, 0, _gen_ref(m, n, seed + 2))


# ---- the generator's own LPs through the dense entry: the generated path's bits
@pytest.mark.parametrize("m,n", [(64, 128), (32, 96)])
@pytest.mark.parametrize("degen", [False, True], ids=["dense", "degenerate"])
def test_generated_vs_dense(m, n, degen):
    nlp, seed = 16, 1900
    gen = dlp.batched_solve(nlp, m, n, seed, degenerate=degen, want_basis=True, log_cap=LOG_CAP)
    res = _solve(*_stack([_gen(m, n, seed + k, degen) for k in range(nlp)]))
    _same_bytes(gen, res)


# ---- device tensors give the bytes of the numpy path.  In a child process: torch brings its own
# HIP runtime, which has to be the one the process loads first (libdlp.so then shares it), and
# this process has long loaded libdlp.so.
DEVICE_SCRIPT = r"""
import json, sys
import torch
torch.cuda.init()
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import oracle_py as O
import distributedlpsolver_amd as dlp

def solve(A, b, c):
    return dlp.batched_solve_dense(A, b, c, want_basis=True, log_cap=512)

def same(r1, r2):
    ok = all(getattr(r1, f).tobytes() == getattr(r2, f).tobytes()
             for f in ("status", "num_pivots", "objective", "basis", "x", "y"))
    return ok and all(r1.logs[k][:r1.num_pivots[k]].tobytes() == r2.logs[k][:r1.num_pivots[k]].tobytes()
                      for k in range(len(r1.status)))

def raises(*args):
    try:
        solve(*args)
    except ValueError:
        return True
    return False

out = {}
for m, n in ((64, 100), (37, 53)):
    lps = [O.gen_dense(m, n, 2100 + k) for k in range(5)]
    A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
    tA, tb, tc = (torch.from_numpy(v).to("cuda:0") for v in (A, b, c))
    host = solve(A, b, c)
    out[f"{m}x{n} optimal"] = bool((host.status == 0).all() and (host.num_pivots > 0).all())
    out[f"{m}x{n} batched"] = same(host, solve(tA, tb, tc))
    out[f"{m}x{n} shared"] = same(solve(A[0], b[0], c), solve(tA[0], tb[0], tc))
    tAt = tA.transpose(1, 2).contiguous().transpose(1, 2)   # a view that has to be made contiguous
    out[f"{m}x{n} view"] = (not tAt.is_contiguous()) and same(host, solve(tAt, tb, tc))
out["float32 raises"] = raises(tA.float(), tb.float(), tc.float())
out["mixed kinds raise"] = raises(tA, b, c)
out["cpu tensors raise"] = raises(tA.cpu(), tb.cpu(), tc.cpu())
print(json.dumps(out))
"""


def test_device_input():
    p = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT, ROOT], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(out) == 11 and all(out.values()), out


def test_oversize_is_unsupported():
    with pytest.raises(dlp.DLPError) as e:
        dlp.batched_solve_dense(np.ones((2, 200, 200)), np.ones(200), np.ones(200))
    assert e.value.status == L.ERR_UNSUPPORTED


def test_context_reuse_and_release():
    small = _stack([_gen(64, 64, 2300 + k) for k in range(4)])
    large = _stack([_gen(64, 128, 2400 + k) for k in range(8)])
    lds = _stack([_gen(37, 53, 2500 + k) for k in range(3)])
    r1, l1 = _solve(*small), _solve(*lds)
    g1 = dlp.batched_solve(4, 64, 64, 2300, want_basis=True, log_cap=LOG_CAP)
    r2 = _solve(*large)
    g2 = dlp.batched_solve(4, 64, 64, 2300, want_basis=True, log_cap=LOG_CAP)
    r3, l3 = _solve(*small), _solve(*lds)
    _same_bytes(r1, r3)
    _same_bytes(l1, l3)
    _same_bytes(g1, g2)
    _same_bytes(g1, r1)   # (the same LPs)
    for k in range(8):
        _same_lp(r2, k, _gen_ref(64, 128, 2400 + k))
    assert dlp.release_cached_memory(0) > 0
    assert dlp.release_cached_memory(0) == 0
    _same_bytes(r1, _solve(*small))   # a fresh context


def test_null_outputs():
    lps = _stack([_gen(64, 100, 2600 + k) for k in range(4)])
    full = _solve(*lps)
    for wx, wy in ((False, False), (True, False), (False, True)):
        part = _solve(*lps, want_x=wx, want_y=wy)
        assert (part.x is None) == (not wx) and (part.y is None) == (not wy)
        _same_bytes(full, part)
    bare = dlp.batched_solve_dense(*lps, want_x=False, want_y=False)
    assert bare.basis is None and bare.logs is None
    assert bare.objective.tobytes() == full.objective.tobytes()
    assert bare.num_pivots.tobytes() == full.num_pivots.tobytes()
