"""Form-23 pass: the coefficient rows fetched once per workgroup (DLP_PASS_CSHARE).

With the shared ring the four waves of a pass workgroup keep private tableau rings and read every
row's 64 coefficients from one ring of supergroups of G = 4 groups, each wave fetching one group of
a supergroup; one workgroup barrier per supergroup orders the reads behind the other waves' DMAs.
The bytes that reach the arithmetic are the same, so nothing may change by a bit.

The reference is the eager session (defer=1), which shares none of this code: pivot log and whole
tableau byte-equal after two full blocks and a 17-step one, the knob on and off, 2 and 4 rows per
group, ring depths 2 and 3 with 4 rows, in place and out of place (lookahead, band publication);
one run on the full tableau and one with pivot-row groups off the DPP chain.  Sparse and untouched
rows (adalloc) and two ranks in one process run with the knob on.  The knob is read once per
process, so every setting runs in a child process.

The shapes are those of test_gpu_pass_stream.py.  What the shared ring can get wrong lies at the
ends of a band, asserted on the CPU first: the groups of a band modulo G in every residue, for 2
and for 4 rows per group (the last supergroup short by 0 to 3 groups), a band shorter than one
supergroup, a last group of a single row, widths that are no multiple of the 256-column tile."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

K = 2 * 64 + 17
G = 4   # groups per supergroup (pass_q_kernel)
# m, n, seed, rows per band
SHAPES = [(67, 900, 1, 16),
          (129, 4000, 2, 37),
          (300, 520, 5, 64),
          (700, 1337, 7, 768),
          (5, 300, 9, 8)]

SCRIPT = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import distributedlpsolver_amd as dlp

def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

out = []
for kind, m, n, seed, rb, la, k, cond in json.loads(sys.argv[2]):
    prob = dlp.Problem.random(m, n, seed) if kind == "random" else dlp.Problem.adalloc(m, n, seed, 0.1, 0.25)
    if kind == "adalloc_full":
        with dlp.Session(prob, defer=64, condensed=cond, lookahead=la) as s:
            s.set_defer_tuning(0, 23)
            s.run(10 ** 6)
            r = s.result()
            out.append(dict(form=s.defer_form(), lookahead=bool(s.lookahead()), status=int(r.status),
                            log=h(r.pivot_log), objective=h(np.float64(r.objective)), x=h(r.x), y=h(r.y),
                            basis=h(r.basis)))
        continue
    with dlp.Session(prob, defer=64, check_interval=64, rows_per_block=rb, lookahead=la, condensed=cond) as s:
        s.set_defer_tuning(0, 23)
        done = 0
        while done < k:
            got = s.run(min(64, k - done))[1]
            assert got > 0, (m, n, seed, done)
            done += got
        out.append(dict(form=s.defer_form(), lookahead=bool(s.lookahead()), log=h(s.result().pivot_log),
                        tableau=h(s.tableau())))
print(json.dumps(out))
"""

RANKS = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

m, n, seed, P = json.loads(sys.argv[2])
prob = dlp.Problem.random(m, n, seed)
sess = [dlp.Session(prob, rank=r, nranks=P, defer=64, condensed=1) for r in range(P)]
try:
    for s in sess:
        s.set_defer_tuning(0, 23)
        assert s.defer_form() == 23
    status = L.RUNNING
    for _ in range(10_000):
        cands = np.concatenate([s.step_candidate() for s in sess])
        st, _ = sess[0].status()
        if st != L.RUNNING:
            status = st
            break
        sends = [s.step_select(cands) for s in sess]
        prow = np.max(np.stack(sends), axis=0)
        for s in sess:
            s.step_update(prow)
    Td = np.concatenate([s.tableau()[:-1] for s in sess] + [sess[0].tableau()[-1:]])
    print(json.dumps(dict(status=int(status), logs=[h(s.result().pivot_log) for s in sess], tableau=h(Td))))
finally:
    for s in sess:
        s.close()
"""


def _h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _oracle_log(m, n, seed):
    A, b, c = O.gen_dense(m, n, seed)
    return O.solve_dense(A, b, c, max_pivots=K).pivot_log


def _bands(m, rb):
    return [min(rb, m - i0) for i0 in range(0, m, rb)]


@functools.lru_cache(maxsize=None)
def _check_inputs():
    """CPU only: the ends of the bands that the shared ring has to get right, and the pivot counts."""
    for U in (2, 4):
        residues = {-(-nr // U) % G for m, _, _, rb in SHAPES for nr in _bands(m, rb)}
        assert residues == set(range(G)), (U, residues)
        assert any(nr % U == 1 for m, _, _, rb in SHAPES for nr in _bands(m, rb)), U   # a one-row last group
        assert any(-(-nr // U) < G for m, _, _, rb in SHAPES for nr in _bands(m, rb)), U   # less than a supergroup
    assert _bands(*[SHAPES[4][i] for i in (0, 3)]) == [5]
    assert sum((n + 1) % 256 != 0 for _, n, _, _ in SHAPES) >= 2
    for m, n, seed, rb in SHAPES[:4]:
        assert len(_oracle_log(m, n, seed)) == K
    assert len(_oracle_log(*SHAPES[4][:3])) == 10


def test_inputs_cover_the_ends_of_a_band():
    _check_inputs()


@functools.lru_cache(maxsize=None)
def _eager(kind, m, n, seed, k):
    prob = dlp.Problem.random(m, n, seed) if kind == "random" else dlp.Problem.adalloc(m, n, seed, 0.1, 0.25)
    with dlp.Session(prob, defer=1, check_interval=k) as e:
        e.run(k)
        log = e.result().pivot_log
        assert len(log) == k
        return _h(log), _h(e.tableau())


def _run(script, arg, env):
    e = dict(os.environ)
    for k in ("DLP_Q_U", "DLP_Q_DEPTH", "DLP_PASS_PIVG", "DLP_PASS_SADDR", "DLP_PASS_CSHARE", "DLP_CONDENSED",
              "DLP_CHAIN_CUS", "DLP_BAND_PUB", "DLP_PASS_LDS"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", script, ROOT, json.dumps(arg)], env=e, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _compare(cases, env):
    for (kind, m, n, seed, rb, la, k, cond), got in zip(cases, _run(SCRIPT, cases, env)):
        tag = (kind, m, n, seed, rb, la, k, cond, env)
        assert got["form"] == 23 and got["lookahead"] == bool(la), (tag, got)
        log, tab = _eager(kind, m, n, seed, k)
        assert got["log"] == log, tag
        assert got["tableau"] == tab, tag


def _shape_cases(cond):
    return [("random", m, n, seed, rb, la, len(_oracle_log(m, n, seed)), cond) for m, n, seed, rb in SHAPES
            for la in (0, 1)]


@pytest.mark.parametrize("cshare", ["1", "0"])
@pytest.mark.parametrize("qu,qd", [("2", None), ("4", "2"), ("4", "3")])
def test_shared_ring_equals_the_eager_session(qu, qd, cshare):
    _check_inputs()   # before the GPU is asked
    env = {"DLP_Q_U": qu, "DLP_PASS_CSHARE": cshare}
    if qd:
        env["DLP_Q_DEPTH"] = qd
    _compare(_shape_cases(1), env)


def test_shared_ring_full_tableau():
    _check_inputs()
    _compare(_shape_cases(0), {"DLP_Q_U": "4", "DLP_PASS_CSHARE": "1", "DLP_CONDENSED": "0"})


def test_shared_ring_pivot_rows_off_the_chain():
    _check_inputs()
    _compare(_shape_cases(1), {"DLP_Q_U": "4", "DLP_PASS_CSHARE": "1", "DLP_PASS_PIVG": "0"})


AD = (200, 200, 1)   # Problem.adalloc(200, 200, 1, 0.1, 0.25): untouched and sparse rows


@functools.lru_cache(maxsize=None)
def _adalloc():
    """The oracle's solve, and the pivots up to the end of the first full block that has an untouched
    row (every coefficient of the block's steps zero, not one of its pivot rows), found by replaying
    the oracle's pivots on a numpy tableau, whose structural zeros stay exact."""
    M, b, c = O.adalloc_lp(AD[0], AD[1], 0.1, 0.25)
    ref = O.solve_dense(M, b, c)
    log = ref.pivot_log
    m, n = M.shape
    T = np.zeros((m, n + m))
    T[:, :n] = M
    T[:, n:] = np.eye(m)
    for blk in range(len(log) // 64):
        touched = np.zeros(m, bool)
        for e in log[blk * 64:(blk + 1) * 64]:
            q, p = int(e["q"]), int(e["p"])
            f = T[:, q].copy()
            touched |= f != 0.0
            prow = T[p] / T[p, q]
            f[p] = 0.0
            rows = np.nonzero(f)[0]
            T[rows] -= np.outer(f[rows], prow)
            T[p] = prow
        if not touched.all():
            return ref, (blk + 1) * 64
    raise AssertionError("no full block with an untouched row")


@pytest.mark.parametrize("la", [0, 1])
def test_untouched_and_sparse_rows_read_the_shared_slot(la):
    _, k = _adalloc()   # (CPU)
    for qu in ("2", "4"):
        _compare([("adalloc", AD[0], AD[1], AD[2], 64, la, k, 1)], {"DLP_PASS_CSHARE": "1", "DLP_Q_U": qu})


@pytest.mark.parametrize("la", [0, 1])
def test_adalloc_full_solve(la):
    ref, _ = _adalloc()
    got, = _run(SCRIPT, [("adalloc_full", AD[0], AD[1], AD[2], 0, la, 0, 1)], {"DLP_PASS_CSHARE": "1"})
    assert got["form"] == 23 and got["lookahead"] == bool(la), got
    assert got["status"] == ref.status, (got["status"], ref.status)
    assert got["log"] == _h(ref.pivot_log)
    assert got["objective"] == _h(np.float64(ref.objective))
    assert got["x"] == _h(ref.x) and got["y"] == _h(ref.y) and got["basis"] == _h(ref.basis)


def test_two_ranks():
    """Two row-block sessions in one process (75 local rows each, in place), the host doing the
    exchanges, against the oracle and the eager single-rank tableau."""
    m, n, seed, P = 150, 170, 4, 2
    A, b, c = O.gen_dense(m, n, seed)
    ref = O.solve_dense(A, b, c)
    got = _run(RANKS, [m, n, seed, P], {"DLP_PASS_CSHARE": "1"})
    assert got["status"] == L.OK
    assert got["logs"] == [_h(ref.pivot_log)] * P
    with dlp.Session(dlp.Problem.random(m, n, seed), defer=1) as e:
        e.run(10 ** 6)
        assert got["tableau"] == _h(e.tableau())
