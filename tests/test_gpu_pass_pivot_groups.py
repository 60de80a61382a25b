"""Form-23 pass: groups that hold dense pivot rows stay on the DPP chain (DLP_PASS_PIVG).

A pivot row of the block whose every coefficient is non-zero is recomputed after its group's
chain (P[cl], then the steps after cl) instead of sending the whole group through the row-by-row
replay.  The reference is the eager session (defer=1), which shares none of this code: pivot log
and whole tableau byte-equal after two full blocks and a 17-step one, with 2 and 4 rows per group,
the knob on and off, in place and out of place (lookahead, band publication), condensed and full
tableau.  The knobs are read once per process, so every setting runs in a child process.

Pivot rows with a zero coefficient after their step, sparse and untouched rows must still take
the generic path: full solves against the oracle on LPs that have them."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
import structured_lp as S

import distributedlpsolver_amd as dlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

K = 2 * 64 + 17
# m, n, seed, rows per band
SHAPES = [(67, 900, 1, 16),      # more pivots than rows: several pivot rows per group, rows pivoting twice
          (129, 4000, 2, 37),    # the last group of a band holds one row; width no multiple of 256
          (300, 520, 5, 64),
          (700, 1337, 7, 768)]   # one short band

SCRIPT = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import distributedlpsolver_amd as dlp

def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

k, out = int(sys.argv[2]), []
for m, n, seed, rb, la in json.loads(sys.argv[3]):
    with dlp.Session(dlp.Problem.random(m, n, seed), defer=64, check_interval=64, rows_per_block=rb,
                     lookahead=la) as s:
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


def _h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _eager(m, n, seed):
    with dlp.Session(dlp.Problem.random(m, n, seed), defer=1, check_interval=K) as e:
        e.run(K)
        log = e.result().pivot_log
        assert len(log) == K
        return _h(log), _h(e.tableau())


def _child(cases, env):
    e = dict(os.environ)
    for k in ("DLP_Q_U", "DLP_Q_DEPTH", "DLP_PASS_PIVG", "DLP_CONDENSED", "DLP_CHAIN_CUS", "DLP_BAND_PUB",
              "DLP_PASS_LDS"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, str(K), json.dumps(cases)], env=e,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _compare(env):
    cases = [(m, n, seed, rb, la) for m, n, seed, rb in SHAPES for la in (0, 1)]
    for (m, n, seed, rb, la), got in zip(cases, _child(cases, env)):
        tag = (m, n, seed, rb, la, env)
        assert got["form"] == 23 and got["lookahead"] == bool(la), (tag, got)
        log, tab = _eager(m, n, seed)
        assert got["log"] == log, tag
        assert got["tableau"] == tab, tag


@pytest.mark.parametrize("pivg", ["1", "0"])
@pytest.mark.parametrize("qu", ["2", "4"])
def test_pivot_row_groups_equal_the_eager_session(qu, pivg):
    _compare({"DLP_Q_U": qu, "DLP_PASS_PIVG": pivg})


@pytest.mark.parametrize("qu", ["2", "4"])
def test_pivot_row_groups_full_tableau(qu):
    _compare({"DLP_Q_U": qu, "DLP_PASS_PIVG": "1", "DLP_CONDENSED": "0"})


def _same(res, ref, tag):
    assert res.status == ref.status, (tag, res.status, ref.status)
    assert np.ascontiguousarray(res.pivot_log).tobytes() == np.ascontiguousarray(ref.pivot_log).tobytes(), tag
    assert np.float64(res.objective).tobytes() == np.float64(ref.objective).tobytes(), tag
    assert res.x.tobytes() == ref.x.tobytes() and res.y.tobytes() == ref.y.tobytes(), tag
    assert res.basis.tobytes() == ref.basis.tobytes(), tag


def _solve23(prob, **opts):
    with dlp.Session(prob, defer=64, **opts) as s:
        s.set_defer_tuning(0, 23)
        assert s.defer_form() == 23
        s.run(10 ** 6)
        return s.result()


def test_sparse_rows_and_zero_suffix_pivot_rows_take_the_generic_path():
    """The knob at its default (on).  Ad allocation: untouched and sparse rows, pivot rows whose
    later coefficients hold zeros; the degenerate LP: Bland, tied ratios."""
    M, b, c = O.adalloc_lp(200, 200, 0.1, 0.25)
    _same(_solve23(dlp.Problem.adalloc(200, 200, 1, 0.1, 0.25)), O.solve_dense(M, b, c), "adalloc")
    A, b, c = O.gen_dense(128, 128, 3, degenerate=True)
    _same(_solve23(dlp.Problem.dense(A, b, c), check_interval=100), O.solve_dense(A, b, c, pricing=0), "degenerate")


@pytest.mark.parametrize("name", [f"{kind}_{m}x{n}" for kind in ("unbounded_late", "a_at_tol")
                                  for m, n in (S.EDGE_SMALL, S.EDGE_BIG)])
def test_edge_case_lps_under_form23(name):
    assert name in S.EDGE_NAMES
    A, b, c = S.edge_case(name)[:3]
    _same(_solve23(dlp.Problem.dense(A, b, c)), O.solve_dense(A, b, c, nthreads=1), name)
