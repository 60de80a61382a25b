"""Form-23 pass: nontemporal tableau LDS-DMAs (DLP_PASS_NTLOAD).

With the knob on, the pass's tableau LDS-DMAs (scalar-base and per-lane forms, steady state and the
clamped prologue / tail) carry the nt cache policy; the coefficient DMAs and the P / class loads keep
the default one.  A cache policy cannot change a byte.  What is guarded here are the asm variants
and the instances behind the knob: a wrong operand, a dropped DMA, a miscounted wait.

The nt instances exist only for nontemporal sessions, and a session's automatic choice is
nontemporal only from 1 GiB of tableau, so every session here is created with nontemporal=1 and
reports it (get_tuning); tests/test_pass_ntload_isa.py asserts on the CPU that the code object holds
an nt instance for every (U, D, DMA form, coefficient ring) these cases name, publishing and not.

The reference is the eager session (defer=1), which shares none of this code: pivot log and whole
tableau byte-equal after two full blocks and a 17-step one.  The knobs are read once per process,
so every setting runs in a child process.

What the DMA variants can get wrong lies at the ends of a band, asserted on the CPU first: short
last groups, a last group of a single row, a band shorter than one supergroup of the shared
coefficient ring, widths that are no multiple of the 256-column tile."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

K = 2 * 64 + 17
G = 4   # groups per supergroup (pass_q_kernel)
# m, n, seed, rows per band
SHAPES = [(67, 900, 1, 16),
          (129, 4000, 2, 37),
          (300, 520, 5, 64),
          (5, 300, 9, 8)]

SCRIPT = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import distributedlpsolver_amd as dlp

def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

out = []
for m, n, seed, rb, la, k, cond in json.loads(sys.argv[2]):
    prob = dlp.Problem.random(m, n, seed)
    with dlp.Session(prob, defer=64, check_interval=64, rows_per_block=rb, lookahead=la, condensed=cond,
                     nontemporal=1) as s:
        s.set_defer_tuning(0, 23)
        done = 0
        while done < k:
            got = s.run(min(64, k - done))[1]
            assert got > 0, (m, n, seed, done)
            done += got
        out.append(dict(form=s.defer_form(), lookahead=bool(s.lookahead()), chain_cus=s.chain_cus(),
                        nontemporal=s.get_tuning()[2],
                        log=h(s.result().pivot_log), tableau=h(s.tableau())))
print(json.dumps(out))
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
    """CPU only: the ends of the bands that the DMA variants have to get right, and the pivot counts."""
    bands = [nr for m, _, _, rb in SHAPES for nr in _bands(m, rb)]
    for U in (2, 4):
        assert any(nr % U for nr in bands), U                 # a short last group
        assert any(nr % U == 1 for nr in bands), U            # a one-row last group
        assert any(-(-nr // U) < G for nr in bands), U        # a band shorter than one supergroup
        assert any(nr // U > 4 for nr in bands), U            # refills in the steady state (D <= 4)
    assert _bands(SHAPES[3][0], SHAPES[3][3]) == [5]
    assert sum((n + 1) % 256 != 0 for _, n, _, _ in SHAPES) >= 2
    for m, n, seed, rb in SHAPES[:3]:
        assert len(_oracle_log(m, n, seed)) == K
    assert len(_oracle_log(*SHAPES[3][:3])) == 10


def test_inputs_cover_the_ends_of_a_band():
    _check_inputs()


@functools.lru_cache(maxsize=None)
def _eager(m, n, seed, k):
    with dlp.Session(dlp.Problem.random(m, n, seed), defer=1, check_interval=k) as e:
        e.run(k)
        log = e.result().pivot_log
        assert len(log) == k
        return _h(log), _h(e.tableau())


def _run(arg, env):
    e = dict(os.environ)
    for k in ("DLP_Q_U", "DLP_Q_DEPTH", "DLP_PASS_PIVG", "DLP_PASS_SADDR", "DLP_PASS_CSHARE", "DLP_CONDENSED",
              "DLP_CHAIN_CUS", "DLP_BAND_PUB", "DLP_PASS_LDS", "DLP_PASS_NTLOAD", "DLP_CHAIN_NTLOAD",
              "DLP_RATIO_ROWS", "DLP_RATIO_RP", "DLP_FAT_PROW", "DLP_PROW_GROUP", "DLP_MID_CHAIN", "DLP_CHAIN_RING"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, json.dumps(arg)], env=e, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _compare(cases, env, chain_cus=None):
    for (m, n, seed, rb, la, k, cond), got in zip(cases, _run(cases, env)):
        tag = (m, n, seed, rb, la, k, cond, env)
        assert got["form"] == 23 and got["lookahead"] == bool(la), (tag, got)
        assert got["nontemporal"] == 1, (tag, got)   # else no nt instance runs, whatever the knob says
        if chain_cus is not None:
            assert got["chain_cus"] == chain_cus, (tag, got)
        log, tab = _eager(m, n, seed, k)
        assert got["log"] == log, tag
        assert got["tableau"] == tab, tag


def _shape_cases(cond, las=(0, 1)):
    return [(m, n, seed, rb, la, len(_oracle_log(m, n, seed)), cond) for m, n, seed, rb in SHAPES for la in las]


@pytest.mark.parametrize("ntload", ["1", "0"])
@pytest.mark.parametrize("qu", ["2", "4"])
def test_nt_tableau_dmas_equal_the_eager_session(qu, ntload):
    """In place and with lookahead (band publication), condensed: U = 2 (D = 4) and U = 4 (D = 2, the
    shared coefficient ring), the scalar-base DMAs."""
    _check_inputs()   # before the GPU is asked
    _compare(_shape_cases(1), {"DLP_Q_U": qu, "DLP_PASS_NTLOAD": ntload})


def test_nt_tableau_dmas_full_tableau():
    _check_inputs()
    _compare(_shape_cases(0), {"DLP_Q_U": "4", "DLP_PASS_NTLOAD": "1", "DLP_CONDENSED": "0"})


@pytest.mark.parametrize("qu", ["2", "4"])
def test_nt_tableau_dmas_per_lane_form(qu):
    _check_inputs()
    _compare(_shape_cases(1), {"DLP_Q_U": qu, "DLP_PASS_NTLOAD": "1", "DLP_PASS_SADDR": "0"})


def test_nt_tableau_dmas_private_coefficient_rings():
    _check_inputs()
    _compare(_shape_cases(1), {"DLP_Q_U": "4", "DLP_PASS_NTLOAD": "1", "DLP_PASS_CSHARE": "0"})


@pytest.mark.parametrize("ntload", ["1", "0"])
def test_nt_tableau_dmas_beside_the_grouped_ring_chain(ntload):
    """The C3 arrangement: lookahead with the chain on 64 CUs of its own and 64 rows per wave (the
    grouped-ring selection kernel, the register pivot-row kernel), the publishing pass on the rest.
    (The chain's own nt reads, DLP_CHAIN_NTLOAD, were measured and taken out: DESIGN.md 16.5.)"""
    _check_inputs()
    _compare(_shape_cases(1, las=(1,)), {"DLP_PASS_NTLOAD": ntload, "DLP_CHAIN_CUS": "64", "DLP_RATIO_ROWS": "64"},
             chain_cus=64)
