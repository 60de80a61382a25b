"""CPU: dlp_session_set_rhs_in_place's interface (the symbol, its binding, its argument checks, the
wrapper's shape and dtype checks with in_place=True), and a count on the C++ dual oracle's traces
showing that the inputs of tests/test_gpu_session_rhs_defer.py exercise what is new in a deferred
dual block: a variable that enters in the block in which it left (on the condensed layout its slot
restarted inside the block, so the replays of row p and of column q meet a restart) and a pivot row
that is the pivot row again inside a block (the replays meet an overwrite by an earlier step).
Blocks are counted from the phase's first pivot.  Conditions, not measurements: should a count fall
to zero, change the seed in tests/dual_lp.py.

Counted here (re-entries, repeated rows), printed with -s:
  input                          dual pivots   K = 16     K = 64
  dense 65 x 449                 104           33, 27     53, 52
  dense 300 x 740                853           272, 96    488, 270
  cone 300 x 740, always Bland   880           453, 266   643, 531
  dense 63 x 70                  25            6, 3       -
"""
import ctypes as C
import functools

import numpy as np
import pytest

import dual_lp as D
import oracle_py as O
import reopt_ref as R
import rhs_ref as RR

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

NAME = "dlp_session_set_rhs_in_place"


def test_symbol_and_signature():
    sig = {name: (res, args) for name, res, args in L.SIGNATURES}
    assert NAME in sig
    assert sig[NAME] == sig["dlp_session_set_rhs"]
    fn = getattr(L.lib(), NAME)          # exported by libdlp.so and bound
    assert fn.restype is C.c_int and len(fn.argtypes) == 4


def test_null_arguments():
    b = np.ones(3)
    assert L.lib().dlp_session_set_rhs_in_place(None, b.ctypes.data_as(L._DP), 3, None) == L.ERR_ARG
    assert L.lib().dlp_session_set_rhs_in_place(None, None, 3, None) == L.ERR_ARG
    # (a NULL b with a live session needs a device: tests/test_gpu_session_rhs_defer.py)


class _NoDevice(dlp.Session):
    """The wrapper's own checks come before any call into the library."""

    def __init__(self, m, n):
        self.problem = type("P", (), dict(m=m, n=n))()
        self._h = None

    def __del__(self):
        pass


@pytest.mark.parametrize("in_place", [False, True])
def test_wrapper_checks_shape_and_dtype(in_place):
    s = _NoDevice(5, 7)
    for bad in (np.ones(4), np.ones(6), np.ones((5, 1)), np.ones((1, 5)), 1.0):
        with pytest.raises(ValueError, match="shape"):
            s.set_rhs(bad, in_place=in_place)
    for bad in (np.ones(5, dtype=complex), np.array(["a"] * 5), np.ones(5, dtype=bool), np.array([None] * 5)):
        with pytest.raises(ValueError, match="real-valued"):
            s.set_rhs(bad, in_place=in_place)


# ---- the inputs put restarts and repeated pivot rows inside a block

@functools.lru_cache(maxsize=None)
def _trace(kind, m, n):
    if kind == "dense":
        A, b, c, b2 = D.dense_lp(m, n)
        T, basis = R.oracle_tableau(A, b, c, D.BIG)
        return O.resolve_rhs(T, basis, n, b2)
    A, b, c = D.cone_lp(m, n)
    T, basis = RR.from_dense(A, np.abs(b), c)
    return O.resolve_rhs(T, basis, n, b, pricing=1)


def _block_counts(log, K):
    """(pivots whose entering variable left earlier in the same block of K, pivots whose row was a
    pivot row earlier in the same block)."""
    reentries = repeats = 0
    for k0 in range(0, len(log), K):
        left, rows = set(), set()
        for e in log[k0:k0 + K]:
            reentries += int(e["q"]) in left
            repeats += int(e["p"]) in rows
            left.add(int(e["leaving"]))
            rows.add(int(e["p"]))
    return reentries, repeats


CASES = [
    ("dense", 65, 449, 104, (33, 27), (53, 52)),
    ("dense", 300, 740, 853, (272, 96), (488, 270)),
    ("cone", 300, 740, 880, (453, 266), (643, 531)),
    ("dense", 63, 70, 25, (6, 3), None),
]


@pytest.mark.parametrize("kind,m,n,pivots,k16,k64", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in CASES])
def test_blocks_hold_restarts_and_repeated_rows(kind, m, n, pivots, k16, k64):
    ref = _trace(kind, m, n)
    assert ref["status"] == RR.OK and ref["done"] == pivots == len(ref["log"])
    got16 = _block_counts(ref["log"], 16)
    got64 = _block_counts(ref["log"], 64) if k64 else None
    print(f"{kind} {m}x{n}: {pivots} dual pivots; K = 16: {got16}, K = 64: {got64}")
    assert got16[0] > 0 and got16[1] > 0, got16          # the condition
    assert got16 == k16, (got16, k16)                    # the docstring's table
    if k64:
        assert got64[0] > 0 and got64[1] > 0 and got64 == k64, (got64, k64)
