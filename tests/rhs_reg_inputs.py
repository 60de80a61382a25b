"""Inputs of tests/test_gpu_batch_rhs_reg.py (the dual re-solve in the register kernel at m = 64,
DESIGN.md §23), built here so that tests/test_batch_rhs_reg_api.py can hold them against the
reference on the CPU before any GPU sees them: the warm batches on the wave boundaries, the LPs
whose optimum has every slack nonbasic, the c <= 0 LPs that stay at the slack basis, and the
exact-tie LPs with the counters of their ties.

The CPU side works on the oracle's optimal tableau (the batch's cold solve gives the oracle's
bits: tests/test_gpu_batched_dense.py) and on the slot map the kernels keep: slot s holds
variable s at creation, and an entering variable's slot takes the leaving variable.

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import functools

import numpy as np

import oracle_py as O
import reopt_ref as R

M = 64
NLP = 6
# n on the wave boundaries of the register kernel (lane = slot, 64 lanes per wave): lanes past
# the slots in wave 0, a full wave less one and a full wave, one slot in wave 1, two full waves
# and one slot in wave 2, three full waves
WARM_N = (5, 63, 64, 65, 128, 129, 192)
SCALES = (0.02, 0.3)
TOL = 1e-9


def _ro(*arrays):
    for v in arrays:
        v.setflags(write=False)   # shared between tests: copy before changing
    return arrays


def perturbed(b, seed, scale):
    """b * (1 + scale * u), u ~ U(-1, 1) seeded (tests/test_gpu_batch_rhs.py's)."""
    return np.ascontiguousarray(b * (1.0 + scale * np.random.default_rng(seed).uniform(-1.0, 1.0, b.shape)))


def stack(lps):
    return tuple(np.stack([p[i] for p in lps]) for i in range(3))


# ---- the warm batches
# Generator seeds of the LPs.  At 64 x 5 few optima move under +-2 %: the seeds there are chosen
# (by the reference alone) so that every LP does at least one dual pivot in every case.
WARM_SEEDS = {(n, degen): [9100 + 20 * i + (10 if degen else 0) + k for k in range(NLP)]
              for i, n in enumerate(WARM_N) for degen in (False, True)}
WARM_SEEDS[5, False] = [9001, 9004, 9007, 9008, 9011, 9013]
WARM_SEEDS[5, True] = [9013, 9027, 9036, 9051, 9056, 9094]
CONE_ROWS_AT_5 = 8


@functools.lru_cache(maxsize=None)
def warm_lps(n, degen):
    """The generator's LPs, dense or degenerate family.  64 x 5 degenerate is the exception: the
    family's ~32 cone rows (b_i = 0, entries of both signs) leave no ray in 5 dimensions, x = 0
    is the only feasible point (no seed of 4,000 has a nonzero optimum) and no b moves the basis.
    There the last 8 rows alone are the degenerate family's and the rest the dense family's of
    the same seed, which keeps zero right-hand sides and ties and lets the optimum move."""
    lps = []
    for seed in WARM_SEEDS[n, degen]:
        A, b, c = O.gen_dense(M, n, seed, degen)
        if degen and n == 5:
            Ad, bd = A, b
            A, b, c = (v.copy() for v in O.gen_dense(M, n, seed, False))
            A[M - CONE_ROWS_AT_5:], b[M - CONE_ROWS_AT_5:] = Ad[M - CONE_ROWS_AT_5:], bd[M - CONE_ROWS_AT_5:]
        lps.append(_ro(A, b, c))
    return lps


def warm_b2(n, degen, scale):
    """The (NLP, M) right-hand sides of the warm case: each b of creation moved by +-scale."""
    return np.stack([perturbed(lp[1], seed + int(1000 * scale), scale)
                     for lp, seed in zip(warm_lps(n, degen), WARM_SEEDS[n, degen])])


# ---- the oracle's cold solve with its slot map
def cold(A, b, c, pricing=0, max_pivots=10 ** 6):
    """(T, basis, var): the oracle's full-layout tableau and basis after the cold primal solve of
    (A, b, c) (R.oracle_tableau with the pricing mode), and var[s], the variable slot s holds."""
    m, n = A.shape
    e = O.OracleEngine(A, b, c, 0, 1, 0, m, pricing=pricing)
    try:
        for _ in range(max_pivots):
            cand = e.step_candidate()
            if e.state != 4:
                break
            bits = e.step_select(cand)
            if e.state != 4:
                break
            e.step_update(bits)
        T = np.zeros((m + 1, e.ld))
        O.lib().oracle_slice_tableau(e.h, O._d(T))
        log = e.log()
    finally:
        e.close()
    return T, R.basis_from_log(m, n, log), slots_after(np.arange(n), log)


def slots_after(var, log):
    """The slot map after the pivots of log: the entering variable's slot takes the leaving one."""
    var = np.array(var, dtype=np.int64)
    for e in log:
        s = np.nonzero(var == e["q"])[0]
        assert len(s) == 1, (e, var)
        var[s[0]] = e["leaving"]
    return var


@functools.lru_cache(maxsize=None)
def warm_cold(n, degen, pricing):
    return [cold(*lp, pricing=pricing) for lp in warm_lps(n, degen)]


# ---- every slack nonbasic at the optimum
ALLNB_N = 70


@functools.lru_cache(maxsize=None)
def all_nonbasic_lps():
    """64 x 70: the first 64 columns are I + 0.005 U with costs in [1, 2), the other 6 cost 1e-3
    with entries in [0.5, 1): at the optimum every row is tight on a structural of the first
    block and every slack is nonbasic (asserted on the reference by the CPU test)."""
    lps = []
    for k in range(NLP):
        rng = np.random.default_rng(9500 + k)
        A = np.concatenate([np.eye(M) + 0.005 * rng.uniform(size=(M, M)),
                            rng.uniform(0.5, 1.0, (M, ALLNB_N - M))], axis=1)
        b = rng.uniform(1.0, 2.0, M)
        c = np.concatenate([rng.uniform(1.0, 2.0, M), np.full(ALLNB_N - M, 1e-3)])
        lps.append(_ro(A, b, c))
    return lps


def all_nonbasic_b2():
    b = np.stack([lp[1] for lp in all_nonbasic_lps()])
    return perturbed(b, 9500, 0.3)


# ---- the slack basis (every slack basic, B^-1 = I)
SLACK_N = 100


@functools.lru_cache(maxsize=None)
def slack_basis_lps():
    """64 x 100 with c <= 0: the cold solve does no pivot and leaves the slack basis, which is
    dual feasible.  A in [-1, 1) (rows of both signs can still be satisfied after b turns
    negative), b of creation >= 0."""
    lps = []
    for k in range(NLP):
        rng = np.random.default_rng(9600 + k)
        A = rng.uniform(-1.0, 1.0, (M, SLACK_N))
        b = rng.uniform(0.5, 1.5, M)
        c = -rng.uniform(0.0, 1.0, SLACK_N)
        lps.append(_ro(A, b, c))
    return lps


def slack_basis_b2():
    """b = A x0 + u with rows pushed negative, by more from LP to LP."""
    out = []
    for k, (A, b, c) in enumerate(slack_basis_lps()):
        rng = np.random.default_rng(9650 + k)
        b2 = A @ rng.uniform(0.0, 1.0, SLACK_N) + rng.uniform(0.0, 1.0, M)
        b2[rng.choice(M, 2 + k, replace=False)] -= 0.5 * (1 + k)
        out.append(b2)
    return np.stack(out)


# ---- exact ties
TIE_N = 100
TIE_SEED = 9700


@functools.lru_cache(maxsize=None)
def tie_lps():
    """tests/test_gpu_batch_rhs.py's integer_lps at 64 x 100: twin columns j and j + 50 (ratio
    ties, one twin in wave 0's slots and one in wave 1's while neither has moved) and twin rows
    (leaving-row ties).  Returns (lps, b2)."""
    m, n = M, TIE_N
    rng = np.random.default_rng(TIE_SEED)
    lps, b2 = [], []
    h = n // 2
    for _ in range(NLP):
        A = rng.integers(0, 3, (m, n)).astype(np.float64)
        c = rng.integers(1, 3, n).astype(np.float64)
        dec = rng.uniform(size=(m, h)) < 0.05
        A[:, h:2 * h], c[h:2 * h] = np.maximum(A[:, :h] - dec, 0.0), c[:h]
        b = rng.integers(4, 12, m).astype(np.float64)
        bk = np.maximum(b + rng.integers(-3, 2, m), 0.0)
        for i in range(m - 2 * (m // 8), m, 2):   # the last m // 8 pairs of rows: twins
            A[i + 1], b[i + 1], bk[i + 1] = A[i], b[i], bk[i]
        lps.append(_ro(A, b, c))
        b2.append(bk)
    return lps, np.stack(b2)


def count_ties(T, basis, var, n, bk, resolve=O.resolve_rhs):
    """Replays the reference's dual run from (T, basis) one pivot at a time and counts, before
    each pivot, (exact leaving-row ties: a Dantzig-mode selection among >= 2 rows sharing the most
    negative RHS; exact entering-slot ties that cross a wave boundary: the minimum ratio held by
    a slot < 64 and a slot >= 64).  var is the slot map before the run."""
    m = len(basis)
    N = n + m
    var = np.array(var)
    first = resolve(T, basis, n, bk, max_pivots=0)
    T, basis, cont = first["T"], first["basis"], None
    if first["status"] != 3:
        return 0, 0, first
    bland = False
    rows = slots = 0
    last = first
    for _ in range(10 ** 4):
        rhs = T[:m, N]
        elig = np.nonzero(rhs < -TOL)[0]
        if len(elig) == 0:
            break
        if bland:
            p = int(elig[np.argmin(basis[elig])])
        else:
            ties = elig[rhs[elig] == rhs[elig].min()]
            rows += len(ties) >= 2
            p = int(ties[np.argmin(basis[ties])])
        a = T[p, var]
        cand = np.nonzero(a < -TOL)[0]                 # slots
        if len(cand):
            z = T[m, var[cand]]
            r = np.where(z > 0.0, z, 0.0) / (-a[cand])
            held = cand[r == r.min()]
            slots += len(held) >= 2 and held.min() < 64 <= held.max()
        last = resolve(T, basis, n, bk, max_pivots=1, continued=bland)
        if last["done"] == 0:
            break
        assert last["log"][0]["p"] == p
        var = slots_after(var, last["log"])
        T, basis, bland = last["T"], last["basis"], last["bland"]
    return int(rows), int(slots), last
