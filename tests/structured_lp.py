"""LPs with structure the generated ones lack, shared by tests/test_structured_ref.py (CPU) and
tests/test_gpu_structured.py (GPU): exact Dantzig ties, exact ratio ties at a nonzero ratio,
values exactly at the tolerances, subnormal and huge right-hand sides, signed zeros.

interval_lp   0/1 interval matrices (totally unimodular) with small integer b and c: every
              tableau entry stays an integer, the arithmetic is exact, and ties abound.
dup_lp        [A0 | A0] with U(0,1) data: the two copies of a column have bit-equal reduced
              costs until one of them becomes basic.
tie_stats     a plain numpy simplex of the pivot rule (oracle/oracle.cpp) that counts the ties
              and simulates the condensed slot map.
edge_cases    small named LPs at the edges of the rule.

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import functools
import types

import numpy as np

TOL = 1e-9
TOL_UP = float(np.nextafter(TOL, 1.0))


def interval_lp(m, n, seed, cmax, bmax, maxlen):
    rng = np.random.default_rng(seed)
    A = np.zeros((m, n))
    for j in range(n):
        a = rng.integers(0, m)
        l = rng.integers(1, maxlen + 1)
        A[a:a + l, j] = 1.0
    b = rng.integers(1, bmax + 1, m).astype(np.float64)
    c = rng.integers(1, cmax + 1, n).astype(np.float64)
    return A, b, c


def dup_lp(m, n_half, seed, spacing):
    """m x 2 n_half: every column of A0 (U(0,1), as c0) twice, the copy `spacing` columns after
    the original (blocks of `spacing` originals followed by their copies)."""
    assert n_half % spacing == 0
    rng = np.random.default_rng(seed)
    A0 = rng.random((m, n_half))
    b = rng.uniform(1.0, 2.0, m)
    c0 = rng.random(n_half)
    j = np.arange(n_half)
    first = 2 * spacing * (j // spacing) + j % spacing
    A = np.zeros((m, 2 * n_half))
    c = np.zeros(2 * n_half)
    for pos in (first, first + spacing):
        A[:, pos] = A0
        c[pos] = c0
    return A, b, c


def _simplex(A, b, c, pricing, by_slot, max_pivots=100000):
    """The rule in numpy (products rounded, then sums: exact on integer data).  Dantzig: the
    smallest z_j, ties to the smallest variable (by_slot: to the smallest condensed slot, the
    wrong rule); Bland (first z_j < -tol) after a degenerate pivot or always (pricing 1); ratio
    max(b_i, 0) / a_iq over a_iq > tol, ties to the smaller basis variable.  The condensed slot
    map: variable j < n starts in slot j, the leaving variable takes the entering one's slot."""
    m, n = A.shape
    N = n + m
    T = np.zeros((m + 1, N + 1))
    T[:m, :n] = A
    T[:m, n:N] = np.eye(m)
    T[:m, N] = b
    T[m, :n] = -np.asarray(c, dtype=np.float64)
    basis = np.arange(n, N)
    slot = np.full(N, -1)
    slot[:n] = np.arange(n)
    bland = pricing == 1
    s = types.SimpleNamespace(log=[], dantzig_pivots=0, dantzig_ties=0, slot_order_ties=0,
                              nonzero_ratio_ties=0, zero_ratio_ties=0, ratio_tie_rows=[], status=3)
    for _ in range(max_pivots):
        z = T[m, :N]
        if bland:
            neg = np.nonzero(z < -TOL)[0]
            if len(neg) == 0:
                s.status = 0
                break
            q = int(neg[0])
        else:
            zmin = z.min()
            if not zmin < -TOL:
                s.status = 0
                break
            tied = np.nonzero(z == zmin)[0]     # nonbasic: a basic variable has z = 0
            by_s = int(tied[np.argmin(slot[tied])])
            s.dantzig_pivots += 1
            if len(tied) > 1:
                s.dantzig_ties += 1
                s.slot_order_ties += int(by_s != tied[0])
            q = by_s if by_slot else int(tied[0])
        col = T[:m, q]
        elig = np.nonzero(col > TOL)[0]
        if len(elig) == 0:
            s.status = 2
            break
        rhs = T[elig, N]
        ratio = np.where(rhs > 0.0, rhs, 0.0) / col[elig]
        best = ratio.min()
        ties = elig[ratio == best]
        if len(ties) > 1:
            if best == 0.0:
                s.zero_ratio_ties += 1
            else:
                s.nonzero_ratio_ties += 1
                s.ratio_tie_rows.append(ties.copy())
        p = int(ties[np.argmin(basis[ties])])
        bland = pricing == 1 or best == 0.0
        slot[basis[p]], slot[q] = slot[q], -1
        basis[p] = q
        prow = T[p] / T[p, q]
        f = T[:, q].copy()
        f[p] = 0.0
        rows = np.nonzero(f != 0.0)[0]
        T[rows] = T[rows] - np.outer(f[rows], prow)
        T[p] = prow
        s.log.append((q, p))
    s.T, s.basis = T, basis
    s.x = np.zeros(n)
    for i in range(m):
        if basis[i] < n:
            s.x[basis[i]] = T[i, N]
    s.y = T[m, n:N].copy()
    s.objective = float(T[m, N])
    return s


def tie_stats(A, b, c, pricing=0):
    """The numpy simplex's solution (log of (q, p), status, objective, x, y, basis, final tableau
    T) with the tie counts: dantzig_pivots, dantzig_ties, slot_order_ties (Dantzig ties whose
    smallest-slot column is not the smallest-variable one), nonzero_ratio_ties (their row sets
    in ratio_tie_rows), zero_ratio_ties, and first_divergence: the pivot at which the log of the
    slot-order rule first differs (None if it never does)."""
    s = _simplex(A, b, c, pricing, False)
    w = _simplex(A, b, c, pricing, True).log
    k = next((i for i, (u, v) in enumerate(zip(s.log, w)) if u != v), None)
    if k is None and len(w) != len(s.log):
        k = min(len(w), len(s.log))
    s.first_divergence = k
    return s


# ---- the cases the GPU tests use; tests/test_structured_ref.py asserts that each has the ties
INTERVAL = dict(cmax=2, bmax=3, maxlen=6)
# session and rank paths: name -> interval_lp arguments
SESSION_INTERVAL = {
    "iv300x520_s0": dict(m=300, n=520, seed=0, **INTERVAL),
    "iv300x520_s3": dict(m=300, n=520, seed=3, **INTERVAL),
    "iv37x53_s40": dict(m=37, n=53, seed=40, **INTERVAL),
}
# sessions: name -> dup_lp arguments (the copy in the same lane pair / 25 columns on)
DUP = {
    "dup40x50_sp1": dict(m=40, n_half=25, seed=0, spacing=1),
    "dup40x50_sp25": dict(m=40, n_half=25, seed=0, spacing=25),
}
# batches of six dup LPs: (m, n) -> (seed, spacing) per LP (64 x 128: the copy in the next wave
# of the register kernel, half a wave on, in the same lane pair, two lanes on)
BATCH_DUP = {
    (64, 128): ((0, 64), (1, 32), (2, 1), (3, 64), (4, 2), (5, 64)),
    (40, 50): ((0, 25), (1, 1), (2, 5), (3, 25), (4, 1), (5, 5)),
}
# batches of six interval LPs: (m, n) -> (seeds, other interval_lp arguments)
BATCH_REGISTER = {
    (64, 64): ((1, 5, 9, 13, 18, 19), INTERVAL),
    (64, 128): ((0, 2, 4, 8, 9, 10), INTERVAL),
    (64, 191): ((0, 1, 2, 3, 4, 6), INTERVAL),
}
BATCH_LDS = {
    (37, 53): ((0, 1, 4, 5, 7, 8), dict(cmax=2, bmax=2, maxlen=10)),
    (65, 30): ((13, 14, 21, 44, 46, 57), INTERVAL),
}
NLP = 6


def _frozen(lp):
    for v in lp:
        v.setflags(write=False)   # shared between tests: copy before changing
    return lp


@functools.lru_cache(maxsize=None)
def session_lp(name):
    if name in SESSION_INTERVAL:
        return _frozen(interval_lp(**SESSION_INTERVAL[name]))
    return _frozen(dup_lp(**DUP[name]))


@functools.lru_cache(maxsize=None)
def batch_lp(m, n, k):
    seeds, kw = {**BATCH_REGISTER, **BATCH_LDS}[(m, n)]
    return _frozen(interval_lp(m, n, seeds[k], **kw))


@functools.lru_cache(maxsize=None)
def batch_dup_lp(m, n, k):
    seed, spacing = BATCH_DUP[(m, n)][k]
    return _frozen(dup_lp(m, n // 2, seed, spacing))


# ---- edge cases
EDGE_SMALL, EDGE_BIG = (5, 7), (64, 150)   # 64 x 150: three waves of the batched register kernel


def _positive(m, n, seed):
    rng = np.random.default_rng(seed)
    return rng, rng.uniform(0.5, 1.5, (m, n)), rng.uniform(1.0, 2.0, m), rng.uniform(0.1, 1.0, n)


def _z_at_tol(m, n):
    # only column 1 is eligible; A > 0, so the pivot raises every z_j and nothing becomes eligible
    rng, A, b, _ = _positive(m, n, 11)
    c = rng.uniform(0.0, TOL, n)
    c[2::3] = 0.0
    c[4::5] = -0.5
    c[0], c[1] = TOL, TOL_UP
    return A, b, c, dict(status=0, num_pivots=1, first_q=1, never_q=[0])


def _z_all_at_tol(m, n):
    rng, A, b, _ = _positive(m, n, 12)
    c = np.where(rng.random(n) < 0.5, 0.0, TOL)
    c[0], c[n - 1] = TOL, 0.0
    return A, b, c, dict(status=0, num_pivots=0)


_BELOW = [0.0, -0.0, -0.7, 5e-10, -TOL]


def _a_at_tol(m, n):
    # column q enters first; its only eligible row is r1, at a ratio of 1.5e9
    _, A, b, c = _positive(m, n, 13)
    q, r0, r1 = n // 2, 1, m - 2
    c[q] = 2.0
    A[:, q] = [_BELOW[i % len(_BELOW)] for i in range(m)]
    A[r0, q], A[r1, q] = TOL, TOL_UP
    b[r1] = 1.5
    return A, b, c, dict(status=0, first_q=q, first_p=r1)


def _a_all_at_tol(m, n):
    _, A, b, c = _positive(m, n, 14)
    q = n // 2
    c[q] = 2.0
    A[:, q] = [([TOL] + _BELOW)[i % (1 + len(_BELOW))] for i in range(m)]
    return A, b, c, dict(status=2, num_pivots=0)


def _subnormal_b(m, n):
    _, A, b, c = _positive(m, n, 15)
    idx = np.arange(0, m, 3)
    b[idx] = 5e-324 * (1 + np.arange(len(idx)) % 4)
    return A, b, c, dict(status=0)


def _huge_b(m, n):
    rng = np.random.default_rng(16)
    A, c = rng.uniform(0.25, 1.0, (m, n)), rng.uniform(0.1, 1.0, n)
    b = 1e300 * rng.uniform(1.0, 2.0, m)
    return A, b, c, dict(status=0, finite=True)


def _signed_zero(m, n):
    # c_j = +0.0 gives z_j = -0.0; A holds -0.0 in about a third of its entries
    rng, A, b, c = _positive(m, n, 17)
    mask = rng.random((m, n)) < 0.3
    mask[np.arange(n) % m, np.arange(n)] = False   # every column keeps a positive entry
    A[mask] = -0.0
    c[::3] = 0.0
    return A, b, c, dict(status=0, negzero_enters=True)


def _unbounded_late(m, n):
    # signed_zero with a column of +0.0, -0.0 and negative entries and a middling cost: it enters
    # after some pivots, mid-block on the deferred paths, and no row is eligible
    A, b, c, _ = _signed_zero(m, n)
    q = n // 2
    A[:, q] = [[0.0, -0.0, -0.7][i % 3] for i in range(m)]
    c[q] = 0.45
    return A, b, c, dict(status=2, min_pivots=1)


def _zero_column_rows(m, n):
    A, b, c = interval_lp(m, n, 18, cmax=3, bmax=4, maxlen=3)
    return A, b, c, dict(status=0, zero_rows=True)


_EDGE = dict(z_at_tol=_z_at_tol, z_all_at_tol=_z_all_at_tol, a_at_tol=_a_at_tol,
             a_all_at_tol=_a_all_at_tol, subnormal_b=_subnormal_b, huge_b=_huge_b,
             signed_zero=_signed_zero, unbounded_late=_unbounded_late,
             zero_column_rows=_zero_column_rows)
EDGE_NAMES = [f"{k}_{m}x{n}" for k in _EDGE for (m, n) in (EDGE_SMALL, EDGE_BIG)]


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(A, b, c, expectation) of one edge case; expectation: status, and where they are fixed
    num_pivots, first_q / first_p (the first pivot), never_q (columns that never enter)."""
    kind, shape = name.rsplit("_", 1)
    m, n = map(int, shape.split("x"))
    A, b, c, exp = _EDGE[kind](m, n)
    return _frozen((np.ascontiguousarray(A), np.ascontiguousarray(b), np.ascontiguousarray(c))) + (exp,)


def edge_cases():
    return {name: edge_case(name) for name in EDGE_NAMES}


# ---- comparison helpers of the GPU tests (here so that a child process can import them)
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def tableau_diff(T, Tref):
    """Positions (row, column) at which two tableaus differ in their bits."""
    return np.argwhere(bits(T) != bits(Tref))
