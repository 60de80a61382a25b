"""Inputs that put the decisions of the session's dual phase (dlp_dual.hip) on its kernel
boundaries, shared by tests/test_dual_inputs.py (CPU: every property claimed here, on the C++
oracle alone) and tests/test_gpu_session_rhs_wide.py (GPU, bit for bit).

The boundaries: rhs_rebuild_kernel gives one wave 64 stored rows (m + 1 of them, the objective
row last) and folds the slack block in 64-column tiles; dual_row_kernel takes 256 rows per
workgroup; dual_col_kernel 512 columns per workgroup, 2 per lane.  From the second workgroup on
the winner is reduced by the last workgroup to arrive.

SHAPES        (m, n) -> the boundary crossed
dense_lp      the generated LP, then b moved by +-30 % (tests/test_gpu_session_rhs.py's)
cone_lp       c <= 0, A in [-1, 1): optimal at the slack basis for |b|; b has m // 16 + 4
              negative entries, spread over the rows so that both row workgroups hold some when
              m > 256 (no zero cost: a nonbasic z_j = 0 stays one for good and makes most pivots
              zero-ratio ones, 2,891 instead of 105 at 300 x 740; dup_cols has the zero ratios)
tied_lp       "dup_rows": rows i and i + 256 identical with an equal b: they stay bit-equal until
              one of them is the pivot row, so the leaving-row argmin ties across the two row
              workgroups; "dup_cols": columns j and j + 512 identical with an equal cost: bit-equal
              until one is basic, so the entering ratio ties across column workgroups
trace         the oracle stepped one pivot at a time, with the ties of every decision counted

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import functools
import types

import numpy as np

import oracle_py as O
import rhs_ref as RR

ROW_BLOCK, COL_BLOCK = 256, 512      # dual_row_kernel / dual_col_kernel: decisions per workgroup
TOL = 1e-9

SHAPES = {
    (63, 70): "64 stored rows: exactly one rebuild workgroup",
    (64, 66): "the last rebuild workgroup holds the objective row alone; one full tile, no partial one",
    (65, 449): "a partial tile of 1; N = 514 is even and crosses the column tile by 2",
    (128, 385): "two full tiles; N = 513 is odd: the last pair is (column 512, RHS)",
    (255, 258): "one short of a full row workgroup; N = 513",
    (256, 257): "exactly one row workgroup; N = 513",
    (257, 260): "the second row workgroup holds one row",
    (300, 740): "2 row workgroups, 3 column workgroups, 5 tiles",
}
WIDEST = (300, 740)
BIG = 10 ** 6
# seeds: chosen so that tests/test_dual_inputs.py's conditions hold (change the seed, not the condition)
DENSE_SEED = {s: 7300 + i for i, s in enumerate(SHAPES)}
CONE_SEED = {s: 7400 + i for i, s in enumerate(SHAPES)}


def _frozen(lp):
    for v in lp:
        v.setflags(write=False)   # shared between tests: copy before changing
    return lp


@functools.lru_cache(maxsize=None)
def dense_lp(m, n):
    """(A, b, c, b2): the generated LP and b2 = b (1 + 0.3 u)."""
    seed = DENSE_SEED[(m, n)]
    A, b, c = O.gen_dense(m, n, seed)
    b2 = b * (1.0 + 0.3 * np.random.default_rng(seed).uniform(-1.0, 1.0, m))
    return _frozen((A, b, c, b2))


def _rhs(rng, A):
    """b = A x0 + u with a small x0 >= 0 and u in [0.2, 1): x0 is feasible and b is positive but
    for the entries the caller pushes negative afterwards (a U(0, 1) x0 makes |A x0| ~ sqrt(n) / 3,
    half of b negative and the dual phase thousands of pivots long)."""
    m, n = A.shape
    return A @ (rng.uniform(0.0, 1.0, n) * (0.3 / np.sqrt(n))) + rng.uniform(0.2, 1.0, m)


def _negative_rows(m, k):
    """k rows spread evenly over 0 .. m-1, the last row among them (with m > 256 both row
    workgroups hold some)."""
    return np.unique(np.linspace(0, m - 1, k).round().astype(np.int64))


@functools.lru_cache(maxsize=None)
def cone_lp(m, n):
    """(A, b, c): c <= 0, so the slack basis is dual feasible; the session is created with |b|
    (optimal without a pivot) and handed b."""
    rng = np.random.default_rng(CONE_SEED[(m, n)])
    A = rng.uniform(-1.0, 1.0, (m, n))
    b = _rhs(rng, A)
    rows = _negative_rows(m, m // 16 + 4)
    b[rows] = -rng.uniform(0.1, 0.5, len(rows))
    c = -rng.uniform(0.0, 1.0, n)
    return _frozen((A, b, c))


# ---- ties across workgroups
# name -> (generator, arguments).  The wide ones sit on the kernels' boundaries; the small ones
# have the same construction at a size tests/rhs_ref.py can afford (tests/test_oracle_dual.py),
# with "workgroups" of 20 rows / 16 columns that exist only in the counting of trace().
TIED = {
    "dup_rows": ("rows", dict(m=300, n=740, block=ROW_BLOCK, pairs=12, seed=7500)),
    "dup_cols": ("cols", dict(m=300, n=740, block=COL_BLOCK, dups=120, lane=40, slack=8, seed=7600)),
    "dup_rows_small": ("rows", dict(m=40, n=40, block=20, pairs=6, seed=7501)),
    "dup_cols_small": ("cols", dict(m=30, n=40, block=16, dups=8, lane=2, slack=2, seed=7601)),
}


def dup_rows_lp(m, n, block, pairs, seed):
    """(A, b, c).  Rows i and i + block (i < pairs) are equal in A and in b, and their b is the
    most negative: from the slack basis both rows go through the same operations on the same
    values until one of them is the pivot row, so T[i][N] == T[i + block][N] bit for bit at
    every pivot before, and the leaving-row argmin ties between row workgroup 0 and 1.

    At the slack basis basis[i] = n + i, so the lower row would win every tie.  For the even
    pairs the higher row r = i + block therefore gets a column of its own, e_r at column
    n - pairs + i with a small positive cost: the cold solve (b >= 0, so it is a primal one)
    enters exactly these pairs / 2 columns, each in its only row, and leaves basis[r] < n <=
    basis[i].  Such a pivot divides row r by 1 and touches the objective row alone; the costs are
    small enough (pairs / 2 x 0.004 < 0.1 <= -c_j) that no other reduced cost turns negative.
    The column stays a unit vector afterwards, so the two rows stay equal in every column both of
    them store."""
    assert block + pairs <= m and pairs <= 40
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1.0, 1.0, (m, n))
    c = -rng.uniform(0.1, 1.0, n)
    lo = np.arange(pairs)
    flipped = lo[::2]
    own = n - pairs + flipped
    A[:, own] = 0.0
    A[lo + block] = A[lo]
    A[flipped + block, own] = 1.0
    c[own] = 0.002 + 0.002 * rng.random(len(own))
    b = _rhs(rng, A)
    other = _negative_rows(m, 6)                 # untied negative rows in both workgroups
    other = other[(other % block >= pairs) | (other >= 2 * block)]
    b[other] = -rng.uniform(0.05, 0.2, len(other))
    b[lo] = -rng.uniform(0.3, 0.6, pairs)
    b[lo + block] = b[lo]
    return A, b, c


def dup_cols_lp(m, n, block, dups, lane, slack, seed):
    """(A, b, c).  Columns j and j + block (j < dups) are equal in A and in c: a column's update
    reads nothing but the column itself and values shared by all columns, so the two stay
    bit-equal until one is basic, and whenever one of them has the smallest ratio the other ties
    with it from the next column workgroup; the rule gives the pivot to the smaller j.  Columns
    lane and lane + 1 are equal too (one lane's pair in dual_col_kernel; with their copies a
    4-way tie).  Every fifth duplicated column has cost 0: its ratio is 0 whenever it is a
    candidate, which adds ties at ratio 0 and, with Dantzig pricing, pivots chosen in Bland mode.
    Columns dups + k and their copies (k < slack) are e_r, r = m - slack + k, with cost 0:
    the very column of slack r, which sits at n + r in the last column workgroup (300 x 740:
    1032 + k, the third).  Once row r has been the pivot row that slack is nonbasic and bit-equal
    to its two copies.  b is negative in those rows so that they leave."""
    assert lane % 2 == 0 and lane + 1 < dups and dups + slack <= block and block + dups + slack <= n
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1.0, 1.0, (m, n))
    c = -rng.uniform(0.1, 1.0, n)
    j = np.arange(dups)
    c[j[::5]] = 0.0
    A[:, lane + 1] = A[:, lane]
    c[lane + 1] = c[lane]
    k = np.arange(slack)
    A[:, dups + k] = 0.0
    A[m - slack + k, dups + k] = 1.0
    c[dups + k] = 0.0
    for src in (j, dups + k):
        A[:, src + block] = A[:, src]
        c[src + block] = c[src]
    b = _rhs(rng, A)
    rows = np.concatenate([_negative_rows(m - slack, 6), m - slack + k])
    b[rows] = -rng.uniform(0.1, 0.5, len(rows))
    return A, b, c


@functools.lru_cache(maxsize=None)
def tied_lp(name):
    kind, kw = TIED[name]
    return _frozen((dup_rows_lp if kind == "rows" else dup_cols_lp)(**kw))


def tied_blocks(name):
    """(rows, columns) per workgroup in the counting of trace()."""
    kind, kw = TIED[name]
    return (kw["block"], COL_BLOCK) if kind == "rows" else (ROW_BLOCK, kw["block"])


def cold_start(A, b, c):
    """(T0, basis0, cold pivots): the tableau and basis the session holds after its cold solve of
    (A, |b|, c), from the C++ oracle (the GPU tests take the session's own)."""
    import reopt_ref as R
    T, basis = R.oracle_tableau(A, np.abs(b), c, 10 ** 6)
    ref = O.solve_dense(A, np.abs(b), c)
    assert ref.status == RR.OK and ref.basis.tobytes() == basis.tobytes()
    return T, basis, ref.num_pivots


def trace(T0, basis0, n, b, pricing=0, max_pivots=BIG, blocks=(ROW_BLOCK, COL_BLOCK)):
    """The oracle's dual phase on (T0, basis0) with the new b, one pivot per call (the
    continuation of include/dlp.h) for up to max_pivots, and what each decision looked like just before it was taken.
    Returns a namespace: res (the last call's dict, its log the whole phase's), and per pivot
      row_tied      rows whose candidate equals the winner's (Dantzig: equal T[i][N]; Bland: every
                    other eligible row, since only basis[i] orders them) in another row workgroup
      row_higher    the winner sits in a higher row workgroup than one of those
      both_blocks   eligible rows in more than one row workgroup
      col_tied      columns with the winner's ratio in another column workgroup
      col_blocks    the number of column workgroups the tied set (winner included) spans
      lane_pair     the winner's lane partner (q ^ 1) ties with it
      bland         the decision was taken in Bland mode"""
    m = len(basis0)
    N = n + m
    RB, CB = blocks
    res = O.resolve_rhs(T0, basis0, n, b, max_pivots=0, pricing=pricing)
    t = types.SimpleNamespace(row_tied=[], row_higher=[], both_blocks=[], col_tied=[], col_blocks=[],
                              lane_pair=[], bland=[], res=res)
    logs = []
    while res["status"] == RR.PIVOT_LIMIT and len(logs) < max_pivots:
        T, basis, bland = res["T"], res["basis"], res["bland"]
        res = O.resolve_rhs(T, basis, n, b, max_pivots=1, pricing=pricing, continued=bland)
        if res["done"] == 0:                             # no entering column
            assert res["status"] == RR.INFEASIBLE
            break
        q, p = int(res["log"]["q"][0]), int(res["log"]["p"][0])
        logs.append(res["log"])
        rhs = T[:m, N]
        elig = np.nonzero(rhs < -TOL)[0]
        tied = elig if bland else elig[rhs[elig] == rhs[p]]
        tied = tied[tied != p]
        other = tied[tied // RB != p // RB]
        assert bland or rhs[p] == rhs[elig].min()
        assert (basis[tied] > basis[p]).all()            # the rule: ties to the smallest basis[i]
        t.row_tied.append(len(other))
        t.row_higher.append(bool((other // RB < p // RB).any()))
        t.both_blocks.append(len(np.unique(elig // RB)) > 1)
        nonbasic = np.ones(N, bool)
        nonbasic[basis] = False
        a, z = T[p, :N], T[m, :N]
        cand = np.nonzero(nonbasic & (a < -TOL))[0]
        r = np.where(z[cand] > 0.0, z[cand], 0.0) / -a[cand]
        same = cand[r == res["log"]["ratio"][0]]
        assert q in same and q == same.min() and r.min() == res["log"]["ratio"][0]
        t.col_tied.append(int((same // CB != q // CB).sum()))
        t.col_blocks.append(len(np.unique(same // CB)))
        t.lane_pair.append((q ^ 1) in same)
        t.bland.append(bool(bland))
    res = dict(res, log=np.concatenate(logs) if logs else np.zeros(0, O.PIVOT_DTYPE), done=sum(map(len, logs)))
    t.res = res
    for k, v in list(vars(t).items()):
        if isinstance(v, list):
            setattr(t, k, np.array(v))
    return t
