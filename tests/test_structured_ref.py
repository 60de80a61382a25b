"""CPU: the structured LPs of tests/structured_lp.py against the oracle.

On the interval LPs every tableau entry is an integer and the arithmetic is exact, so the plain
numpy simplex of tie_stats and the oracle must take the same pivots and reach the same values:
that pins the oracle's tie rules (Dantzig ties to the smaller variable, ratio ties to the smaller
basis variable) independently of the oracle's own code.  The edge cases' expectations hold on the
oracle, and every case the GPU file (tests/test_gpu_structured.py) uses has the ties it is there
for: these conditions keep the GPU tests from going blind."""
import functools

import numpy as np
import pytest

import oracle_py as O
import structured_lp as S

BATCH = {**S.BATCH_REGISTER, **S.BATCH_LDS}
BATCH_IDS = [(m, n, k) for (m, n) in BATCH for k in range(S.NLP)]


@functools.lru_cache(maxsize=None)
def _stats(name, pricing=0):
    return S.tie_stats(*S.session_lp(name), pricing=pricing)


@functools.lru_cache(maxsize=None)
def _batch_stats(m, n, k, pricing=0):
    return S.tie_stats(*S.batch_lp(m, n, k), pricing=pricing)


def _same_as_oracle(lp, st, pricing):
    A, b, c = lp
    ref = O.solve_dense(A, b, c, pricing=pricing, nthreads=1)
    assert ref.status == st.status == 0
    assert [(int(e["q"]), int(e["p"])) for e in ref.pivot_log] == st.log
    assert ref.num_pivots == len(st.log)
    assert np.array_equal(st.T, np.round(st.T))          # the arithmetic was exact
    assert ref.objective == st.objective
    assert np.array_equal(ref.x, st.x) and np.array_equal(ref.y, st.y)
    assert np.array_equal(ref.basis, st.basis)
    # a feasible point of the LP that attains the objective
    assert (A @ ref.x <= b).all() and (ref.x >= 0).all() and c @ ref.x == ref.objective


@pytest.mark.parametrize("pricing", [0, 1])
@pytest.mark.parametrize("name", list(S.SESSION_INTERVAL))
def test_oracle_takes_the_numpy_simplex_pivots(name, pricing):
    _same_as_oracle(S.session_lp(name), _stats(name, pricing), pricing)


@pytest.mark.parametrize("pricing", [0, 1])
@pytest.mark.parametrize("m,n,k", BATCH_IDS)
def test_oracle_takes_the_numpy_simplex_pivots_batch_lps(m, n, k, pricing):
    _same_as_oracle(S.batch_lp(m, n, k), _batch_stats(m, n, k, pricing), pricing)


def test_interval_lp_is_the_stated_family():
    """Column j is one run of ones; b and c are integers in range; the draws are in the stated
    order (a and l per column, then b, then c)."""
    m, n, seed = 37, 53, 0
    A, b, c = S.interval_lp(m, n, seed, cmax=2, bmax=2, maxlen=10)
    rng = np.random.default_rng(seed)
    for j in range(n):
        a, l = int(rng.integers(0, m)), int(rng.integers(1, 11))
        want = np.zeros(m)
        want[a:a + l] = 1.0
        assert np.array_equal(A[:, j], want)
    assert np.array_equal(b, rng.integers(1, 3, m)) and np.array_equal(c, rng.integers(1, 3, n))
    assert A.dtype == b.dtype == c.dtype == np.float64


@pytest.mark.parametrize("name", list(S.DUP))
def test_dup_lp_copies(name):
    kw = S.DUP[name]
    A, b, c = S.session_lp(name)
    sp, nh = kw["spacing"], kw["n_half"]
    assert A.shape == (kw["m"], 2 * nh)
    first = [j for j in range(2 * nh) if (j // sp) % 2 == 0]
    assert len(first) == nh
    for j in first:
        assert A[:, j].tobytes() == A[:, j + sp].tobytes() and c[j] == c[j + sp]
    assert len({A[:, j].tobytes() for j in first}) == nh
    assert (A > 0).all() and (A < 1).all() and (c > 0).all() and (c < 1).all()


# ---- the conditions
@pytest.mark.parametrize("name", list(S.SESSION_INTERVAL))
def test_session_cases_have_the_ties(name):
    st = _stats(name)
    print(name, len(st.log), st.dantzig_ties, st.slot_order_ties, st.nonzero_ratio_ties,
          st.zero_ratio_ties, st.first_divergence)
    assert st.dantzig_ties >= 20
    assert st.slot_order_ties >= (3 if name.startswith("iv37x53") else 5)
    assert st.nonzero_ratio_ties >= 5
    assert st.first_divergence is not None and st.first_divergence < len(st.log) - 1


@pytest.mark.parametrize("m,n,k", [i for i in BATCH_IDS if i[:2] in S.BATCH_REGISTER])
def test_register_kernel_cases_have_slot_order_ties(m, n, k):
    assert m == 64 and _batch_stats(m, n, k).slot_order_ties >= 5


@pytest.mark.parametrize("m,n,k", [i for i in BATCH_IDS if i[:2] in S.BATCH_LDS])
def test_lds_kernel_cases_have_the_ties(m, n, k):
    """Fewer columns than rows leave few slots to permute: at least one slot-order tie, ten
    Dantzig ties and five nonzero ratio ties in every LP of these batches."""
    st = _batch_stats(m, n, k)
    assert st.slot_order_ties >= 1 and st.dantzig_ties >= 10 and st.nonzero_ratio_ties >= 5
    assert st.first_divergence is not None


DUP_LPS = [(name,) for name in S.DUP] + [(m, n, k) for (m, n) in S.BATCH_DUP for k in range(S.NLP)]


@pytest.mark.parametrize("case", DUP_LPS, ids=lambda c: "-".join(map(str, c)))
def test_dup_cases_tie_in_half_their_dantzig_pivots(case):
    lp = S.session_lp(*case) if len(case) == 1 else S.batch_dup_lp(*case)
    st = S.tie_stats(*lp)
    print(case, st.dantzig_pivots, st.dantzig_ties)
    assert st.status == 0 and st.dantzig_pivots == len(st.log) > 0
    assert 2 * st.dantzig_ties >= st.dantzig_pivots
    # the oracle (fma arithmetic) takes the same columns and rows on these LPs
    ref = O.solve_dense(*lp, nthreads=1)
    assert [(int(e["q"]), int(e["p"])) for e in ref.pivot_log] == st.log


def test_ratio_ties_span_eight_ranks():
    """With the rows cut into 8 blocks (rank r holds rows [m r / 8, m (r + 1) / 8), the partition
    of dlp_rank_rows), the tied rows of several of the 300 x 520 case's nonzero ratio ties lie
    in different blocks (an interval column ties neighbouring rows, so most ties stay within
    a block: at least 3, so that the comparison across ranks decides more than once)."""
    m = 300
    edges = [m * r // 8 for r in range(1, 8)]
    st = _stats("iv300x520_s0")
    spans = [len(set(np.searchsorted(edges, rows, side="right"))) > 1 for rows in st.ratio_tie_rows]
    assert sum(spans) >= 3


# ---- the edge cases on the oracle
@pytest.mark.parametrize("name", S.EDGE_NAMES)
def test_edge_case_expectations(name):
    A, b, c, exp = S.edge_case(name)
    m, n = A.shape
    assert (m, n) in (S.EDGE_SMALL, S.EDGE_BIG) and S.EDGE_BIG[0] == 64 and 65 <= S.EDGE_BIG[1] <= 191
    ref = O.solve_dense(A, b, c, nthreads=1)
    log = ref.pivot_log
    assert ref.status == exp["status"]
    if "num_pivots" in exp:
        assert ref.num_pivots == exp["num_pivots"]
    if "min_pivots" in exp:   # unbounded_late: the column without an eligible row enters later
        assert ref.num_pivots >= exp["min_pivots"]
        col = A[:, n // 2]
        assert (col <= 0.0).all() and np.signbit(col[col == 0.0]).any() and (col < 0.0).any()
    if "first_q" in exp:
        assert log[0]["q"] == exp["first_q"]
    if "first_p" in exp:
        assert log[0]["p"] == exp["first_p"]
    for j in exp.get("never_q", []):
        assert j not in log["q"]
    if exp.get("finite"):
        assert np.isfinite(ref.x).all() and np.isfinite(ref.y).all() and np.isfinite(ref.objective)
        assert np.isfinite(log["ratio"]).all() and ref.objective > 1e299
    if exp.get("negzero_enters"):
        neg = (A == 0.0) & np.signbit(A)
        entered = [q for q in log["q"] if q < n]
        assert sum(neg[:, q].any() for q in entered) >= 2
        assert np.signbit(-c[c == 0.0]).all() and (c == 0.0).sum() >= 2
    if exp.get("zero_rows"):
        assert ref.num_pivots >= 3 and all((A[:, q] == 0.0).sum() >= m // 2 for q in log["q"] if q < n)
        assert np.array_equal(A, np.round(A))


def test_edge_case_data_is_what_the_names_say():
    for shape in ("5x7", "64x150"):
        A, b, c, _ = S.edge_case(f"z_at_tol_{shape}")
        assert c[0] == 1e-9 and c[1] == np.nextafter(1e-9, 1) and (np.delete(c, 1) <= 1e-9).all()
        A, b, c, _ = S.edge_case(f"z_all_at_tol_{shape}")
        assert set(c) == {0.0, 1e-9}
        A, b, c, exp = S.edge_case(f"a_at_tol_{shape}")
        col = A[:, exp["first_q"]]
        assert col[exp["first_p"]] == np.nextafter(1e-9, 1) and (col == 1e-9).sum() >= 1
        assert (np.delete(col, exp["first_p"]) <= 1e-9).all() and int(np.argmax(c)) == exp["first_q"]
        A, b, c, _ = S.edge_case(f"a_all_at_tol_{shape}")
        col = A[:, int(np.argmax(c))]
        assert (col <= 1e-9).all() and (col == 1e-9).any()
        A, b, c, _ = S.edge_case(f"subnormal_b_{shape}")
        sub = b[b < 1e-300]
        assert len(sub) >= 2 and (sub > 0).all() and np.array_equal(sub / 5e-324, np.round(sub / 5e-324))
        assert (b[b >= 1e-300] >= 1.0).all()
        A, b, c, _ = S.edge_case(f"huge_b_{shape}")
        assert (b >= 1e300).all() and (A > 0).all() and (A <= 1).all() and (c > 0).all() and (c <= 1).all()


def test_subnormal_ratios_reach_the_division():
    """The first pivots of subnormal_b divide a subnormal b_i: the logged ratio is subnormal."""
    for shape in ("5x7", "64x150"):
        A, b, c, _ = S.edge_case(f"subnormal_b_{shape}")
        r = O.solve_dense(A, b, c, nthreads=1).pivot_log["ratio"]
        assert ((r > 0) & (r < 2.3e-308)).any()
