"""MW path at the envelope, search and report size boundaries: the CPU side (the GPU side is
tests/test_gpu_mw_edges.py; the shapes and what each is for are in tests/mw_shapes.py).

  * every shape's (maxdeg, empty impressions, bids) from the generator is pinned, and the envelope
    kernel, sort size, search path and report blocks that csrc/dlp_mw.hip's dispatch derives from
    them are the ones the shape is listed for;
  * dlp_mw_create's refusals, all taken before the device is touched;
  * the fp64 spec against the reference's own long-double run at the envelope shapes
    (tests/golden/ref_mw_edges.json, written by tests/golden/make_golden.py mw_edges), 30
    iterations: the comparison of tests/test_mw.py, with dual values of exactly 0 left out.  In
    binary mode a critical ratio that lands on a common slope leaves no region in (lower, upper]
    and that iteration prints 0, in either program, about once in 30 to 40 iterations
    (DESIGN.md §9): in these runs the spec at 175x175x0.1 (iteration index 27, the reference
    does not) and the reference at 244x244x0.5 (index 15, the spec does not).  At most one
    iteration per run and side may be left out besides iteration 1 of binary mode, which is 0
    in both."""
import math

import numpy as np
import pytest

import mw_shapes as S
import oracle_py as O
from conftest import load_golden

import distributedlpsolver_amd as dlp
from distributedlpsolver_amd import _lib as L

REF = load_golden("ref_mw_edges.json")["runs"]

# what each shape is listed for: envelope kernel and sort size of the largest impression
ENVELOPE_PATH = {
    "63x63x0.1": ("seg16", 16), "61x61x0.1": ("seg32", 32), "175x175x0.1": ("seg32", 32),
    "180x180x0.1": ("wave", 64), "238x238x0.2": ("wave", 64), "396x396x0.1": ("wave", 128),
    "244x244x0.5": ("wave", 128), "268x268x0.5": ("wave", 256), "354x354x1": ("wave", 256),
    "1520x1520x1": ("wave", 1024), "1502x1502x1": ("refused", 0),
}
FULL_SORT = {"63x63x0.1", "175x175x0.1", "238x238x0.2", "244x244x0.5", "354x354x1"}   # n == sort size
# (spec blocks, one launch, rounds of the 1,024 lanes), report blocks
SIZE_PATH = {
    "64x255x0.06": ((1, True, 1), 1), "64x256x0.06": ((1, True, 1), 1), "64x257x0.06": ((2, True, 1), 1),
    "128x1024x0.0166": ((4, True, 1), 1), "128x1025x0.0166": ((5, True, 2), 1),
    "1024x16384x0.0003": ((64, True, 16), 4), "1024x16385x0.0003": ((65, False, 0), 4),
    "256x256x0.015": ((1, True, 1), 1), "257x257x0.015": ((2, True, 1), 2),
}


@pytest.mark.parametrize("s", S.ALL, ids=S.shape_id)
def test_shape_properties_are_pinned(s):
    assert S.generator_props(s.A, s.I, s.sparsity) == (s.maxdeg, s.empties, s.bids)
    assert s.I // s.A >= 1          # budgets 0.5 * (I // A) * scaling are positive
    key = S.shape_id(s)
    if key in ENVELOPE_PATH:
        kernel, np2 = ENVELOPE_PATH[key]
        assert S.envelope_path(s.maxdeg) == (kernel, np2)
        assert (s.maxdeg + 1 == np2) == (key in FULL_SORT)
    else:                           # the size shapes stay in the 4-per-workgroup segment kernel
        assert S.envelope_path(s.maxdeg) == ("seg16", 16)
    if key in SIZE_PATH:
        assert (S.search_path(s.I), S.report_blocks(s.A)) == SIZE_PATH[key]
        assert s.empties > 0
    assert S.search_path(s.I)[1] == (s.I <= 16384)


def test_shape_list_covers_both_sides_of_every_edge():
    deg = sorted(s.maxdeg for s in S.ALL)
    for edge in (S.SEG16, S.SEG32, 64, 128):            # n = edge and n = edge + 1
        assert edge - 1 in deg and edge in deg, edge
    assert 255 in deg                                   # n = np2 = 256, four full rounds
    assert S.DEG_MAX - 2 in deg and S.DEG_MAX in deg    # n = 1023 accepted, n = 1025 refused
    imps = {s.I for s in S.SIZES}
    assert {255, 256, 257, 1024, 1025, 16384, 16385} <= imps
    assert {256, 257} <= {s.A for s in S.SIZES if s.A == s.I}
    assert S.SINGLE_BLOCKS * S.BIN_BLOCK == 16384 and S.CACHE_REGIONS * 16 == 144 * 1024
    odd32 = [s for s in S.ENVELOPE if S.envelope_path(s.maxdeg)[0] == "seg32" and s.I % 2]
    assert len(odd32) == 2 and any(s.empties for s in odd32)   # a tail segment with i >= I


def test_cache_shape_crosses_the_region_cache():
    s = S.CACHE
    assert s.I <= S.SINGLE_BLOCKS * S.BIN_BLOCK        # the one-launch search, where the cache lives
    r = S.spec(s.A, s.I, s.sparsity, s.T, True)
    R = r["regions"]
    assert tuple(R) == S.CACHE_REGIONS_RUN
    assert R[0] == s.I - s.empties                      # all weights 1: every hull is one line
    assert R[0] <= S.CACHE_REGIONS and R[1] <= S.CACHE_REGIONS
    assert (R[2:] > S.CACHE_REGIONS).all()
    assert (R <= s.bids).all()


@pytest.mark.parametrize("binary", [False, True])
def test_regions_of_the_first_iteration(binary):
    for s in S.ENVELOPE[:4]:
        r = S.spec(s.A, s.I, s.sparsity, 3, binary)
        assert r["regions"][0] == s.I - s.empties
        assert r["regions"][2] > r["regions"][0]        # the weights have separated


@pytest.mark.parametrize("binary", [False, True])
def test_tolerance_case_reaches_the_tight_set_branch(binary):
    """tests/test_gpu_mw_edges.py compares the GPU under tolerance 1e-6 with the spec under the
    same tolerance.  That sees the max(tol, 1e-12) branch only if 1e-6 changes the result: it
    does at 180x180 from iteration 27 (sort) / 26 (binary) on, hence S.TOLERANCE_T = 30
    iterations there; at 63x63 it changes nothing within 30."""
    A, I, sp = 180, 180, 0.1
    a = S.spec(A, I, sp, S.TOLERANCE_T, binary)
    b = S.spec(A, I, sp, S.TOLERANCE_T, binary, tolerance=1e-6)
    differ = np.nonzero(a["dual"] != b["dual"])[0]
    assert len(differ) and differ[0] == (26 if binary else 27)
    assert (a["x_avg"] != b["x_avg"]).any()
    c = S.spec(A, I, sp, S.TOLERANCE_T, binary, tolerance=1e-13)   # below 1e-12: the default's bits
    assert c["dual"].tobytes() == a["dual"].tobytes() and c["x_avg"].tobytes() == a["x_avg"].tobytes()


# ---------------------------------------------------------------- refusals (no device call)
def _refused(problem, status, text, **kw):
    with pytest.raises(dlp.DLPError) as e:
        dlp.MW(problem, **kw)
    assert e.value.status == status
    assert text in L.last_error() and text in str(e.value)


def test_create_refuses_more_points_than_the_envelope_kernel_holds():
    s = S.REFUSED
    _refused(dlp.Problem.adalloc(s.A, s.I, 1, s.sparsity, 0.25), L.ERR_UNSUPPORTED, "more bids")
    _refused(dlp.Problem.adalloc(s.A, s.I, 1, s.sparsity, 0.25), L.ERR_UNSUPPORTED, "more bids", binary=True)


def test_create_refuses_a_dense_problem():
    A, b, c = O.gen_dense(4, 6, 1)
    _refused(dlp.Problem.dense(A, b, c), L.ERR_ARG, "ad-allocation")


def test_create_refuses_a_problem_without_bids():
    p = dlp.Problem.adalloc(8, 16, 1, 0.0, 0.25)
    assert p.n == 0
    _refused(p, L.ERR_ARG, "no bids")
    _refused(p, L.ERR_ARG, "no bids", binary=True)


@pytest.mark.parametrize("intervals", [0, 9, -1])
def test_create_refuses_binary_intervals_outside_1_to_8(intervals):
    p = dlp.Problem.adalloc(63, 63, 1, 0.1, 0.25)
    _refused(p, L.ERR_ARG, "intervals", binary=True, intervals=intervals)


@pytest.mark.parametrize("epsilon", [0.0, 1.0, math.nan, -0.01, 1.5])
def test_create_refuses_epsilon_outside_the_open_unit_interval(epsilon):
    p = dlp.Problem.adalloc(63, 63, 1, 0.1, 0.25)
    _refused(p, L.ERR_ARG, "epsilon", epsilon=epsilon)
    _refused(p, L.ERR_ARG, "epsilon", epsilon=epsilon, binary=True)


# ---------------------------------------------------------------- spec against the reference
@pytest.mark.parametrize("key", sorted(REF))
def test_mw_spec_tracks_reference_dual_at_the_edge_shapes(key):
    ref = REF[key]
    binary = ref["mode"] == "binary"
    T = ref["iterations"]
    assert T == 30
    r = S.spec(ref["A"], ref["I"], ref["sparsity"], T, binary)
    rd, d = np.array(ref["dual_values"]), r["dual"]
    assert len(rd) == T
    first = 0
    if binary:                      # iteration 1: the search brackets the common slope 1 from above
        assert rd[0] == 0.0 and d[0] == 0.0
        first = 1
    assert (d[first:] == 0.0).sum() <= 1 and (rd[first:] == 0.0).sum() <= 1
    keep = (d != 0.0) & (rd != 0.0)
    assert keep[first:].sum() >= T - first - 2
    rel = np.abs(d - rd) / np.where(keep, rd, 1.0)
    head = keep.copy()
    head[first + 5:] = False
    print(f"{key}: left out {np.nonzero(~keep)[0].tolist()}, first five {rel[head].max():.3g}, "
          f"run {rel[keep].max():.3g}")
    assert head.sum() >= 4
    assert rel[head].max() < 1e-5   # the reference prints 6 significant digits
    assert rel[keep].max() < 1e-3   # tie-order drift (tests/test_mw.py)
    assert (d[keep] > 0.0).all() and np.isfinite(d).all()


def test_reference_binary_runs_only_where_every_impression_has_a_bid():
    """The reference's binary mode ends with SIGSEGV when an impression has no bid, so the
    fixture holds a binary run for exactly the envelope shapes without one."""
    want = set()
    for s in S.ENVELOPE:
        want.add(f"{S.shape_id(s)}/sort")
        if s.empties == 0:
            want.add(f"{S.shape_id(s)}/binary")
    assert set(REF) == want
    assert "61x61x0.1/binary" not in REF
