"""Shapes of the MW edge tests (tests/test_mw_edges.py on the CPU, tests/test_gpu_mw_edges.py on
the GPU), each with the path of csrc/dlp_mw.hip it is there for, the constants of
that file's dispatch, and the shared "GPU log and solution equal the fp64 spec, bit for bit"
comparison.

The generated ad-allocation instance is fixed by (A, I, sparsity): the generator's seed is 1
(oracle_gen_adalloc).  So a shape decides the largest bid count of an impression (`maxdeg`), the
number of impressions without a bid and the number of bids, and with them which kernels run.
tests/test_mw_edges.py pins these three per shape and derives the paths from them, so that a
change of the generator or of this list cannot move a case off its edge unnoticed.

Not collected (no test_ prefix); imported as a plain module (tests/ is on sys.path)."""
import functools
from collections import namedtuple

import numpy as np

import oracle_py as O

# ---- dispatch constants of distributedlpsolver_amd/csrc/dlp_mw.hip (the line each comes from)
SEG16 = 16              # :1248  maxdeg + 1 <= 16 -> envelope_seg_kernel<16>, 4 impressions / workgroup
SEG32 = 32              # :1251  maxdeg + 1 <= 32 -> envelope_seg_kernel<32>, 2 impressions / workgroup
WAVE = 64               # :180   envelope_kernel: 64 lanes take the np2 points in rounds of 64
DEG_MAX = 1024          # :52    kDegMax, points (bids + origin) per impression; :1086 refuses more
BIN_BLOCK = 256         # :575   kBinBlock, impressions per block of the spec's blocked sum
SEARCH_LANES = 1024     # :810   bin_search_single_kernel: 4 groups of 256 lanes; :831 one round
SINGLE_BLOCKS = 64      # :576   kBinSingleBlocks; :1191 the whole search in one launch up to 64 blocks
CACHE_REGIONS = 9216    # :1192  kCacheMax = 144 KiB; :1202 regions cached in LDS while R * 16 fits
REPORT_BLOCK = 256      # :1125  report_kernel: one block per 256 advertisers (at most 1024 blocks)
MAX_RATIOS = 8          # :573   kBinMaxRatios, `intervals` accepted in binary mode

Shape = namedtuple("Shape", "A I sparsity maxdeg empties bids T why")

# ---- envelope kernels: (maxdeg, empty impressions, bids) from oracle_gen_adalloc.  12 iterations:
# the weights separate only after iteration 1 (2 in binary mode), before that every hull is a line.
ENVELOPE = [
    Shape(63, 63, 0.1, 15, 0, 415, 12, "<16>, a full 16-point segment (origin in the last lane)"),
    Shape(61, 61, 0.1, 16, 1, 408, 12, "<32>, first size past <16>, one empty impression, odd I"),
    Shape(175, 175, 0.1, 31, 0, 3016, 12, "<32>, a full 32-point segment, odd I"),
    Shape(180, 180, 0.1, 32, 0, 3265, 12, "envelope_kernel, n = 33, np2 = 64"),
    Shape(238, 238, 0.2, 63, 0, 10371, 12, "envelope_kernel, n = np2 = 64"),
    Shape(396, 396, 0.1, 64, 0, 15051, 12, "envelope_kernel, n = 65, np2 = 128 (two rounds)"),
    Shape(244, 244, 0.5, 127, 0, 23322, 12, "envelope_kernel, n = np2 = 128"),
    Shape(268, 268, 0.5, 128, 0, 28305, 12, "envelope_kernel, np2 = 256"),
    Shape(354, 354, 1.0, 255, 0, 79466, 12, "envelope_kernel, n = np2 = 256"),
]
# np2 = 1024 = kDegMax.  A search at sparsity 1.0 of A = I in 1495..1534 and of A = 1480, 1483,
# .. 1528 with I = A - 20 and A + 20 (74 shapes, none above 1.5 M bids) found no maxdeg == 1023
# (n == kDegMax exactly); 1022 is the closest from below, so this shape, n = 1023, stands for
# the largest sort.
DEG_MAX_SHAPE = Shape(1520, 1520, 1.0, 1022, 0, 1460814, 4, "envelope_kernel, np2 = 1024 = kDegMax")
REFUSED = Shape(1502, 1502, 1.0, 1024, 0, 1425877, 0, "n = 1025 > kDegMax: DLP_ERR_UNSUPPORTED")

# ---- size edges of the binary search and of the report, a few thousand bids at the most, with
# impressions without a bid (their lanes add 0 to the blocked sums).  Advertisers and draws are
# chosen so that the budgets bind (bids per advertiser > (I // A) / 4): where they do not, no
# threshold holds the budget and every search ends at the 2,048-level cap.
SIZES = [
    Shape(64, 255, 0.06, 10, 5, 992, 12, "I = 255: one spec block, its last lane idle"),
    Shape(64, 256, 0.06, 9, 9, 985, 12, "I = 256: one full spec block"),
    Shape(64, 257, 0.06, 10, 2, 990, 12, "I = 257: a second spec block of one impression"),
    Shape(128, 1024, 0.0166, 7, 127, 2154, 12, "I = 1024: four blocks, one round of the 1,024 lanes"),
    Shape(128, 1025, 0.0166, 7, 95, 2288, 12, "I = 1025: five blocks, two rounds"),
    Shape(1024, 16384, 0.0003, 4, 11979, 5120, 6, "I = 16384: 64 blocks, the last single launch"),
    Shape(1024, 16385, 0.0003, 5, 11976, 5120, 6, "I = 16385: 65 blocks, one launch per level"),
    Shape(256, 256, 0.015, 10, 9, 1013, 12, "A = 256: report_kernel in one block"),
    Shape(257, 257, 0.015, 10, 2, 1020, 12, "A = 257: report_kernel in two blocks + last-block combine"),
]

# ---- LDS region cache of the one-launch search: R = 7080 non-empty impressions at iterations 1
# and 2 (cached), above 9216 from iteration 3 on (regions read from HBM), without the test knob
CACHE = Shape(300, 9000, 0.005, 9, 1920, 13775, 6, "R crosses 9216 between iterations 2 and 3")
CACHE_REGIONS_RUN = (7080, 7080, 9778, 9818, 9820, 9825)   # binary mode, default options

# iterations of the tolerance = 1e-6 case: the wider tight set first changes a result at
# iteration 27 of 180x180x0.1 (tests/test_mw_edges.py pins that)
TOLERANCE_T = 30

ACCEPTED = ENVELOPE +[DEG_MAX_SHAPE] + SIZES + [CACHE]
ALL = ACCEPTED + [REFUSED]


def shape_id(s):
    return f"{s.A}x{s.I}x{s.sparsity:g}"


def generator_props(A, I, sparsity):
    """(maxdeg, impressions without a bid, bids) of the generated instance."""
    g = O.gen_adalloc(A, I, sparsity, 0.25)
    deg = np.bincount(g["imp"], minlength=I)
    return int(deg.max()), int((deg == 0).sum()), int(len(g["bid"]))


def envelope_path(maxdeg):
    """(kernel, sort size of the largest impression) as mw_iteration dispatches: the segment
    kernels sort SEG points, envelope_kernel the next power of two of n = deg + 1."""
    n = maxdeg + 1
    if n <= SEG16:
        return "seg16", SEG16
    if n <= SEG32:
        return "seg32", SEG32
    if n > DEG_MAX:
        return "refused", 0
    np2 = 1
    while np2 < n:
        np2 <<= 1
    return "wave", np2


def search_path(I):
    """(spec blocks, one launch for the whole search, rounds of the 1,024 lanes per level)."""
    nb = (I + BIN_BLOCK - 1) // BIN_BLOCK
    single = nb <= SINGLE_BLOCKS
    per_round = SEARCH_LANES // BIN_BLOCK
    return nb, single, (nb + per_round - 1) // per_round if single else 0


def report_blocks(A):
    return max(1, min(1024, (A + REPORT_BLOCK - 1) // REPORT_BLOCK))


@functools.lru_cache(maxsize=None)
def spec(A, I, sparsity, T, binary=False, scaling=0.25, epsilon=0.01, tolerance=1e-18, scale=None,
         intervals=3):
    """The fp64 spec's run (oracle/oracle_mw.cpp), computed once per argument set and shared;
    callers leave the arrays unchanged."""
    r = O.mw_run(A, I, sparsity, scaling, epsilon, T, tol=tolerance, binary=binary, scale=scale,
                 intervals=intervals)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def same_bits(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype)
    np.testing.assert_array_equal(got, want, err_msg=name)    # names the first differing entries
    assert got.tobytes() == want.tobytes(), f"{name}: equal values, different bits (signed zero)"


LOG_FIELDS = (("dual_value", "dual"), ("weighted_budget", "budget"), ("max_infeasibility", "infeas"),
              ("infeasible_advertiser", "infeas_idx"), ("min_weight", "wmin"), ("max_weight", "wmax"))


def assert_log_equals_spec(log, r, binary):
    for field, key in LOG_FIELDS:
        same_bits(field, log[field], r[key])
    if binary:
        same_bits("search_levels", log["search_levels"], r["levels"])
    else:
        assert (log["search_levels"] == 0).all()


def impression_major(problem):
    """Permutation from the problem's variable order (advertiser, impression) to the spec's
    (impression, advertiser) order."""
    adv, imp, _ = problem.adalloc_bids()
    return np.lexsort((adv, imp))


def assert_gpu_equals_spec(A, I, sparsity, T, binary=False, scaling=0.25, epsilon=0.01,
                           tolerance=1e-18, scale=None, intervals=3):
    """Run T iterations of the HIP MW path and of the spec under the same options; the
    per-iteration log (dual value, weighted budget, worst infeasibility and its advertiser,
    min / max weight; binary mode also the search levels), the weights and the averaged primal
    have the spec's bits.  Returns (log, x_avg, weights, spec run)."""
    import distributedlpsolver_amd as dlp
    p = dlp.Problem.adalloc(A, I, 1, sparsity, scaling)
    kw = dict(intervals=intervals, scale=scale) if binary else {}
    mw = dlp.MW(p, epsilon=epsilon, tolerance=tolerance, binary=binary, **kw)
    try:
        log, _ = mw.run(T)
        x, w = mw.solution()
    finally:
        mw.close()
    r = spec(A, I, sparsity, T, binary, scaling, epsilon, tolerance, scale, intervals)
    assert_log_equals_spec(log, r, binary)
    same_bits("weights", w, r["weights"])
    same_bits("x_avg", x[impression_major(p)], r["x_avg"])
    p.close()
    return log, x, w, r
