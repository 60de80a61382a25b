"""The inputs of tests/test_gpu_general_defer.py, pinned on the CPU oracle.  These tests pin
INPUTS, not the product: they run no product code.  Each generated general LP
(general_lp.exact_general) must place the boundaries the GPU file is about — priced columns
nprice < N on or beside a 512-column tile, the carried Phase II objective row (local row m') on
or beside a 128-lane ratio workgroup — and must make a kernel that forgets either boundary
visibly wrong:

 - Phase I and Phase II both span full 64-pivot blocks and a partial one;
 - an artificial is still basic at the end (a redundant row), and equality-row duals have both
   signs, so whatever the sign convention some artificial column has a negative reduced cost at
   the optimum: a kernel that prices past nprice cannot stop there;
 - the LP minimises and c_q > 0 for the first entering column q: the carried row then holds a
   positive entry over RHS 0 in that column and would win the first ratio test with ratio 0 if it
   were eligible."""
import numpy as np
import pytest

import oracle_py as O
from general_lp import DEFER_INPUTS, defer_input, fixture_lp


@pytest.mark.parametrize("label", list(DEFER_INPUTS))
def test_defer_input_properties(label):
    m_std, nprice, _ = DEFER_INPUTS[label]
    cs = defer_input(label)
    lp = fixture_lp(cs)
    m_got, ncols, nprice_got, nart = O.general_std_dims(lp)
    assert (m_got, nprice_got) == (m_std, nprice)
    assert ncols == nprice + nart and nart > 0
    assert np.all(lp.col_lo == 0) and np.all(np.isinf(lp.col_hi))   # no bound rows: m' = m

    ref = O.solve_general(lp)
    assert ref.status == 0
    assert ref.phase1_pivots >= 2 * 64 + 1
    assert ref.num_pivots - ref.phase1_pivots >= 65
    assert int((ref.basis >= nprice).sum()) >= 1, "no artificial left basic"

    eq = lp.row_lo == lp.row_hi
    assert eq.sum() > max(np.isinf(lp.row_lo).sum(), np.isinf(lp.row_hi).sum()), "E is the largest share"
    assert (ref.y[eq] > 0).any() and (ref.y[eq] < 0).any(), "equality duals of one sign only"

    assert lp.sense == 1
    q = int(ref.pivot_log[0]["q"])
    assert q < lp.n and lp.c[q] > 0, (q, "the carried row would not win the first ratio test")

    # a degenerate artificial departure in Phase I (the zero-rhs equality rows)
    p1 = ref.pivot_log[:ref.phase1_pivots]
    assert ((p1["leaving"] >= nprice) & (p1["ratio"] == 0)).any()


def test_defer_inputs_differ_only_where_meant():
    """T- / T0 / T+ share m' and straddle the tile; R- / R+ share nprice and straddle the workgroup."""
    d = DEFER_INPUTS
    assert {d[k][0] for k in ("T0", "Tm", "Tp")} == {128}
    assert [d[k][1] for k in ("Tm", "T0", "Tp")] == [511, 512, 513]
    assert [d[k][0] for k in ("Rm", "Rp")] == [127, 129] and d["Rm"][1] == d["Rp"][1]
