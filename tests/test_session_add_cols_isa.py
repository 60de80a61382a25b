"""The two kernels of dlp_session_add_cols in the shipped code object (CPU test, no GPU needed).

Checked on the gfx950 code object bundled in libdlp.so: widen_copy_kernel and
col_fold_kernel are there; the column fold is a multiply and an add that is never contracted (a
tile of kColTile list entries x kColCT new columns of v_mul_f64 / v_add_f64 pairs, at least the
tile length of each, and not one v_fma_f64); the copy computes nothing in f64; neither kernel spills
to scratch.  The tile length and the group size the GPU tests put their edge cases on
(tests/add_cols_lp.py) are the source's."""
import os
import re

import pytest

import add_cols_lp as AC
from test_isa import ROOT, _disasm, _functions


@pytest.fixture(scope="module")
def kernels():
    out = {}
    for name, ins in _functions(_disasm()).items():
        m = re.match(r"_ZN3dlp12_GLOBAL__N_1\d+(widen_copy_kernel|col_fold_kernel)", name)
        if m:
            assert m.group(1) not in out, "one instantiation of each is shipped"
            out[m.group(1)] = ins
    return out


def _count(ins, op):
    return sum(1 for x in ins if x.split()[0].startswith(op))


def test_both_kernels_are_shipped(kernels):
    assert set(kernels) == {"widen_copy_kernel", "col_fold_kernel"}


def test_edge_case_constants_are_the_sources():
    src = open(os.path.join(ROOT, "distributedlpsolver_amd", "csrc", "dlp_addcols.hip")).read()
    assert int(re.search(r"constexpr int kColTile = (\d+);", src).group(1)) == AC.T
    assert int(re.search(r"constexpr int kColCT = (\d+);", src).group(1)) == AC.CT


def test_col_fold_is_a_multiply_and_an_add(kernels):
    fold = kernels["col_fold_kernel"]
    assert _count(fold, "v_fma_f64") == 0 and _count(fold, "v_fmac_f64") == 0
    assert _count(fold, "v_mul_f64") >= AC.T and _count(fold, "v_add_f64") >= AC.T
    # the copy computes nothing
    widen = kernels["widen_copy_kernel"]
    assert not [x for x in widen if re.match(r"v_\w+_f64", x)]


def test_neither_kernel_uses_scratch(kernels):
    for name, ins in kernels.items():
        assert not [x for x in ins if x.startswith("scratch_")], name
