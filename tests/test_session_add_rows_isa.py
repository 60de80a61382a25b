"""The two kernels of dlp_session_add_rows in the shipped code object (CPU test, no GPU needed).

Checked on the gfx950 code object bundled in libdlp.so: grow_copy_kernel and
row_fold_kernel are there; the row fold is a multiply and a subtract that is never contracted (a
batch of kFoldRows old rows x kFoldRT new rows of v_mul_f64 / v_add_f64 pairs, at least the batch
length of each, and not one v_fma_f64); neither kernel spills to scratch.  The batch length and the
group size the GPU tests put their edge cases on (tests/add_rows_lp.py) are the source's."""
import os
import re

import pytest

import add_rows_lp as AL
from test_isa import ROOT, _disasm, _functions


@pytest.fixture(scope="module")
def kernels():
    out = {}
    for name, ins in _functions(_disasm()).items():
        m = re.match(r"_ZN3dlp12_GLOBAL__N_1\d+(grow_copy_kernel|row_fold_kernel)", name)
        if m:
            assert m.group(1) not in out, "one instantiation of each is shipped"
            out[m.group(1)] = ins
    return out


def _count(ins, op):
    return sum(1 for x in ins if x.split()[0].startswith(op))


def test_both_kernels_are_shipped(kernels):
    assert set(kernels) == {"grow_copy_kernel", "row_fold_kernel"}


def test_edge_case_constants_are_the_sources():
    src = open(os.path.join(ROOT, "distributedlpsolver_amd", "csrc", "dlp_addrows.hip")).read()
    assert int(re.search(r"constexpr int kFoldRows = (\d+);", src).group(1)) == AL.B
    assert int(re.search(r"constexpr int kFoldRT = (\d+);", src).group(1)) == AL.RT


def test_row_fold_is_a_multiply_and_a_subtract(kernels):
    fold = kernels["row_fold_kernel"]
    assert _count(fold, "v_fma_f64") == 0 and _count(fold, "v_fmac_f64") == 0
    assert _count(fold, "v_mul_f64") >= AL.B and _count(fold, "v_add_f64") >= AL.B
    # the copy computes nothing
    grow = kernels["grow_copy_kernel"]
    assert not [x for x in grow if re.match(r"v_(fma|fmac|mul|add)_f64", x)]


def test_neither_kernel_uses_scratch(kernels):
    for name, ins in kernels.items():
        assert not [x for x in ins if x.startswith("scratch_")], name
