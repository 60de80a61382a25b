"""The column source of the batch kernel in the shipped code object (CPU test, no GPU needed).

dlp_batch_add_cols runs batched_solve_kernel<ColsIn>.  Checked on the gfx950 code
object bundled in libdlp.so: the instantiation is there; the register kernel has none of that
source; the column fold is not contracted (the new prologue adds rounded products and sums and
not one v_fma_f64 to what the primal instantiation of dlp_batch_resolve has: its pivot loop is
the same code); nothing spills to scratch."""
import re

import pytest

from test_isa import _disasm, _functions


@pytest.fixture(scope="module")
def kernels():
    out = {}
    for name, ins in _functions(_disasm()).items():
        m = re.match(r"_ZN3dlp12_GLOBAL__N_1\d+(batched_solve_kernel|batched_reg_kernel)I(.*?)NS0_\d+([A-Za-z]+In)EEE", name)
        if m:
            out[(m.group(1), m.group(3), m.group(2))] = ins
    assert out
    return out


def _count(ins, op):
    return sum(1 for x in ins if x.split()[0].startswith(op))


def test_column_source_is_an_lds_kernel_instantiation_only(kernels):
    assert ("batched_solve_kernel", "ColsIn", "") in kernels
    assert not [k for k in kernels if k[0] == "batched_reg_kernel" and k[1] == "ColsIn"]
    assert [k for k in kernels if k[0] == "batched_reg_kernel" and k[1] == "ResIn"]   # (the pattern sees them)


def test_column_fold_adds_no_fma_and_no_scratch(kernels):
    cols = kernels[("batched_solve_kernel", "ColsIn", "")]
    res = kernels[("batched_solve_kernel", "ResIn", "")]
    assert _count(cols, "v_fma_f64") == _count(res, "v_fma_f64") > 0
    assert not [x for x in cols if x.startswith("scratch_")]
