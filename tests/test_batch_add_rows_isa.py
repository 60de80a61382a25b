"""The growth source of the batch kernel in the shipped code object (CPU test, no GPU needed).

dlp_batch_add_rows runs batched_solve_kernel<AddIn>.  Checked on the gfx950 code
object bundled in libdlp.so: the instantiation is there; the register kernel has none of that
source; the row fold is not contracted (the new prologue adds v_mul_f64 / v_add_f64 pairs and
not one v_fma_f64 to what the dual instantiation of dlp_batch_resolve_rhs has: its pivot loop
is the same code); nothing spills to scratch."""
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


def test_growth_source_is_an_lds_kernel_instantiation_only(kernels):
    assert ("batched_solve_kernel", "AddIn", "") in kernels
    assert not [k for k in kernels if k[0] == "batched_reg_kernel" and k[1] == "AddIn"]
    assert [k for k in kernels if k[0] == "batched_reg_kernel" and k[1] == "RhsIn"]   # (the pattern sees them)


def test_row_fold_is_a_multiply_and_an_add(kernels):
    add = kernels[("batched_solve_kernel", "AddIn", "")]
    rhs = kernels[("batched_solve_kernel", "RhsIn", "")]
    assert _count(add, "v_fma_f64") == _count(rhs, "v_fma_f64") > 0
    # eight fold steps in flight behind their eight loads
    assert _count(add, "v_mul_f64") >= 8 and _count(add, "v_add_f64") >= 8
    assert not [x for x in add if x.startswith("scratch_")]
