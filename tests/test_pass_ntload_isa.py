"""The nt instances of the form-23 pass in the shipped code object (CPU test, no GPU needed).

tests/test_gpu_pass_ntload.py compares the pass with DLP_PASS_NTLOAD on and off against the eager
session; that says something about the nt DMAs only if an nt instance exists for every combination its
cases name, since the launcher falls back to the default-policy instance where none was compiled.
Checked here on the gfx950 code object bundled in libdlp.so: for a nontemporal session and each
(rows per group U, ring depth D, scalar-base DMAs SA, shared coefficient ring CS) of those cases, the
instance with NL = 1 is there, publishing and not; it carries nt on its tableau DMAs and on no
coefficient DMA (half of its global_load_lds_dwordx4 each); and its default-policy twin carries none."""
import re

import pytest

from test_isa import _disasm, _functions

# (U, D, SA, CS) of the cases of tests/test_gpu_pass_ntload.py: DLP_Q_U = 2 (D = 4, no shared ring by
# default) and 4 (D = 2, shared ring), DLP_PASS_SADDR = 0 with both, DLP_PASS_CSHARE = 0 with U = 4
CASES = [(2, 4, 1, 0), (4, 2, 1, 1), (2, 4, 0, 0), (4, 2, 0, 0), (4, 2, 1, 0)]


@pytest.fixture(scope="module")
def instances():
    """{(NT, U, D, SA, CS, NL, PUB): instruction lines} of every pass_q_kernel instance."""
    out = {}
    for name, ins in _functions(_disasm()).items():
        m = re.match(r"_ZN3dlp12_GLOBAL__N_113pass_q_kernelILb(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)EE", name)
        if m:
            out[tuple(int(x) for x in m.groups())] = ins
    assert out
    return out


def _dmas(ins):
    return [x for x in ins if x.startswith("global_load_lds_dwordx4")]


@pytest.mark.parametrize("U,D,SA,CS", CASES)
@pytest.mark.parametrize("PUB", [0, 1])
def test_nt_instance_exists_and_marks_the_tableau_dmas_only(instances, U, D, SA, CS, PUB):
    nl = instances.get((1, U, D, SA, CS, 1, PUB))
    assert nl is not None, "no nt instance: the launcher would run the default-policy one"
    dm = _dmas(nl)
    nt = [x for x in dm if re.search(r"\bnt\b", x)]
    assert dm and 2 * len(nt) == len(dm), (len(nt), len(dm))
    twin = instances[(1, U, D, SA, CS, 0, PUB)]
    assert len(_dmas(twin)) == len(dm) and not any(re.search(r"\bnt\b", x) for x in _dmas(twin))


def test_no_nt_instance_without_a_nontemporal_session(instances):
    assert not any(k[0] == 0 and k[5] == 1 for k in instances)
    assert not any(re.search(r"\bnt\b", x) for k, v in instances.items() if k[5] == 0 for x in _dmas(v))
