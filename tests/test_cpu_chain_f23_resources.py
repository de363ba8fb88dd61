"""Register / scratch budget of resblock_chain_f23_kernel (wetts_amd/csrc/resblock_chain_f23.hip), read from the code objects
inside libwetts_hip.so (no GPU needed).  The kernel is built for three waves per SIMD (three blocks of four waves per CU,
as the F(2,3) single convs): at most 168 unified registers, no scratch, no spills.  k = 7 is the tight one (64
accumulators, a four-set A ring of 48, the residual pair behind c1)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402
from wetts_amd import _lib  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(kernel_resources.READELF) or shutil.which("c++filt") is None or
                                not os.path.exists(_lib.LIB_PATH),
                                reason="needs llvm-readelf, c++filt and a built wetts_amd/lib/libwetts_hip.so "
                                       "(the library is git-ignored: run __graft_entry__.build() first)")

# measured with this hipcc; another compiler may allocate differently without anything being wrong in the sources
# (tests/test_cpu_kernel_resources.py: the same rule)
BUDGETS_MEASURED_WITH = "HIP version: 7.2"
INSTANCES = ("resblock_chain_f23_kernel<32, 7>", "resblock_chain_f23_kernel<32, 11>")


@pytest.fixture(autouse=True)
def _other_compiler_is_xfail(request):
    try:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        out = ""
    if BUDGETS_MEASURED_WITH not in out:
        request.node.add_marker(pytest.mark.xfail(reason="register budgets were measured with " + BUDGETS_MEASURED_WITH,
                                                  strict=False))


@pytest.fixture(scope="module")
def table():
    return kernel_resources.library_table(_lib.LIB_PATH)


@pytest.mark.parametrize("inst", INSTANCES)
def test_chain_f23_kernels_keep_three_waves_per_simd(table, inst):
    rows = {k: v for k, v in table.items() if inst in k}
    assert len(rows) == 1, (inst, sorted(k for k in table if "chain_f23" in k))
    (name, v), = rows.items()
    print(name, v)
    assert v["VGPRs"] <= 168, (name, v)  # (vgpr_count of the metadata = VGPRs + AGPRs, the unified file)
    assert v.get("ScratchSize", 0) == 0 and v.get("VGPRSpill", 0) == 0 and v.get("SGPRSpill", 0) == 0, (name, v)
