"""Register / scratch budget of the duration-loss kernels (csrc/duration_loss.hip), read from the code objects inside
libwetts_hip.so with tools/kernel_resources.py (no GPU needed).

Every one of them is a one-thread-per-position or one-block-per-utterance kernel with no reason to give up occupancy:
at most 64 VGPRs (eight waves per SIMD), no scratch, no spills.  spline_forward_kernel in particular must not hold its
knot tables in a run-time-indexed array, which is what costs spline_inverse_kernel its scratch (80 bytes per lane with
this compiler, under the 128 tests/test_cpu_kernel_resources.py allows that one kernel)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402
from wetts_amd import _lib  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(kernel_resources.READELF) or shutil.which("c++filt") is None or
                                not os.path.exists(_lib.LIB_PATH),
                                reason="needs llvm-readelf, c++filt and a built wetts_amd/lib/libwetts_hip.so")

KERNELS = ("wetts::spline_forward_kernel", "wetts::affine_forward_kernel", "wetts::dequant_log_kernel",
           "wetts::duration_pre_kernel", "wetts::duration_add_kernel", "wetts::duration_unswap_kernel",
           "wetts::duration_reduce_kernel", "wetts::dp_mse_kernel", "wetts::logw_target_kernel",
           "wetts::duration_total_kernel")


def _clean(row):
    return row.get("ScratchSize", 0) == 0 and row.get("VGPRSpill", 0) == 0 and row.get("SGPRSpill", 0) == 0


@pytest.mark.parametrize("name", KERNELS)
def test_duration_kernel_exists_once_without_scratch_at_full_occupancy(name):
    t = kernel_resources.library_table(_lib.LIB_PATH)
    ks = [k for k in t if k == name or k.startswith("void " + name + "<")]
    assert len(ks) == 1, (name, ks)
    row = t[ks[0]]
    print(ks[0], row)
    assert _clean(row), (ks[0], row)
    assert row["VGPRs"] + row.get("AGPRs", 0) <= 64, (ks[0], row)
