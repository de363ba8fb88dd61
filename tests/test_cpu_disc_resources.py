"""Register / scratch / LDS budget of the discriminator kernels (csrc/discriminator.hip), read from the code objects
inside libwetts_hip.so with tools/kernel_resources.py (no GPU needed).

strided_conv_mfma_kernel is designed for TWO waves per SIMD: a block is four waves (one per SIMD) and stages a
128-channel x 80-k weight chunk (41.5 KB with the bank padding) plus an 80 x 64 input chunk (20 KB), 62 KB of the CU's
160 KB, so two blocks share a CU and a wave may hold 512 / 2 = 256 registers (VGPRs + AGPRs): four 32 x 32 accumulators
(the running sum and the chunk's own), the 60 prefetched values of the next chunk and their addresses.  A spill would
sit inside the MFMA loop."""
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

DESIGNED_WAVES_PER_SIMD = 2
LDS_PER_CU, REGS_PER_SIMD = 160 * 1024, 512


def _clean(row):
    return row.get("ScratchSize", 0) == 0 and row.get("VGPRSpill", 0) == 0 and row.get("SGPRSpill", 0) == 0


def test_strided_conv_mfma_kernel_fits_two_waves_per_simd():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    ks = [k for k in t if "wetts::strided_conv_mfma_kernel" in k]
    assert len(ks) == 2, ks  # stride 3 and stride 1
    for k in ks:
        row = t[k]
        assert _clean(row), (k, row)
        assert row["VGPRs"] + row.get("AGPRs", 0) <= REGS_PER_SIMD // DESIGNED_WAVES_PER_SIMD, (k, row)
        assert 0 < row["LDSSize"] <= LDS_PER_CU // DESIGNED_WAVES_PER_SIMD, (k, row)


def test_small_discriminator_kernels_have_no_scratch():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    for name in ("wetts::period_fold_conv0_kernel", "wetts::conv_post_kernel", "wetts::grouped_conv1d_kernel",
                 "wetts::disc_rows_kernel", "wetts::disc_totals_kernel"):
        ks = [k for k in t if k.startswith(name)]
        assert len(ks) == 1, (name, ks)
        assert _clean(t[ks[0]]) and t[ks[0]]["VGPRs"] <= 64, (ks[0], t[ks[0]])
