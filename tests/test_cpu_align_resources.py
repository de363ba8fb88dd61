"""Register / scratch / LDS budget of the alignment kernels (csrc/align.hip), read from the code objects inside
libwetts_hip.so with tools/kernel_resources.py (no GPU needed).

align_scores_kernel is designed for FOUR waves per SIMD: a block is four waves (one per SIMD) and four blocks share a
CU, so a block may hold 160 KB / 4 = 40 KB of LDS and a wave 512 / 4 = 128 registers (VGPRs + AGPRs).  It stages two
16-channel operand chunks of 8 KB each plus the column-constant partials; a spill would sit inside the MFMA loop."""
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

DESIGNED_WAVES_PER_SIMD = 4
LDS_PER_CU, REGS_PER_SIMD = 160 * 1024, 512


def _clean(row):
    return row.get("ScratchSize", 0) == 0 and row.get("VGPRSpill", 0) == 0 and row.get("SGPRSpill", 0) == 0


def test_align_scores_kernel_fits_four_waves_per_simd():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    ks = [k for k in t if k.startswith("wetts::align_scores_kernel")]
    assert len(ks) == 1, ks
    row = t[ks[0]]
    assert _clean(row), row
    assert row["VGPRs"] + row.get("AGPRs", 0) <= REGS_PER_SIMD // DESIGNED_WAVES_PER_SIMD, row
    assert 0 < row["LDSSize"] <= LDS_PER_CU // DESIGNED_WAVES_PER_SIMD, row


def test_small_align_kernels_have_no_scratch_and_full_occupancy():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    for name in ("wetts::align_lengths_kernel", "wetts::path_to_durations_kernel", "wetts::counts_kernel"):
        ks = [k for k in t if k.startswith(name)]
        assert len(ks) == 1, (name, ks)
        assert _clean(t[ks[0]]) and t[ks[0]]["VGPRs"] <= 64, (ks[0], t[ks[0]])
