"""Register / scratch / LDS budget of the duration discriminator kernels (csrc/duration_disc.hip), read from the code
objects inside libwetts_hip.so with tools/kernel_resources.py (no GPU needed).

dur_disc_conv_kernel<LN, MODE, NT> is designed for TWO waves per SIMD wherever a wave holds at most three 32-channel
tiles (NT <= 3, filter_channels <= 192: what every recipe uses): a block is four waves (one per SIMD) and stages a
256-row x 48-k weight chunk (49 KB with the bank padding), a 48 x 64 input chunk (12 KB) and the LayerNorm's partial sums
(2 KB), 63 KB of the CU's 160 KB, so two blocks share a CU and a wave may hold 512 / 2 = 256 registers.  NT = 4
(filter_channels 224 and 256) holds eight accumulator tiles and is budgeted for one block per CU.  A spill would sit inside
the MFMA loop."""
import os
import re
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

LDS_PER_CU, REGS_PER_SIMD = 160 * 1024, 512


def _clean(row):
    return row.get("ScratchSize", 0) == 0 and row.get("VGPRSpill", 0) == 0 and row.get("SGPRSpill", 0) == 0


def test_conv_kernel_instantiations_fit_the_designed_occupancy():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    ks = [k for k in t if "wetts::dur_disc_conv_kernel" in k]
    assert len(ks) == 2 * 3 * 4, ks  # LN x MODE x NT
    seen = set()
    for k in ks:
        row = t[k]
        nt = int(re.search(r"<\s*(?:true|false)\s*,\s*\d+\s*,\s*(\d+)\s*>", k).group(1))
        seen.add(nt)
        waves = 2 if nt <= 3 else 1
        assert row.get("ScratchSize", 0) == 0 and row.get("VGPRSpill", 0) == 0, (k, row)
        assert row["VGPRs"] + row.get("AGPRs", 0) <= REGS_PER_SIMD // waves, (k, row)
        assert 0 < row["LDSSize"] <= LDS_PER_CU // 2, (k, row)
    assert seen == {1, 2, 3, 4}


def test_row_means_kernel_has_no_scratch():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    ks = [k for k in t if k.startswith("wetts::dur_disc_row_means_kernel")]
    assert len(ks) == 1, ks
    assert _clean(t[ks[0]]) and t[ks[0]]["VGPRs"] <= 96, (ks[0], t[ks[0]])
