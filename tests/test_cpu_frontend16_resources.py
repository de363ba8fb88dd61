"""Register / scratch / LDS budget of the 16-bit frontend kernels (csrc/frontend16.hip), read from the code objects inside
libwetts_hip.so with tools/kernel_resources.py (no GPU needed).

fe16_ksplit_kernel<F16, EPI> keeps fe_linear_kernel's design: 8 waves, 64 KB of LDS, TWO blocks per CU, so a wave may hold
128 registers (32 accumulators, a ring of 3 K steps of 20 registers each).  fe16_tile_kernel<F16, EPI, NT> is a block of 4
waves (one per SIMD) with 2 NT accumulator tiles per wave and (128 + 64 NT) x 64 bytes x 2 LDS buffers; two blocks per CU
need at most 256 registers a wave and 80 KB.  No kernel may use scratch: a spill would sit inside the MFMA loop."""
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


def _clean(row):
    return row.get("ScratchSize", 0) == 0 and row.get("VGPRSpill", 0) == 0 and row.get("SGPRSpill", 0) == 0


def test_every_instantiation_exists_without_scratch_and_fits_two_blocks_per_cu():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    ks = {k: v for k, v in t.items() if "wetts::fe16_" in k}
    split = [k for k in ks if "fe16_ksplit_kernel" in k]
    tile = [k for k in ks if "fe16_tile_kernel" in k]
    pack = [k for k in ks if "fe16_pack_kernel" in k]
    assert len(split) == 8 and len(tile) == 16 and len(pack) == 2, sorted(ks)  # 2 types x 4 epilogues (x 2 token tiles)
    for k, row in ks.items():
        assert _clean(row), (k, row)
    for k in split:
        row = ks[k]
        assert row["VGPRs"] + row.get("AGPRs", 0) <= 128 and row["LDSSize"] == 64 * 1024, (k, row)
    for k in tile:
        row = ks[k]
        nt = int(re.search(r",\s*(\d+)\s*>", k).group(1))
        assert nt in (1, 2) and row["LDSSize"] == 2 * (128 + 64 * nt) * 64, (k, row)
        assert row["VGPRs"] + row.get("AGPRs", 0) <= 256, (k, row)
        assert row.get("AGPRs", 0) + row["VGPRs"] >= 32 * nt  # the accumulator tiles are registers
