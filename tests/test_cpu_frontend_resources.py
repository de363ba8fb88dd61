"""Register / scratch / LDS budget of the text frontend kernels (csrc/frontend.hip), read from the code objects inside
libwetts_hip.so with tools/kernel_resources.py (no GPU needed).

fe_linear_kernel<EPI> is a block of 8 waves (two per SIMD) whose 8 partial tiles meet in 64 KB of LDS; it is designed
for TWO blocks per CU (128 of the CU's 160 KB, four waves per SIMD), so a wave may hold 512 / 4 = 128 registers: 32 of
them are the two accumulator tiles, 48 the ring of four K steps in flight.  A spill would sit inside the MFMA loop.
fe_attention_kernel keeps a 64-key chunk, the queries and the scores of its 16 queries in under 64 KB (two blocks per
CU).  fe_heads_kernel is one block of 16 waves (four per SIMD: at most 128 registers) with four weight rows in flight
per wave.  The row kernels (embeddings + LayerNorm, residual + LayerNorm, the decisions) hold a token's row in registers
and must not spill either."""
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


def test_linear_kernel_instantiations_fit_two_blocks_per_cu():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    ks = [k for k in t if "wetts::fe_linear_kernel" in k]
    assert len(ks) == 4, ks  # bias, GELU, ReLU, residual
    assert {int(re.search(r"<\s*(\d+)\s*>", k).group(1)) for k in ks} == {0, 1, 2, 3}
    for k in ks:
        row = t[k]
        assert _clean(row), (k, row)
        assert row["VGPRs"] + row.get("AGPRs", 0) <= REGS_PER_SIMD // 4, (k, row)
        assert 0 < row["LDSSize"] <= LDS_PER_CU // 2, (k, row)


def test_attention_kernel_fits_two_blocks_per_cu():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    ks = [k for k in t if k.startswith("wetts::fe_attention_kernel")]
    assert len(ks) == 1, ks
    row = t[ks[0]]
    assert _clean(row) and row["VGPRs"] + row.get("AGPRs", 0) <= 128 and 0 < row["LDSSize"] <= 64 * 1024, row


def test_row_kernels_have_no_scratch():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    for name, regs in (("fe_embed_ln_kernel", 64), ("fe_add_ln_kernel", 64), ("fe_heads_kernel", 128), ("fe_decide_kernel", 32)):
        ks = [k for k in t if k.startswith("wetts::" + name)]
        assert len(ks) == 1, (name, ks)
        assert _clean(t[ks[0]]) and t[ks[0]]["VGPRs"] <= regs, (ks[0], t[ks[0]])
