"""Register / scratch / LDS budget of the frontend scoring kernels (csrc/frontend_score.hip), read from the code objects
inside libwetts_hip.so with tools/kernel_resources.py (no GPU needed).

fe_score_tile_kernel is fe_linear_kernel's block (8 waves whose partial tiles meet in LDS) with a softmax epilogue that
reuses the partial tiles' LDS for the logits tile; like fe_linear it is meant for TWO blocks per CU: at most 512 / 4 = 128
registers per wave and at most 80 KB of the CU's 160 KB of LDS.  The per-token and the reduction kernel are small and must
not spill."""
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


def _clean(row):
    return row.get("ScratchSize", 0) == 0 and row.get("VGPRSpill", 0) == 0 and row.get("SGPRSpill", 0) == 0


def _one(t, name):
    ks = [k for k in t if k.startswith("wetts::" + name)]
    assert len(ks) == 1, (name, ks)
    return t[ks[0]]


def test_score_kernels_have_no_scratch_and_the_tile_kernel_fits_two_blocks_per_cu():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    assert len([k for k in t if "wetts::fe_score_" in k]) == 3
    tile = _one(t, "fe_score_tile_kernel")
    assert _clean(tile) and tile["VGPRs"] + tile.get("AGPRs", 0) <= 128 and 0 < tile["LDSSize"] <= 80 * 1024, tile
    for name, regs in (("fe_score_token_kernel", 64), ("fe_score_reduce_kernel", 128)):
        row = _one(t, name)
        assert _clean(row) and row["VGPRs"] + row.get("AGPRs", 0) <= regs, (name, row)


def test_the_serving_kernels_are_unchanged_in_number():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    assert len([k for k in t if "wetts::fe_linear_kernel" in k]) == 4
    for name in ("fe_heads_kernel", "fe_decide_kernel", "fe_embed_ln_kernel", "fe_add_ln_kernel", "fe_attention_kernel"):
        _one(t, name)
