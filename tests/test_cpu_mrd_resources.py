"""Register / scratch / LDS budget of the MPMRD kernels (csrc/mrd.hip and the complex STFT of csrc/stft.hip), read from the
code objects inside libwetts_hip.so with tools/kernel_resources.py (no GPU needed).

mrd_band_conv_mfma_kernel is designed for TWO waves per SIMD (its header comment): a block is four waves, one per SIMD,
and stages a chunk's A fragments and its 128 columns of taps -- 33.75 KB for the (3, 9) convs, 45 KB for the (3, 3)
conv -- so at least two blocks share a CU's 160 KB, and a wave may hold 512 / 2 = 256 registers: the running sum and the
chunk's own accumulator (32), the prefetched taps and fragments of the next chunk (up to 36 + 9) and their addresses.
A spill would sit inside the MFMA loop."""
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


def test_band_conv_kernel_fits_two_waves_per_simd():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    ks = [k for k in t if "wetts::mrd_band_conv_mfma_kernel" in k]
    assert len(ks) == 3, ks  # (9, 1) on two channels, (9, 2) and (3, 1) on 32
    for k in ks:
        row = t[k]
        assert _clean(row), (k, row)
        assert row["VGPRs"] + row.get("AGPRs", 0) <= REGS_PER_SIMD // DESIGNED_WAVES_PER_SIMD, (k, row)
        assert 0 < row["LDSSize"] <= LDS_PER_CU // DESIGNED_WAVES_PER_SIMD, (k, row)


def test_small_mrd_kernels_have_no_scratch():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    for name in ("wetts::mrd_normalize_kernel", "wetts::mrd_conv_post_kernel", "wetts::mrd_pack_kernel"):
        ks = [k for k in t if k.startswith(name)]
        assert len(ks) == 1, (name, ks)
        assert _clean(t[ks[0]]) and t[ks[0]]["VGPRs"] <= 64, (ks[0], t[ks[0]])
    ks = [k for k in t if "wetts::stft_cplx_kernel<" in k]
    assert len(ks) == 2, ks
    mag = sorted(k for k in t if "wetts::stft_mag_kernel<" in k)
    for k, m in zip(sorted(ks), mag):
        assert _clean(t[k]), (k, t[k])
        # one body: the complex form holds the registers of the magnitude form, give or take its epilogue
        assert abs(t[k]["VGPRs"] - t[m]["VGPRs"]) <= 16, (k, t[k], t[m])
