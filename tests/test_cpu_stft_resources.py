"""Register / scratch budget of the spectrogram kernels (csrc/stft.hip), read from the code objects inside
libwetts_hip.so with tools/kernel_resources.py (no GPU needed).  stft_mag_kernel runs two blocks of four waves per CU
(its LDS strip is up to 72 KB), so it has room for 256 registers; it needs far fewer, and a spill would sit inside the
MFMA loop."""
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


def test_stft_kernels_fit_their_budget():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    mag = {k: v for k, v in t.items() if "stft_mag_kernel<" in k}
    assert len(mag) == 2, sorted(k for k in t if "stft" in k)
    for k, v in mag.items():
        assert v["VGPRs"] <= 128 and v.get("ScratchSize", 0) == 0, (k, v)
    for name in ("wetts::stft_basis_kernel", "wetts::mel_log_kernel"):
        ks = [k for k in t if k.startswith(name)]
        assert len(ks) == 1, (name, ks)
        assert t[ks[0]]["VGPRs"] <= 64 and t[ks[0]].get("ScratchSize", 0) == 0, (ks[0], t[ks[0]])
