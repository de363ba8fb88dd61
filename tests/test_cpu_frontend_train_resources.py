"""Register / scratch / LDS budget of the training kernels (csrc/frontend_train.hip), read from the code objects inside
libwetts_hip.so with tools/kernel_resources.py (no GPU needed).

fe_bgemm_kernel<A_ICONTIG> (dgrad and wgrad) is a block of 4 waves with one 32 x 32 output tile per wave held as three
levels of partial sums (48 accumulator registers) and two 16 x 66-float operand tiles in LDS (stride 66: no bank conflict
in the transposed write): 8448 bytes and at most 128 registers a wave (the staging addresses of the k-contiguous operand
take the most), so four blocks fit a CU by registers (4 x 128 = 512) and by LDS.
fe_attn_bwd_q_kernel holds 8 scores and 8 dP per lane (T <= 512) and 11 KB of wave-private LDS; at most 96 registers.
The row kernels (LayerNorm backward: two float4 rows of up to 1024 channels) stay within 64.  No kernel may use scratch."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402
from wetts_amd import _lib  # noqa: E402
from wetts_amd import frontend_train  # noqa: E402,F401  (the module whose kernels these are)

pytestmark = pytest.mark.skipif(not os.path.exists(kernel_resources.READELF) or shutil.which("c++filt") is None or
                                not os.path.exists(_lib.LIB_PATH),
                                reason="needs llvm-readelf, c++filt and a built wetts_amd/lib/libwetts_hip.so")

KERNELS = {  # name -> (instantiations, most registers, LDS bytes)
    "fe_ce_bwd_kernel": (1, 64, 0), "fe_bgemm_kernel": (2, 128, 2 * 16 * 66 * 4), "fe_split_sum_kernel": (1, 32, 0),
    "fe_colsum_part_kernel": (1, 32, 4 * 64 * 4), "fe_colsum_final_kernel": (1, 32, 0), "fe_ln_bwd_kernel": (1, 64, 0),
    "fe_attn_bwd_q_kernel": (1, 96, (2 * 4 * 96 + 4 * 512) * 4), "fe_attn_bwd_kv_kernel": (1, 64, 0),
    "fe_adamw_kernel": (1, 64, 0),
}


def _clean(row):
    return row.get("ScratchSize", 0) == 0 and row.get("VGPRSpill", 0) == 0 and row.get("SGPRSpill", 0) == 0


def test_every_training_kernel_exists_without_scratch_and_within_its_budget():
    t = kernel_resources.library_table(_lib.LIB_PATH)
    for name, (count, regs, lds) in KERNELS.items():
        ks = {k: v for k, v in t.items() if "wetts::" + name in k}
        assert len(ks) == count, (name, sorted(ks))
        for k, row in ks.items():
            assert _clean(row), (k, row)
            assert row["VGPRs"] + row.get("AGPRs", 0) <= regs and row["LDSSize"] == lds, (k, row)
    bg = [v for k, v in t.items() if "wetts::fe_bgemm_kernel" in k]
    assert all(r["VGPRs"] + r.get("AGPRs", 0) >= 48 for r in bg)  # the three accumulator tiles are registers
