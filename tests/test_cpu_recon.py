"""CPU tier of teacher-forced reconstruction: the float64 oracle of tests/recon_oracle.py pinned to the reference's
fixtures (tests/golden/recon_*.npz, made by make_golden_recon.py), argument validation of reconstruct() that needs no
device, header / binding agreement of the new entries and the new status bit, and the resource budget of the new
kernels (csrc/losses.hip)."""
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import align_oracle as ao, recon_oracle as ro
from wetts_amd import SynthesizerTrn, _lib, commons, config, losses, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SPEC = ao.SPEC
ENTRIES = ("wetts_rand", "wetts_slice_ids", "wetts_slice_segments", "wetts_kl_loss", "wetts_l1_loss")


# ---- the oracle against the reference's fixtures ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ro.RECON_CASES)
def test_float64_oracle_reproduces_the_fixture(name):
    """ids_slice from u and the lengths exactly (one row at id 0, one at len - segment), slice_segments equal to the
    stored slices exactly, loss_kl from the alignment fixture's stage tensors to 1e-6 relative."""
    c = ro.load_recon_case(name)
    seg = int(c["segment"])
    assert seg == ro.segment_of(name) and os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20
    yl = c["y_lengths"]
    ids, short = ro.slice_ids(c["u"], yl, seg)
    assert not short.any() and np.array_equal(ids, c["ids_slice"]) and c["ids_slice"].dtype == np.int64
    assert c["ids_slice"][0] == 0 and c["ids_slice"][1] == yl[1] - seg
    assert ((c["ids_slice"] >= 0) & (c["ids_slice"] <= yl - seg)).all()
    hop = c["o"].shape[-1] // seg
    assert c["o"].shape == (len(yl), 1, seg * hop)
    if "sub_stride" in c:  # full-size case: the alignment fixture holds every stride-th frame
        st = int(c["sub_stride"])
        mask = c["y_mask"][:, ::st]
        kl = ro.kl_loss(c["z_p_sub"], c["logs_q_sub"], c["m_p_sub"], c["logs_p_sub"], mask)
        ref = float(c["loss_kl_sub"])
        for b, i in enumerate(c["ids_slice"]):  # the stored slice at the frames the sub-sampled z holds
            for j in range(seg):
                if (int(i) + j) % st == 0:
                    assert np.array_equal(c["z_slice"][b, :, j], c["z_sub"][b, :, (int(i) + j) // st])
    else:
        kl = ro.kl_loss(c["z_p"], c["logs_q"], c["m_p"], c["logs_p"], c["y_mask"])
        ref = float(c["loss_kl"])
        assert abs(kl["abs_total"] - float(c["kl_abs_mean"])) <= 1e-9 * kl["abs_total"]
        assert np.array_equal(ro.slice_segments(c["z"], c["ids_slice"], seg), c["z_slice"])
    print(name, "loss_kl float64 oracle", kl["total"], "reference", ref, "rel", abs(kl["total"] - ref) / abs(ref))
    assert abs(kl["total"] - ref) <= 1e-6 * abs(ref)
    if name in ro.MEL_CASES:
        l1 = ro.l1_loss(c["y_mel"], c["y_hat_mel"])
        assert abs(l1["total"] - float(c["loss_mel"])) <= 1e-6 * l1["total"]
        assert c["y_mel"].shape == c["y_hat_mel"].shape == (len(yl), ro.MEL["n_mel_channels"], seg)
        rel = abs(float(c["loss_mel_shift1"]) - float(c["loss_mel"])) / float(c["loss_mel"])
        print(name, "loss_mel", float(c["loss_mel"]), "shifted by one frame", float(c["loss_mel_shift1"]), "rel", rel)
        assert rel >= 10 * ro.MEL_GATE  # the gate can see an off-by-one slice


def test_slice_ids_oracle_at_the_ends_of_u_and_at_large_lengths():
    """u = 1 - 2^-24, the largest value torch.rand's 24-bit mapping gives, at small and at large lengths -- up to where
    float32 no longer holds len - segment + 1 exactly: the id is in range and equals the truncated float32 product.
    (With a 24-bit u the product stays below len - segment + 1 at every length tried here, so the clamp does not act;
    it acts for u = 1.0, which only an injected draw can hold.)"""
    u = np.array([1.0 - 2.0 ** -24], np.float32)
    for n in (1, 2, 17, 593, 4096, 2 ** 23 + 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 26 + 5, 2 ** 30 + 77):
        ids, short = ro.slice_ids(u, np.array([n - 1 + 8]), 8)  # len - segment + 1 = n
        raw = int(np.float32(u[0]) * np.float32(n))
        assert not short[0] and 0 <= ids[0] <= n - 1 and ids[0] == min(raw, n - 1), (n, ids, raw)
        if n <= 2 ** 24:
            assert ids[0] == n - 1  # the last valid start is reached
        assert ro.slice_ids(np.zeros(1, np.float32), np.array([n - 1 + 8]), 8)[0][0] == 0
        assert ro.slice_ids(np.ones(1, np.float32), np.array([n - 1 + 8]), 8)[0][0] == n - 1  # clamped
    assert int(np.float32(1.0) * np.float32(593)) == 593  # what the reference computes from u = 1.0: out of range
    ids, short = ro.slice_ids(np.array([0.5, 0.5], np.float32), np.array([7, 8]), 8)
    assert ids.tolist() == [0, 0] and short.tolist() == [True, False]
    assert ro.shifted_ids(np.array([0, 3, 5]), np.array([13, 13, 13]), 8).tolist() == [1, 4, 4]


def test_oracle_reductions_against_plain_numpy():
    rs = np.random.RandomState(3)
    a, b = rs.randn(3, 5, 7), rs.randn(3, 5, 7)
    assert np.isclose(ro.l1_loss(a, b)["total"], np.abs(a - b).mean())
    mask = (np.arange(7)[None] < np.array([7, 4, 1])[:, None]).astype(np.float32)
    zp, lq, mp, lp = (rs.randn(3, 5, 7) for _ in range(4))
    want = ((lp - lq - 0.5 + 0.5 * (zp - mp) ** 2 * np.exp(-2 * lp)) * mask[:, None]).sum() / mask.sum()
    got = ro.kl_loss(zp, lq, mp, lp, mask)
    assert np.isclose(got["total"], want) and np.isclose((got["per_utt"] * mask.sum(-1)).sum() / mask.sum(), want)


# ---- argument validation before any device work ----------------------------------------------------------------------
def _net(n_spk=3):
    cfg = config.make_config(dict(config.MODEL_CONFIGS["tiny"]), 40, n_spk)
    sd = dict(synth.make_state_dict(cfg, 1), **synth.make_posterior_state_dict(cfg, SPEC, 2))
    return SynthesizerTrn(40, SPEC, 8, n_speakers=n_spk, **config.MODEL_CONFIGS["tiny"]).load_state_dict(sd)


def test_reconstruct_argument_validation_needs_no_device():
    net = _net()
    x, xl = torch.zeros(2, 5, dtype=torch.long), torch.tensor([5, 3])
    y, yl = torch.zeros(2, SPEC, 9), torch.tensor([9, 8])
    sid = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="x must be"):
        net.reconstruct(x[0], xl, y, yl, sid)
    with pytest.raises(ValueError, match="y must be"):
        net.reconstruct(x, xl, y[:, :80], yl, sid)
    with pytest.raises(ValueError, match="x_lengths must be"):
        net.reconstruct(x, xl[:1], y, yl, sid)
    with pytest.raises(ValueError, match="y_lengths must be"):
        net.reconstruct(x, xl, y, torch.tensor([[9, 8]]), sid)
    with pytest.raises(ValueError, match="sid is required"):
        net.reconstruct(x, xl, y, yl)
    with pytest.raises(ValueError, match="eps_q must be"):
        net.reconstruct(x, xl, y, yl, sid, eps_q=torch.zeros(2, 192, 8))
    with pytest.raises(ValueError, match="segment_size must be"):
        net.reconstruct(x, xl, y, yl, sid, segment_size=10)  # > Ty = 9
    with pytest.raises(ValueError, match="segment_size must be"):
        net.reconstruct(x, xl, y, yl, sid, segment_size=0)
    with pytest.raises(ValueError, match="segment_size must be"):
        net.reconstruct(x, xl, y[:, :, :7], yl, sid)  # the constructor's 8 > Ty = 7
    for bad in (torch.zeros(3, dtype=torch.long), torch.zeros(2, 1, dtype=torch.long), torch.tensor(0)):
        with pytest.raises(ValueError, match="ids_slice must be"):
            net.reconstruct(x, xl, y, yl, sid, ids_slice=bad)
    for kw in ({}, dict(segment_size=4), dict(ids_slice=torch.tensor([0, 1])), dict(eps_q=torch.zeros(2, 192, 9))):
        with pytest.raises(_lib.WettsError):  # valid arguments: the product path has no CPU fallback
            net.reconstruct(x, xl, y, yl, sid, **kw)


def test_forward_still_raises_and_the_helpers_refuse_host_tensors():
    with pytest.raises(NotImplementedError):
        _net().forward()
    with pytest.raises(ValueError, match="HIP device"):
        commons.slice_segments(torch.zeros(2, 3, 8), torch.zeros(2, dtype=torch.long), 4)
    with pytest.raises(ValueError, match="HIP device"):
        commons.rand_slice_segments(torch.zeros(2, 3, 8))
    with pytest.raises(ValueError, match="HIP device"):
        losses.l1_loss(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(ValueError, match="equally shaped"):
        losses.l1_loss(torch.zeros(2, 3), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="HIP device"):
        losses.kl_loss(*(torch.zeros(2, 3, 4) for _ in range(4)), torch.ones(2, 1, 4))

    class _H(dict):
        __getattr__ = dict.__getitem__

    net = _net()
    hps = _H(data=_H(hop_length=net.hop_length + 1), model=_H(), train=_H(c_mel=45, c_kl=1.0))
    with pytest.raises(ValueError, match="hop_length"):
        losses.teacher_forced_losses(net, hps, None, None, None, None)


# ---- header / binding agreement ---------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_new_entries():
    src = open(os.path.join(ROOT, "include", "wetts_hip.h")).read()
    assert int(re.search(r"#define WETTS_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 12  # additive only
    lib = _lib.load()
    kinds = {"int32_t": _lib._I32, "int64_t": _lib._I64, "uint64_t": _lib.C.c_uint64, "float": _lib._F}
    for name in ENTRIES:
        m = re.search(r"int32_t " + name + r"\(([^;]*)\);", src)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib._I32 and len(argtypes) == len(args), (name, args)
        for a, t in zip(args, argtypes):  # pointers bind as void*, scalars by their C type
            assert t is (_lib._P if "*" in a else kinds[a.split()[0]]), (name, a, t)
        assert hasattr(lib, name)
    assert int(re.search(r"#define WETTS_STATUS_SEGMENT_LONGER (\d+)", src).group(1)) == _lib.STATUS_SEGMENT_LONGER == 64
    bits = [_lib.STATUS_SPLINE_DOMAIN, _lib.STATUS_PHONE_ID_RANGE, _lib.STATUS_SPEAKER_ID_RANGE,
            _lib.STATUS_DURATION_NONFINITE, _lib.STATUS_ALIGN_TEXT_LONGER, _lib.STATUS_DURATION_NEGATIVE,
            _lib.STATUS_SEGMENT_LONGER]
    assert sorted(bits) == [1, 2, 4, 8, 16, 32, 64]


def test_null_and_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.wetts_slice_ids(None, None, None, 1, 8, 4, None, None, None) == -1
    assert lib.wetts_slice_segments(None, 0, 0, None, 1, 1, 8, 4, 1, None, None) == -1
    assert lib.wetts_kl_loss(None, None, None, None, None, 1, 1, 1, 1.0, None, None, None, None) == -1
    assert lib.wetts_l1_loss(None, None, 1, 1, 1.0, None, None, None, None) == -1
    assert lib.wetts_rand(None, 4, 0, 0, None) == -1
    one = _lib.C.c_void_p(16)  # never dereferenced: the shape checks come first
    assert lib.wetts_slice_segments(one, 8, 8, one, 1, 1, 8, 3, 3, one, None) == -1  # segment * scale > T
    assert b"exceeds" in lib.wetts_last_error()
    assert lib.wetts_slice_segments(one, 8, 8, one, 1, 0, 8, 4, 1, one, None) == -1  # C = 0
    assert lib.wetts_slice_ids(one, None, None, 1, 8, 0, one, None, None) == -1  # segment = 0


# ---- kernel resources -------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(kernel_resources.READELF) or shutil.which("c++filt") is None or
                    not os.path.exists(_lib.LIB_PATH),
                    reason="needs llvm-readelf, c++filt and a built wetts_amd/lib/libwetts_hip.so")
def test_new_kernels_have_no_scratch_and_full_occupancy():
    """The reconstruction kernels are streaming gathers and reductions: no scratch, no spills, at most 64 VGPRs (eight
    waves per SIMD), and only the four floats of LDS the block reductions pass their wave sums through."""
    t = kernel_resources.library_table(_lib.LIB_PATH)
    for name, n, lds in (("wetts::slice_ids_kernel", 1, 0), ("wetts::slice_segments_kernel", 2, 0),
                         ("wetts::kl_rows_kernel", 1, 16), ("wetts::l1_rows_kernel", 1, 16),
                         ("wetts::ratio_total_kernel", 1, 0), ("wetts::rand_kernel", 1, 0)):
        ks = [k for k in t if k == name or k.startswith("void " + name + "<")]
        assert len(ks) == n, (name, ks)
        for k in ks:
            row = t[k]
            assert row.get("ScratchSize", 0) == 0 and row.get("VGPRSpill", 0) == 0 and row.get("SGPRSpill", 0) == 0, (k, row)
            assert row["VGPRs"] <= 64 and row.get("LDSSize", 0) == lds, (k, row)
