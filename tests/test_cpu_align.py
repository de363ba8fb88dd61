"""CPU tier of forced alignment: the fixtures of tests/golden/make_golden_align.py (integrity, path stability), the
float64 oracle composition the GPU tests use pinned to the reference's stage tensors, argument validation of align()
and infer(durations=) that needs no device, and header / binding agreement of the new entries."""
import os
import re

import numpy as np
import pytest
import torch

from tests import align_oracle as ao, util
from wetts_amd import SynthesizerTrn, _lib, config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = ao.SPEC
REL_RMS, LOCAL = 1e-5, 1e-4  # the stage gates of tests/test_gpu_vc_oracle.py
ENTRIES = ("wetts_align_scores", "wetts_align_lengths", "wetts_path_to_durations", "wetts_counts_to_lengths")


def _largest_vc_fixture():
    return max(os.path.getsize(os.path.join(util.GOLDEN, f)) for f in os.listdir(util.GOLDEN) if f.startswith("vc_"))


@pytest.mark.parametrize("name", ao.ALIGN_CASES)
def test_fixture_integrity_and_path_stability(name):
    """The fixture reloads with its inputs rebuilt, both blob checksums match, the generator recorded a stable path,
    the stored path is a valid monotonic alignment with x_lengths <= y_lengths, w is its column sum, and the search
    over the stored scores gives the stored path (full-size case: over the oracle's float64 scores, which the stored
    rows of the reference's scores are held to)."""
    assert os.path.getsize(os.path.join(util.GOLDEN, name + ".npz")) <= _largest_vc_fixture()
    c = ao.load_align_case(name)
    cfg, sd, psd = util.vc_case_model(c, SPEC)  # asserts both checksums
    assert int(c["path_stable"]) == 1 and c["attn"].dtype == np.uint8
    xl, yl = c["x_lengths"], c["y_lengths"]
    assert (xl <= yl).all()
    B, Ty, Tx = c["attn"].shape
    assert (Ty, Tx) == (int(yl.max()), int(xl.max()))
    ao.check_monotonic(c["attn"], xl, yl)
    assert np.array_equal(c["w"], c["attn"].sum(1).astype(np.float32))
    assert np.array_equal(c["w"].sum(-1), yl.astype(np.float32))
    assert np.array_equal(c["attn"].sum(-1).astype(np.float32), c["y_mask"])
    assert np.array_equal(c["x_mask"], (np.arange(Tx)[None] < xl[:, None]).astype(np.float32))
    if "neg_cent" in c:
        from oracle import vits_oracle as vo
        assert np.array_equal(vo.maximum_path_numpy(c["neg_cent"], yl, xl), c["attn"].astype(np.int32))


@pytest.mark.parametrize("name", ao.ALIGN_CASES)
def test_float64_oracle_reproduces_the_reference_stages(name):
    """oracle_align in float64 on the fixture's inputs: path EQUAL to the reference's attn (stability (a) of the
    generator, re-established here), the six stage tensors and the scores within rel RMS 1e-5 and max|d|/rms 1e-4
    of the reference's f32 tensors."""
    c = ao.load_align_case(name)
    cfg, sd, psd = util.vc_case_model(c, SPEC)
    W = util.vc_weights(cfg, sd, psd, torch.float64)
    st = ao.oracle_align(W, util.cfg_dict(cfg), *ao.case_tensors(c))
    assert np.array_equal(st["path"], c["attn"].astype(np.int32))
    assert np.array_equal(st["w"].numpy(), c["w"])
    assert np.array_equal(st["y_mask"][:, 0].numpy(), c["y_mask"]) and np.array_equal(st["x_mask"][:, 0].numpy(), c["x_mask"])
    stride = int(c["sub_stride"]) if "sub_stride" in c else None
    rows = {}
    for k in ao.STAGES + ("neg_cent",):
        got = st[k].numpy()
        if stride:
            got, ref = (got[:, ::stride] if k == "neg_cent" else got[..., ::stride]), c[k + "_sub"]
        else:
            ref = c[k]
        if k == "neg_cent":  # valid cells only: the rest is never read by the search
            v = ao.valid_mask(c["x_lengths"], c["y_lengths"], st[k].shape[2], st[k].shape[1])
            v = v[:, ::stride] if stride else v
            got, ref = got[v], ref[v]
        scale = max(util.rms(ref), 1e-30)
        rows[k] = (util.rms(got - ref) / scale, float(np.abs(got - ref).max()) / scale)
    print(name, "float64 oracle vs reference (rel RMS, max|d|/rms):", rows)
    for k, (rel, loc) in rows.items():
        assert rel <= REL_RMS and loc <= LOCAL, (k, rows)


# ---- argument validation before any device work ----------------------------------------------------------------------
def _net(n_spk=3):
    cfg = config.make_config(dict(config.MODEL_CONFIGS["tiny"]), 40, n_spk)
    sd = dict(synth.make_state_dict(cfg, 1), **synth.make_posterior_state_dict(cfg, SPEC, 2))
    return SynthesizerTrn(40, SPEC, 32, n_speakers=n_spk, **config.MODEL_CONFIGS["tiny"]).load_state_dict(sd)


def test_align_argument_validation_needs_no_device():
    net = _net()
    x, xl = torch.zeros(2, 5, dtype=torch.long), torch.tensor([5, 3])
    y, yl = torch.zeros(2, SPEC, 9), torch.tensor([9, 4])
    sid = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="x must be"):
        net.align(x[0], xl, y, yl, sid)
    with pytest.raises(ValueError, match="y must be"):
        net.align(x, xl, y[:, :80], yl, sid)
    with pytest.raises(ValueError, match="y must be"):
        net.align(x, xl, y[:1], yl, sid)
    with pytest.raises(ValueError, match="x_lengths must be"):
        net.align(x, xl[:1], y, yl, sid)
    with pytest.raises(ValueError, match="y_lengths must be"):
        net.align(x, xl, y, torch.tensor([[9, 4]]), sid)
    with pytest.raises(ValueError, match="sid is required"):
        net.align(x, xl, y, yl)
    with pytest.raises(ValueError, match="eps_q must be"):
        net.align(x, xl, y, yl, sid, eps_q=torch.zeros(2, 192, 8))
    with pytest.raises(_lib.WettsError):  # valid arguments: the product path has no CPU fallback
        net.align(x, xl, y, yl, sid)


def test_infer_durations_argument_validation_needs_no_device():
    net = _net()
    x, xl, sid = torch.zeros(2, 5, dtype=torch.long), torch.tensor([5, 3]), torch.tensor([0, 1])
    for bad in (torch.ones(2, 4, dtype=torch.long), torch.ones(5, dtype=torch.long), torch.ones(2, 2, 5, dtype=torch.long),
                torch.ones(1, 1, 5, dtype=torch.long)):
        with pytest.raises(ValueError, match="durations must be"):
            net.infer(x, xl, sid, durations=bad)
    with pytest.raises(ValueError, match="integer tensor"):
        net.infer(x, xl, sid, durations=torch.ones(2, 5, dtype=torch.bool))
    for ok in (torch.ones(2, 5, dtype=torch.long), torch.ones(2, 1, 5, dtype=torch.int32), torch.ones(2, 1, 5)):
        with pytest.raises(_lib.WettsError):  # accepted shape: fails only for want of a device
            net.infer(x, xl, sid, durations=ok)


def test_forward_still_raises():
    with pytest.raises(NotImplementedError):
        _net().forward()


# ---- header / binding agreement ---------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_new_entries():
    src = open(os.path.join(ROOT, "include", "wetts_hip.h")).read()
    assert int(re.search(r"#define WETTS_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 12
    lib = _lib.load()
    for name in ENTRIES:
        m = re.search(r"int32_t " + name + r"\(([^;]*)\);", src)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib._I32 and len(argtypes) == len(args), (name, args)
        for a, t in zip(args, argtypes):  # pointers bind as void*, int32_t as c_int32
            assert (t is _lib._P) == ("*" in a) and (t is _lib._I32) == (a.startswith("int32_t ") and "*" not in a), (name, a)
        assert hasattr(lib, name)
    for macro, value in (("WETTS_STATUS_ALIGN_TEXT_LONGER", _lib.STATUS_ALIGN_TEXT_LONGER),
                         ("WETTS_STATUS_DURATION_NEGATIVE", _lib.STATUS_DURATION_NEGATIVE)):
        assert int(re.search(r"#define " + macro + r" (\d+)", src).group(1)) == value
    bits = [_lib.STATUS_SPLINE_DOMAIN, _lib.STATUS_PHONE_ID_RANGE, _lib.STATUS_SPEAKER_ID_RANGE,
            _lib.STATUS_DURATION_NONFINITE, _lib.STATUS_ALIGN_TEXT_LONGER, _lib.STATUS_DURATION_NEGATIVE]
    assert sorted(bits) == [1, 2, 4, 8, 16, 32]


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.wetts_align_scores(None, None, None, 1, 1, 1, None, None) == -1
    assert lib.wetts_align_lengths(None, None, None, 1, 1, 1, None, None, None) == -1
    assert lib.wetts_path_to_durations(None, None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert lib.wetts_counts_to_lengths(None, None, 1, 1, None, None, None, None, None) == -1
