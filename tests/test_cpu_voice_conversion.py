"""CPU tier of voice conversion: the posterior encoder's blob layout (held to the live reference's `enc_q.*` keys and
shapes in tests/golden/reference_state_dicts.npz), its packing, the state_dict surface with and without `enc_q`, the
untouched main blob, and the resources of the new kernels (no GPU needed)."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import util
from wetts_amd import SynthesizerTrn, _lib, checkpoint, config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_STATE_DICTS = os.path.join(util.GOLDEN, "reference_state_dicts.npz")
SPEC = 513
# (model, n_vocab, n_speakers) of the pinned reference state_dicts (make_golden.py:STATE_DICT_MODELS)
PINNED = [("v1", 50, 1), ("v3", 50, 2), ("vocos", 50, 2), ("vits2_vocos_v1", 50, 1), ("tiny_preconv2_spk", 50, 3)]


def _cfg(mname, n_vocab=40, n_spk=3):
    return config.make_config(dict(config.MODEL_CONFIGS[mname]), n_vocab, n_spk)


@pytest.mark.parametrize("mname,n_vocab,n_spk", PINNED)
def test_posterior_layout_matches_reference_enc_q(mname, n_vocab, n_spk):
    ref = json.loads(str(np.load(REF_STATE_DICTS)[f"sd_{mname}_{n_spk}"]))
    want = {k: tuple(v) for k, v in ref.items() if k.startswith("enc_q.")}
    assert len(want) == 70
    got = {name: shape for name, _, _, shape in checkpoint.posterior_layout(_cfg(mname, n_vocab, n_spk), SPEC)}
    assert got == want
    lay = checkpoint.posterior_layout(_cfg(mname, n_vocab, n_spk), SPEC)
    assert checkpoint.posterior_numel(_cfg(mname, n_vocab, n_spk), SPEC) >= lay[-1][1] + lay[-1][2]
    assert all(off % 64 == 0 for _, off, _, _ in lay)  # 256-byte aligned, like the main blob


def test_posterior_layout_rejects_bad_spec_channels():
    assert _lib.load().wetts_posterior_blob_numel(_cfg("tiny"), 0) < 0
    with pytest.raises(_lib.WettsError):
        checkpoint.posterior_layout(_cfg("tiny"), -3)


def test_pack_posterior_blob_round_trip_and_shape_check():
    cfg = _cfg("tiny")
    psd = synth.make_posterior_state_dict(cfg, SPEC, 5)
    assert any(k.endswith(".weight_g") for k in psd)  # WN layers carry weight-norm pairs like a reference checkpoint
    blob = checkpoint.pack_posterior_blob(cfg, SPEC, psd)
    folded = checkpoint.fold_weight_norm(psd)
    for name, off, numel, shape in checkpoint.posterior_layout(cfg, SPEC):
        assert torch.equal(blob[off:off + numel].view(shape), folded[name].float())
    bad = dict(psd)
    bad["enc_q.proj.bias"] = torch.zeros(7)
    with pytest.raises(ValueError):
        checkpoint.pack_posterior_blob(cfg, SPEC, bad)
    short = {k: v for k, v in psd.items() if not k.startswith("enc_q.proj.")}
    with pytest.raises(KeyError):
        checkpoint.pack_posterior_blob(cfg, SPEC, short)
    assert not checkpoint.has_posterior(cfg, SPEC, short)
    assert checkpoint.has_posterior(cfg, SPEC, psd)


def _net(mname="tiny", n_spk=3):
    return SynthesizerTrn(40, SPEC, 32, n_speakers=n_spk, **config.MODEL_CONFIGS[mname])


def test_state_dict_with_enc_q_round_trips():
    cfg = _cfg("tiny")
    sd = synth.make_state_dict(cfg, 3)
    psd = synth.make_posterior_state_dict(cfg, SPEC, 4)
    net = _net().load_state_dict(dict(sd, **psd))
    out = net.state_dict()
    main = [name for name, _, _, _ in checkpoint.blob_layout(cfg)]
    post = [name for name, _, _, _ in checkpoint.posterior_layout(cfg, SPEC)]
    assert list(out) == main + post  # appended after today's keys, folded
    again = _net().load_state_dict(out)
    assert torch.equal(again._blob, net._blob)
    assert torch.equal(again._post_blob, net._post_blob)
    assert torch.equal(net._post_blob, checkpoint.pack_posterior_blob(cfg, SPEC, psd))


def test_state_dict_without_enc_q_is_unchanged():
    cfg = _cfg("tiny")
    sd = synth.make_state_dict(cfg, 3)
    net = _net().load_state_dict(sd)
    assert net._post_blob is None
    out = net.state_dict()
    assert list(out) == [name for name, _, _, _ in checkpoint.blob_layout(cfg)]
    blob = checkpoint.pack_blob(cfg, sd)
    for name, off, numel, shape in checkpoint.blob_layout(cfg):
        assert torch.equal(out[name], blob[off:off + numel].view(shape))
    # a partial enc_q set is not a posterior encoder: it is ignored, as before
    psd = synth.make_posterior_state_dict(cfg, SPEC, 4)
    part = dict(sd, **{k: v for k, v in psd.items() if k.startswith("enc_q.pre.")})
    assert _net().load_state_dict(part)._post_blob is None


def test_voice_conversion_errors_before_any_device_work():
    net = _net(n_spk=0).load_state_dict(synth.make_state_dict(_cfg("tiny", 40, 0), 1))
    with pytest.raises(AttributeError):  # no emb_g, as in the reference
        net.voice_conversion(torch.zeros(1, SPEC, 4), torch.tensor([4]), torch.tensor([0]), torch.tensor([0]))


@pytest.mark.parametrize("name", util.INFER_CASES[:6] + ["aishell3_b4x128"])
def test_main_blob_checksums_untouched(name):
    util.case_model(util.load_case(name))  # asserts the stored blob checksum


def test_new_kernels_have_no_scratch_and_full_occupancy():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    if not os.path.exists(kernel_resources.READELF) or shutil.which("c++filt") is None:
        pytest.skip("needs llvm-readelf and c++filt")
    table = kernel_resources.library_table(_lib.LIB_PATH)
    names = ["wetts::coupling_fwd_flip_kernel", "wetts::mono_coupling_fwd_kernel", "wetts::seq_mask_kernel",
             "wetts::posterior_sample_kernel"]
    for k in names:
        assert k in table, k
        # element-wise kernels: no spills, and few enough registers for eight waves per SIMD
        assert table[k]["ScratchSize"] == 0 and table[k]["VGPRs"] <= 64, (k, table[k])


# ---- the oracle's voice conversion (oracle/vits_oracle.py) pinned to the reference's goldens --------------------------
VC_CASES = ["vc_tiny_b3", "vc_vits2_v1_b2", "vc_tiny_preconv2_spk_b3", "vc_tiny_mono_post_b2", "vc_tiny_mono_inter_b3",
            "vc_tiny_vocos_b2", "vc_aishell3_b4x600"]
# one fixture per flow type: plain, pre_conv, pre_conv2, mono_layer_post_residual, mono_layer_inter_residual
FLOW_TYPE_CASES = VC_CASES[:5]


@pytest.mark.parametrize("name", VC_CASES)
def test_oracle_voice_conversion_matches_reference_golden(name):
    """oracle.voice_conversion at f32 on the fixture's input and injected draw against the live reference's outputs:
    y_mask equal, every stage within 1e-5 rel RMS, audio within 1e-5 abs RMS (the full-size fixture: its stored
    strided sub-samples)."""
    from oracle import vits_oracle as vo
    case = util.load_vc_case(name)
    cfg, sd, psd = util.vc_case_model(case, SPEC)
    W = util.vc_weights(cfg, sd, psd)
    st = vo.voice_conversion(W, util.cfg_dict(cfg), torch.from_numpy(case["y"]), torch.from_numpy(case["y_lengths"]),
                             torch.from_numpy(case["sid_src"]), torch.from_numpy(case["sid_tgt"]),
                             torch.from_numpy(case["eps"]), return_stages=True)
    assert np.array_equal(st["y_mask"].numpy(), case["y_mask"])
    rows = {}
    if "sub_strides" in case:
        sa, sz = (int(v) for v in case["sub_strides"])
        assert tuple(st["o_hat"].shape) == tuple(int(v) for v in case["audio_shape"])
        for k in ("z", "m_q", "logs_q", "z_p", "z_hat"):
            rows[k] = util.rel_rms(st[k].numpy()[..., ::sz], case[k + "_sub"])
        rows["audio_abs_rms"] = util.rms(st["o_hat"].numpy()[..., ::sa] - case["audio_sub"])
    else:
        for k in ("z", "m_q", "logs_q", "z_p", "z_hat"):
            rows[k] = util.rel_rms(st[k].numpy(), case[k])
        assert st["o_hat"].shape == case["audio"].shape
        rows["audio_abs_rms"] = util.rms(st["o_hat"].numpy() - case["audio"])
    print(name, "oracle vs reference", rows)
    for k, v in rows.items():
        assert v < 1e-5, (k, rows)


@pytest.mark.parametrize("name", FLOW_TYPE_CASES)
def test_oracle_flow_round_trip_float64(name):
    """flow_reverse(flow_forward(z)) == z on valid frames to 1e-12 in float64, for every flow type (mean-only couplings
    are exact inverses on mask-1 frames), and the forward flow is not the identity."""
    from oracle import vits_oracle as vo
    case = util.load_vc_case(name)
    cfg, sd, psd = util.vc_case_model(case, SPEC)
    W = util.vc_weights(cfg, sd, psd, torch.float64)
    cd = util.cfg_dict(cfg)
    yl = torch.from_numpy(case["y_lengths"])
    B, Ty = len(yl), int(case["y"].shape[2])
    y_mask = (torch.arange(Ty)[None, :] < yl[:, None]).to(torch.float64).unsqueeze(1)
    z = torch.randn(B, cd["inter_channels"], Ty, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    z = z * y_mask
    g = torch.nn.functional.embedding(torch.from_numpy(case["sid_src"]), W["emb_g.weight"]).unsqueeze(-1)
    with torch.no_grad():
        z_p = vo.flow_forward(W, cd, z, y_mask, g)
        back = vo.flow_reverse(W, cd, z_p, y_mask, g)
    assert z_p.dtype == back.dtype == torch.float64
    valid = y_mask.bool().expand_as(z)
    err = float((back - z)[valid].abs().max())
    moved = util.rel_rms(z_p[valid].numpy(), z[valid].numpy())
    print(name, "float64 round trip max |error|", err, "forward flow moves z by", moved)
    assert moved > 1e-2
    assert err < 1e-12
