"""CPU tier of the WavLM loss (csrc/wavlm.hip, wetts_amd/wavlm.py): the plain-torch oracle of tests/wavlm_oracle.py against
the reference's fixtures (tests/golden/wavlm_*.npz), the C library's bucket table and frame counts against transformers'
own known answers, the resampler's analytic facts, the state-dict round trip under both weight-norm spellings, the
refused configs, and the sensitivity of the fixtures to every injected defect.  No GPU: what runs here is host code
(layouts, tables, checks) and the oracle."""
import math
import os

import numpy as np
import pytest
import torch

from tests import wavlm_oracle as wo
from wetts_amd import _lib, discriminators, losses, wavlm

CASES = [(c, s) for c in wo.CONFIGS for s in wo.SHAPES]
SENS_CASES = [(c, s) for c, s in CASES if wo.frames(c, -(-16000 * s[1] // s[0])) >= 18]


def _fixture_figures(c, cname, B, o):
    """{figure: (rel, local)} of a forward dict `o` against the reference's stored float32 values."""
    if "hidden" in c.files:
        hid = None
        for a, r in zip(o["hidden"], torch.from_numpy(c["hidden"])):
            hid = wo.worst(hid, wo.gates(a.float(), r))
    else:
        hid = wo.gates(o["hidden"][-1][[0, B]].float(), torch.from_numpy(c["hidden_last"]))
    res = wo.gates(o["resampled"][:c["resampled"].shape[0]].float(), torch.from_numpy(c["resampled"]))
    figs = dict(resample=res, hidden=hid, d=wo.gates(o["d"].float(), torch.from_numpy(c["d"])))
    for k in ("loss_lm", "loss_lm_gen", "loss_slm"):
        figs[k] = wo.rel_err(o[k], c[k])
    return figs


@pytest.mark.parametrize("cname,shape", CASES)
def test_oracle_matches_reference_fixture(cname, shape):
    """The float32 evaluation of the restatement against the reference's float32 (two evaluations one floor from
    float64 each: GATE_FACTOR + 1 floors), and the float64 oracle within one fixture gate too."""
    c = wo.load_fixture(cname, shape)
    wav, rec, o64 = wo.reference(cname, shape)
    assert o64["hidden"][0].shape[1] == int(c["frames"]) and o64["resampled"].shape[1] == int(c["resampled_len"])
    o32 = wo.forward(cname, shape, wav, rec, torch.float32)
    for tag, o in (("float32", o32), ("float64", o64)):
        for k, v in _fixture_figures(c, cname, shape[2], o).items():
            g = wo.fixture_gate(c["floor_" + k])
            assert wo.within(v, g), f"{tag} {k}: {v} against the gate {g}"


@pytest.mark.parametrize("nb,md", [(16, 12), (320, 800)])
def test_bucket_table_equals_transformers(nb, md):
    kat = np.load(os.path.join(wo.GOLDEN, "wavlm_bucket_kat.npz"))
    lib = _lib.load()
    got = np.array([lib.wetts_wavlm_bucket(nb, md, int(r)) for r in kat["rel"]], dtype=np.int32)
    assert np.array_equal(got, kat[f"bucket_{nb}_{md}"])
    if nb == 16:  # the oracle's own table, and the ranges the test configs reach within 18 frames
        T = 40
        assert np.array_equal(wo.buckets("tiny", T).numpy(),
                              np.array([[lib.wetts_wavlm_bucket(nb, md, j - i) for j in range(T)] for i in range(T)]))
        row = [lib.wetts_wavlm_bucket(nb, md, r) for r in range(18)]
        assert row[:4] == [0, 9, 10, 11] and row[4] == 12 and row[7] == 14 and row[12] == 15 and row[17] == 15
    assert lib.wetts_wavlm_bucket(2, 12, 1) == -1 and lib.wetts_wavlm_bucket(16, 4, 1) == -1


def test_frame_counts_equal_transformers():
    kat = np.load(os.path.join(wo.GOLDEN, "wavlm_lengths_kat.npz"))
    cfg = wavlm.wavlm_config(wo.HF_CONFIGS["tiny"])
    got = [wavlm.num_frames(cfg, int(L)) for L in kat["samples"]]
    assert got == kat["frames"].tolist() and got == [wo.frames("tiny", int(L)) for L in kat["samples"]]
    assert wavlm.num_frames(cfg, 399) == 0 and wavlm.num_frames(cfg, 400) == 1 and wavlm.min_samples(cfg) == 400
    # the issue's three lengths: 552 -> 401 -> 1, 1024 -> 744 -> 2, 8192 -> 5945 -> 18
    r = wavlm.Resample(22050, 16000)
    assert [(r.output_length(L), wavlm.num_frames(cfg, r.output_length(L))) for L in (552, 1024, 8192)] == \
        [(401, 1), (744, 2), (5945, 18)]


def test_resampler_kernel_and_facts():
    k, width, o, n = wavlm.resample_kernel(22050, 16000)
    assert (width, o, n) == (9, 441, 320) and tuple(k.shape) == (320, 459)
    assert torch.equal(k, wo.resample_kernel(22050, 16000)[0])  # product and oracle state the same arithmetic
    assert wavlm.resample_kernel(24000, 16000)[1:] == (10, 3, 2)
    x = torch.randn(2, 700)
    assert wo.resample(x, 16000, 16000, torch.float32) is not None and torch.equal(wo.resample(x, 16000, 16000, torch.float32), x)
    assert wavlm.Resample(16000, 16000)(x) is x  # identity returns its input, on any device
    for rate, L in ((22050, 552), (22050, 8192), (24000, 2048), (24000, 2047), (8000, 333)):
        g = math.gcd(rate, 16000)
        y = wo.resample(torch.randn(1, L), rate, 16000)
        assert y.shape[1] == -(-(16000 // g) * L // (rate // g)) == wavlm.Resample(rate, 16000).output_length(L)
    # DC gain.  Away from the edges the response to a constant is the sum of the kernel row of the output's phase, and
    # that is the filter's, not the implementation's: a Hann-windowed sinc cut at 6 zero crossings with rolloff 0.99 has
    # the gain 1.00047 (+- 4e-5 over the 320 phases), not 1 -- by this restatement of the kernel; torchaudio itself was
    # not available to confirm the figure.  So: the oracle reproduces the row sums within the float32 floor of the stage,
    # and the row sums are within 1e-3 of 1.
    floor = wo.gate_of(wo.load_fixture("tiny", wo.SHAPES[2])["floor_resample"])[1]
    rows = wavlm.resample_kernel(22050, 16000)[0].double().sum(1)
    y = wo.resample(torch.ones(1, 8192), 22050, 16000)[0]
    inner = torch.arange(64, y.numel() - 64)
    assert float((y[inner] - rows[inner % 320]).abs().max()) <= floor
    assert float((rows - 1).abs().max()) <= 1e-3 and float((rows - rows.mean()).abs().max()) <= 1e-4
    # a 1 kHz sinusoid keeps its amplitude; a tone above the new Nyquist (9.5 kHz) is attenuated
    t = torch.arange(8192, dtype=torch.float64) / 22050
    # (cutoff 0.99 x 8 kHz; 9.5 kHz lies at the end of the transition band: 20 dB down; at 11 kHz a Hann-windowed design
    # is at its stop-band level of -44 dB = 0.0063)
    for f, lo, hi in ((1000.0, 0.995, 1.005), (9500.0, 0.0, 0.1), (11000.0, 0.0, 0.01)):
        y = wo.resample(torch.sin(2 * math.pi * f * t)[None], 22050, 16000)[0, 200:-200]
        amp = float(y.abs().max())
        assert lo <= amp <= hi, (f, amp)


def test_state_dict_round_trip_under_both_weight_norm_spellings():
    sd = wo.weights("tiny")[0][0]
    a = wavlm.WavLM(wo.HF_CONFIGS["tiny"]).load_state_dict(sd)
    legacy = {}
    for k, v in sd.items():
        k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        legacy[k] = v
    assert any(k.endswith("conv.weight_g") for k in legacy)
    b = wavlm.WavLM(wo.HF_CONFIGS["tiny"]).load_state_dict(legacy)
    assert torch.equal(a._blob, b._blob)
    folded = dict(sd)
    folded[wavlm.POS_CONV + "weight"] = wo.pos_conv_weight(sd)
    del folded[wavlm.POS_CONV + "parametrizations.weight.original0"], folded[wavlm.POS_CONV + "parametrizations.weight.original1"]
    assert torch.allclose(wavlm.WavLM(wo.HF_CONFIGS["tiny"]).load_state_dict(folded)._blob, a._blob, rtol=1e-6, atol=0)
    for net, src in ((a, sd), (b, legacy)):
        out = net.state_dict()
        assert set(out) == set(src) - {"masked_spec_embed"}
        assert all(torch.equal(out[k], src[k]) for k in out)
        assert torch.equal(wavlm.WavLM(wo.HF_CONFIGS["tiny"]).load_state_dict(out)._blob, a._blob)
    # the blob holds what the layout says: tap-major convs, the folded positional conv, [heads] constants
    lay = {n: (off, numel, shape) for n, off, numel, shape in wavlm.blob_layout(a.config)}
    off, numel, shape = lay["feature_extractor.conv_layers.1.conv.weight"]
    assert shape == (32, 3, 32)
    assert torch.equal(a._blob[off:off + numel].reshape(shape), sd["feature_extractor.conv_layers.1.conv.weight"].permute(0, 2, 1))
    off, numel, shape = lay[wavlm.POS_CONV + "weight"]
    assert torch.allclose(a._blob[off:off + numel].reshape(shape), wo.pos_conv_weight(sd).permute(0, 2, 1), rtol=1e-6, atol=0)
    missing = {k: v for k, v in sd.items() if k != "encoder.layers.1.attention.gru_rel_pos_const"}
    with pytest.raises(KeyError, match="gru_rel_pos_const"):
        wavlm.WavLM(wo.HF_CONFIGS["tiny"]).load_state_dict(missing)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        wavlm.WavLM(wo.HF_CONFIGS["tiny"]).state_dict()
    # the discriminator: both spellings and folded weights give one blob
    dd = wo.weights("tiny")[1][0]
    mk = lambda: discriminators.WavLMDiscriminator(48, 3, 8)  # noqa: E731
    d0 = mk().load_state_dict(dd)
    par = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): v
           for k, v in dd.items()}
    assert torch.equal(mk().load_state_dict(par)._blob, d0._blob)
    assert torch.equal(mk().load_state_dict(d0.state_dict())._blob, d0._blob)
    assert tuple(d0.state_dict()["pre.weight"].shape) == (8, 3 * 48, 1)
    assert mk()._folded is None
    for name, bad in (("convs.1.weight_v", dd["convs.1.weight_v"][:, :, :3]), ("pre.bias", dd["pre.bias"][:4]),
                      ("conv_post.weight_v", dd["conv_post.weight_v"].transpose(1, 2))):
        with pytest.raises(ValueError, match=name.rsplit("_v", 1)[0].replace(".", r"\.")):
            mk().load_state_dict(dict(dd, **{name: bad}))


@pytest.mark.parametrize("key,value", [("feat_extract_norm", "layer"), ("do_stable_layer_norm", True), ("conv_bias", True),
                                       ("add_adapter", True), ("hidden_act", "relu"), ("feat_extract_activation", "relu")])
def test_refused_configs_name_the_key(key, value):
    with pytest.raises(ValueError, match=key):
        wavlm.WavLM(dict(wo.HF_CONFIGS["tiny"], **{key: value}))


def test_refused_shapes_and_arguments():
    for key, value in (("hidden_size", 50), ("num_attention_heads", 5), ("num_conv_pos_embedding_groups", 16),
                       ("conv_dim", [32] * 6 + [1032]), ("conv_kernel", [10, 3, 3])):
        with pytest.raises(ValueError):
            wavlm.WavLM(dict(wo.HF_CONFIGS["tiny"], **{key: value}))
    with pytest.raises(NotImplementedError, match="use_spectral_norm"):
        discriminators.WavLMDiscriminator(use_spectral_norm=True)
    with pytest.raises(ValueError, match="initial_channel"):
        discriminators.WavLMDiscriminator(48, 3, 6)
    with pytest.raises(FileNotFoundError, match="pytorch_model.bin"):
        wavlm.load_wavlm(os.path.join(wo.GOLDEN, "no_such_model"))
    with pytest.raises(FileNotFoundError, match="pytorch_model.bin"):
        losses.WavLMLoss(os.path.join(wo.GOLDEN, "no_such_model"), None, 22050)
    net = wavlm.WavLM(wo.HF_CONFIGS["tiny"]).load_state_dict(wo.weights("tiny")[0][0])
    with pytest.raises(ValueError, match="HIP device"):
        net.to("cpu")
    with pytest.raises(RuntimeError, match="not on a device"):
        net.hidden_states(torch.zeros(1, 400))
    lib = _lib.load()
    assert lib.wetts_wavlm_workspace_bytes(None, 1, 400) < 0 and "null handle" in _lib.last_error()

    class H(dict):
        def __getattr__(self, k):
            return self[k]
    assert discriminators.wavlm_discriminator_from_hparams(H(model=H(use_wd=False))) is None
    assert discriminators.wavlm_discriminator_from_hparams(H(model=H(inter_channels=192))) is None
    wd = discriminators.wavlm_discriminator_from_hparams(H(model=H(use_wd=True, slm_hidden=768, slm_nlayers=13, slm_initial_channel=64)))
    assert (wd.slm_hidden, wd.slm_layers, wd.initial_channel) == (768, 13, 64)
    assert [n for n, *_ in wd.layout()][:2] == ["pre.weight", "pre.bias"] and wd.layout()[0][3] == (64, 13 * 768)


def test_load_wavlm_reads_a_model_directory(tmp_path):
    import json
    sd = wo.weights("tiny")[0][0]
    with open(tmp_path / "config.json", "w") as f:
        json.dump(wo.HF_CONFIGS["tiny"], f)
    torch.save({"wavlm." + k if i % 2 else k: v for i, (k, v) in enumerate(sd.items())}, tmp_path / "pytorch_model.bin")
    net = wavlm.load_wavlm(str(tmp_path))
    assert torch.equal(net._blob, wavlm.pack_blob(net.config, sd)) and net.num_layers == 2 and net.hidden_size == 48
    assert "transformers" not in wavlm.__dict__ and "transformers" not in losses.__dict__


@pytest.mark.parametrize("cname,shape", SENS_CASES)
def test_every_injected_defect_is_seen(cname, shape):
    """Each defect moves its figure (the last hidden state; the discriminator's output for the channel order) to at
    least 10 x the gate, here and when the fixture was made (the stored sens_<fault>)."""
    c = wo.load_fixture(cname, shape)
    wav, rec, o = wo.reference(cname, shape)
    assert wo.faults("tiny") == wo.FAULTS and "own_table" not in wo.faults("wide")
    for f in wo.faults(cname):
        bad = wo.forward(cname, shape, wav, rec, fault=f)
        if wo.FAULT_STAGE[f] == "disc":
            fig, gate = wo.gates(bad["d"], o["d"]), wo.gate_of(c["floor_d"])
        else:
            fig, gate = wo.gates(bad["hidden"][-1], o["hidden"][-1]), wo.gate_of(c["floor_hidden"])
        assert fig[0] >= 10 * gate[0] and fig[1] >= 10 * gate[1], (f, fig, gate)
        assert np.allclose(fig, c["sens_" + f], rtol=1e-6), (f, fig, c["sens_" + f])
