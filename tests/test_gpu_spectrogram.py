"""GPU tier of the spectrograms (csrc/stft.hip through wetts_amd/mel_processing.py): the linear spectrogram and the
log-mel against the float64 oracle (tests/spec_oracle.py) and the reference's own output (spec_kat / mel_kat),
padding invariance, audio -> posterior_spectrogram -> voice_conversion against every vc_* golden, and the error
surface."""
import math
import os

import numpy as np
import pytest
import torch

from tests import spec_oracle, util, vc_input
from tests.spec_oracle import utterance
from wetts_amd import SynthesizerTrn, _lib, config, mel_processing as mp

pytestmark = pytest.mark.gpu

DEV = "cuda"
REL_GATE, MAX_GATE = 2e-6, 5e-5  # rel RMS, max|d| / rms
WORST = {"rel": 0.0, "max": 0.0}


def _gate(got, ref, what):
    rel = util.rel_rms(got, ref)
    mx = float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(util.rms(ref), 1e-30)
    WORST["rel"], WORST["max"] = max(WORST["rel"], rel), max(WORST["max"], mx)
    print(f"{what}: rel rms {rel:.2e}  max|d|/rms {mx:.2e}  (worst so far {WORST['rel']:.2e} / {WORST['max']:.2e})")
    assert rel <= REL_GATE, (what, rel)
    assert mx <= MAX_GATE, (what, mx)


def _batch(lengths, sr, seed, fill=0.0):
    utts = [utterance(seed + b, sr, n) for b, n in enumerate(lengths)]
    a = torch.full((len(lengths), max(lengths)), fill, dtype=torch.float32)
    for b, u in enumerate(utts):
        a[b, :len(u)] = u
    return a, utts


# (n_fft, hop, win, center, lengths)
SWEEP = [
    (16, 4, 16, False, [100]),
    (16, 16, 16, True, [9, 40, 77]),
    (16, 4, 10, True, [7, 64]),
    (64, 16, 64, False, [25, 1003, 640, 333]),
    (64, 16, 48, True, [517, 26]),
    (1024, 256, 1024, False, [9000, 385, 4097, 20000, 12345, 777, 1024, 3000]),
    (1024, 256, 1024, True, [9001, 385]),
    (1024, 256, 800, False, [7777, 2000]),
    (1024, 255, 1024, True, [5000]),
    (2048, 512, 2048, False, [30000, 1537]),
    (2048, 2048, 2048, True, [40000]),
]


@pytest.mark.parametrize("n,h,w,center,lengths", SWEEP)
def test_linear_spectrogram_matches_float64_oracle(n, h, w, center, lengths):
    a, utts = _batch(lengths, 22050, 3)
    spec, sl = mp.spectrogram_torch(a.to(DEV), n, 22050, h, w, center, lengths=torch.tensor(lengths))
    ref, frames = spec_oracle.batch_spectrogram([u.double().numpy() for u in utts], n, h, w, center)
    torch.cuda.synchronize()
    assert sl.cpu().tolist() == frames.tolist()
    got = spec.cpu().numpy()
    assert got.shape == ref.shape
    _gate(got, ref, f"{n}/{h}/{w} center={center} B={len(lengths)}")


def test_ten_seconds_at_48k():
    a = utterance(7, 48000, 480000).unsqueeze(0)
    spec = mp.spectrogram_torch(a.to(DEV), 2048, 48000, 512, 2048)
    ref = spec_oracle.spectrogram(a[0].double().numpy(), 2048, 512, 2048)
    _gate(spec[0].cpu().numpy(), ref, "10 s at 48 kHz, 2048/512")


def test_unbatched_call_equals_dense_lengths():
    a, _ = _batch([3000, 3000, 3000], 22050, 9)
    s0 = mp.spectrogram_torch(a.to(DEV), 1024, 22050, 256, 1024)
    s1, _ = mp.spectrogram_torch(a.to(DEV), 1024, 22050, 256, 1024, lengths=[3000] * 3)
    assert torch.equal(s0, s1)
    # the 1-D-in-spirit call of data_utils: y.unsqueeze(0), float64 input is converted
    s2 = mp.spectrogram_torch(a[:1].double().to(DEV), 1024, 22050, 256, 1024)
    assert torch.equal(s2, s0[:1])


def test_matches_reference_spec_kat():
    d = np.load(os.path.join(util.GOLDEN, "spec_kat.npz"))
    for i, (n, h, w, c, sr, seed, length) in enumerate(d["cases"]):
        a = utterance(int(seed), int(sr), int(length)).unsqueeze(0).to(DEV)
        got = mp.spectrogram_torch(a, int(n), int(sr), int(h), int(w), bool(c))[0].cpu().numpy()
        _gate(got, d[f"spec_{i}"], f"spec_kat[{i}] {int(n)}/{int(h)}/{int(w)} center={bool(c)} L={int(length)}")


def _mel_check(got, ref64):
    big = ref64 >= math.log(1e-4)  # at least 10x the clamp
    err = float(np.abs(got[big] - ref64[big]).max())
    clamped_ref = ref64 <= math.log(1e-5)
    both = clamped_ref & (got <= np.float32(math.log(1e-5)))
    assert np.all(got[both] == got[both].flat[0]) if both.any() else True
    assert err <= 1e-4, err
    return err


def test_log_mel_matches_float64_oracle_and_mel_kat():
    d = np.load(os.path.join(util.GOLDEN, "mel_kat.npz"))
    for i, (sr, nm, fmin, fmax, seed, length) in enumerate(d["cases"]):
        sr, nm, seed, length = int(sr), int(nm), int(seed), int(length)
        fmax = None if fmax < 0 else float(fmax)
        a = utterance(seed, sr, length).unsqueeze(0)
        got = mp.mel_spectrogram_torch(a.to(DEV), 1024, nm, sr, 256, 1024, float(fmin), fmax)[0].cpu().numpy()
        ref64 = spec_oracle.log_mel(spec_oracle.spectrogram(a[0].double().numpy(), 1024, 256, 1024),
                                    spec_oracle.mel_basis(sr, 1024, nm, float(fmin), fmax))
        e64 = _mel_check(got, ref64)
        eref = _mel_check(got, d[f"mel_{i}"].astype(np.float64))
        print(f"mel_kat[{i}] sr {sr} mels {nm}: max abs err vs float64 {e64:.2e}, vs reference {eref:.2e}")
        # spec_to_mel of the linear spectrogram is the same computation
        spec = mp.spectrogram_torch(a.to(DEV), 1024, sr, 256, 1024)
        assert torch.equal(mp.spec_to_mel_torch(spec, 1024, nm, sr, float(fmin), fmax)[0].cpu(), torch.from_numpy(got))


@pytest.mark.parametrize("center", [False, True])
def test_padding_invariance_bit_exact(center):
    lengths = [5000, 385, 4097, 2600]
    clean, _ = _batch(lengths, 22050, 21, fill=0.0)
    dirty, _ = _batch(lengths, 22050, 21, fill=float("nan"))
    for b, n in enumerate(lengths):
        dirty[b, n::2] = 1e30
    outs = []
    for a in (clean, dirty):
        s, sl = mp.mel_spectrogram_torch(a.to(DEV), 1024, 80, 22050, 256, 1024, 0.0, None, center,
                                         lengths=torch.tensor(lengths).to(DEV))
        lin, _ = mp.spectrogram_torch(a.to(DEV), 1024, 22050, 256, 1024, center, lengths=lengths)
        outs.append((s.cpu(), lin.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[1][1]).all()
    for b, n in enumerate(lengths):  # each row equals the utterance run alone, zero-padded to the batch
        alone = mp.spectrogram_torch(clean[b:b + 1, :n].to(DEV), 1024, 22050, 256, 1024, center).cpu()
        T = alone.shape[-1]
        assert torch.equal(outs[0][1][b, :, :T], alone[0])
        assert torch.all(outs[0][1][b, :, T:] == 0)
        mel_alone = mp.mel_spectrogram_torch(clean[b:b + 1, :n].to(DEV), 1024, 80, 22050, 256, 1024, 0.0, None,
                                             center).cpu()
        assert torch.equal(outs[0][0][b, :, :T], mel_alone[0])
        assert torch.all(outs[0][0][b, :, T:] == 0)


# ---- audio -> posterior_spectrogram -> voice_conversion -------------------------------------------------------------

VC_CASES = ["vc_tiny_b3", "vc_vits2_v1_b2", "vc_tiny_preconv2_spk_b3", "vc_tiny_mono_post_b2", "vc_tiny_mono_inter_b3",
            "vc_tiny_vocos_b2", "vc_aishell3_b4x600"]
MEL_VC_CASES = ["vc_vits2_v1_mel_b2", "vc_tiny_vits2_vocos_mel_b2"]


def _hps(mname, sr, n_mels, use_mel):
    return config.HParams(data=dict(filter_length=vc_input.N_FFT, hop_length=vc_input.HOP, win_length=vc_input.WIN,
                                    sampling_rate=sr, n_mel_channels=n_mels, mel_fmin=0.0, mel_fmax=None),
                          model=dict(config.MODEL_CONFIGS[mname], use_mel_posterior_encoder=use_mel))


def _audio(frames, sr, seed):
    utts = vc_input.utterances(frames, sr, seed)
    a = torch.zeros(len(utts), max(len(u) for u in utts))
    for b, u in enumerate(utts):
        a[b, :len(u)] = u
    return a, [len(u) for u in utts]


def _load_mel_case(name):
    d = np.load(os.path.join(util.GOLDEN, name + ".npz"))
    return {k: d[k] for k in d.files}


def _run_vc(case, spec_channels, use_mel):
    mname, sr = str(case["model"]), int(case["sampling_rate"])
    cfg, sd, psd = util.vc_case_model(case, spec_channels)
    net = SynthesizerTrn(int(case["n_vocab"]), spec_channels, 32, n_speakers=int(case["n_speakers"]),
                         **config.MODEL_CONFIGS[mname])
    net.load_state_dict(dict(sd, **psd))
    net.to(DEV)
    a, lens = _audio([int(v) for v in case["y_lengths"]], sr, int(case["input_seed"]))
    y, yl = mp.posterior_spectrogram(a.to(DEV), torch.tensor(lens).to(DEV), _hps(mname, sr, spec_channels, use_mel))
    assert yl.cpu().tolist() == [int(v) for v in case["y_lengths"]]
    o_hat, y_mask, (z, z_p, z_hat) = net.voice_conversion(
        y, yl, torch.from_numpy(case["sid_src"]).to(DEV), torch.from_numpy(case["sid_tgt"]).to(DEV),
        eps_q=torch.from_numpy(case["eps"]).to(DEV))
    torch.cuda.synchronize()
    st = net._last_vc
    return y.cpu().numpy(), o_hat, y_mask, dict(z=z, m_q=st["m_q"], logs_q=st["logs_q"], z_p=z_p, z_hat=z_hat)


def _stage_gates(name, case, o_hat, y_mask, got):
    """The gates of test_gpu_voice_conversion.py:test_voice_conversion_matches_reference_golden."""
    rows = {"y_mask_equal": bool(np.array_equal(y_mask.cpu().numpy(), case["y_mask"]))}
    if "sub_strides" in case:
        sa, sz = (int(v) for v in case["sub_strides"])
        assert tuple(o_hat.shape) == tuple(int(v) for v in case["audio_shape"])
        for k, v in got.items():
            rows[k] = util.rel_rms(v.cpu().numpy()[..., ::sz], case[k + "_sub"])
        audio = o_hat.cpu().numpy()
        rows["audio_abs_rms"] = util.rms(audio[..., ::sa] - case["audio_sub"])
        rows["audio_sqsum_rel"] = abs(float((audio.astype(np.float64) ** 2).sum()) - float(case["audio_sqsum"])) / \
            float(case["audio_sqsum"])
    else:
        for k, v in got.items():
            rows[k] = util.rel_rms(v.cpu().numpy(), case[k])
        assert o_hat.shape == case["audio"].shape
        rows["audio_abs_rms"] = util.rms(o_hat.cpu().numpy() - case["audio"])
    print(name, rows)
    assert rows["y_mask_equal"], rows
    for k in ("z", "m_q", "logs_q"):
        assert rows[k] < 1e-4, (k, rows)
    for k in ("z_p", "z_hat"):
        assert rows[k] < 2e-4, (k, rows)
    assert rows["audio_abs_rms"] < 1e-4, rows
    if "audio_sqsum_rel" in rows:
        assert rows["audio_sqsum_rel"] < 1e-3, rows


@pytest.mark.parametrize("name", VC_CASES)
def test_audio_to_voice_conversion_matches_linear_goldens(name):
    case = util.load_vc_case(name)
    y, o_hat, y_mask, got = _run_vc(case, vc_input.SPEC, use_mel=False)
    _gate(y, case["y"], f"{name} y")  # the spectrogram make_input builds with torch
    _stage_gates(name, case, o_hat, y_mask, got)


@pytest.mark.parametrize("name", MEL_VC_CASES)
def test_audio_to_voice_conversion_matches_mel_goldens(name):
    case = _load_mel_case(name)
    nm = int(case["spec_channels"])
    y, o_hat, y_mask, got = _run_vc(case, nm, use_mel=True)
    ref = case["y"].astype(np.float64)
    for b, T in enumerate(case["y_lengths"]):
        _mel_check(y[b, :, :T], ref[b, :, :T])
        assert np.all(y[b, :, T:] == 0)
    _stage_gates(name, case, o_hat, y_mask, got)


# ---- error surface --------------------------------------------------------------------------------------------------

def test_errors():
    a = torch.zeros(2, 4000, device=DEV)
    for n, h, w in [(15, 4, 15), (2, 1, 2), (0, 1, 1), (64, 0, 64), (64, 65, 64), (64, 16, 0), (64, 16, 65)]:
        with pytest.raises(ValueError):
            mp.spectrogram_torch(a, n, 22050, h, w)
    lib = _lib.load()
    s = _lib.current_stream_ptr()
    basis = mp._stft_basis(64, 64, a.device)
    out = torch.empty(2, 33, 8, device=DEV)
    for n, h, w in [(15, 4, 15), (2, 1, 2), (64, 0, 64), (64, 65, 64), (64, 16, 0), (64, 16, 65)]:
        rc = lib.wetts_spectrogram(_lib.ptr(a), None, 2, 4000, n, h, w, 0, _lib.ptr(basis), 8, _lib.ptr(out), s)
        assert rc == -1, (n, h, w, rc)
        assert "stft" in _lib.last_error()
    assert lib.wetts_stft_basis_numel(15, 15) == -1
    with pytest.raises(RuntimeError, match="Padding size"):
        mp.spectrogram_torch(a[:, :384], 1024, 22050, 256, 1024)
    with pytest.raises(RuntimeError, match="Padding size"):
        mp.spectrogram_torch(a, 1024, 22050, 256, 1024, lengths=[4000, 384])
    with pytest.raises(RuntimeError):
        mp.spectrogram_torch(a[:, :15], 16, 22050, 16, 16)
    mp.spectrogram_torch(a[:, :385], 1024, 22050, 256, 1024)  # the shortest length torch accepts
    for bad in (a[0], a[None]):
        with pytest.raises(ValueError, match="rank|\\[B, samples\\]"):
            mp.spectrogram_torch(bad, 1024, 22050, 256, 1024)
    with pytest.raises(ValueError):
        mp.spectrogram_torch(a.cpu(), 1024, 22050, 256, 1024)
    with pytest.raises(ValueError):
        mp.spectrogram_torch(a, 1024, 22050, 256, 1024, lengths=[4000, 4001])
    with pytest.raises(ValueError):
        mp.spec_to_mel_torch(torch.zeros(1, 100, 5, device=DEV), 1024, 80, 22050, 0.0, None)
    # still usable after the refusals
    ok = mp.spectrogram_torch(a, 64, 22050, 16, 64)
    torch.cuda.synchronize()
    assert torch.isfinite(ok).all()
