#!/usr/bin/env python3
"""Generates the spectrogram golden vectors by running the REAL reference's utils/mel_processing.py (imported unmodified
through oracle/ref_import.py) on seeded synthetic speech (tests/vc_input.py).  Run in the build container only:

    python tests/golden/make_golden_spec.py

  spec_kat.npz   spectrogram_torch for the recipes' 1024/256/1024 (center False and True), a short window (800 of
                 1024), a small n_fft (64/16/64) and lengths that are not multiples of hop, the shortest length torch
                 accepts among them.  One utterance per case: the audio is rebuilt from (seed, sampling rate, length).
  mel_kat.npz    mel_spectrogram_torch and spec_to_mel_torch at 22050 Hz / 80 mels, 24000 Hz / 100 mels (both
                 fmax=None, the VITS2 recipes) and 16000 Hz / 80 mels with fmin 55, fmax 7600, plus the filter bank.
  vc_vits2_v1_mel_b2.npz, vc_tiny_vits2_vocos_mel_b2.npz
                 the reference's voice_conversion of a model built with spec_channels = n_mel_channels (what
                 inference.py:68-71 builds for use_mel_posterior_encoder), fed the reference's mel spectrogram of the
                 seeded audio, one utterance at a time and zero-padded to the batch.

librosa is not installed here and oracle/ref_import.py stubs librosa.filters.mel as a raiser; utils.mel_processing
binds it at import as `librosa_mel_fn`, so that module attribute is patched with `_librosa_mel` below, written from
librosa's published definition (Slaney mel scale and area normalisation, float32 output).  It is the ONE non-reference
piece in these fixtures; the basis it produced is stored in mel_kat.npz.
"""
import contextlib
import io
import os
import sys
import unittest.mock as mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OUT, ROOT  # noqa: E402

sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests import vc_input  # noqa: E402
from tests.spec_oracle import utterance  # noqa: E402
from wetts_amd import checkpoint, config, synth  # noqa: E402


def _librosa_mel(sr, n_fft, n_mels=128, fmin=0.0, fmax=None, htk=False, norm="slaney", dtype=np.float32):
    """librosa.filters.mel (librosa/filters.py) for its defaults htk=False, norm="slaney": mel_frequencies on the
    Slaney scale (f_sp = 200/3 Hz per mel, logarithmic from 1 kHz with step log(6.4)/27), triangular ramps against
    fft_frequencies, weights assigned into a float32 array and scaled in place by enorm = 2 / (f[i+2] - f[i])."""
    assert not htk and norm == "slaney"
    if fmax is None:
        fmax = float(sr) / 2
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def hz_to_mel(f):
        f = np.asanyarray(f, dtype=np.float64)
        mels = f / f_sp
        if f.ndim:
            log_t = f >= min_log_hz
            mels[log_t] = min_log_mel + np.log(f[log_t] / min_log_hz) / logstep
        elif f >= min_log_hz:
            mels = min_log_mel + np.log(f / min_log_hz) / logstep
        return mels

    def mel_to_hz(mels):
        mels = np.asanyarray(mels, dtype=np.float64)
        freqs = f_sp * mels
        log_t = mels >= min_log_mel
        freqs[log_t] = min_log_hz * np.exp(logstep * (mels[log_t] - min_log_mel))
        return freqs

    weights = np.zeros((n_mels, int(1 + n_fft // 2)), dtype=dtype)
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]
    return weights


# (n_fft, hop, win, center, sampling rate, seed, length)
SPEC_CASES = [
    (1024, 256, 1024, 0, 22050, 11, 9000),
    (1024, 256, 1024, 1, 22050, 12, 9001),
    (1024, 256, 800, 0, 22050, 13, 7777),
    (1024, 256, 800, 1, 22050, 14, 6543),
    (64, 16, 64, 0, 16000, 15, 1003),
    (64, 16, 64, 1, 16000, 16, 517),
    (1024, 256, 1024, 0, 22050, 17, 385),   # the shortest: p + 1 = 385 (p = 384 must be < length)
    (1024, 256, 1024, 1, 22050, 18, 385),
    (64, 16, 64, 0, 16000, 19, 25),        # p + 1 = 25
    (64, 16, 48, 0, 16000, 20, 300),
]
# (sampling rate, n_mels, fmin, fmax, seed, length); n_fft / hop / win = 1024 / 256 / 1024
MEL_CASES = [(22050, 80, 0.0, None, 31, 12345), (24000, 100, 0.0, None, 32, 11111), (16000, 80, 55.0, 7600.0, 33, 9999)]
# name -> (model config, n_vocab, n_speakers, frames per utterance, sid_src, sid_tgt, weight seed, posterior seed,
#          noise seed); input seed = noise seed + 7; spec channels = n_mels of the config's sampling rate
VC_MEL_CASES = {
    "vc_vits2_v1_mel_b2": ("vits2_v1", 64, 2, [29, 17], [0, 1], [1, 0], 81, 91, 101, 80),
    "vc_tiny_vits2_vocos_mel_b2": ("tiny_vits2_vocos", 40, 2, [33, 21], [1, 0], [0, 0], 82, 92, 102, 100),
}
N_FFT, HOP, WIN = vc_input.N_FFT, vc_input.HOP, vc_input.WIN


def vc_noise(seed, shape):
    return np.random.RandomState(int(seed)).standard_normal(shape).astype(np.float32)


def main():
    if not ref_import.available():
        raise SystemExit("reference tree not found")
    SynthesizerTrn, *_ = ref_import.import_reference()
    from utils import mel_processing as mp  # the reference's own module
    quiet = contextlib.redirect_stdout(io.StringIO())
    with mock.patch.object(mp, "librosa_mel_fn", _librosa_mel), quiet:
        out = {"cases": np.array(SPEC_CASES, dtype=np.int64)}
        for i, (n, h, w, c, sr, seed, length) in enumerate(SPEC_CASES):
            a = utterance(seed, sr, length)
            s = mp.spectrogram_torch(a.unsqueeze(0), n, sr, h, w, center=bool(c))
            out[f"spec_{i}"] = s[0].numpy()
        np.savez_compressed(os.path.join(OUT, "spec_kat.npz"), **out)

        out = {"cases": np.array([(sr, nm, fmin, -1.0 if fmax is None else fmax, seed, length)
                                  for sr, nm, fmin, fmax, seed, length in MEL_CASES])}
        for i, (sr, nm, fmin, fmax, seed, length) in enumerate(MEL_CASES):
            mp.mel_basis.clear()
            a = utterance(seed, sr, length).unsqueeze(0)
            mel = mp.mel_spectrogram_torch(a, N_FFT, nm, sr, HOP, WIN, fmin, fmax, center=False)
            spec = mp.spectrogram_torch(a, N_FFT, sr, HOP, WIN, center=False)
            mel2 = mp.spec_to_mel_torch(spec, N_FFT, nm, sr, fmin, fmax)
            assert torch.equal(mel, mel2)
            out[f"mel_{i}"] = mel[0].numpy()
            out[f"basis_{i}"] = _librosa_mel(sr=sr, n_fft=N_FFT, n_mels=nm, fmin=fmin, fmax=fmax)
        np.savez_compressed(os.path.join(OUT, "mel_kat.npz"), **out)

        for name, (mname, n_vocab, n_spk, frames, src, tgt, wseed, pseed, nseed, nm) in VC_MEL_CASES.items():
            sr = config.SAMPLING_RATES[mname]
            cfg = config.make_config(dict(config.MODEL_CONFIGS[mname]), n_vocab, n_spk)
            sd = synth.make_state_dict(cfg, wseed)
            psd = synth.make_posterior_state_dict(cfg, nm, pseed)
            net = SynthesizerTrn(n_vocab, nm, 32, n_speakers=n_spk, **config.MODEL_CONFIGS[mname]).eval()
            missing, unexpected = net.load_state_dict(dict(sd, **psd), strict=False)
            assert not unexpected, unexpected
            assert not [k for k in missing if k.startswith("enc_q.")]
            B, Ty = len(frames), max(frames)
            y = torch.zeros(B, nm, Ty)
            mp.mel_basis.clear()
            for b, a in enumerate(vc_input.utterances(frames, sr, nseed + 7)):
                m = mp.mel_spectrogram_torch(a.unsqueeze(0), N_FFT, nm, sr, HOP, WIN, 0.0, None, center=False)
                assert m.shape == (1, nm, frames[b]), m.shape
                y[b, :, :frames[b]] = m[0]
            y_len = torch.tensor(frames, dtype=torch.long)
            eps = torch.from_numpy(vc_noise(nseed, (B, cfg.inter_channels, Ty)))
            seen = {}

            def fake_randn_like(t, **kw):
                assert tuple(t.shape) == (B, cfg.inter_channels, Ty)
                seen["n"] = seen.get("n", 0) + 1
                return eps.clone()

            with torch.no_grad(), mock.patch.object(torch, "randn_like", fake_randn_like):
                o_hat, y_mask, (z, z_p, z_hat) = net.voice_conversion(y, y_len, torch.tensor(src), torch.tensor(tgt))
                g_src = net.emb_g(torch.tensor(src)).unsqueeze(-1)
                z2, m_q, logs_q, _ = net.enc_q(y, y_len, g=g_src)
            assert seen["n"] == 2 and torch.equal(z2, z)
            np.savez_compressed(
                os.path.join(OUT, name + ".npz"), model=mname, n_vocab=n_vocab, n_speakers=n_spk, weight_seed=wseed,
                posterior_seed=pseed, noise_seed=nseed, spec_channels=nm, sampling_rate=sr,
                blob_checksum=synth.blob_checksum(checkpoint.pack_blob(cfg, sd)),
                posterior_checksum=synth.blob_checksum(checkpoint.pack_posterior_blob(cfg, nm, psd)),
                input_seed=nseed + 7, y=y.numpy(), y_lengths=y_len.numpy(), sid_src=np.array(src),
                sid_tgt=np.array(tgt), y_mask=y_mask.numpy(), eps=eps.numpy(), audio=o_hat.numpy(), z=z.numpy(),
                m_q=m_q.numpy(), logs_q=logs_q.numpy(), z_p=z_p.numpy(), z_hat=z_hat.numpy())
    for f in ["spec_kat", "mel_kat"] + list(VC_MEL_CASES):
        print(f, os.path.getsize(os.path.join(OUT, f + ".npz")), "bytes")


if __name__ == "__main__":
    main()
