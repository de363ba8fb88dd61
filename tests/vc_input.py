"""Seeded voice-conversion input (test infrastructure): synthetic speech-like audio and its linear spectrogram.

The golden generator (tests/golden/make_golden_vc.py) feeds the reference the spectrogram its own
`utils.mel_processing.spectrogram_torch(audio, 1024, sr, 256, 1024)` computes, and checks there that `spectrogram()`
below gives the same tensor bit for bit.  The fixtures then need not carry the input: the tests rebuild it from
(frames, sampling rate, seed) and hold it to the float64 sums the fixture records."""
import numpy as np
import torch

SPEC = 513  # n_fft // 2 + 1 for the recipes' filter_length 1024
N_FFT, HOP, WIN = 1024, 256, 1024


def synth_audio(frames, sr, gen):
    """Speech-like test signal of frames * HOP samples: a harmonic series on a gliding f0 with two formant-like
    resonance weights, an amplitude envelope and a little noise, scaled into [-1, 1]."""
    n = frames * HOP
    t = torch.arange(n, dtype=torch.float64) / sr
    f0 = 110.0 + 120.0 * float(torch.rand(1, generator=gen))
    glide = f0 * (1.0 + 0.15 * torch.sin(2 * np.pi * 1.3 * t + 6.0 * float(torch.rand(1, generator=gen))))
    phase = 2 * np.pi * torch.cumsum(glide, 0) / sr
    formants = (500.0 + 400.0 * float(torch.rand(1, generator=gen)), 1500.0 + 800.0 * float(torch.rand(1, generator=gen)))
    x = torch.zeros(n, dtype=torch.float64)
    for k in range(1, 25):
        fk = k * f0
        if fk > sr / 2 - 200:
            break
        w = sum(np.exp(-((fk - f) / 250.0) ** 2) for f in formants) + 0.05 / k
        x += w * torch.sin(k * phase)
    env = 0.6 + 0.4 * torch.sin(2 * np.pi * 3.1 * t) ** 2
    x = x * env + 0.02 * torch.randn(n, generator=gen, dtype=torch.float64)
    x = 0.8 * x / x.abs().max()
    return x.to(torch.float32)


def spectrogram(audio):
    """Linear STFT magnitude [B, SPEC, frames] of float32 audio [B, samples]: reflect padding of (n_fft - hop) / 2 per
    side, Hann window, no centring, sqrt(re^2 + im^2 + 1e-6) -- the input convention of the VITS recipes."""
    p = (N_FFT - HOP) // 2
    a = torch.nn.functional.pad(audio.unsqueeze(1), (p, p), mode="reflect").squeeze(1)
    s = torch.stft(a, N_FFT, hop_length=HOP, win_length=WIN, window=torch.hann_window(WIN, dtype=audio.dtype),
                   center=False, normalized=False, onesided=True, return_complex=True)
    return torch.sqrt(torch.view_as_real(s).pow(2).sum(-1) + 1e-6)


def utterances(frames, sr, seed):
    """The audio of each utterance of a case, in batch order."""
    gen = torch.Generator().manual_seed(int(seed))
    return [synth_audio(int(fr), sr, gen) for fr in frames]


def make_input(frames, sr, seed):
    """y [B, SPEC, max(frames)]: each utterance's spectrogram, zero-padded to the batch's frame count."""
    y = torch.zeros(len(frames), SPEC, max(int(f) for f in frames))
    for b, a in enumerate(utterances(frames, sr, seed)):
        s = spectrogram(a.unsqueeze(0))[0]
        y[b, :, :s.shape[1]] = s
    return y


def input_sums(y):
    """(sum, sum of squares) in float64: what a fixture records of the input it was made with."""
    y64 = y.double()
    return float(y64.sum()), float(y64.pow(2).sum())
