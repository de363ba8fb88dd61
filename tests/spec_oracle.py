"""Float64 restatement of the reference's utils/mel_processing.py inference side (test infrastructure only).

Written from the published definitions, not from the product code: the frames are cut from the reflect-padded signal
by index arithmetic and transformed with np.fft.rfft in float64; the mel filter bank is built per filter from the
Slaney mel scale (linear below 1 kHz at 200/3 Hz per mel, logarithmic above with step ln(6.4)/27) as explicit
triangles with peak 2 / (right edge - left edge) -- area normalisation -- evaluated at k * sr / n_fft."""
import math

import numpy as np


def utterance(seed, sr, length):
    """Seeded audio of `length` samples (float32 torch tensor): tests/vc_input.py's synthetic speech, cut to length."""
    from tests import vc_input
    frames = -(-int(length) // vc_input.HOP)
    return vc_input.utterances([frames], sr, seed)[0][:int(length)]


def _reflect(x, pad):
    """F.pad(mode="reflect") of a 1-D float64 array; pad < len(x) (the caller's rule)."""
    n = len(x)
    idx = np.arange(-pad, n + pad)
    idx = np.abs(idx)
    idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
    return x[idx]


def spectrogram(audio, n_fft, hop, win, center=False):
    """[n_fft // 2 + 1, frames] float64 magnitude of ONE utterance (1-D array)."""
    x = np.asarray(audio, dtype=np.float64)
    p = int((n_fft - hop) / 2)
    if p > 0:
        x = _reflect(x, p)
    if center:
        x = _reflect(x, n_fft // 2)
    frames = 1 + (len(x) - n_fft) // hop
    w = np.zeros(n_fft)
    left = (n_fft - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)  # periodic Hann
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    S = np.fft.rfft(x[idx] * w[None, :], axis=1)
    return np.sqrt(S.real ** 2 + S.imag ** 2 + 1e-6).T


def batch_spectrogram(utts, n_fft, hop, win, center=False):
    """[B, bins, max frames]: each utterance alone, zero-padded to the batch (data_utils' collate)."""
    specs = [spectrogram(u, n_fft, hop, win, center) for u in utts]
    T = max(s.shape[1] for s in specs)
    out = np.zeros((len(specs), n_fft // 2 + 1, T))
    for b, s in enumerate(specs):
        out[b, :, :s.shape[1]] = s
    return out, np.array([s.shape[1] for s in specs])


def slaney_hz_to_mel(f):
    return f * 3.0 / 200.0 if f < 1000.0 else 15.0 + math.log(f / 1000.0) * 27.0 / math.log(6.4)


def slaney_mel_to_hz(m):
    return m * 200.0 / 3.0 if m < 15.0 else 1000.0 * math.exp((m - 15.0) * math.log(6.4) / 27.0)


def mel_basis(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """[n_mels, n_fft // 2 + 1] float64 Slaney filter bank."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    lo, hi = slaney_hz_to_mel(float(fmin)), slaney_hz_to_mel(fmax)
    edges = [slaney_mel_to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    freqs = [k * sr / n_fft for k in range(n_fft // 2 + 1)]
    out = np.zeros((n_mels, len(freqs)))
    for m in range(n_mels):
        a, c, b = edges[m], edges[m + 1], edges[m + 2]
        peak = 2.0 / (b - a)
        for k, f in enumerate(freqs):
            if a < f < b:
                out[m, k] = peak * ((f - a) / (c - a) if f <= c else (b - f) / (b - c))
    return out


def log_mel(spec, basis):
    """log(max(basis @ spec, 1e-5)) in float64; spec [..., bins, frames]."""
    return np.log(np.maximum(np.einsum("mk,...kt->...mt", basis, spec), 1e-5))
