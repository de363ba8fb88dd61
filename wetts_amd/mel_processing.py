"""Spectrograms on the device: drop-ins for the inference side of the reference's utils/mel_processing.py
(spectrogram_torch, spec_to_mel_torch, mel_spectrogram_torch), computed by the HIP kernels of csrc/stft.hip through
include/wetts_hip.h, plus `posterior_spectrogram`, the input of SynthesizerTrn.voice_conversion for a given `hps`.

torch does plumbing only: device memory, the caller's stream, and the host-side frame count.  The STFT is a GEMM
against a window-folded DFT basis on the f32 matrix cores (built on the device, once per (n_fft, win, device)); the
mel filter bank is librosa.filters.mel's Slaney definition, built here in float64 and stored as float32 like librosa,
uploaded once per (sr, n_fft, n_mels, fmin, fmax, device) -- the reference's module-level `mel_basis` dict.

Differences from the reference, all deliberate:
  * the reference prints the minimum / maximum of `y` when they leave [-1, 1] (mel_processing.py:44-47); reading
    them back would cost a host synchronisation per call, so nothing is printed;
  * the optional keyword `lengths=` (valid samples per row) computes a ragged batch in one call: each utterance is
    padded at its own length and its frames past its own frame count are zeros -- the reference run one utterance at
    a time and zero-padded to the batch, as data_utils' collate builds a batch.  The call then returns
    (spec, spec_lengths).
"""
import numpy as np
import torch

from . import _lib

MAX_WAV_VALUE = 32768.0

mel_basis = {}   # (sr, n_fft, n_mels, fmin, fmax, device) -> [n_mels, n_fft // 2 + 1] float32 device tensor
stft_basis = {}  # (n_fft, win, device) -> packed window-folded DFT basis (wetts_stft_basis)


# ---- librosa.filters.mel (Slaney mel scale, Slaney area normalisation), host side ---------------------------------

_F_SP = 200.0 / 3           # Hz per mel below 1 kHz
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP
_LOGSTEP = np.log(6.4) / 27.0


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    m = f / _F_SP
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, 1e-300) / _MIN_LOG_HZ) / _LOGSTEP, m)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), _F_SP * m)


def mel_filter_bank(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
    """librosa.filters.mel(sr=sr, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax) with its defaults (htk=False,
    norm="slaney", dtype=float32): triangles on n_mels + 2 points equally spaced in Slaney mel between fmin and fmax
    (None = sr / 2), evaluated at the rfft bin frequencies in float64, stored into float32 and scaled in place by
    2 / (f[i + 2] - f[i]), the same two roundings librosa makes.  Returns a numpy float32 [n_mels, n_fft // 2 + 1]."""
    if fmax is None:
        fmax = float(sr) / 2
    nb = 1 + int(n_fft) // 2
    weights = np.zeros((int(n_mels), nb), dtype=np.float32)
    fftfreqs = np.fft.rfftfreq(n=int(n_fft), d=1.0 / float(sr))
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(float(fmin)), _hz_to_mel(float(fmax)), int(n_mels) + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(int(n_mels)):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:int(n_mels) + 2] - mel_f[:int(n_mels)])
    weights *= enorm[:, np.newaxis]
    return weights


# ---- host-side shape rules ------------------------------------------------------------------------------------------

def reflect_pad(n_fft, hop_size):
    """Samples of reflect padding per side: int((n_fft - hop_size) / 2), as mel_processing.py:65 computes it."""
    return int((n_fft - hop_size) / 2)


def num_frames(length, n_fft, hop_size, center=False):
    """Frames of an utterance of `length` samples; raises RuntimeError where F.pad(reflect) / torch.stft raise, at the
    same lengths: the reflect pad must be smaller than the utterance (and, with center, torch's n_fft // 2 pad smaller
    than the padded one), and the padded utterance must hold at least one frame."""
    length = int(length)
    p = reflect_pad(n_fft, hop_size)
    if p > 0 and p >= length:
        raise RuntimeError(f"Argument #4: Padding size should be less than the corresponding input dimension, but got: "
                           f"padding ({p}, {p}) at dimension 2 of input [1, 1, {length}]")
    padded = length + 2 * p
    if center:
        c = n_fft // 2
        if c >= padded:
            raise RuntimeError(f"Argument #4: Padding size should be less than the corresponding input dimension, but "
                               f"got: padding ({c}, {c}) at dimension 2 of input [1, 1, {padded}]")
        padded += 2 * c
    if padded < n_fft:
        raise RuntimeError(f"stft: expected 0 < n_fft <= {padded}, but got n_fft={n_fft}")
    return 1 + (padded - n_fft) // hop_size


def _check_params(n_fft, hop_size, win_size):
    n_fft, hop_size, win_size = int(n_fft), int(hop_size), int(win_size)
    if n_fft < 4 or n_fft % 2:
        raise ValueError(f"n_fft must be even and >= 4, got {n_fft}")
    if not 1 <= hop_size <= n_fft:
        raise ValueError(f"hop_size must be in [1, n_fft={n_fft}], got {hop_size}")
    if not 1 <= win_size <= n_fft:
        raise ValueError(f"win_size must be in [1, n_fft={n_fft}], got {win_size}")
    return n_fft, hop_size, win_size


def _audio(y):
    if not torch.is_tensor(y):
        raise TypeError("y must be a torch tensor")
    if y.dim() != 2:
        raise ValueError(f"y must be [B, samples], got shape {tuple(y.shape)}")
    if y.device.type != "cuda":
        raise ValueError("y must be on a HIP device (there is no CPU path)")
    return y.to(dtype=torch.float32).contiguous()


def _lengths(lengths, y):
    """(host list, device int64 tensor) of per-row valid sample counts (one read-back if they live on the device)."""
    B, L = y.shape
    if torch.is_tensor(lengths):
        host = [int(v) for v in lengths.detach().to("cpu", torch.int64).reshape(-1).tolist()]
    else:
        host = [int(v) for v in lengths]
    if len(host) != B:
        raise ValueError(f"lengths has {len(host)} entries for a batch of {B}")
    for v in host:
        if v > L:
            raise ValueError(f"a length ({v}) exceeds the row length {L}")
    return host, torch.tensor(host, dtype=torch.int64, device=y.device)


def _stft_basis(n_fft, win_size, device):
    key = (n_fft, win_size, str(device))
    if key not in stft_basis:
        lib = _lib.load()
        n = int(lib.wetts_stft_basis_numel(n_fft, win_size))
        if n <= 0:
            raise _lib.WettsError(f"stft_basis_numel({n_fft}, {win_size}): {_lib.last_error()}")
        w = torch.empty(n, dtype=torch.float32, device=device)
        _lib.check(lib.wetts_stft_basis(n_fft, win_size, _lib.ptr(w), n, _lib.current_stream_ptr()), "stft_basis")
        stft_basis[key] = w
    return stft_basis[key]


def _mel_basis(sampling_rate, n_fft, num_mels, fmin, fmax, device):
    key = (sampling_rate, n_fft, num_mels, fmin, fmax, str(device))
    if key not in mel_basis:
        mel = mel_filter_bank(sampling_rate, n_fft, num_mels, fmin, fmax)
        mel_basis[key] = torch.from_numpy(mel).to(device)
    return mel_basis[key]


# ---- the reference's functions --------------------------------------------------------------------------------------

def spectrogram_torch(y, n_fft, sampling_rate, hop_size, win_size, center=False, *, lengths=None):
    """mel_processing.py:43-94: sqrt(re^2 + im^2 + 1e-6) of torch.stft(F.pad(y, p, "reflect"), n_fft, hop_size,
    win_size, hann_window(win_size), center) with p = int((n_fft - hop_size) / 2); y [B, samples] on the device,
    converted to float32.  Returns [B, n_fft // 2 + 1, frames] float32, or (spec, spec_lengths) when `lengths=` is
    given.  The reference's print of out-of-range min / max is not mirrored (it would need a host sync)."""
    del sampling_rate  # unused by the reference too (mel_processing.py:43)
    n_fft, hop_size, win_size = _check_params(n_fft, hop_size, win_size)
    y = _audio(y)
    B, L = y.shape
    if lengths is None:
        frames = [num_frames(L, n_fft, hop_size, center)] * B
        dev_len = None
    else:
        host, dev_len = _lengths(lengths, y)
        frames = [num_frames(v, n_fft, hop_size, center) for v in host]
    T = max(frames) if frames else 0
    spec = torch.empty(B, n_fft // 2 + 1, T, dtype=torch.float32, device=y.device)
    basis = _stft_basis(n_fft, win_size, y.device)
    _lib.check(_lib.load().wetts_spectrogram(_lib.ptr(y), _lib.ptr(dev_len), B, L, n_fft, hop_size, win_size,
                                             int(bool(center)), _lib.ptr(basis), T, _lib.ptr(spec),
                                             _lib.current_stream_ptr()), "spectrogram")
    if lengths is None:
        return spec
    return spec, torch.tensor(frames, dtype=torch.int64, device=y.device)


def spec_to_mel_torch(spec, n_fft, num_mels, sampling_rate, fmin, fmax, *, lengths=None):
    """mel_processing.py:97-111: log(clamp(mel_basis @ spec, 1e-5)) with librosa's Slaney filter bank.  spec
    [B, n_fft // 2 + 1, frames]; `lengths=` (frames per row) writes zeros past each row's frames."""
    if not torch.is_tensor(spec) or spec.dim() != 3:
        raise ValueError(f"spec must be [B, n_fft // 2 + 1, frames], got {getattr(spec, 'shape', type(spec))}")
    nb = int(n_fft) // 2 + 1
    if spec.shape[1] != nb:
        raise ValueError(f"spec has {spec.shape[1]} bins, n_fft={n_fft} gives {nb}")
    if spec.device.type != "cuda":
        raise ValueError("spec must be on a HIP device (there is no CPU path)")
    if int(num_mels) < 1:
        raise ValueError(f"num_mels must be >= 1, got {num_mels}")
    spec = spec.to(dtype=torch.float32).contiguous()
    B, _, T = spec.shape
    dev_len = None
    if lengths is not None:
        dev_len = (lengths if torch.is_tensor(lengths) else torch.tensor(lengths)).to(spec.device, torch.int64)
        if dev_len.numel() != B:
            raise ValueError(f"lengths has {dev_len.numel()} entries for a batch of {B}")
        dev_len = dev_len.contiguous()
    mel = _mel_basis(sampling_rate, int(n_fft), int(num_mels), fmin, fmax, spec.device)
    out = torch.empty(B, int(num_mels), T, dtype=torch.float32, device=spec.device)
    _lib.check(_lib.load().wetts_spec_to_mel(_lib.ptr(spec), _lib.ptr(mel), _lib.ptr(dev_len), B, nb, int(num_mels),
                                             T, _lib.ptr(out), _lib.current_stream_ptr()), "spec_to_mel")
    return out


def mel_spectrogram_torch(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False, *,
                          lengths=None):
    """mel_processing.py:114-: spec_to_mel_torch(spectrogram_torch(y, ...)).  Returns [B, num_mels, frames], or
    (mel, mel_lengths) when `lengths=` is given."""
    if lengths is None:
        spec = spectrogram_torch(y, n_fft, sampling_rate, hop_size, win_size, center)
        return spec_to_mel_torch(spec, n_fft, num_mels, sampling_rate, fmin, fmax)
    spec, spec_lengths = spectrogram_torch(y, n_fft, sampling_rate, hop_size, win_size, center, lengths=lengths)
    return spec_to_mel_torch(spec, n_fft, num_mels, sampling_rate, fmin, fmax, lengths=spec_lengths), spec_lengths


def posterior_spectrogram(audio, lengths, hps):
    """(y, y_lengths) for SynthesizerTrn.voice_conversion from waveforms `audio` [B, samples] in [-1, 1] with
    `lengths` valid samples per row: the mel spectrogram when hps.model.use_mel_posterior_encoder (the VITS2 recipes),
    else the linear one, with filter_length / hop_length / win_length / sampling_rate / n_mel_channels / mel_fmin /
    mel_fmax from hps.data and center=False -- what data_utils.get_audio feeds the posterior encoder."""
    d, m = hps.data, hps.model
    use_mel = "use_mel_posterior_encoder" in m.keys() and bool(m.use_mel_posterior_encoder)
    if use_mel:
        return mel_spectrogram_torch(audio, d.filter_length, d.n_mel_channels, d.sampling_rate, d.hop_length,
                                     d.win_length, d.mel_fmin, d.mel_fmax, center=False, lengths=lengths)
    return spectrogram_torch(audio, d.filter_length, d.sampling_rate, d.hop_length, d.win_length, center=False,
                             lengths=lengths)
