"""CPU tier of the spectrograms (wetts_amd/mel_processing.py): the float64 oracle (tests/spec_oracle.py) against the
reference's own mel_processing (tests/golden/spec_kat.npz, mel_kat.npz), the product's host-built mel filter bank
against the fixture's and against its defining properties, and the host frame-count / error rules against torch."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import spec_oracle, util
from tests.spec_oracle import utterance
from wetts_amd import mel_processing as mp

GOLDEN = util.GOLDEN
N_SPEC_CASES, N_MEL_CASES = 10, 3  # tests/golden/make_golden_spec.py: SPEC_CASES, MEL_CASES


def _kat(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_fixture_case_counts():
    assert len(_kat("spec_kat")["cases"]) == N_SPEC_CASES and len(_kat("mel_kat")["cases"]) == N_MEL_CASES


def mel_case(d, i):
    sr, nm, fmin, fmax, seed, length = d["cases"][i]
    return int(sr), int(nm), float(fmin), None if fmax < 0 else float(fmax), int(seed), int(length)


@pytest.mark.parametrize("i", range(N_SPEC_CASES))
def test_oracle_matches_reference_spectrogram(i):
    d = _kat("spec_kat")
    n, h, w, c, sr, seed, length = (int(v) for v in d["cases"][i])
    ref = d[f"spec_{i}"]
    got = spec_oracle.spectrogram(utterance(seed, sr, length).double().numpy(), n, h, w, bool(c))
    assert got.shape == ref.shape
    assert util.rel_rms(got, ref) < 1e-6
    assert np.abs(got - ref).max() < 1e-5 * util.rms(ref) * 10


@pytest.mark.parametrize("i", range(N_MEL_CASES))
def test_oracle_matches_reference_mel(i):
    d = _kat("mel_kat")
    sr, nm, fmin, fmax, seed, length = mel_case(d, i)
    ref = d[f"mel_{i}"]
    basis = spec_oracle.mel_basis(sr, 1024, nm, fmin, fmax)
    spec = spec_oracle.spectrogram(utterance(seed, sr, length).double().numpy(), 1024, 256, 1024)
    got = spec_oracle.log_mel(spec, basis)
    assert got.shape == ref.shape
    big = got > math.log(1e-4)  # at least 10x the clamp
    assert big.mean() > 0.5
    assert np.abs(got - ref)[big].max() < 1e-4
    clamped = (got == math.log(1e-5)) & (ref == np.float32(math.log(1e-5)))
    assert np.array_equal(got == math.log(1e-5), clamped)
    # the independently written float64 bank against the stand-in the fixture was made with
    assert np.abs(basis - d[f"basis_{i}"]).max() <= 2e-7 * np.abs(basis).max()


@pytest.mark.parametrize("i", range(N_MEL_CASES))
def test_product_mel_bank_equals_fixture(i):
    d = _kat("mel_kat")
    sr, nm, fmin, fmax, _, _ = mel_case(d, i)
    got = mp.mel_filter_bank(sr, 1024, nm, fmin, fmax)
    ref = d[f"basis_{i}"]
    assert got.dtype == np.float32 and got.shape == ref.shape == (nm, 513)
    # equal to float32 rounding: at most one ulp apart
    assert np.all(np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)) <= 1)


@pytest.mark.parametrize("sr,n_fft,nm,fmin,fmax", [(22050, 1024, 80, 0.0, None), (24000, 1024, 100, 0.0, None),
                                                  (16000, 512, 40, 80.0, 7000.0), (48000, 2048, 128, 0.0, None)])
def test_product_mel_bank_defining_properties(sr, n_fft, nm, fmin, fmax):
    W = mp.mel_filter_bank(sr, n_fft, nm, fmin, fmax).astype(np.float64)
    top = sr / 2 if fmax is None else fmax
    lo, hi = spec_oracle.slaney_hz_to_mel(fmin), spec_oracle.slaney_hz_to_mel(top)
    edges = [spec_oracle.slaney_mel_to_hz(lo + (hi - lo) * i / (nm + 1)) for i in range(nm + 2)]
    freqs = np.arange(n_fft // 2 + 1) * sr / n_fft
    for m in range(nm):
        a, c, b = edges[m], edges[m + 1], edges[m + 2]
        peak = 2.0 / (b - a)  # area normalisation: a triangle of base b - a and area 1
        tri = peak * np.clip(np.minimum((freqs - a) / (c - a), (b - freqs) / (b - c)), 0, None)
        assert np.abs(W[m] - tri).max() <= 1e-6 * peak, m  # vertices on the Slaney grid
        assert np.all(W[m][(freqs <= a) | (freqs >= b)] == 0)
        if (b - a) * n_fft / sr > 20:  # wide filters: the bins integrate the triangle's unit area
            assert abs(W[m].sum() * sr / n_fft - 1.0) < 0.02, m
    if fmax is None:
        assert np.array_equal(W.astype(np.float32), mp.mel_filter_bank(sr, n_fft, nm, fmin, sr / 2))
    # the Slaney scale itself: linear below 1 kHz, log step ln(6.4)/27 above
    assert spec_oracle.slaney_hz_to_mel(1000.0) == 15.0
    assert abs(mp._hz_to_mel(600.0) - 9.0) < 1e-12
    assert abs(mp._hz_to_mel(6400.0) - 42.0) < 1e-12
    assert abs(mp._mel_to_hz(42.0) - 6400.0) < 1e-9


def _torch_frames(L, n, h, center):
    y = torch.zeros(1, L)
    p = int((n - h) / 2)
    try:
        a = F.pad(y.unsqueeze(1), (p, p), mode="reflect").squeeze(1)
        return torch.stft(a, n, hop_length=h, win_length=n, window=torch.hann_window(n), center=center,
                          pad_mode="reflect", normalized=False, onesided=True, return_complex=True).shape[-1]
    except RuntimeError:
        return RuntimeError


@pytest.mark.parametrize("n,h", [(1024, 256), (1024, 255), (64, 16), (16, 16), (16, 4), (6, 1), (2048, 600)])
@pytest.mark.parametrize("center", [False, True])
def test_frame_count_and_error_boundaries_match_torch(n, h, center):
    p = int((n - h) / 2)
    lengths = set()
    for v in (p, h, n, n // 2, n - 2 * p, n // 2 - 2 * p):
        lengths.update(range(v - 2, v + 3))
    lengths.update(range(1, 4))
    for L in sorted(x for x in lengths if x >= 1):
        want = _torch_frames(L, n, h, center)
        try:
            got = mp.num_frames(L, n, h, center)
        except RuntimeError:
            got = RuntimeError
        assert got == want, (L, got, want)
