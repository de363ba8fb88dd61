#!/usr/bin/env python3
"""Generates the MPMRD golden vectors (tests/golden/mrd_*.npz) by running the REAL reference's
MultiPeriodMultiResolutionDiscriminator (model/discriminators.py, imported unmodified through oracle/ref_import.py) and
its losses.py under no_grad and eval, on the seeded synthetic checkpoint of synth.make_mrd_state_dict.  Run in the build
container only:

    python tests/golden/make_golden_mrd.py

torchaudio is not installed, and oracle/ref_import.py stubs torchaudio.transforms.Spectrogram as a raiser.  This script
therefore installs a torchaudio stub of its own BEFORE install_stubs() (which leaves a module that is already present
alone).  Its Spectrogram is the ONE non-reference piece of these vectors: torchaudio's class with the arguments
DiscriminatorR gives it (n_fft, hop_length, win_length, power=None) and its defaults otherwise is exactly
torch.stft(x, n_fft, hop_length, win_length, window=torch.hann_window(win_length), center=True, pad_mode="reflect",
normalized=False, onesided=True, return_complex=True).  InverseSpectrogram is ref_import's own stand-in.

One fixture per shape of mrd_oracle.FIXTURE_SHAPES.  A fixture holds the weights' seed and the sha256 of the generated
state_dict's bytes instead of the 170 MB of weights.  Stored: y, y_hat, the sixteen discriminator outputs, the 93
per-layer mean |r - g|, the scalar losses with their per-discriminator terms, and one whole band map, fmap_rs[2][1]
(window 512, band 0, layer 2)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests import mrd_oracle as mo  # noqa: E402
from tests.golden.make_golden_disc import state_dict_digest  # noqa: E402


class _Spectrogram:
    """torchaudio.transforms.Spectrogram(n_fft, hop_length, win_length, power=None) with that class's defaults."""

    def __init__(self, n_fft=400, win_length=None, hop_length=None, power=2.0, **kw):
        assert power is None and not kw, (power, kw)
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2

    def __call__(self, x):
        return torch.stft(x, self.n_fft, self.hop_length, self.win_length, window=torch.hann_window(self.win_length),
                          center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)


def install_torchaudio_stub():
    """Puts the stub in place of a missing torchaudio or of ref_import's own stub (never of a real installation), and,
    where another importer in this process got model.discriminators first, rebinds the raiser that module took from
    ref_import's stub: the same stand-in, installed late."""
    have = sys.modules.get("torchaudio")
    assert have is None or getattr(have, "__file__", None) is None, "a real torchaudio is installed: use it instead"
    ta = types.ModuleType("torchaudio")
    tr = types.ModuleType("torchaudio.transforms")
    tr.Spectrogram = _Spectrogram
    tr.InverseSpectrogram = ref_import._InverseSpectrogram
    tr.MelSpectrogram = ref_import._raiser("MelSpectrogram")
    tr.Resample = ref_import._raiser("Resample")
    ta.transforms = tr
    sys.modules["torchaudio"] = ta
    sys.modules["torchaudio.transforms"] = tr
    md = sys.modules.get("model.discriminators")
    if md is not None and getattr(md, "Spectrogram", None) is not _Spectrogram:
        md.Spectrogram = _Spectrogram


def import_reference():
    install_torchaudio_stub()
    ref_import.install_stubs()
    if "transformers" not in sys.modules:  # never the real one: its import probes torchaudio, which is a stub here
        m = types.ModuleType("transformers")
        m.AutoModel = None
        sys.modules["transformers"] = m
    if ref_import.REF_VITS not in sys.path:
        sys.path.insert(0, ref_import.REF_VITS)
    from model.discriminators import MultiPeriodMultiResolutionDiscriminator
    import losses
    return MultiPeriodMultiResolutionDiscriminator, losses


def run_reference(net, losses, y, y_hat):
    with torch.no_grad():
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = net(y, y_hat)
        loss_disc, r_losses, g_losses = losses.discriminator_loss(y_d_rs, y_d_gs)
        loss_gen, gen_losses = losses.generator_loss(y_d_gs)
        loss_fm = losses.feature_loss(fmap_rs, fmap_gs)
        layer_means = [torch.mean(torch.abs(r - g)) for dr, dg in zip(fmap_rs, fmap_gs) for r, g in zip(dr, dg)]
    return y_d_rs, y_d_gs, fmap_rs, fmap_gs, dict(
        loss_disc=float(loss_disc), losses_disc_r=np.asarray(r_losses, np.float32),
        losses_disc_g=np.asarray(g_losses, np.float32), loss_gen=float(loss_gen),
        losses_gen=np.asarray([float(v) for v in gen_losses], np.float32), loss_fm=float(loss_fm),
        layer_means=np.asarray([float(v) for v in layer_means], np.float32))


def main():
    sd, _, _ = mo.weights()
    digest = state_dict_digest(sd)
    MPMRD, losses = import_reference()
    net = MPMRD(False)
    net.load_state_dict(sd)
    net.eval()
    for B, T in mo.FIXTURE_SHAPES:
        y, y_hat = mo.inputs(B, T, mo.case_seed(B, T))
        y_d_rs, y_d_gs, fmap_rs, fmap_gs, sc = run_reference(net, losses, y, y_hat)
        assert len(y_d_rs) == 8 and sum(len(f) for f in fmap_rs) == mo.N_MAPS
        out = dict(sc, y=y.numpy(), y_hat=y_hat.numpy(), weight_seed=mo.WSEED, state_dict_sha256=digest,
                   fmap_r_2_1=fmap_rs[2][1].numpy())
        for d in range(8):
            out[f"y_d_r_{d}"] = y_d_rs[d].numpy()
            out[f"y_d_g_{d}"] = y_d_gs[d].numpy()
        path = os.path.join(HERE, f"mrd_b{B}x{T}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
