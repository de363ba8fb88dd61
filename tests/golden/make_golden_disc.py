#!/usr/bin/env python3
"""Generates the discriminator golden vectors (tests/golden/disc_*.npz) by running the REAL reference's
MultiPeriodDiscriminator (model/discriminators.py, imported unmodified through oracle/ref_import.py) and its losses.py
(feature_loss, discriminator_loss, generator_loss; `transformers`, which that module imports at its top for another
loss, is stubbed) under no_grad and eval, on the seeded synthetic checkpoint of
synth.make_discriminator_state_dict.  Run in the build container only:

    python tests/golden/make_golden_disc.py

One fixture per shape of disc_oracle.FIXTURE_SHAPES.  The weights are 187 MB, so a fixture holds their seed and the
sha256 of the generated state_dict's bytes (keys in order, each tensor's float32 bytes) instead.  Stored: y, y_hat, the
twelve discriminator outputs, the 37 per-layer mean |r - g|, the scalar losses with their per-discriminator terms, and
one whole feature map, fmap_rs[5][0] (period 11, layer 0)."""
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests import disc_oracle as do  # noqa: E402


def state_dict_digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().to(torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()


def import_reference():
    ref_import.install_stubs()
    if "transformers" not in sys.modules:  # never the real one: its import probes torchaudio, which is a stub here
        m = types.ModuleType("transformers")
        m.AutoModel = None
        sys.modules["transformers"] = m
    if ref_import.REF_VITS not in sys.path:
        sys.path.insert(0, ref_import.REF_VITS)
    from model.discriminators import MultiPeriodDiscriminator
    import losses
    return MultiPeriodDiscriminator, losses


def build_reference(sd):
    MPD, losses = import_reference()
    net = MPD(False)
    net.load_state_dict(sd)
    return net.eval(), losses


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
    sd, _, _ = do.weights()
    digest = state_dict_digest(sd)
    net, losses = build_reference(sd)
    for B, T in do.FIXTURE_SHAPES:
        y, y_hat = do.inputs(B, T, do.case_seed(B, T))
        y_d_rs, y_d_gs, fmap_rs, fmap_gs, sc = run_reference(net, losses, y, y_hat)
        out = dict(sc, y=y.numpy(), y_hat=y_hat.numpy(), weight_seed=do.WSEED, state_dict_sha256=digest,
                   fmap_r_5_0=fmap_rs[5][0].numpy())
        for d in range(6):
            out[f"y_d_r_{d}"] = y_d_rs[d].numpy()
            out[f"y_d_g_{d}"] = y_d_gs[d].numpy()
        path = os.path.join(HERE, f"disc_b{B}x{T}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
