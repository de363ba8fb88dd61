#!/usr/bin/env python3
"""Generates the duration discriminator golden vectors (tests/golden/durdisc_v{1,2}_b{B}x{Tx}.npz) by running the REAL
reference's DurationDiscriminatorV1 / V2 (model/discriminators.py, imported unmodified through oracle/ref_import.py) and
its losses.py (discriminator_loss, generator_loss, called as train.py:441-453,481-495 calls them; `transformers`, which
that module imports at its top for another loss, is stubbed) under no_grad and eval, on the seeded synthetic checkpoint of
synth.make_duration_discriminator_state_dict.  Run in the build container only:

    python tests/golden/make_golden_durdisc.py

One fixture per version and shape of durdisc_oracle.FIXTURE_SHAPES.  Stored: the weight seed and the sha256 of the
generated state_dict's bytes, the input seed and the sha256 of the four input tensors' bytes, lens, both probability
tensors, and the three losses with their term lists AS THE REFERENCE'S ZIP PRODUCES THEM (B terms for V1, whose two
returned tensors it walks row by row; one for V2)."""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import durdisc_oracle as dd  # noqa: E402
from tests.golden.make_golden_disc import import_reference as _import_mpd, state_dict_digest  # noqa: E402


def inputs_digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().to(torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()


def import_reference():
    """(DurationDiscriminatorV1, DurationDiscriminatorV2, the reference's losses module)."""
    _, losses = _import_mpd()
    from model.discriminators import DurationDiscriminatorV1, DurationDiscriminatorV2
    return DurationDiscriminatorV1, DurationDiscriminatorV2, losses


def build_reference(version, sd):
    V1, V2, losses = import_reference()
    net = (V1 if version == 1 else V2)(dd.CHANNELS, dd.CHANNELS, dd.KERNEL, 0.1, gin_channels=0)
    net.load_state_dict(sd)
    return net.eval(), losses


def run_reference(net, losses, x, x_mask, dur_r, dur_hat):
    """train.py:442-452,482-494 -> (y_dur_hat_r, y_dur_hat_g as the class returns them, dict of the scalars)."""
    with torch.no_grad():
        y_r, y_g = net(x, x_mask, dur_r, dur_hat)
        loss_disc, r_losses, g_losses = losses.discriminator_loss(y_r, y_g)
        loss_gen, gen_losses = losses.generator_loss(y_g)
    return y_r, y_g, dict(loss_dur_disc=float(loss_disc), losses_dur_disc_r=np.asarray(r_losses, np.float32),
                          losses_dur_disc_g=np.asarray(g_losses, np.float32), loss_dur_gen=float(loss_gen),
                          losses_dur_gen=np.asarray([float(v) for v in gen_losses], np.float32))


def main():
    for version in dd.VERSIONS:
        sd = dd.weights(version)[0]
        digest = state_dict_digest(sd)
        net, losses = build_reference(version, sd)
        for B, Tx, lens in dd.FIXTURE_SHAPES:
            seed = dd.case_seed(B, Tx)
            inp = dd.inputs(B, Tx, lens, seed)
            y_r, y_g, sc = run_reference(net, losses, *inp)
            pr, pg = (y_r, y_g) if version == 1 else (y_r[0], y_g[0])
            out = dict(sc, weight_seed=dd.WSEED, state_dict_sha256=digest, input_seed=seed,
                       inputs_sha256=inputs_digest(inp), lens=np.asarray(lens, np.int64), prob_r=pr.numpy(),
                       prob_g=pg.numpy())
            path = os.path.join(HERE, f"durdisc_v{version}_b{B}x{Tx}.npz")
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path), "bytes", {k: np.asarray(v).shape for k, v in sc.items()})


if __name__ == "__main__":
    main()
