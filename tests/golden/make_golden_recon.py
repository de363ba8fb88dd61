#!/usr/bin/env python3
"""Generates the teacher-forced reconstruction golden vectors (tests/golden/recon_*.npz), one for every case of
make_golden_align.CASES, by running the REAL reference's SynthesizerTrn.forward (models.py:161-226; imported unmodified
through oracle/ref_import.py) under no_grad and eval, its losses.kl_loss and, for the hop-256 cases, its
utils/mel_processing functions.  Run in the build container only, after make_golden_align.py:

    python tests/golden/make_golden_recon.py

Each case reuses the inputs and the stable noise seed recorded in align_<name>.npz, so the alignment path is the one
already proven stable.  torch.randn_like is patched by shape as there; torch.rand is patched by shape [B] and fed a
seeded `u` whose first two values are set by hand to 0 and 1 - 2^-24, which puts one row at id 0 and one at
len - segment.  The segment is 4 frames for the tiny configs and 8 for the two hop-256 cases (tests/recon_oracle.py).

Stored: u, ids_slice, z_slice, the decoder's audio `o`, loss_kl from the reference's losses.kl_loss on forward()'s own
tensors, kl_abs_mean = sum|kl * mask| / sum(mask) in float64 (the scale of the GPU test's gate), and for the hop-256
cases y_mel, y_hat_mel, loss_mel = F.l1_loss(y_mel, y_hat_mel) (train.py:402-432,486, librosa_mel_fn patched exactly as
make_golden_spec.py patches it) and loss_mel_shift1, the same loss with every id moved by one frame
(recon_oracle.shifted_ids).  The full-size case keeps its stage tensors sub-sampled, so it also stores loss_kl_sub, the
reference's kl_loss on the sub-sampled tensors the alignment fixture holds.

A mel fixture is only written if |loss_mel_shift1 - loss_mel| / loss_mel >= 10 * ro.MEL_GATE, the relative gate of
tests/test_gpu_recon.py (recon_oracle.MEL_GATE): that is what shows the gate can see an off-by-one slice.
"""
import contextlib
import io
import os
import sys
import unittest.mock as mock

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OUT, ROOT, build_reference  # noqa: E402
from make_golden_align import CASES, build_unconditioned_reference  # noqa: E402
from make_golden_spec import _librosa_mel  # noqa: E402

sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests import align_oracle as ao, recon_oracle as ro, util  # noqa: E402
from wetts_amd import config, synth  # noqa: E402

SPEC = ao.SPEC
ONLY = os.environ.get("WETTS_GOLDEN_ONLY")


def run_case(aname, spec, ref_losses, ref_commons, mp):
    mname, n_vocab, n_spk = spec[0], spec[1], spec[2]
    name = "recon_" + aname[len("align_"):]
    seg = ro.segment_of(name)
    c = ao.load_align_case(aname)
    cfg, sd, psd = util.vc_case_model(c, SPEC)
    full_sd = dict(sd, **psd)
    net = build_reference(mname, n_vocab, n_spk, full_sd) if n_spk > 0 else build_unconditioned_reference(mname, n_vocab,
                                                                                                          full_sd)
    net.segment_size = seg
    x, x_len, y, y_len, sid, eps = ao.case_tensors(c)
    B, I, Ty = eps.shape
    assert int(y_len.min()) >= seg
    u = np.random.RandomState(int(c["noise_seed"]) + 29).random_sample(B).astype(np.float32)
    assert B >= 2
    u[0], u[1] = 0.0, 1.0 - 2.0 ** -24
    real_randn_like, real_rand = torch.randn_like, torch.rand
    seen = {"randn_like": 0, "rand": 0}

    def fake_randn_like(t, **kw):
        if tuple(t.shape) == (B, I, Ty):  # encoders.py:98, the posterior draw
            seen["randn_like"] += 1
            return eps.clone()
        return real_randn_like(t, **kw)

    def fake_rand(*size, **kw):
        if len(size) == 1 and list(size[0]) == [B]:  # commons.py:54
            seen["rand"] += 1
            return torch.from_numpy(u.copy())
        return real_rand(*size, **kw)

    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()), \
            mock.patch.object(torch, "randn_like", fake_randn_like), mock.patch.object(torch, "rand", fake_rand):
        o, _, attn, ids_slice, x_mask, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q), _ = net.forward(
            x, x_len, y, y_len, sid if n_spk > 0 else None)
        loss_kl = ref_losses.kl_loss(z_p, logs_q, m_p, logs_p, y_mask)
    assert seen == {"randn_like": 1, "rand": 1}, seen
    assert np.array_equal(attn[:, 0].numpy().astype(np.uint8), c["attn"]), "forward() took another path than the fixture's"
    ids = ids_slice.numpy()
    want_ids, short = ro.slice_ids(u, y_len.numpy(), seg)
    assert not short.any() and np.array_equal(ids, want_ids), (ids, want_ids)
    assert ids[0] == 0 and ids[1] == int(y_len[1]) - seg, ids
    z_slice = ref_commons.slice_segments(z, ids_slice, seg).numpy()
    assert np.array_equal(z_slice, ro.slice_segments(z.numpy(), ids, seg))
    kl64 = ro.kl_loss(z_p.numpy(), logs_q.numpy(), m_p.numpy(), logs_p.numpy(), y_mask[:, 0].numpy())
    assert abs(kl64["total"] - float(loss_kl)) <= 1e-5 * kl64["abs_total"]
    out = dict(model=mname, noise_seed=int(c["noise_seed"]), segment=seg, u=u, ids_slice=ids, z_slice=z_slice,
               o=o.numpy(), loss_kl=np.float32(loss_kl), kl_abs_mean=np.float64(kl64["abs_total"]))
    if "sub_stride" in c:
        st = int(c["sub_stride"])
        with torch.no_grad():
            out["loss_kl_sub"] = np.float32(ref_losses.kl_loss(z_p[..., ::st], logs_q[..., ::st], m_p[..., ::st],
                                                               logs_p[..., ::st], y_mask[..., ::st]))
    msg = f"{name}: ids {ids.tolist()}  loss_kl {float(loss_kl):.6g}  mean|terms| {kl64['abs_total']:.6g}"
    if name in ro.MEL_CASES:
        assert o.shape[-1] == seg * ro.MEL["hop_length"]
        sr = config.SAMPLING_RATES[mname]
        M = ro.MEL
        mp.mel_basis.clear()
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()), mock.patch.object(mp, "librosa_mel_fn", _librosa_mel):
            mel = mp.spec_to_mel_torch(y.float(), M["filter_length"], M["n_mel_channels"], sr, M["mel_fmin"], M["mel_fmax"])
            y_mel = ref_commons.slice_segments(mel, ids_slice, seg)
            y_hat_mel = mp.mel_spectrogram_torch(o.squeeze(1).float(), M["filter_length"], M["n_mel_channels"], sr,
                                                 M["hop_length"], M["win_length"], M["mel_fmin"], M["mel_fmax"])
            loss_mel = F.l1_loss(y_mel, y_hat_mel)
            ids1 = torch.from_numpy(ro.shifted_ids(ids, y_len.numpy(), seg))
            loss_mel_shift1 = F.l1_loss(ref_commons.slice_segments(mel, ids1, seg), y_hat_mel)
        rel = abs(float(loss_mel_shift1) - float(loss_mel)) / float(loss_mel)
        msg += f"  loss_mel {float(loss_mel):.6g}  shift1 {float(loss_mel_shift1):.6g}  (rel {rel:.3g}, gate {ro.MEL_GATE:.3g})"
        if rel < 10 * ro.MEL_GATE:
            raise SystemExit(msg + "\nan off-by-one slice moves loss_mel by less than 10x the gate: fixture not written")
        out.update(y_mel=y_mel.numpy(), y_hat_mel=y_hat_mel.numpy(), loss_mel=np.float32(loss_mel),
                   loss_mel_shift1=np.float32(loss_mel_shift1), sampling_rate_mel=sr)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(msg, f" {os.path.getsize(path)} bytes")


def main():
    if not ref_import.available():
        raise SystemExit("reference tree not found")
    _, _, ref_commons, _ = ref_import.import_reference()
    # the reference's own wetts/vits/losses.py (ref_import put its directory on sys.path).  It imports
    # transformers.AutoModel for WavLMLoss, which kl_loss never touches and whose import trips over ref_import's
    # torchaudio stub: a stand-in module for the duration of the import
    import types
    stub = types.ModuleType("transformers")
    stub.AutoModel = None
    with mock.patch.dict(sys.modules, {"transformers": stub}):
        import losses as ref_losses
    from utils import mel_processing as mp
    for aname, spec in CASES.items():
        if ONLY and aname not in ONLY.split(","):
            continue
        run_case(aname, spec, ref_losses, ref_commons, mp)


if __name__ == "__main__":
    main()
