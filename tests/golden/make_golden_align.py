#!/usr/bin/env python3
"""Generates the forced-alignment golden vectors (tests/golden/align_*.npz) by running the REAL reference's
SynthesizerTrn.forward (models.py:161-226; imported unmodified through oracle/ref_import.py) under no_grad and eval on
seeded synthetic checkpoints, with a small segment_size; its audio slice, duration loss and slice ids are discarded.
Run in the build container only:

    python tests/golden/make_golden_align.py

Inputs: the spectrograms tests/vc_input.py rebuilds (as for voice conversion), seeded token ids, x_lengths <= y_lengths
on every row.  The posterior encoder's torch.randn_like draw (encoders.py:98) is injected by shape from numpy
RandomState(noise_seed); the tests regenerate it.  Stored: attn (uint8), w, the masks, the six stage tensors of
forward()'s fifth return value (sub-sampled by frame stride in the full-size case) and neg_cent, recomputed here from
the reference's own enc_p output and z_p with its expression of models.py:173-184 and checked to give forward()'s attn
(full-size case: every `stride`-th frame row; the tests rebuild the rest from the float64 oracle).

PATH STABILITY is a condition of a fixture.  A MAS path is a discrete function of the scores and flips at near-ties
under any f32 reordering, so a case is only written when eighteen searches agree: over (a) the float64 scores of the
float64 oracle stages, (b) the reference's f32 scores, and (c) sixteen copies of (a) with independent uniform noise of
amplitude 1e-4 * rms(neg_cent) -- the local-error gate of the stage tests.  A case that fails moves to another noise
seed (+1000); the seed used is recorded, with path_stable = 1.
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
from make_golden import OUT, ROOT, build_reference  # noqa: E402

sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from oracle import vits_oracle as vo  # noqa: E402
from tests import align_oracle as ao, util, vc_input  # noqa: E402
from wetts_amd import checkpoint, config, synth  # noqa: E402

SPEC = vc_input.SPEC
SEGMENT = 4  # frames of the decoder slice forward() draws; every utterance has at least this many

# name -> (model config, n_vocab, n_speakers, frames, x_lengths, sid, weight seed, posterior seed, noise seed,
#          frame stride of the sub-sampled full-size case or None); input seed = noise seed + 7, token seed = + 13
CASES = {
    "align_tiny_b3": ("tiny", 40, 3, [37, 20, 29], [12, 7, 9], [0, 1, 2], 151, 161, 171, None),
    "align_vits2_v1_b2": ("vits2_v1", 64, 2, [31, 18], [9, 6], [0, 1], 152, 162, 172, None),
    "align_tiny_preconv2_spk_b3": ("tiny_preconv2_spk", 40, 3, [26, 13, 33], [8, 5, 11], [2, 0, 1], 153, 163, 173, None),
    "align_tiny_mono_post_b2": ("tiny_mono_post", 40, 2, [41, 22], [10, 6], [0, 1], 154, 164, 174, None),
    "align_tiny_mono_inter_b3": ("tiny_mono_inter", 40, 3, [35, 10, 27], [12, 4, 9], [1, 2, 0], 155, 165, 175, None),
    "align_tiny_vocos_b2": ("tiny_vocos", 40, 2, [30, 17], [10, 6], [1, 0], 156, 166, 176, None),
    "align_tiny_dp_b2": ("tiny_dp", 40, 2, [28, 15], [9, 5], [1, 0], 157, 167, 177, None),  # use_sdp = False
    "align_tiny_nospk_b2": ("tiny", 40, 0, [25, 33], [7, 11], [0, 0], 158, 168, 178, None),  # n_speakers = 0: g = None
    # BASELINE.json configs[3]: AISHELL-3 v1, 4 x 128 phonemes x 600 frames, ragged in both, sids at both table ends
    "align_aishell3_b4x600": ("v1", 256, 218, [600, 411, 537, 128], [128, 57, 100, 33], [0, 217, 57, 3], 159, 169, 179,
                              48),
}
ONLY = os.environ.get("WETTS_GOLDEN_ONLY")
NOISY_COPIES = 16
MAX_SEEDS = 200  # noise seeds tried per case before giving up
LOCAL_GATE = 1e-4


def stable_paths(nc64, nc32, yl, xl, seed):
    """The eighteen searches of the module docstring -> (all equal, the float64 path)."""
    p64 = vo.maximum_path_numpy(nc64, yl, xl)
    if not np.array_equal(vo.maximum_path_numpy(nc32, yl, xl), p64):
        return False, p64
    valid = ao.valid_mask(xl, yl, nc64.shape[2], nc64.shape[1])
    amp = LOCAL_GATE * util.rms(nc64[valid])
    rs = np.random.RandomState(int(seed) + 99)
    for _ in range(NOISY_COPIES):
        noisy = nc64 + rs.uniform(-amp, amp, size=nc64.shape)
        if not np.array_equal(vo.maximum_path_numpy(noisy, yl, xl), p64):
            return False, p64
    return True, p64


def build_unconditioned_reference(mname, n_vocab, sd):
    """build_reference for n_speakers = 0: the reference still builds the speaker-conditioning layers of a config
    with gin_channels > 0 (dec.cond, dp.cond, the WN cond_layers), which a checkpoint without speakers does not carry
    and which are never applied when g is None (modules.py:68-70, decoders.py:66-67, duration_predictors.py:226-228)."""
    SynthesizerTrn, _, _, _ = ref_import.import_reference()
    with contextlib.redirect_stdout(io.StringIO()):
        net = SynthesizerTrn(n_vocab, SPEC, 32, n_speakers=0, **config.MODEL_CONFIGS[mname]).eval()
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    bad = [k for k in missing if not (k.startswith("dp.post_") or k.startswith("dp.flows.1.") or ".cond_layer." in k
                                      or k.startswith("dec.cond.") or k.startswith("dp.cond."))]
    assert not bad, bad
    return net


def run_case(name, spec):
    mname, n_vocab, n_spk, frames, xls, sids, wseed, pseed, nseed0, stride = spec
    sr = config.SAMPLING_RATES[mname]
    cfg = config.make_config(dict(config.MODEL_CONFIGS[mname]), n_vocab, n_spk)
    cd = util.cfg_dict(cfg)
    sd = synth.make_state_dict(cfg, wseed)
    psd = synth.make_posterior_state_dict(cfg, SPEC, pseed)
    blob = checkpoint.pack_blob(cfg, sd)
    pblob = checkpoint.pack_posterior_blob(cfg, SPEC, psd)
    full_sd = dict(sd, **psd)
    net = build_reference(mname, n_vocab, n_spk, full_sd) if n_spk > 0 else build_unconditioned_reference(mname, n_vocab,
                                                                                                          full_sd)
    net.segment_size = SEGMENT
    assert not net.use_noise_scaled_mas and not net.training
    W64 = util.vc_weights(cfg, sd, psd, torch.float64)
    B, Ty, Tx = len(frames), max(frames), max(xls)
    assert all(a <= b for a, b in zip(xls, frames)) and min(frames) >= SEGMENT
    y_len, x_len = torch.tensor(frames, dtype=torch.long), torch.tensor(xls, dtype=torch.long)
    sid = torch.tensor(sids, dtype=torch.long)
    I = cfg.inter_channels
    for attempt in range(MAX_SEEDS):
        nseed = nseed0 + 1000 * attempt
        y = vc_input.make_input(frames, sr, nseed + 7)
        x = torch.from_numpy(ao.align_tokens(nseed + 13, n_vocab, xls))
        eps = torch.from_numpy(ao.align_noise(nseed, (B, I, Ty)))
        real = torch.randn_like
        seen = {"n": 0}

        def fake_randn_like(t, **kw):
            if tuple(t.shape) == (B, I, Ty):  # encoders.py:98, the posterior draw; anything else is the real one
                seen["n"] += 1
                return eps.clone()
            return real(t, **kw)

        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()), \
                mock.patch.object(torch, "randn_like", fake_randn_like):
            _, _, attn, _, x_mask, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q), _ = net.forward(
                x, x_len, y, y_len, sid if n_spk > 0 else None)
            g = net.emb_g(sid).unsqueeze(-1) if n_spk > 0 else None
            _, m_px, logs_px, x_mask2 = net.enc_p(x, x_len, g=g)
            nc32 = ao.neg_cent_four_term(z_p, m_px, logs_px)  # the reference's expression on its own tensors
        assert seen["n"] == 1 and torch.equal(x_mask2, x_mask)
        attn_np = attn[:, 0].numpy()
        ref_path = vo.maximum_path_numpy(nc32.numpy(), y_len.numpy(), x_len.numpy())
        assert np.array_equal(ref_path, attn_np.astype(np.int32)), "recomputed scores do not give forward()'s path"
        st64 = ao.oracle_align(W64, cd, x, x_len, y, y_len, sid, eps)
        ok, p64 = stable_paths(st64["neg_cent"].numpy(), nc32.numpy(), y_len.numpy(), x_len.numpy(), nseed)
        print(f"{name}: noise seed {nseed} path stable: {ok}")
        if ok:
            break
    else:
        raise SystemExit(f"{name}: no stable seed found")
    assert np.array_equal(p64, attn_np.astype(np.int32))
    ao.check_monotonic(attn_np, xls, frames)
    w = attn.sum(2)
    out = dict(model=mname, n_vocab=n_vocab, n_speakers=n_spk, weight_seed=wseed, posterior_seed=pseed,
               noise_seed=nseed, input_seed=nseed + 7, token_seed=nseed + 13, spec_channels=SPEC, sampling_rate=sr,
               blob_checksum=synth.blob_checksum(blob), posterior_checksum=synth.blob_checksum(pblob),
               y_shape=np.array(y.shape), y_sums=np.array(vc_input.input_sums(y)), y_lengths=y_len.numpy(),
               x_lengths=x_len.numpy(), sid=sid.numpy(), path_stable=1, attn=attn_np.astype(np.uint8),
               w=w[:, 0].numpy(), x_mask=x_mask[:, 0].numpy(), y_mask=y_mask[:, 0].numpy())
    stages = dict(z=z, z_p=z_p, m_p=m_p, logs_p=logs_p, m_q=m_q, logs_q=logs_q)
    if stride:
        out["sub_stride"] = stride
        for k, v in stages.items():
            out[k + "_sub"] = v.numpy()[..., ::stride].copy()
        out["neg_cent_sub"] = nc32.numpy()[:, ::stride].copy()
    else:
        out.update({k: v.numpy() for k, v in stages.items()})
        out["neg_cent"] = nc32.numpy()
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path)} bytes  neg_cent rms {util.rms(nc32.numpy()):.1f}  w max {float(w.max()):.0f}")


def main():
    if not ref_import.available():
        raise SystemExit("reference tree not found")
    ref_import.import_reference()
    for name, spec in CASES.items():
        if ONLY and name not in ONLY.split(","):
            continue
        run_case(name, spec)


if __name__ == "__main__":
    main()
