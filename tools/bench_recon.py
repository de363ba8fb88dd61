#!/usr/bin/env python3
"""Teacher-forced scoring timing (GPU box only): wetts_amd.losses.teacher_forced_losses on HiFi-GAN v1 with the 218-row
AISHELL-3 speaker table, synthetic weights, synthetic spectrogram and token ids, at 16 x 128 phonemes x 768 frames
(v1's benched batch), segment 32 frames, every row full.  After a warm-up, device events time the whole call, then
reconstruct() and align() alone, and on the call's own device tensors each new stage: slice ids, the z slice, the
decoder on the slice, the target mel, its slice, the mel of the decoded slice, and the two reductions.  Prints one JSON
line.
    python tools/bench_recon.py [--steps 20] [--warmup 5] [--out profiles/recon_bench.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wetts_amd import SynthesizerTrn, commons, config, losses, mel_spectrogram_torch, spec_to_mel_torch, synth  # noqa: E402

SPEC = 513
MEL = dict(filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, mel_fmin=0.0, mel_fmax=None,
           sampling_rate=22050)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    for _ in range(steps):
        fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    n_spk, B, Tx, Ty, seg = 218, 16, 128, 768, 32
    cfg = config.make_config(dict(config.MODEL_CONFIGS["v1"]), 256, n_spk)
    sd = dict(synth.make_state_dict(cfg, 35), **synth.make_posterior_state_dict(cfg, SPEC, 36))
    net = SynthesizerTrn(256, SPEC, seg, n_speakers=n_spk, **config.MODEL_CONFIGS["v1"]).load_state_dict(sd).to("cuda")
    hps = config.HParams(data=MEL, model={}, train=dict(c_mel=45, c_kl=1.0))
    d = hps.data
    gen = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (B, Tx), generator=gen).cuda()
    xl = torch.full((B,), Tx, dtype=torch.long).cuda()
    y = (torch.rand(B, SPEC, Ty, generator=gen) ** 4 * 20.0).cuda()
    yl = torch.full((B,), Ty, dtype=torch.long).cuda()
    sid = torch.randint(0, n_spk, (B,), generator=gen).cuda()
    eps = torch.randn(B, cfg.inter_channels, Ty, generator=gen).cuda()
    total_ms = timed(lambda: losses.teacher_forced_losses(net, hps, x, xl, y, yl, sid=sid, eps_q=eps), a.steps, a.warmup)
    recon_ms = timed(lambda: net.reconstruct(x, xl, y, yl, sid=sid, eps_q=eps), a.steps, a.warmup)
    align_ms = timed(lambda: net.align(x, xl, y, yl, sid=sid, eps_q=eps), a.steps, a.warmup)
    lr = net._last_recon
    z, g, ids, z_slice, o = lr["z"], lr["g"], lr["ids_slice"], lr["z_slice"], lr["o"]
    mel = spec_to_mel_torch(y, d.filter_length, d.n_mel_channels, d.sampling_rate, d.mel_fmin, d.mel_fmax)
    y_mel = commons.slice_segments(mel, ids, seg)
    mel_args = (d.filter_length, d.n_mel_channels, d.sampling_rate, d.hop_length, d.win_length, d.mel_fmin, d.mel_fmax)
    y_hat_mel = mel_spectrogram_torch(o[:, 0], *mel_args)
    stages = dict(
        slice_ids_and_z_slice_ms=lambda: commons.rand_slice_segments(z, yl, seg),
        z_slice_ms=lambda: commons.slice_segments(z, ids, seg),
        decoder_on_slice_ms=lambda: net.hifigan(z_slice, g),
        target_mel_ms=lambda: spec_to_mel_torch(y, d.filter_length, d.n_mel_channels, d.sampling_rate, d.mel_fmin,
                                                d.mel_fmax),
        mel_slice_ms=lambda: commons.slice_segments(mel, ids, seg),
        mel_of_decoded_slice_ms=lambda: mel_spectrogram_torch(o[:, 0], *mel_args),
        l1_loss_ms=lambda: losses.l1_loss(y_mel, y_hat_mel, per_utterance=True),
        kl_loss_ms=lambda: losses.kl_loss(lr["z_p"], lr["logs_q"], lr["m_p"], lr["logs_p"], lr["y_mask"],
                                          per_utterance=True))
    line = dict(tool="bench_recon", shape="v1_16x128x768_seg32", batch=B, phonemes=Tx, frames=Ty, segment=seg,
                steps=a.steps, teacher_forced_losses_ms_per_call=round(total_ms, 3),
                reconstruct_ms_per_call=round(recon_ms, 3), align_ms_per_call=round(align_ms, 3))
    for k, fn in stages.items():
        line[k] = round(timed(fn, a.steps, a.warmup), 4)
    line["device"] = torch.cuda.get_device_name()
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
