#!/usr/bin/env python3
"""Voice conversion throughput (GPU box only): SynthesizerTrn.voice_conversion on HiFi-GAN v1 with the 218-row
AISHELL-3 speaker table (BASELINE.json configs[3]), synthetic weights and a synthetic linear spectrogram, B x Ty frames
(default 16 x 768: the decoder work of the headline step).  After a warm-up, device events time the whole call and its
two parts: posterior encoder + forward flow + reverse flow, and the decoder.  Prints one JSON line.
--from-audio starts from B waveforms of Ty * 256 samples at 22050 Hz instead: the call is then
wetts_amd.mel_processing.spectrogram_torch (1024 / 256 / 1024, the recipe's) followed by voice_conversion, and the
spectrogram is timed as a part of its own, with its GEMM FLOPs and the fraction of the f32 MFMA peak they reach.
    python tools/bench_vc.py [--batch 16] [--frames 768] [--steps 10] [--warmup 3] [--from-audio]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wetts_amd import SynthesizerTrn, _lib, config, mel_processing, synth  # noqa: E402

SPEC = 513
N_FFT, HOP, WIN, SR = 1024, 256, 1024, 22050
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X, v_mfma_f32_32x32x2_f32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=768)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--from-audio", action="store_true", help="time spectrogram_torch + voice_conversion from waveforms")
    a = ap.parse_args()
    B, Ty, n_spk = a.batch, a.frames, 218
    cfg = config.make_config(dict(config.MODEL_CONFIGS["v1"]), 256, n_spk)
    sd = dict(synth.make_state_dict(cfg, 35), **synth.make_posterior_state_dict(cfg, SPEC, 36))
    net = SynthesizerTrn(256, SPEC, 32, n_speakers=n_spk, **config.MODEL_CONFIGS["v1"]).load_state_dict(sd).to("cuda")
    gen = torch.Generator().manual_seed(0)
    y = (torch.rand(B, SPEC, Ty, generator=gen) ** 4 * 20.0).cuda()  # heavy-tailed magnitudes, like a spectrogram
    yl = torch.full((B,), Ty, dtype=torch.long).cuda()
    ss = torch.randint(0, n_spk, (B,), generator=gen).cuda()
    st = torch.randint(0, n_spk, (B,), generator=gen).cuda()
    eps = torch.randn(B, cfg.inter_channels, Ty, generator=gen).cuda()
    if a.from_audio:  # a harmonic tone on a random f0 per row plus noise, in [-1, 1]
        t = torch.arange(Ty * HOP, dtype=torch.float64) / SR
        f0 = 100.0 + 150.0 * torch.rand(B, 1, generator=gen, dtype=torch.float64)
        wav = sum(torch.sin(2 * torch.pi * k * f0 * t) / k for k in range(1, 9))
        wav = wav + 0.05 * torch.randn(B, Ty * HOP, generator=gen, dtype=torch.float64)
        audio = (0.9 * wav / wav.abs().amax(dim=1, keepdim=True)).float().cuda()

        def spec():
            s, sl = mel_processing.spectrogram_torch(audio, N_FFT, SR, HOP, WIN, lengths=[Ty * HOP] * B)
            assert s.shape == (B, SPEC, Ty)
            return s, sl

        y, _ = spec()

    def call():
        if a.from_audio:
            ys, ysl = spec()
            return net.voice_conversion(ys, ysl, ss, st, eps_q=eps)
        return net.voice_conversion(y, yl, ss, st, eps_q=eps)
    lib = _lib.load()
    I = cfg.inter_channels

    def stages():
        """voice_conversion's launches, split at the decoder (same calls as the method, events in between)."""
        nws = max(int(lib.wetts_posterior_workspace_bytes(net._handle, B, Ty)),
                  int(lib.wetts_workspace_bytes(net._handle, B, 0, Ty)))
        ws = net._ws.get(nws, net.device)
        g = net._speaker(torch.cat([ss, st]), 2 * B).view(2, B, -1)
        z, m_q, logs_q = (torch.empty(B, I, Ty, device="cuda") for _ in range(3))
        y_mask = torch.empty(B, Ty, device="cuda")
        _lib.check(lib.wetts_posterior_encoder(net._handle, _lib.ptr(y), _lib.ptr(yl), _lib.ptr(g[0]), _lib.ptr(eps), B,
                                               Ty, _lib.ptr(z), None, None, _lib.ptr(y_mask), _lib.ptr(ws), nws,
                                               _lib.current_stream_ptr()), "posterior_encoder")
        z_p = net._flow_pass(z, y_mask, g[0], False, ws, nws)
        z_hat = net._flow_pass(z_p, y_mask, g[1], True, ws, nws)
        return z_hat, g[1], y_mask

    call()  # uploads the posterior encoder
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(a.steps):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    call_ms = ev[0].elapsed_time(ev[1]) / a.steps
    enc_ms = dec_ms = 0.0
    for _ in range(a.steps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        z_hat, g_tgt, y_mask = stages()
        e[1].record()
        net._decode(z_hat, g_tgt, y_mask, Ty)
        e[2].record()
        torch.cuda.synchronize()
        enc_ms += e[0].elapsed_time(e[1]) / a.steps
        dec_ms += e[1].elapsed_time(e[2]) / a.steps
    extra = {}
    if a.from_audio:
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        for _ in range(a.steps):
            mel_processing.spectrogram_torch(audio, N_FFT, SR, HOP, WIN, lengths=[Ty * HOP] * B)
        e[1].record()
        torch.cuda.synchronize()
        spec_ms = e[0].elapsed_time(e[1]) / a.steps
        flops = 2.0 * N_FFT * WIN * Ty * B  # the basis GEMM: n_fft rows x win columns x frames
        extra = dict(from_audio=True, spectrogram_ms=round(spec_ms, 4), spectrogram_gflop=round(flops / 1e9, 2),
                     spectrogram_f32_peak_fraction=round(flops / (spec_ms * 1e-3) / (F32_MFMA_PEAK_TFLOPS * 1e12), 3),
                     spectrogram_share=round(spec_ms / call_ms, 4))
    samples = B * Ty * net.hop_length
    print(json.dumps(dict(tool="bench_vc", model="v1", n_speakers=n_spk, batch=B, frames=Ty, steps=a.steps,
                          ms_per_call=round(call_ms, 3), samples_per_s=round(samples / (call_ms * 1e-3), 1),
                          posterior_flow_ms=round(enc_ms, 3), decoder_ms=round(dec_ms, 3),
                          posterior_flow_share=round(enc_ms / (enc_ms + dec_ms), 4), **extra,
                          device=torch.cuda.get_device_name())))


if __name__ == "__main__":
    main()
