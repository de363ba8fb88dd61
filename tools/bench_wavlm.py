#!/usr/bin/env python3
"""WavLM loss timing (GPU box only): losses.WavLMLoss at the Baker v1 recipe's training shape -- wavlm-base-plus
dimensions, 13 hidden states, 16 real + 16 generated rows of 8192 samples at 22050 Hz, synthetic weights.  After a
warm-up, device events time every repeat on its own and the MEDIAN is reported: the three terms of a step from one pass
(all_terms), each of the reference's three methods, and -- through the stand-alone stage entries, on the pass's own
tensors -- the resampler, conv 0 with its normalisation, the six strided convs (with their share of the f32 MFMA peak,
from the layer shapes), projection + positional conv, the twelve encoder layers, the discriminator and the reductions.
Next to it the same network as tests/wavlm_oracle.py states it in torch, in float32 on the same device and weights.
Prints one JSON line.
    python tools/bench_wavlm.py [--steps 10] [--warmup 3] [--out profiles/wavlm_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import wavlm_oracle as wo  # noqa: E402
from wetts_amd import _lib, discriminators, losses, synth, wavlm  # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X, v_mfma_f32_32x32x2_f32
BASE_PLUS = dict(wo.HF_CONFIGS["wide"], intermediate_size=3072, num_hidden_layers=12, num_buckets=320, max_bucket_distance=800)


def timed(fn, steps, warmup):
    """Median ms of `steps` repeats, each between its own pair of events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    B, L, rate = 16, 8192, 22050
    cfg = BASE_PLUS
    sd = synth.make_wavlm_state_dict(cfg, 31)
    dd = synth.make_wavlm_discriminator_state_dict(768, 13, 64, 32)
    net = wavlm.WavLM(cfg).load_state_dict(sd).to("cuda")
    wd = discriminators.WavLMDiscriminator(768, 13, 64).load_state_dict(dd).to("cuda")
    wl = losses.WavLMLoss(net, wd, rate)
    gen = torch.Generator().manual_seed(0)
    y = (0.3 * torch.randn(B, L, generator=gen)).cuda()
    y_hat = y + (0.1 * torch.randn(B, L, generator=gen)).cuda()
    t = lambda fn: round(timed(fn, a.steps, a.warmup), 4)  # noqa: E731

    all_ms = t(lambda: wl.all_terms(y, y_hat))
    call_ms, gen_ms, disc_ms = t(lambda: wl(y, y_hat)), t(lambda: wl.generator(y_hat)), t(lambda: wl.discriminator(y, y_hat))

    # the stages, on the pass's own tensors
    lib, h, s, P = _lib.load(), net._handle, _lib.current_stream_ptr, _lib.ptr
    both = torch.cat([y, y_hat], 0)
    R = 2 * B
    x16 = wl.resample(both).contiguous()
    L16 = x16.shape[1]
    new = lambda *shp: torch.empty(*shp, dtype=torch.float32, device="cuda")  # noqa: E731
    lens = [L16]
    for k, st in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        lens.append((lens[-1] - k) // st + 1)
    feats = [new(R, n, 512) for n in lens[1:]]
    _lib.check(lib.wetts_wavlm_conv0(h, P(x16), L16, R, L16, P(feats[0]), s()), "conv0")

    def convs():
        for i in range(1, 7):
            _lib.check(lib.wetts_wavlm_conv(h, i, P(feats[i - 1]), R, lens[i], P(feats[i]), s()), "conv")

    convs()
    T = lens[-1]
    normed, proj, pos = new(R, T, 512), new(R, T, 768), new(R, T, 768)

    def project_pos():
        _lib.check(lib.wetts_wavlm_project(h, P(feats[-1]), R * T, P(normed), P(proj), s()), "project")
        _lib.check(lib.wetts_wavlm_pos_conv(h, P(proj), R, T, P(pos), s()), "pos_conv")

    hidden = net._hidden(x16)
    ws = new(int(lib.wetts_wavlm_layer_workspace_bytes(h, R, T)) // 4)
    out = new(R, T, 768)

    def layers():
        for i in range(12):
            _lib.check(lib.wetts_wavlm_layer(h, i, P(hidden[i]), R, T, P(out), P(ws), s()), "layer")

    d = wd.on_hidden(hidden)

    def reduce():
        wl._lm(hidden, B)
        losses.discriminator_loss([d[:B]], [d[B:]], per_utterance=True)
        losses.generator_loss([d[B:]], per_utterance=True)

    conv_flops = sum(2.0 * R * lens[i + 1] * 512 * 512 * cfg["conv_kernel"][i] for i in range(1, 7))
    convs_ms = t(convs)

    # the oracle's torch restatement, float32, same device and weights
    wo.HF_CONFIGS["base_plus"] = cfg
    W = {k: v.cuda() for k, v in sd.items()}
    D = {k: v.cuda() for k, v in dd.items()}

    def torch_all():
        with torch.no_grad():
            hs = wo.hidden_states(W, "base_plus", wo.resample(both, rate, wo.SLM_SR, torch.float32))
            return wo.losses(hs, wo.disc(D, hs), B)

    torch_ms = t(torch_all)
    ref, got = torch_all(), wl.all_terms(y, y_hat)
    agree = {k: round(abs(float(got[k]) - float(ref[k])) / abs(float(ref[k])), 9) for k in ("loss_lm", "loss_lm_gen", "loss_slm")}

    line = dict(tool="bench_wavlm", shape="16+16x8192@22050", rows=R, samples=L, frames=T, steps=a.steps, statistic="median",
                all_terms_ms_per_call=all_ms, call_ms=call_ms, generator_ms=gen_ms, discriminator_ms=disc_ms,
                resample_ms=t(lambda: wl.resample(both)),
                conv0_norm_ms=t(lambda: _lib.check(lib.wetts_wavlm_conv0(h, P(x16), L16, R, L16, P(feats[0]), s()), "conv0")),
                strided_convs_ms=convs_ms, strided_convs_gflop=round(conv_flops / 1e9, 2),
                strided_convs_f32_peak_fraction=round(conv_flops / (convs_ms * 1e-3) / (F32_MFMA_PEAK_TFLOPS * 1e12), 4),
                project_pos_conv_ms=t(project_pos), encoder_layers_ms=t(layers), discriminator_head_ms=t(lambda: wd.on_hidden(hidden)),
                reductions_ms=t(reduce), torch_restatement_ms=torch_ms, torch_over_hip=round(torch_ms / all_ms, 3),
                rel_diff_to_torch=agree, device=torch.cuda.get_device_name())
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
