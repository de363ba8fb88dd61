#!/usr/bin/env python3
"""MultiPeriodMultiResolutionDiscriminator timing (GPU box only): net_d(y, y_hat) and the three adversarial losses at the
vits2_vocos_v1 recipe's training shape, 16 utterances x 8192 samples (32 rows), synthetic weights.  After a warm-up,
device events time the whole forward pass, the three loss calls (93 feature maps), and -- on the call's own tensors,
through the stand-alone stage entries -- each kernel class of the three DiscriminatorR stacks: normalise, the complex
STFTs, the band convs (with their share of the f32 MFMA peak, from their algorithmic flops) and conv_post; the five
period stacks (with the host's allocation and launches) are the forward pass minus those stages (tools/bench_disc.py
splits their kernels).  Next to it the same three DiscriminatorR written with
torch.stft + torch.nn.functional.conv2d on the same device and weights (a restatement inside this tool), whole and its
band convs alone.  Prints one JSON line.
    python tools/bench_mrd.py [--steps 10] [--warmup 3] [--out profiles/mrd_bench.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wetts_amd import MultiPeriodMultiResolutionDiscriminator, _lib, checkpoint, losses, synth  # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X, v_mfma_f32_32x32x2_f32
WINDOWS = (2048, 1024, 512)
BANDS = ((0.0, 0.1), (0.1, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0))
LAYERS = ((2, 9, 1), (32, 9, 2), (32, 9, 2), (32, 9, 2), (32, 3, 1))  # Cin, kf, stride


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


def torch_spec_bands(x, w, window):
    """discriminators.py:189-200 on x [R, T] -> the five band tensors [R, 2, frames, F]."""
    x = x - x.mean(dim=-1, keepdim=True)
    x = 0.8 * x / (x.abs().max(dim=-1, keepdim=True)[0] + 1e-9)
    s = torch.stft(x, w, w // 4, w, window=window, center=True, pad_mode="reflect", normalized=False, onesided=True,
                   return_complex=True)
    s = torch.view_as_real(s).transpose(1, 3)
    nb = w // 2 + 1
    return [s[..., int(lo * nb):int(hi * nb)] for lo, hi in BANDS]


def torch_band_convs(W, r, bands):
    last = []
    for b, h in enumerate(bands):
        for l, (_, kf, sf) in enumerate(LAYERS):
            h = F.leaky_relu(F.conv2d(h, W[f"discriminators.{r}.band_convs.{b}.{l}.weight"],
                                      W[f"discriminators.{r}.band_convs.{b}.{l}.bias"], (1, sf), (1, kf // 2)), 0.1)
        last.append(h)
    return last


def torch_forward_r(W, x, windows):
    out = []
    for r, w in enumerate(WINDOWS):
        last = torch_band_convs(W, r, torch_spec_bands(x, w, windows[r]))
        out.append(F.conv2d(torch.cat(last, -1), W[f"discriminators.{r}.conv_post.weight"],
                            W[f"discriminators.{r}.conv_post.bias"], 1, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    B, T = 16, 8192
    sd = synth.make_mrd_state_dict(31)
    net = MultiPeriodMultiResolutionDiscriminator().load_state_dict(sd).to("cuda")
    W = {k: v.cuda() for k, v in checkpoint.fold_weight_norm(sd).items() if int(k.split(".")[1]) < 3}
    gen = torch.Generator().manual_seed(0)
    y = (0.5 * torch.randn(B, 1, T, generator=gen)).cuda()
    y_hat = y + (0.2 * torch.randn(B, 1, T, generator=gen)).cuda()
    R = 2 * B

    forward_ms = timed(lambda: net(y, y_hat), a.steps, a.warmup)
    out = net(y, y_hat)
    losses_ms = timed(lambda: (losses.discriminator_loss(out[0], out[1]), losses.generator_loss(out[1]),
                               losses.feature_loss(out[2], out[3])), a.steps, a.warmup)

    lib, h, s, P = _lib.load(), net._handle, _lib.current_stream_ptr, _lib.ptr
    yy = torch.cat([y, y_hat], 0).contiguous()
    norm = torch.empty(R, T, device="cuda")
    frames = [1 + T // (w // 4) for w in WINDOWS]
    widths = [[[lib.wetts_mrd_band_width(r, b, l) for l in range(6)] for b in range(5)] for r in range(3)]
    specs = [torch.empty(R, 2, w // 2 + 1, fr, device="cuda") for w, fr in zip(WINDOWS, frames)]
    layer = [[torch.empty(sum(R * 32 * frames[r] * widths[r][b][l + 1] for b in range(5)), device="cuda") for l in range(5)]
             for r in range(3)]
    posts = [torch.empty(R, 1, frames[r], sum(widths[r][b][5] for b in range(5)), device="cuda") for r in range(3)]

    def normalize():
        _lib.check(lib.wetts_mrd_normalize(P(yy), R, T, P(norm), s()), "normalize")

    def stft():
        for r in range(3):
            _lib.check(lib.wetts_mrd_spectrogram(h, r, P(norm), R, T, P(specs[r]), s()), "spectrogram")

    def band_convs():
        for r in range(3):
            for l in range(5):
                _lib.check(lib.wetts_mrd_band_conv(h, r, l, P(specs[r] if l == 0 else layer[r][l - 1]), R, frames[r],
                                                   P(layer[r][l]), s()), "band_conv")

    def conv_post():
        for r in range(3):
            _lib.check(lib.wetts_mrd_conv_post(h, r, P(layer[r][4]), R, frames[r], P(posts[r]), s()), "conv_post")

    normalize_ms = timed(normalize, a.steps, a.warmup)
    stft_ms = timed(stft, a.steps, a.warmup)
    band_ms = timed(band_convs, a.steps, a.warmup)
    post_ms = timed(conv_post, a.steps, a.warmup)
    flops = 0.0
    for r in range(3):
        for b in range(5):
            for l, (cin, kf, _) in enumerate(LAYERS):
                flops += 2.0 * R * frames[r] * widths[r][b][l + 1] * 32 * cin * 3 * kf

    windows = [torch.hann_window(w, device="cuda") for w in WINDOWS]
    with torch.no_grad():
        torch_ms = timed(lambda: torch_forward_r(W, yy[:, 0], windows), a.steps, a.warmup)
        bands = [torch_spec_bands(yy[:, 0], w, windows[r]) for r, w in enumerate(WINDOWS)]
        torch_band_ms = timed(lambda: [torch_band_convs(W, r, bands[r]) for r in range(3)], a.steps, a.warmup)
    r_ms = normalize_ms + stft_ms + band_ms + post_ms
    line = dict(tool="bench_mrd", shape="16x8192", batch=B, samples=T, steps=a.steps,
                forward_ms_per_call=round(forward_ms, 3), losses_ms_per_call=round(losses_ms, 3),
                normalize_ms=round(normalize_ms, 4), stft_ms=round(stft_ms, 4), band_convs_ms=round(band_ms, 3),
                conv_post_ms=round(post_ms, 4), period_stacks_and_host_ms=round(forward_ms - r_ms, 3),
                band_convs_tflop=round(flops / 1e12, 4),
                band_convs_f32_peak_fraction=round(flops / (band_ms * 1e-3) / (F32_MFMA_PEAK_TFLOPS * 1e12), 4),
                torch_discriminator_r_ms=round(torch_ms, 3), torch_band_convs_ms=round(torch_band_ms, 3),
                torch_band_convs_over_hip=round(torch_band_ms / band_ms, 3),
                torch_discriminator_r_over_hip=round(torch_ms / r_ms, 3), device=torch.cuda.get_device_name())
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
