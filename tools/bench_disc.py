#!/usr/bin/env python3
"""MultiPeriodDiscriminator timing (GPU box only): net_d(y, y_hat) and the three adversarial losses at the recipes'
training shape, 16 utterances x 8192 samples (32 rows), synthetic weights.  After a warm-up, device events time the
whole forward pass, the three loss calls, and -- on the call's own feature maps, through the stand-alone layer entries --
each kernel class: the reflect-pad + fold + conv 0 launches, the MFMA convs (with their share of the f32 MFMA peak, from
the layer shapes), the conv_post dot products and DiscriminatorS's grouped convs.  Next to it the same network written
with torch.nn.functional.conv1d / conv2d on the same device and weights (a restatement inside this tool).  Prints one
JSON line.
    python tools/bench_disc.py [--steps 10] [--warmup 3] [--out profiles/disc_bench.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wetts_amd import MultiPeriodDiscriminator, _lib, checkpoint, losses, synth  # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X, v_mfma_f32_32x32x2_f32
PERIODS = (2, 3, 5, 7, 11)
S_SPEC = ((1, 7, 1), (4, 20, 4), (4, 20, 16), (4, 20, 64), (4, 20, 256), (1, 2, 1))


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


def torch_forward(W, y, y_hat):
    """discriminators.py:76-124,241-254 on cat(y, y_hat) with F.conv1d / F.conv2d -> the 37 maps."""
    x0 = torch.cat([y, y_hat], 0)
    maps, x = [], x0
    for m, (stride, pad, groups) in enumerate(S_SPEC):
        x = F.leaky_relu(F.conv1d(x, W[f"discriminators.0.convs.{m}.weight"], W[f"discriminators.0.convs.{m}.bias"],
                                  stride, pad, 1, groups), 0.1)
        maps.append(x)
    maps.append(F.conv1d(x, W["discriminators.0.conv_post.weight"], W["discriminators.0.conv_post.bias"], 1, 1))
    for d, p in enumerate(PERIODS, 1):
        x = x0
        if x.shape[2] % p:
            x = F.pad(x, (0, p - x.shape[2] % p), "reflect")
        x = x.view(x.shape[0], 1, x.shape[2] // p, p)
        for m in range(5):
            x = F.leaky_relu(F.conv2d(x, W[f"discriminators.{d}.convs.{m}.weight"], W[f"discriminators.{d}.convs.{m}.bias"],
                                      (3 if m < 4 else 1, 1), (2, 0)), 0.1)
            maps.append(x)
        maps.append(F.conv2d(x, W[f"discriminators.{d}.conv_post.weight"], W[f"discriminators.{d}.conv_post.bias"], 1, (1, 0)))
    return maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    B, T = 16, 8192
    sd = synth.make_discriminator_state_dict(29)
    net = MultiPeriodDiscriminator().load_state_dict(sd).to("cuda")
    W = {k: v.cuda() for k, v in checkpoint.fold_weight_norm(sd).items()}
    gen = torch.Generator().manual_seed(0)
    y = (0.5 * torch.randn(B, 1, T, generator=gen)).cuda()
    y_hat = y + (0.2 * torch.randn(B, 1, T, generator=gen)).cuda()

    forward_ms = timed(lambda: net(y, y_hat), a.steps, a.warmup)
    out = net(y, y_hat)
    losses_ms = timed(lambda: (losses.discriminator_loss(out[0], out[1]), losses.generator_loss(out[1]),
                               losses.feature_loss(out[2], out[3])), a.steps, a.warmup)
    with torch.no_grad():
        torch_ms = timed(lambda: torch_forward(W, y, y_hat), a.steps, a.warmup)

    # kernel classes, on the call's own maps
    bufs, _ = net._run(y, y_hat)
    shapes = net.fmap_shapes(B, T)
    lib, h, s, P = _lib.load(), net._handle, _lib.current_stream_ptr, _lib.ptr
    yy = torch.cat([y, y_hat], 0).contiguous()
    scratch = [torch.empty_like(b) for b in bufs]

    def first(d):
        return 0 if d == 0 else 7 + 6 * (d - 1)

    def fold():
        for d in range(1, 6):
            _lib.check(lib.wetts_disc_fold_conv0(h, d, P(yy), 2 * B, T, P(scratch[first(d)]), s()), "fold")

    mfma_layers = [(0, 5)] + [(d, m) for d in range(1, 6) for m in range(1, 5)]

    def mfma():
        for d, m in mfma_layers:
            i = first(d) + m
            _lib.check(lib.wetts_disc_strided_conv(h, d, m, P(bufs[i - 1]), shapes[i - 1][0], shapes[i - 1][2],
                                                   P(scratch[i]), s()), "strided")

    def post():
        for d in range(6):
            i = first(d) + (6 if d == 0 else 5)
            _lib.check(lib.wetts_disc_conv_post(h, d, P(bufs[i - 1]), 2 * B, shapes[i - 1][2], P(scratch[i]), s()), "post")

    def grouped():
        x, Tin = yy, T
        for m in range(5):
            _lib.check(lib.wetts_disc_grouped_conv(h, m, P(x), 2 * B, Tin, P(scratch[m]), s()), "grouped")
            x, Tin = bufs[m], shapes[m][2]

    flops = 0.0
    for d, m in mfma_layers:
        i = first(d) + m
        rows, Cout, H, _ = shapes[i]
        flops += 2.0 * rows * H * Cout * shapes[i - 1][1] * 5
    mfma_ms = timed(mfma, a.steps, a.warmup)
    line = dict(tool="bench_disc", shape="16x8192", batch=B, samples=T, steps=a.steps,
                forward_ms_per_call=round(forward_ms, 3), losses_ms_per_call=round(losses_ms, 3),
                fold_conv0_ms=round(timed(fold, a.steps, a.warmup), 4), mfma_convs_ms=round(mfma_ms, 3),
                conv_post_ms=round(timed(post, a.steps, a.warmup), 4), grouped_convs_ms=round(timed(grouped, a.steps, a.warmup), 4),
                mfma_convs_tflop=round(flops / 1e12, 4),
                mfma_convs_f32_peak_fraction=round(flops / (mfma_ms * 1e-3) / (F32_MFMA_PEAK_TFLOPS * 1e12), 4),
                torch_functional_forward_ms=round(torch_ms, 3), torch_over_hip=round(torch_ms / forward_ms, 3),
                device=torch.cuda.get_device_name())
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
