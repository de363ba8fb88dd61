#!/usr/bin/env python3
"""Forced-alignment timing (GPU box only): SynthesizerTrn.align on HiFi-GAN v1 with the 218-row AISHELL-3 speaker table,
synthetic weights, synthetic spectrogram and token ids, at 16 x 128 phonemes x 768 frames (v1's benched batch) and
4 x 128 x 600 (the AISHELL-3 fixture's shape), every row full.  After a warm-up, device events time the whole call, then
on the call's own device tensors the scores kernel alone, the search, path-to-durations, and the reference's torch
expression of the scores (models.py:173-184: two batched matmuls on rocBLAS and two column sums through four
intermediates) -- the thing the scores kernel is measured against.  Prints one JSON line per shape.
    python tools/bench_align.py [--steps 20] [--warmup 5] [--out profiles/align_bench.json]"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wetts_amd import SynthesizerTrn, _lib, config, synth  # noqa: E402

SPEC = 513
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X, v_mfma_f32_32x32x2_f32
SHAPES = [("v1_16x128x768", 16, 128, 768), ("aishell3_4x128x600", 4, 128, 600)]


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


def torch_scores(z_p, m_p, logs_p):
    r = torch.exp(-2 * logs_p)
    c1 = torch.sum(-0.5 * math.log(2 * math.pi) - logs_p, [1], keepdim=True)
    c2 = torch.matmul(-0.5 * (z_p ** 2).transpose(1, 2), r)
    c3 = torch.matmul(z_p.transpose(1, 2), m_p * r)
    c4 = torch.sum(-0.5 * (m_p ** 2) * r, [1], keepdim=True)
    return c1 + c2 + c3 + c4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result lines to this file")
    a = ap.parse_args()
    n_spk = 218
    cfg = config.make_config(dict(config.MODEL_CONFIGS["v1"]), 256, n_spk)
    sd = dict(synth.make_state_dict(cfg, 35), **synth.make_posterior_state_dict(cfg, SPEC, 36))
    net = SynthesizerTrn(256, SPEC, 32, n_speakers=n_spk, **config.MODEL_CONFIGS["v1"]).load_state_dict(sd).to("cuda")
    lib = _lib.load()
    I = cfg.inter_channels
    lines = []
    for name, B, Tx, Ty in SHAPES:
        gen = torch.Generator().manual_seed(0)
        x = torch.randint(0, 256, (B, Tx), generator=gen).cuda()
        xl = torch.full((B,), Tx, dtype=torch.long).cuda()
        y = (torch.rand(B, SPEC, Ty, generator=gen) ** 4 * 20.0).cuda()
        yl = torch.full((B,), Ty, dtype=torch.long).cuda()
        sid = torch.randint(0, n_spk, (B,), generator=gen).cuda()
        eps = torch.randn(B, I, Ty, generator=gen).cuda()
        call_ms = timed(lambda: net.align(x, xl, y, yl, sid=sid, eps_q=eps), a.steps, a.warmup)
        la = net._last_align
        z_p, stats, nc, path = la["z_p"], la["stats"], la["neg_cent"], la["path"]
        m_p, logs_p = stats[:, :I].contiguous(), stats[:, I:].contiguous()
        values = torch.empty(B * Ty * Tx, device="cuda")
        w, cum = torch.empty(B, Tx, device="cuda"), torch.empty(B, Tx, device="cuda")
        f2p = torch.empty(B, Ty, dtype=torch.int32, device="cuda")
        attn = torch.empty(B, Ty, Tx, device="cuda")
        s = _lib.current_stream_ptr

        def scores():
            _lib.check(lib.wetts_align_scores(net._handle, _lib.ptr(z_p), _lib.ptr(stats), B, Tx, Ty, _lib.ptr(nc), s()),
                       "align_scores")

        def search():
            _lib.check(lib.wetts_mas(_lib.ptr(nc), _lib.ptr(la["t_ys"]), _lib.ptr(la["t_xs"]), B, Ty, Tx, _lib.ptr(path),
                                     _lib.ptr(values), values.numel() * 4, s()), "mas")

        def durations():
            _lib.check(lib.wetts_path_to_durations(_lib.ptr(path), _lib.ptr(la["t_ys"]), _lib.ptr(la["t_xs"]), B, Tx, Ty,
                                                   _lib.ptr(w), _lib.ptr(cum), _lib.ptr(f2p), _lib.ptr(attn), s()),
                       "path_to_durations")

        scores_ms = timed(scores, a.steps, a.warmup)
        mas_ms = timed(search, a.steps, a.warmup)
        dur_ms = timed(durations, a.steps, a.warmup)
        torch_ms = timed(lambda: torch_scores(z_p, m_p, logs_p), a.steps, a.warmup)
        flops = 2.0 * B * Ty * Tx * 2 * I
        lines.append(dict(tool="bench_align", shape=name, batch=B, phonemes=Tx, frames=Ty, steps=a.steps,
                          align_ms_per_call=round(call_ms, 3), scores_ms=round(scores_ms, 4), mas_ms=round(mas_ms, 4),
                          path_to_durations_ms=round(dur_ms, 4),
                          encoders_flow_expand_ms=round(call_ms - scores_ms - mas_ms - dur_ms, 3),
                          scores_gflop=round(flops / 1e9, 3),
                          scores_f32_peak_fraction=round(flops / (scores_ms * 1e-3) / (F32_MFMA_PEAK_TFLOPS * 1e12), 4),
                          torch_expression_ms=round(torch_ms, 4), scores_over_torch=round(scores_ms / torch_ms, 3),
                          device=torch.cuda.get_device_name()))
        print(json.dumps(lines[-1]))
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
