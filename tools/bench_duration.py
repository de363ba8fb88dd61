#!/usr/bin/env python3
"""Duration-loss timing (GPU box only): SynthesizerTrn.duration_loss on HiFi-GAN v1 with the 218-row AISHELL-3 speaker
table, synthetic weights, token ids and durations, at 16 x 128 phonemes (v1's benched batch), every row full.  After a
warm-up, device events time the whole call, then on the call's own device tensors each stage: the SDP forward
(wetts_duration_sdp_forward: nine ConvFlows and four DDSConv stacks), next to it the reverse pass infer() runs on the
same shape (wetts_duration_sdp: three ConvFlows, one DDSConv stack), the logw_ kernel and the batch total.  Prints one
JSON line.
    python tools/bench_duration.py [--steps 20] [--warmup 5] [--out profiles/duration_bench.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wetts_amd import SynthesizerTrn, _lib, config, synth  # noqa: E402

SPEC = 513


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
    n_spk, B, Tx = 218, 16, 128
    cfg = config.make_config(dict(config.MODEL_CONFIGS["v1"]), 256, n_spk)
    sd = dict(synth.make_state_dict(cfg, 35), **synth.make_duration_state_dict(cfg, 37))
    net = SynthesizerTrn(256, SPEC, 32, n_speakers=n_spk, **config.MODEL_CONFIGS["v1"]).load_state_dict(sd).to("cuda")
    gen = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (B, Tx), generator=gen).cuda()
    xl = torch.full((B,), Tx, dtype=torch.long).cuda()
    sid = torch.randint(0, n_spk, (B,), generator=gen).cuda()
    w = torch.randint(1, 13, (B, 1, Tx), generator=gen).float().cuda()
    e_q, eps_w = torch.randn(B, 2, Tx, generator=gen).cuda(), torch.randn(B, 2, Tx, generator=gen).cuda()
    total_ms = timed(lambda: net.duration_loss(x, xl, w, sid=sid, e_q=e_q, eps_w=eps_w), a.steps, a.warmup)
    _, (x_enc, _, _) = net.duration_loss(x, xl, w, sid=sid, e_q=e_q, eps_w=eps_w)
    st = net._last_duration
    lib = _lib.load()
    g = net._speaker(sid, B)
    f32 = dict(dtype=torch.float32, device="cuda")
    nws = max(int(lib.wetts_workspace_bytes(net._handle, B, Tx, 0)),
              int(lib.wetts_duration_loss_workspace_bytes(net._handle, B, Tx)))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    nll, logq, rows, per, l_length = (torch.empty(B, **f32) for _ in range(5))
    logw, tgt, total = torch.empty(B, Tx, **f32), torch.empty(B, Tx, **f32), torch.empty(2, **f32)
    wf, mask = st["w"], st["x_mask"]
    s = _lib.current_stream_ptr
    P = _lib.ptr
    stages = dict(
        sdp_forward_ms=lambda: _lib.check(lib.wetts_duration_sdp_forward(
            net._handle, P(x_enc), P(mask), P(g), P(wf), P(e_q), B, Tx, P(nll), P(logq), P(rows), P(per), None, None,
            None, None, None, P(ws), nws, s()), "duration_sdp_forward"),
        sdp_reverse_ms=lambda: _lib.check(lib.wetts_duration_sdp(
            net._handle, P(x_enc), P(mask), P(g), P(eps_w), 1.0, B, Tx, P(logw), None, P(ws), nws, s()), "duration_sdp"),
        logw_target_ms=lambda: _lib.check(lib.wetts_duration_logw_target(
            P(wf), P(mask), B, Tx, P(tgt), s()), "duration_logw_target"),
        total_ms=lambda: _lib.check(lib.wetts_duration_loss_total(
            P(rows), P(mask), B, Tx, 1.0, P(l_length), P(total), s()), "duration_loss_total"))
    line = dict(tool="bench_duration", shape="v1_16x128", batch=B, phonemes=Tx, steps=a.steps,
                duration_loss_ms_per_call=round(total_ms, 3))
    for k, fn in stages.items():
        line[k] = round(timed(fn, a.steps, a.warmup), 4)
    line["text_encoder_and_rest_ms"] = round(total_ms - sum(line[k] for k in stages), 3)
    line["device"] = torch.cuda.get_device_name()
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
