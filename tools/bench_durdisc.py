#!/usr/bin/env python3
"""Duration discriminator timing (GPU box only): net_dur_disc(hidden_x, x_mask, logw_, logw) at a training batch's shape,
16 utterances x 128 phonemes, all rows full, 192 channels, k = 3, synthetic weights, for DurationDiscriminatorV1 and V2.
After a warm-up, device events time the whole forward pass (four launches) and -- on the call's own stages, through
wetts_durdisc_layer -- each launch, reported as its share of their sum.  Next to it the same network written with
torch.nn.functional on the same device and weights (a restatement inside this tool), and the five loss launches.
Prints one JSON line.
    python tools/bench_durdisc.py [--steps 50] [--warmup 10] [--out profiles/durdisc_bench.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wetts_amd import DurationDiscriminatorV1, DurationDiscriminatorV2, _lib, losses, synth  # noqa: E402

C_, K = 192, 3
LAUNCHES = ("conv_1", "conv_2", "pre_out_conv_1", "pre_out_conv_2+head")


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


def torch_forward(W, version, x, m, dur_r, dur_hat):
    """discriminators.py:334-369 / 418-449 with torch.nn.functional, the trunk once and the head per duration."""
    def conv(name, norm, v):
        v = F.conv1d(v, W[name + ".weight"], W[name + ".bias"], 1, K // 2)
        if version == 2:
            v = F.layer_norm(torch.relu(v).transpose(1, 2), (C_,), W[norm + ".gamma"], W[norm + ".beta"], 1e-5).transpose(1, 2)
        return v
    t = conv("conv_2", "norm_2", conv("conv_1", "norm_1", x * m) * m)
    out = []
    for dur in (dur_r, dur_hat):
        h = torch.cat([t, F.conv1d(dur, W["dur_proj.weight"], W["dur_proj.bias"])], 1)
        h = conv("pre_out_conv_2", "pre_out_norm_2", conv("pre_out_conv_1", "pre_out_norm_1", h * m) * m) * m
        out.append(torch.sigmoid(F.linear(h.transpose(1, 2), W["output_layer.0.weight"], W["output_layer.0.bias"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    B, Tx = 16, 128
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, C_, Tx, generator=gen).cuda()
    m = torch.ones(B, 1, Tx).cuda()
    dur_r = torch.log(torch.randint(1, 20, (B, 1, Tx), generator=gen).float() + 1e-6).cuda()
    dur_hat = dur_r + (0.5 * torch.randn(B, 1, Tx, generator=gen)).cuda()
    line = dict(tool="bench_durdisc", shape="16x128", batch=B, phonemes=Tx, channels=C_, kernel_size=K, steps=a.steps,
                launches_per_call=len(LAUNCHES), device=torch.cuda.get_device_name())
    for version, cls in ((1, DurationDiscriminatorV1), (2, DurationDiscriminatorV2)):
        sd = synth.make_duration_discriminator_state_dict(version, 31, C_, C_, K)
        net = cls(C_, C_, K, 0.1).load_state_dict(sd).to("cuda")
        W = {k: v.cuda() for k, v in sd.items()}
        forward_ms = timed(lambda: net(x, m, dur_r, dur_hat), a.steps, a.warmup)
        with torch.no_grad():
            torch_ms = timed(lambda: torch_forward(W, version, x, m, dur_r, dur_hat), a.steps, a.warmup)
        losses_ms = timed(lambda: losses._duration_disc_losses(net, x, m, dur_r, dur_hat), a.steps, a.warmup) - forward_ms
        t1, t2, h1, h2, prob = net._run(x, m, dur_r, dur_hat)
        lib, h, s, P = _lib.load(), net._handle, _lib.current_stream_ptr, _lib.ptr
        durs = torch.cat([dur_r, dur_hat], 0).contiguous()
        o1, o2, p = torch.empty_like(t1), torch.empty_like(h1), torch.empty_like(prob)
        mm = m.contiguous()
        calls = (lambda: lib.wetts_durdisc_layer(h, 0, P(x), P(mm), None, B, B, Tx, P(o1), None, s()),
                 lambda: lib.wetts_durdisc_layer(h, 1, P(t1), P(mm), None, B, B, Tx, P(o1), None, s()),
                 lambda: lib.wetts_durdisc_layer(h, 2, P(t2), P(mm), P(durs), 2 * B, B, Tx, P(o2), None, s()),
                 lambda: lib.wetts_durdisc_layer(h, 3, P(h1), P(mm), None, 2 * B, B, Tx, P(o2), P(p), s()))
        each = [timed(c, a.steps, a.warmup) for c in calls]
        line[f"v{version}"] = dict(
            forward_ms_per_call=round(forward_ms, 4), losses_ms_per_call=round(losses_ms, 4),
            launch_ms=dict(zip(LAUNCHES, (round(v, 4) for v in each))),
            launch_share=dict(zip(LAUNCHES, (round(v / sum(each), 3) for v in each))),
            torch_functional_forward_ms=round(torch_ms, 4), torch_over_hip=round(torch_ms / forward_ms, 3))
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
