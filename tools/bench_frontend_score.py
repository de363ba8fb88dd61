#!/usr/bin/env python3
"""Frontend scoring timing (GPU box only): FrontendModel.score at real bert-base-chinese dimensions (12 layers, 768 / 12
heads / 3072, vocabulary 21128, 512 positions, transform 8 heads / 2048) with synthetic weights and the reference lexicon's
470 polyphone and 5 prosody classes, at the validation shapes 32 x 64 and 16 x 256 tokens, against the way the same numbers
were obtained before score() existed: forward() logits, then torch.nn.functional.cross_entropy (mean, ignore_index=-100)
and argmax of both heads on the device.  Also the three scoring launches alone (wetts_frontend_score_heads) against the
heads launch with its softmaxes (wetts_frontend_heads) on the same x.

The two ways alternate inside one process, `--repeats` times each after a warm-up of every shape; reported are the
median and the spread (min, max) of the per-call device-event times over the repeats, and their ratio.  Before timing,
the losses and predictions of the two ways are compared (the losses within 1e-5 relative, the predictions equal).
Prints one JSON line.
    python tools/bench_frontend_score.py [--steps 20] [--warmup 5] [--repeats 5] [--out profiles/frontend_score_bench.json]
--dtype f32 | bf16 | f16 runs both ways in that mode of FrontendModel.set_dtype and names it in the line."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wetts_amd import FrontendModel, _lib, synth  # noqa: E402
from wetts_amd.frontend import frontend_config  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_frontend import BERT, timed  # noqa: E402

POLYPHONES, PROSODY, IGNORE_ID = 470, 5, -100
SHAPES = ((32, 64), (16, 256))


def spread(fns, steps, warmup, repeats):
    """{name: (median, min, max) ms per call}; the functions alternate within every repeat."""
    for fn in fns.values():
        timed(fn, 1, warmup)
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            runs[k].append(timed(fn, steps, 0))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    ap.add_argument("--dtype", choices=("f32", "bf16", "f16"), default=None,
                    help="the mode of FrontendModel.set_dtype both ways run in (default: f32; the line then names it)")
    a = ap.parse_args()
    cfg = frontend_config(POLYPHONES, PROSODY, BERT)
    net = FrontendModel(POLYPHONES, PROSODY, BERT).load_state_dict(synth.make_frontend_state_dict(cfg, 5)).to("cuda")
    if a.dtype:
        net.set_dtype(a.dtype)
    d = cfg["hidden_size"]
    line = dict(tool="bench_frontend_score", config=dict(layers=cfg["num_layers"], hidden=d, polyphones=POLYPHONES,
                                                         prosody=PROSODY,
                                                         class_tiles=-(-POLYPHONES // 32) + -(-PROSODY // 32)),
                steps=a.steps, repeats=a.repeats, device=torch.cuda.get_device_name(),
                baseline="forward() logits + F.cross_entropy(ignore_index=-100) + argmax on the device", shapes={})
    if a.dtype:
        line["dtype"] = a.dtype
    lib, P, s = _lib.load(), _lib.ptr, _lib.current_stream_ptr
    gen = torch.Generator().manual_seed(0)
    for B, T in SHAPES:
        N = B * T
        ids = torch.randint(0, cfg["vocab_size"], (B, T), generator=gen).cuda()
        mask = torch.ones(B, T, dtype=torch.int64).cuda()
        pl = torch.where(torch.rand(B, T, generator=gen) < 0.3, torch.randint(0, POLYPHONES, (B, T), generator=gen),
                         torch.full((B, T), IGNORE_ID)).cuda()
        rl = torch.randint(0, PROSODY, (B, T), generator=gen).cuda()
        x = {"input_ids": ids, "attention_mask": mask}

        def fused():
            return net.score(x, pl, rl)

        def baseline():
            lp, lr = net._launch(ids, None, mask, False)
            return (F.cross_entropy(lp.permute(0, 2, 1), pl, ignore_index=IGNORE_ID),
                    F.cross_entropy(lr.permute(0, 2, 1), rl, ignore_index=IGNORE_ID), lp.argmax(-1), lr.argmax(-1))

        sc, (bl_p, bl_r, bp, br) = fused(), baseline()
        torch.cuda.synchronize()
        same = dict(phone_loss_rel=abs(float(sc.phone_loss) - float(bl_p)) / abs(float(bl_p)),
                    prosody_loss_rel=abs(float(sc.prosody_loss) - float(bl_r)) / abs(float(bl_r)),
                    pred_phone_differ=int((sc.pred_phone != bp).sum()), pred_prosody_differ=int((sc.pred_prosody != br).sum()))
        assert same["phone_loss_rel"] < 1e-5 and same["prosody_loss_rel"] < 1e-5, same
        # stages on the same x: the heads launch with its softmaxes, and the three scoring launches
        h, mf = torch.randn(N, d, device="cuda"), torch.ones(N, device="cuda")
        ph, pr = torch.empty(N, POLYPHONES, device="cuda"), torch.empty(N, PROSODY, device="cuda")
        nbytes = int(lib.wetts_frontend_score_workspace_bytes(net._handle, B, T))
        ws = torch.empty(nbytes // 4 + 1, device="cuda")
        losses, counts = torch.empty(2, device="cuda"), torch.empty(22, dtype=torch.int64, device="cuda")
        fns = dict(
            score=fused, forward_plus_torch=baseline,
            forward_logits_only=lambda: net._launch(ids, None, mask, False),
            heads_softmax=lambda: lib.wetts_frontend_heads(net._handle, P(h), P(mf), N, 1, P(ph), P(pr), s()),
            heads_logits=lambda: lib.wetts_frontend_heads(net._handle, P(h), P(mf), N, 0, P(ph), P(pr), s()),
            score_three_launches=lambda: lib.wetts_frontend_score_heads(net._handle, P(h), P(mf), P(pl), P(rl), B, T, None, None,
                                                                        None, None, P(losses), P(counts), P(ws), nbytes, None, s()))
        with torch.no_grad():
            t = spread(fns, a.steps, a.warmup, a.repeats)
        row = {k + "_ms": dict(median=round(v[0], 4), min=round(v[1], 4), max=round(v[2], 4)) for k, v in t.items()}
        row["forward_plus_torch_over_score"] = round(t["forward_plus_torch"][0] / t["score"][0], 3)
        row["heads_softmax_over_score_three_launches"] = round(t["heads_softmax"][0] / t["score_three_launches"][0], 3)
        row["heads_logits_over_score_three_launches"] = round(t["heads_logits"][0] / t["score_three_launches"][0], 3)
        row["logit_bytes_not_written"] = 4 * N * (POLYPHONES + PROSODY)
        row["agreement"] = {k: (round(v, 9) if isinstance(v, float) else v) for k, v in same.items()}
        row["fused_faster_end_to_end"] = bool(t["score"][2] < t["forward_plus_torch"][1])  # beyond the spread of both
        line["shapes"][f"{B}x{T}"] = row
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
