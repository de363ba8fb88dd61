#!/usr/bin/env python3
"""Frontend training timing (GPU box only): FrontendTrainer.step at real bert-base-chinese dimensions (12 layers,
768 / 12 heads / 3072, transform 8 heads / 2048, 470 + 5 classes) with synthetic weights and labels, at 32 x 64 and
16 x 256 tokens.  Per shape, all in ONE process, alternating, `--repeats` times each after a warm-up of every variant
(median, min, max of the per-call device-event times):
  step, grad (forward + loss + backward), the forward pass alone (FrontendModel.score), AdamW alone;
  each backward stage alone through its stand-alone entry at the step's shapes: the dgrad and wgrad of every trained
  Linear (with the share of the f32 MFMA peak, 256 CUs x 4 SIMDs x 64 FLOP / clock at 2.4 GHz = 157 TFLOP/s, that the two
  GEMM forms reach), LayerNorm backward, attention backward, cross-entropy backward;
  the same step written with torch.nn.functional + autograd + torch.optim.AdamW(foreach=False / True) on the same device
  and weights (BERT under no_grad, as its parameters are frozen; a restatement inside this tool: no `transformers`).
Prints one JSON line.
    python tools/bench_frontend_train.py [--steps 10] [--warmup 3] [--repeats 5] [--out profiles/frontend_train_bench.json]"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_frontend import BERT, MFMA_PEAK, _mms, spread  # noqa: E402
from wetts_amd import FrontendModel, _lib, synth  # noqa: E402
from wetts_amd.frontend import frontend_config  # noqa: E402
from wetts_amd.frontend_train import FrontendTrainer  # noqa: E402

POLYPHONES, PROSODY = 470, 5
SHAPES = ((32, 64), (16, 256))
TRAINED = ("transform.", "phone_classifier.", "prosody_classifier.")


def torch_logits(W, cfg, ids, mask):
    """frontend/model.py:52-63 with torch.nn.functional; BERT under no_grad (model.py:30-31 freezes it)."""
    B, T = ids.shape
    d = cfg["hidden_size"]
    bias = torch.zeros(B, 1, 1, T, device=ids.device).masked_fill(mask[:, None, None, :] == 0, float("-inf"))

    def attn(qkv, heads):
        q, k, v = (t.reshape(B, T, heads, d // heads).transpose(1, 2) for t in qkv.split(d, 2))
        p = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(d // heads) + bias, -1)
        return (p @ v).transpose(1, 2).reshape(B, T, d)

    def ln(x, n, eps):
        return F.layer_norm(x, (d,), W[n + ".weight"], W[n + ".bias"], eps)

    with torch.no_grad():
        e = "bert.embeddings."
        h = ln(W[e + "word_embeddings.weight"][ids] + W[e + "position_embeddings.weight"][:T] +
               W[e + "token_type_embeddings.weight"][0], e + "LayerNorm", cfg["layer_norm_eps"])
        for i in range(cfg["num_layers"]):
            p = f"bert.encoder.layer.{i}."
            a = attn(F.linear(h, W[p + "qkv.weight"], W[p + "qkv.bias"]), cfg["num_heads"])
            h = ln(F.linear(a, W[p + "attention.output.dense.weight"], W[p + "attention.output.dense.bias"]) + h,
                   p + "attention.output.LayerNorm", cfg["layer_norm_eps"])
            f = F.gelu(F.linear(h, W[p + "intermediate.dense.weight"], W[p + "intermediate.dense.bias"]))
            h = ln(F.linear(f, W[p + "output.dense.weight"], W[p + "output.dense.bias"]) + h, p + "output.LayerNorm",
                   cfg["layer_norm_eps"])
    a = attn(F.linear(h, W["transform.self_attn.in_proj_weight"], W["transform.self_attn.in_proj_bias"]), cfg["transform_heads"])
    h = ln(F.linear(a, W["transform.self_attn.out_proj.weight"], W["transform.self_attn.out_proj.bias"]) + h, "transform.norm1", 1e-5)
    f = F.relu(F.linear(h, W["transform.linear1.weight"], W["transform.linear1.bias"]))
    h = ln(F.linear(f, W["transform.linear2.weight"], W["transform.linear2.bias"]) + h, "transform.norm2", 1e-5)
    return (F.linear(h, W["phone_classifier.weight"], W["phone_classifier.bias"]),
            F.linear(h, W["prosody_classifier.weight"], W["prosody_classifier.bias"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    cfg = frontend_config(POLYPHONES, PROSODY, BERT)
    sd = synth.make_frontend_state_dict(cfg, 5)
    net = FrontendModel(POLYPHONES, PROSODY, BERT).load_state_dict(sd).to("cuda")
    tr = FrontendTrainer(net, lr=1e-4, num_training_steps=10 ** 6)
    d, ff, H, L = cfg["hidden_size"], cfg["transform_ff"], cfg["transform_heads"], cfg["num_layers"]
    line = dict(tool="bench_frontend_train", steps=a.steps, repeats=a.repeats, device=torch.cuda.get_device_name(),
                config=dict(layers=L, hidden=d, transform_heads=H, transform_ff=ff, polyphones=POLYPHONES, prosody=PROSODY),
                trainable_floats=tr.span[1], f32_mfma_peak_flops=MFMA_PEAK, shapes={})
    lib, P, s = _lib.load(), _lib.ptr, _lib.current_stream_ptr
    gen = torch.Generator().manual_seed(0)
    for B, T in SHAPES:
        N = B * T
        ids = torch.randint(0, cfg["vocab_size"], (B, T), generator=gen).cuda()
        mask = torch.ones(B, T, dtype=torch.int64).cuda()
        pl = torch.where(torch.rand(B, T, generator=gen) < 0.1, torch.randint(0, POLYPHONES, (B, T), generator=gen),
                         torch.full((B, T), -100)).cuda()
        rl = torch.randint(0, PROSODY, (B, T), generator=gen).cuda()
        x = {"input_ids": ids, "attention_mask": mask}
        # the torch twin: its own copy of the weights, the trained ones as parameters
        W = {k: v.cuda().clone() for k, v in sd.items() if v.is_floating_point()}
        for i in range(L):
            p = f"bert.encoder.layer.{i}."
            for kind in ("weight", "bias"):
                W[p + "qkv." + kind] = torch.cat([W.pop(p + f"attention.self.{n}.{kind}") for n in ("query", "key", "value")], 0)
        params = [W[k].requires_grad_(True) for k in W if k.startswith(TRAINED)]
        opts = {fe: torch.optim.AdamW(params, lr=1e-4, foreach=fe) for fe in (False, True)}

        def torch_step(fe):
            zp, zr = torch_logits(W, cfg, ids, mask)
            loss = 0.5 * F.cross_entropy(zp.permute(0, 2, 1), pl, ignore_index=-100) + \
                0.5 * F.cross_entropy(zr.permute(0, 2, 1), rl, ignore_index=-100)
            opts[fe].zero_grad()
            loss.backward()
            opts[fe].step()

        grad = torch.zeros(tr.span[1], device="cuda")
        m, v = torch.zeros_like(grad), torch.zeros_like(grad)
        fns = dict(step=lambda: tr.step(x, pl, rl), grad=lambda: tr.grad(x, pl, rl), forward_and_loss=lambda: net.score(x, pl, rl),
                   adamw=lambda: lib.wetts_frontend_adamw_step(net._handle, P(grad), P(m), P(v), 0.0, 0.9, 0.999, 1e-8, 0.01, 0.1,
                                                               0.001, s()),
                   torch_step_adamw_single=lambda: torch_step(False), torch_step_adamw_foreach=lambda: torch_step(True))
        t = spread(fns, a.steps, a.warmup, a.repeats)
        row = dict(ms={k: _mms(val) for k, val in t.items()},
                   torch_over_hip_step=round(min(t["torch_step_adamw_single"][0], t["torch_step_adamw_foreach"][0]) / t["step"][0], 3),
                   backward_ms=round(t["grad"][0] - t["forward_and_loss"][0], 4))
        # the backward stages alone, at the step's shapes
        C = POLYPHONES + PROSODY
        buf = lambda *shape: torch.randn(*shape, device="cuda")  # noqa: E731
        gemms = dict(in_proj=(3 * d, d), out_proj=(d, d), linear1=(ff, d), linear2=(d, ff), phone_classifier=(POLYPHONES, d))
        st, flops = {}, {}
        keep = []
        for name, (M, K) in gemms.items():
            dy, w, xx, dx, dw, db = buf(N, M), buf(M, K), buf(N, K), buf(N, K), buf(M, K), buf(M)
            nb = int(lib.wetts_frontend_linear_wgrad_workspace_bytes(N, M, K))
            ws = torch.empty(nb // 4 + 1, device="cuda")
            keep += [dy, w, xx, dx, dw, db, ws]
            st["dgrad." + name] = (lambda dy=dy, w=w, dx=dx, M=M, K=K:
                                   lib.wetts_frontend_linear_dgrad(P(dy), M, P(w), N, M, K, 0, None, P(dx), s()))
            st["wgrad." + name] = (lambda dy=dy, xx=xx, dw=dw, db=db, ws=ws, nb=nb, M=M, K=K:
                                   lib.wetts_frontend_linear_wgrad(P(dy), M, P(xx), N, M, K, P(dw), P(db), P(ws), nb, s()))
            flops[name] = 2.0 * N * M * K
        dy, xx, gm, dx, dg, dbt = buf(N, d), buf(N, d), buf(d), buf(N, d), buf(d), buf(d)
        lnws = torch.empty((2 * N + 63) // 64 * 64 + (N + 63) // 64 * d, device="cuda")
        st["layer_norm_backward"] = lambda: lib.wetts_frontend_layer_norm_backward(P(dy), P(xx), P(gm), 1e-5, N, d, P(dx), P(dg),
                                                                                   P(dbt), P(lnws), lnws.numel() * 4, s())
        qkv, mf, ctx, dctx, dqkv = buf(N, 3 * d), torch.ones(N, device="cuda"), buf(N, d), buf(N, d), buf(N, 3 * d)
        aws = torch.empty(2 * ((B * H * T * T + 63) // 64 * 64), device="cuda")
        st["attention_backward"] = lambda: lib.wetts_frontend_attention_backward(P(qkv), P(mf), P(ctx), P(dctx), B, T, H, d // H,
                                                                                 P(dqkv), P(aws), aws.numel() * 4, s())
        zp, zr, dl = buf(N, POLYPHONES), buf(N, PROSODY), buf(N, C)
        counts = torch.full((22,), N, dtype=torch.int64, device="cuda")
        st["ce_backward"] = lambda: lib.wetts_frontend_ce_backward(P(zp), P(zr), P(mf), P(pl), P(rl), P(counts), N, POLYPHONES,
                                                                   PROSODY, 0.5, P(dl), s())
        ts = spread(st, a.steps, a.warmup, a.repeats)
        row["stage_ms"] = {k: _mms(val) for k, val in ts.items()}
        for form in ("dgrad", "wgrad"):
            tot_ms = sum(ts[f"{form}.{n}"][0] for n in gemms)
            row[f"{form}_share_of_f32_mfma_peak"] = round(sum(flops.values()) / (tot_ms * 1e-3) / MFMA_PEAK, 4)
            row[f"{form}_share_of_f32_mfma_peak_by_linear"] = {n: round(flops[n] / (ts[f"{form}.{n}"][0] * 1e-3) / MFMA_PEAK, 4)
                                                                for n in gemms}
        row["attention_backward_share_of_backward"] = round(ts["attention_backward"][0] / max(row["backward_ms"], 1e-9), 3)
        line["shapes"][f"{B}x{T}"] = row
        del keep
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
