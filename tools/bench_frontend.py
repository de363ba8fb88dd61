#!/usr/bin/env python3
"""Text frontend timing (GPU box only): FrontendModel.probs at real bert-base-chinese dimensions -- 12 layers,
768 / 12 heads / 3072, vocabulary 21128, 512 positions, transform 8 heads / 2048 -- with synthetic weights, at the
shapes 1 x 16, 1 x 48 (serving), 16 x 64 and 16 x 256 (batched).  After a warm-up, device events time the whole forward
pass (93 launches) and, through the stand-alone entries, each stage of one BERT layer at the same shape.  Reported per
shape: ms per forward; the stage times and their shares of a layer; the forward pass as a multiple of the
weight-streaming bound (the bytes of every weight matrix read once over the 6.3 TB/s copy bandwidth the
microarchitecture notes list as achievable); for the batched shapes the share of the f32 MFMA peak (256 CUs x 4 SIMDs x
64 FLOP / clock at 2.4 GHz = 157 TFLOP/s) the Linear layers reach; and the same model written with torch.nn.functional
on the same device and weights (a restatement inside this tool: no `transformers`).  Prints one JSON line.
    python tools/bench_frontend.py [--steps 20] [--warmup 5] [--out profiles/frontend_bench.json]

With --dtype (f32, bf16, f16; several may be given) the tool compares the modes of FrontendModel.set_dtype instead: per
shape, the named modes, the same model in torch.nn.functional at f32 and under bf16 autocast, all in ONE process,
alternating, `--repeats` times each after a warm-up of every variant -- median and spread (min, max) of the per-call
device-event times -- and each Linear of a layer alone: the f32 kernel and every kernel form of the 16-bit one (the
weight packed once, outside the timed calls), with the achieved FLOP/s of the launcher's choice over the 2.5 PFLOP/s
dense bf16 MFMA peak (a kernel figure).  470 + 5 classes as in the reference lexicon.
    python tools/bench_frontend.py --dtype f32 bf16 f16 [--repeats 5] [--out profiles/frontend16_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wetts_amd import FrontendModel, _lib, synth  # noqa: E402
from wetts_amd.frontend import frontend_config  # noqa: E402

BERT = dict(_name_or_path="bert-chinese-base", vocab_size=21128, hidden_size=768, num_hidden_layers=12,
            num_attention_heads=12, intermediate_size=3072, max_position_embeddings=512, type_vocab_size=2,
            hidden_act="gelu", layer_norm_eps=1e-12)
POLYPHONES, PROSODY = 1000, 5
SHAPES = ((1, 16), (1, 48), (16, 64), (16, 256))
COPY_BW, MFMA_PEAK = 6.3e12, 256 * 4 * 64 * 2.4e9
BF16_PEAK = 2.5e15  # dense bf16 / f16 MFMA, the microarchitecture notes' figure
PRECISION = {"f32": 0, "bf16": 1, "f16": 2}
BENCH_PACKED = 16  # WETTS_FRONTEND_LINEAR16_BENCH_PACKED: the workspace already holds this weight, packed by the call before


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


def spread(fns, steps, warmup, repeats):
    """{name: (median, min, max) ms per call}; the functions alternate within every repeat, after a warm-up of each."""
    for fn in fns.values():
        timed(fn, 1, warmup)
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            runs[k].append(timed(fn, steps, 0))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}


def _mms(v):
    return dict(median=round(v[0], 4), min=round(v[1], 4), max=round(v[2], 4))


def torch_forward(W, cfg, ids, mask):
    """frontend/model.py:52-73 with torch.nn.functional: BERT (absolute positions), transform, heads, softmaxes."""
    B, T = ids.shape
    d = cfg["hidden_size"]
    bias = torch.zeros(B, 1, 1, T, device=ids.device).masked_fill(mask[:, None, None, :] == 0, float("-inf"))

    def attn(qkv, heads):
        q, k, v = (t.reshape(B, T, heads, d // heads).transpose(1, 2) for t in qkv.split(d, 2))
        p = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(d // heads) + bias, -1)
        return (p @ v).transpose(1, 2).reshape(B, T, d)

    def ln(x, n, eps):
        return F.layer_norm(x, (d,), W[n + ".weight"], W[n + ".bias"], eps)

    e = "bert.embeddings."
    h = ln(W[e + "word_embeddings.weight"][ids] + W[e + "position_embeddings.weight"][:T] + W[e + "token_type_embeddings.weight"][0],
           e + "LayerNorm", cfg["layer_norm_eps"])
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
    return (torch.softmax(F.linear(h, W["phone_classifier.weight"], W["phone_classifier.bias"]), -1),
            torch.softmax(F.linear(h, W["prosody_classifier.weight"], W["prosody_classifier.bias"]), -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    ap.add_argument("--dtype", nargs="+", choices=tuple(PRECISION), default=None,
                    help="compare these modes of FrontendModel.set_dtype (see the module text); default: the f32 report")
    ap.add_argument("--repeats", type=int, default=5, help="with --dtype: alternating repeats per variant")
    a = ap.parse_args()
    if a.dtype:
        return compare(a)
    cfg = frontend_config(POLYPHONES, PROSODY, BERT)
    sd = synth.make_frontend_state_dict(cfg, 5)
    net = FrontendModel(POLYPHONES, PROSODY, BERT).load_state_dict(sd).to("cuda")
    W = {k: v.cuda() for k, v in sd.items() if v.is_floating_point()}
    d, ff, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_layers"]
    for i in range(L):  # the packed projection, for the torch restatement and the stage entry
        p = f"bert.encoder.layer.{i}."
        for kind in ("weight", "bias"):
            W[p + "qkv." + kind] = torch.cat([W.pop(p + f"attention.self.{n}.{kind}") for n in ("query", "key", "value")], 0)
    # every weight matrix and vector a call reads whole (the embedding tables are gathered, not streamed)
    wbytes = 4 * sum(v.numel() for k, v in W.items() if "embeddings." not in k and "pooler" not in k)
    lin_flops_per_token = 2 * (L * (4 * d * d + 2 * d * ff) + 4 * d * d + 2 * d * cfg["transform_ff"] + d * (POLYPHONES + PROSODY))
    line = dict(tool="bench_frontend", config=dict(layers=L, hidden=d, heads=cfg["num_heads"], intermediate=ff,
                                                   vocab=cfg["vocab_size"], positions=512, polyphones=POLYPHONES),
                steps=a.steps, launches_per_call=7 * (L + 1) + 2, weight_bytes=wbytes,
                weight_stream_bound_ms=round(wbytes / COPY_BW * 1e3, 4), device=torch.cuda.get_device_name(), shapes={})
    lib, P, s = _lib.load(), _lib.ptr, _lib.current_stream_ptr
    p0 = "bert.encoder.layer.0."
    gen = torch.Generator().manual_seed(0)
    for B, T in SHAPES:
        N = B * T
        ids = torch.randint(0, cfg["vocab_size"], (B, T), generator=gen).cuda()
        mask = torch.ones(B, T, dtype=torch.int64).cuda()
        ms = timed(lambda: net._launch(ids, None, mask, True), a.steps, a.warmup)
        with torch.no_grad():
            torch_ms = timed(lambda: torch_forward(W, cfg, ids, mask), a.steps, a.warmup)
        h, mf = torch.randn(N, d, device="cuda"), torch.ones(N, device="cuda")
        qkv, ctx, o, f1 = (torch.empty(N, c, device="cuda") for c in (3 * d, d, d, ff))
        ph, pr = torch.empty(N, POLYPHONES, device="cuda"), torch.empty(N, PROSODY, device="cuda")
        w = lambda n: P(W[p0 + n])  # noqa: E731
        stages = dict(
            embed_ln=lambda: lib.wetts_frontend_embed(net._handle, P(ids), None, P(mask), B, T, P(o), P(mf), None, s()),
            qkv_linear=lambda: lib.wetts_frontend_linear(P(h), w("qkv.weight"), w("qkv.bias"), None, N, d, 3 * d, 0, P(qkv), s()),
            attention=lambda: lib.wetts_frontend_attention(P(qkv), P(mf), B, T, cfg["num_heads"], d // cfg["num_heads"], P(ctx), s()),
            out_linear_residual=lambda: lib.wetts_frontend_linear(P(ctx), w("attention.output.dense.weight"),
                                                                  w("attention.output.dense.bias"), P(h), N, d, d, 3, P(o), s()),
            layer_norm=lambda: lib.wetts_frontend_add_layer_norm(P(o), None, w("output.LayerNorm.weight"),
                                                                 w("output.LayerNorm.bias"), 1e-12, N, d, P(ctx), s()),
            ff1_linear_gelu=lambda: lib.wetts_frontend_linear(P(h), w("intermediate.dense.weight"), w("intermediate.dense.bias"),
                                                              None, N, d, ff, 1, P(f1), s()),
            ff2_linear_residual=lambda: lib.wetts_frontend_linear(P(f1), w("output.dense.weight"), w("output.dense.bias"), P(h),
                                                                  N, ff, d, 3, P(o), s()),
            heads_softmax=lambda: lib.wetts_frontend_heads(net._handle, P(h), P(mf), N, 1, P(ph), P(pr), s()))
        each = {k: timed(fn, a.steps, a.warmup) for k, fn in stages.items()}
        layer = sum(v for k, v in each.items() if k not in ("embed_ln", "heads_softmax")) + each["layer_norm"]
        lin_ms = each["qkv_linear"] + each["out_linear_residual"] + each["ff1_linear_gelu"] + each["ff2_linear_residual"]
        row = dict(forward_ms=round(ms, 4), torch_functional_ms=round(torch_ms, 4), torch_over_hip=round(torch_ms / ms, 3),
                   forward_over_weight_stream_bound=round(ms / (wbytes / COPY_BW * 1e3), 2),
                   stage_ms={k: round(v, 4) for k, v in each.items()},
                   stage_share_of_layer={k: round(v / layer, 3) for k, v in each.items() if k not in ("embed_ln", "heads_softmax")})
        if B > 1:
            row["linear_share_of_f32_mfma_peak"] = round(2 * N * (4 * d * d + 2 * d * ff) / (lin_ms * 1e-3) / MFMA_PEAK, 3)
            row["forward_share_of_f32_mfma_peak"] = round(N * lin_flops_per_token / (ms * 1e-3) / MFMA_PEAK, 3)
        line["shapes"][f"{B}x{T}"] = row
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


def compare(a):
    """The --dtype report."""
    P_, R_ = 470, 5
    cfg = frontend_config(P_, R_, BERT)
    sd = synth.make_frontend_state_dict(cfg, 5)
    modes = list(dict.fromkeys(a.dtype))
    nets = {m: FrontendModel(P_, R_, BERT).set_dtype(m).load_state_dict(sd).to("cuda") for m in modes}
    W = {k: v.cuda() for k, v in sd.items() if v.is_floating_point()}
    d, ff, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_layers"]
    for i in range(L):
        p = f"bert.encoder.layer.{i}."
        for kind in ("weight", "bias"):
            W[p + "qkv." + kind] = torch.cat([W.pop(p + f"attention.self.{n}.{kind}") for n in ("query", "key", "value")], 0)
    lin_elems = L * (4 * d * d + 2 * d * ff) + 4 * d * d + 2 * d * cfg["transform_ff"]
    line = dict(tool="bench_frontend --dtype", modes=modes, steps=a.steps, repeats=a.repeats, launches_per_call=7 * (L + 1) + 2,
                config=dict(layers=L, hidden=d, heads=cfg["num_heads"], intermediate=ff, polyphones=P_, prosody=R_),
                linear_weight_bytes=dict(f32=4 * lin_elems, bf16=2 * lin_elems, f16=2 * lin_elems),
                bf16_mfma_peak_flops=BF16_PEAK, device=torch.cuda.get_device_name(), shapes={})
    lib, P, s = _lib.load(), _lib.ptr, _lib.current_stream_ptr
    p0 = "bert.encoder.layer.0."
    gen = torch.Generator().manual_seed(0)
    for B, T in SHAPES:
        N = B * T
        ids = torch.randint(0, cfg["vocab_size"], (B, T), generator=gen).cuda()
        mask = torch.ones(B, T, dtype=torch.int64).cuda()
        fns = {m: (lambda n=n: n._launch(ids, None, mask, True)) for m, n in nets.items()}
        fns["torch_functional_f32"] = lambda: torch_forward(W, cfg, ids, mask)

        def autocast():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return torch_forward(W, cfg, ids, mask)

        fns["torch_functional_bf16_autocast"] = autocast
        with torch.no_grad():
            t = spread(fns, a.steps, a.warmup, a.repeats)
        row = dict(forward_ms={k: _mms(v) for k, v in t.items()})
        if "f32" in t:
            for m in modes:
                if m != "f32":
                    row[f"f32_over_{m}"] = round(t["f32"][0] / t[m][0], 3)
                    row[f"{m}_faster_beyond_the_spread"] = bool(t[m][2] < t["f32"][1])
        # the stages of one layer alone: attention and LayerNorm (f32 in every mode), each Linear in f32 and in every form
        h, mf = torch.randn(N, d, device="cuda"), torch.ones(N, device="cuda")
        qkv, ctx, o, f1 = (torch.empty(N, c, device="cuda") for c in (3 * d, d, d, ff))
        w = lambda n: P(W[p0 + n])  # noqa: E731
        linears = dict(qkv_linear=(h, "qkv", None, d, 3 * d, 0, qkv), out_linear_residual=(ctx, "attention.output.dense", h, d, d, 3, o),
                       ff1_linear_gelu=(h, "intermediate.dense", None, d, ff, 1, f1),
                       ff2_linear_residual=(f1, "output.dense", h, ff, d, 3, o))
        st = dict(attention=lambda: lib.wetts_frontend_attention(P(qkv), P(mf), B, T, cfg["num_heads"], d // cfg["num_heads"], P(ctx), s()),
                  layer_norm=lambda: lib.wetts_frontend_add_layer_norm(P(o), None, w("output.LayerNorm.weight"),
                                                                       w("output.LayerNorm.bias"), 1e-12, N, d, P(ctx), s()))
        keep = []
        for name, (x, wn, res, K, M, epi, out) in linears.items():
            st[name + ".f32"] = (lambda x=x, wn=wn, res=res, K=K, M=M, epi=epi, out=out:
                                 lib.wetts_frontend_linear(P(x), w(wn + ".weight"), w(wn + ".bias"), P(res), N, K, M, epi, P(out), s()))
            for m in modes:
                if m == "f32":
                    continue
                ws = torch.empty(K * M // 2, device="cuda")
                keep.append(ws)
                _lib.check(lib.wetts_frontend_linear16(P(x), w(wn + ".weight"), w(wn + ".bias"), P(res), N, K, M, epi, PRECISION[m],
                                                       0, P(out), P(ws), 2 * K * M, s()), "linear16")  # packs the weight once
                for form in (0, 1, 2, 3):
                    st[f"{name}.{m}.form{form}"] = (
                        lambda x=x, wn=wn, res=res, K=K, M=M, epi=epi, out=out, m=m, form=form, ws=ws:
                        lib.wetts_frontend_linear16(P(x), w(wn + ".weight"), w(wn + ".bias"), P(res), N, K, M, epi, PRECISION[m],
                                                    form | BENCH_PACKED, P(out), P(ws), 2 * K * M, s()))
        ts = spread(st, a.steps, a.warmup, a.repeats)
        row["stage_ms"] = {k: _mms(v) for k, v in ts.items()}
        row["launcher_form"] = {k: int(lib.wetts_frontend_linear16_form(N, M)) for k, (_, _, _, _, M, _, _) in linears.items()}
        for m in modes:
            sfx = ".f32" if m == "f32" else f".{m}.form0"
            lin = sum(ts[k + sfx][0] for k in linears)
            layer = lin + ts["attention"][0] + 2 * ts["layer_norm"][0]
            row[f"layer_ms_{m}"] = round(layer, 4)
            row[f"attention_share_of_layer_{m}"] = round(ts["attention"][0] / layer, 3)
            row[f"linear_share_of_layer_{m}"] = round(lin / layer, 3)
            if m != "f32" and B > 1:
                row[f"linear_kernels_share_of_bf16_mfma_peak_{m}"] = round(2 * N * (4 * d * d + 2 * d * ff) / (lin * 1e-3) / BF16_PEAK, 4)
        line["shapes"][f"{B}x{T}"] = row
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
