"""Float64 restatement of the text frontend (frontend/model.py:21-73: an HF BertModel with absolute positions, one
nn.TransformerEncoderLayer(batch_first) at its defaults, two Linear classifiers) in plain torch, with its stages, the two
test configurations, the fixture shapes, the inputs, the error measures and the injected defects.  No `transformers`.

Activations are token-major here too: [B, T, C].  `forward` evaluates at the dtype of the weights it is given: float64 is
the oracle, float32 the float32 floor's second opinion (the FIRST one is the reference itself, in the fixtures).

Gates.  The floor of a figure is the error of a float32 evaluation against the float64 oracle on the same inputs,
measured on the CPU when the fixtures are made (tests/golden/make_golden_frontend.py) and stored in every fixture of the
config as floor_<stage>: for the logits and probabilities the evaluation is the reference's own forward pass, for a
stand-alone stage torch's float32 kernels on the stage's input.  The device has to stay within GATE_FACTOR x floor; against
the reference's stored float32 values, themselves one floor from float64, within GATE_FACTOR + 1 floors."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import decoder_input as di

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = os.path.join(GOLDEN, "frontend_toy")
NUM_POLYPHONES, NUM_PROSODY, VOCAB, POSITIONS = 34, 5, 48, 80
WSEED = 20260
GATE_FACTOR = 4.0
HALF_ULP = 2.0 ** -24

# HF config.json dicts; `_name_or_path` carries the reference's model name so that its own branch (model.py:33-42) runs
BERT_CONFIGS = {
    "tiny": dict(_name_or_path="TinyBERT_4L_zh_backup", vocab_size=VOCAB, hidden_size=312, num_hidden_layers=2,
                 num_attention_heads=12, intermediate_size=1200, max_position_embeddings=POSITIONS, type_vocab_size=2,
                 hidden_act="gelu", layer_norm_eps=1e-12, position_embedding_type="absolute", hidden_dropout_prob=0.1,
                 attention_probs_dropout_prob=0.1, model_type="bert"),
    "base": dict(_name_or_path="bert-chinese-base", vocab_size=VOCAB, hidden_size=768, num_hidden_layers=1,
                 num_attention_heads=12, intermediate_size=256, max_position_embeddings=POSITIONS, type_vocab_size=2,
                 hidden_act="gelu", layer_norm_eps=1e-12, position_embedding_type="absolute", hidden_dropout_prob=0.1,
                 attention_probs_dropout_prob=0.1, model_type="bert"),
}
TRANSFORM = {"tiny": (12, 1200), "base": (8, 2048)}  # (nhead, dim_feedforward) of the reference's two branches
CONFIGS = tuple(BERT_CONFIGS)

# token counts per row, [CLS] and [SEP] included: one character; a padded pair; the attention tile edge (16 queries, 64
# keys per chunk: 33 / 32 / 31 cross the query tiles, 65 / 64 / 63 the key chunk AND the GEMM's 64-column tile, whose
# 32-column halves 3 x 33 = 99 and 3 x 65 = 195 tokens leave ragged); the position table's last row
FIXTURE_SHAPES = ((3,), (9, 6), (33, 32, 31), (65, 64, 63), (80,))
STAGES = ("embed", "linear_bias", "linear_gelu", "linear_relu", "linear_residual", "add_layer_norm", "attention_bert",
          "attention_transform", "heads_logits", "heads_probs")
OUTPUTS = ("phone_logits", "prosody_logits", "phone_prob", "prosody_prob")


def config(cname):
    """The config dict of wetts_frontend_config_t (what wetts_amd.frontend.frontend_config derives from the HF dict)."""
    bc = BERT_CONFIGS[cname]
    return dict(vocab_size=bc["vocab_size"], hidden_size=bc["hidden_size"], num_layers=bc["num_hidden_layers"],
                num_heads=bc["num_attention_heads"], intermediate_size=bc["intermediate_size"],
                max_position_embeddings=bc["max_position_embeddings"], type_vocab_size=bc["type_vocab_size"],
                layer_norm_eps=bc["layer_norm_eps"], transform_heads=TRANSFORM[cname][0], transform_ff=TRANSFORM[cname][1],
                num_polyphones=NUM_POLYPHONES, num_prosody=NUM_PROSODY)


_W = {}


def weights(cname):
    """(float32 state_dict, float64 state_dict) of a config, generated once per process."""
    if cname not in _W:
        from wetts_amd import synth
        sd = synth.make_frontend_state_dict(config(cname), WSEED)
        _W[cname] = (sd, {k: v.to(torch.float64) for k, v in sd.items() if v.is_floating_point()})
    return _W[cname]


def case_name(cname, lens):
    return f"frontend_{cname}_b{len(lens)}x{max(lens)}"


def case_seed(lens):
    return 7000 + 100 * len(lens) + max(lens)


def inputs(lens, seed):
    """(input_ids [B, T], attention_mask [B, T]) int64: [CLS] (2), characters (5 .. 44), [SEP] (3), [PAD] (0)."""
    g = torch.Generator().manual_seed(int(seed))
    B, T = len(lens), max(lens)
    ids = torch.zeros(B, T, dtype=torch.int64)
    mask = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        ids[b, 0], ids[b, n - 1] = 2, 3
        ids[b, 1:n - 1] = torch.randint(5, 45, (n - 2,), generator=g)
        mask[b, :n] = 1
    return ids, mask


def texts(ids, mask):
    """The strings whose cli tokenisation gives the rows of `ids`."""
    vocab = [l.rstrip("\n") for l in open(os.path.join(TOY, "vocab.txt"), encoding="utf-8")]
    return ["".join(vocab[int(i)] for i in row[1:int(m.sum()) - 1]) for row, m in zip(ids, mask)]


# ---- the stages -------------------------------------------------------------------------------------------------------
def embed(W, ids, tt, eps=1e-12, fault=None):
    T = ids.shape[1]
    x = W["bert.embeddings.word_embeddings.weight"][ids] + W["bert.embeddings.token_type_embeddings.weight"][tt]
    if fault != "no_position":
        x = x + W["bert.embeddings.position_embeddings.weight"][:T].unsqueeze(0)
    return layer_norm(x, W["bert.embeddings.LayerNorm.weight"], W["bert.embeddings.LayerNorm.bias"], eps)


def layer_norm(x, g, b, eps):
    return F.layer_norm(x, (x.shape[-1],), g, b, eps)


def gelu(x, fault=None):
    return F.gelu(x, approximate="tanh" if fault == "tanh_gelu" else "none")


def attention(qkv, mask, heads, fault=None):
    """qkv [B, T, 3 d] (q | k | v) -> [B, T, d]; keys with mask 0 excluded; a row without a valid key gives zeros."""
    B, T, d3 = qkv.shape
    d = d3 // 3
    dk = d // heads
    q, k, v = (t.reshape(B, T, heads, dk).transpose(1, 2) for t in qkv.split(d, dim=2))
    if fault == "swap_qk":
        q, k = k, q
    s = q @ k.transpose(2, 3) / math.sqrt(dk)
    if fault != "pad_key":
        s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return (p @ v).transpose(1, 2).reshape(B, T, d)


def block(W, names, h, mask, heads, act, eps, fault=None, qk_fault=None):
    """One post-norm layer.  names: (wqkv, bqkv, out, norm1, lin1, lin2, norm2) -- wqkv / bqkv tensors, the rest prefixes."""
    wqkv, bqkv, out, n1, l1, l2, n2 = names
    a = attention(F.linear(h, wqkv, bqkv), mask, heads, qk_fault if qk_fault else fault)
    a = F.linear(a, W[out + ".weight"], W[out + ".bias"])
    h = layer_norm(a if fault == "no_residual" else a + h, W[n1 + ".weight"], W[n1 + ".bias"], eps)
    f = act(F.linear(h, W[l1 + ".weight"], W[l1 + ".bias"]))
    f = F.linear(f, W[l2 + ".weight"], W[l2 + ".bias"])
    return layer_norm(f + h, W[n2 + ".weight"], W[n2 + ".bias"], eps)


def bert_block_names(W, i):
    p = f"bert.encoder.layer.{i}."
    wqkv = torch.cat([W[p + f"attention.self.{n}.weight"] for n in ("query", "key", "value")], 0)
    bqkv = torch.cat([W[p + f"attention.self.{n}.bias"] for n in ("query", "key", "value")], 0)
    return (wqkv, bqkv, p + "attention.output.dense", p + "attention.output.LayerNorm", p + "intermediate.dense",
            p + "output.dense", p + "output.LayerNorm")


def transform_names(W):
    return (W["transform.self_attn.in_proj_weight"], W["transform.self_attn.in_proj_bias"], "transform.self_attn.out_proj",
            "transform.norm1", "transform.linear1", "transform.linear2", "transform.norm2")


def heads(W, x, mask, axis=-1):
    """-> (phone logits, prosody logits, phone probabilities, prosody probabilities), zeros at padded tokens."""
    m = (mask != 0).unsqueeze(2).to(x.dtype)
    lp = F.linear(x, W["phone_classifier.weight"], W["phone_classifier.bias"])
    lr = F.linear(x, W["prosody_classifier.weight"], W["prosody_classifier.bias"])
    return lp * m, lr * m, torch.softmax(lp, dim=axis) * m, torch.softmax(lr, dim=axis) * m


FAULTS = ("no_position", "tanh_gelu", "eps_1e-5", "pad_key", "swap_qk", "transform_12_heads", "no_residual", "softmax_axis")


def forward(W, cname, ids, mask, tt=None, fault=None):
    """-> dict: embed, layer0 .., bert (the last layer), transform, phone_logits, prosody_logits, phone_prob,
    prosody_prob; all [B, T, .] at W's dtype, the four outputs zero at padded tokens.  `fault`: one of FAULTS --
    a dropped position embedding; tanh GELU; eps 1e-5 in BERT's LayerNorms; padded keys admitted; q and k swapped in
    transform's packed projection; 12 heads in transform (the tiny branch's count at 768); a lost residual (the first
    one of every layer); the softmaxes over the token axis."""
    c = config(cname)
    tt = torch.zeros_like(ids) if tt is None else tt
    eps = 1e-5 if fault == "eps_1e-5" else c["layer_norm_eps"]
    common = fault if fault in ("pad_key", "no_residual") else None
    out = {}
    h = out["embed"] = embed(W, ids, tt, eps, fault)
    for i in range(c["num_layers"]):
        h = out[f"layer{i}"] = block(W, bert_block_names(W, i), h, mask, c["num_heads"], lambda x: gelu(x, fault), eps, common)
    out["bert"] = h
    th = 12 if fault == "transform_12_heads" else c["transform_heads"]
    h = out["transform"] = block(W, transform_names(W), h, mask, th, F.relu, 1e-5, common,
                                 "swap_qk" if fault == "swap_qk" else None)
    axis = 1 if fault == "softmax_axis" else -1
    out["phone_logits"], out["prosody_logits"], out["phone_prob"], out["prosody_prob"] = heads(W, h, mask, axis)
    return out


# ---- stand-alone stage cases --------------------------------------------------------------------------------------------
def stage_cases(cname, ids, mask):
    """The inputs of every stand-alone stage, taken from the float64 forward pass and rounded to float32 (what the
    device entry receives), and the function that evaluates the stage on them at a given dtype:
    {stage: (dict of float32 / int inputs, fn(W, inputs at W's dtype) -> tensor)}."""
    sd, W64 = weights(cname)
    c = config(cname)
    st = forward(W64, cname, ids, mask)
    f32 = lambda t: t.to(torch.float32)  # noqa: E731
    h0, hb = f32(st["embed"]), f32(st["bert"])
    L0 = bert_block_names(W64, 0)
    qkv_b = f32(F.linear(st["embed"], L0[0], L0[1]))
    TN = transform_names(W64)
    qkv_t = f32(F.linear(st["bert"], TN[0], TN[1]))
    ctx = f32(attention(qkv_b.double(), mask, c["num_heads"]))
    p0 = "bert.encoder.layer.0."
    cast = lambda W, t: t.to(W["phone_classifier.bias"].dtype)  # noqa: E731

    def lin(name, act=None, res=False):
        def fn(W, i):
            y = F.linear(cast(W, i["x"]), W[name + ".weight"], W[name + ".bias"])
            if res:
                y = y + cast(W, i["res"])
            return act(y) if act else y
        return fn

    def qkv_fn(W, i):
        n = bert_block_names(W, 0)
        return F.linear(cast(W, i["x"]), n[0], n[1])

    return {
        "embed": (dict(ids=ids, mask=mask), lambda W, i: embed(W, i["ids"], torch.zeros_like(i["ids"]), c["layer_norm_eps"])),
        "linear_bias": (dict(x=h0), qkv_fn),
        "linear_gelu": (dict(x=h0, name=p0 + "intermediate.dense"), lin(p0 + "intermediate.dense", gelu)),
        "linear_relu": (dict(x=hb, name="transform.linear1"), lin("transform.linear1", F.relu)),
        "linear_residual": (dict(x=ctx, res=h0, name=p0 + "attention.output.dense"),
                            lin(p0 + "attention.output.dense", None, True)),
        "add_layer_norm": (dict(x=ctx, res=h0, name=p0 + "attention.output.LayerNorm"),
                           lambda W, i: layer_norm(cast(W, i["x"]) + cast(W, i["res"]),
                                                   W[p0 + "attention.output.LayerNorm.weight"],
                                                   W[p0 + "attention.output.LayerNorm.bias"], c["layer_norm_eps"])),
        "attention_bert": (dict(qkv=qkv_b, mask=mask, heads=c["num_heads"]),
                           lambda W, i: attention(cast(W, i["qkv"]), i["mask"], c["num_heads"])),
        "attention_transform": (dict(qkv=qkv_t, mask=mask, heads=c["transform_heads"]),
                                lambda W, i: attention(cast(W, i["qkv"]), i["mask"], c["transform_heads"])),
        "heads_logits": (dict(x=f32(st["transform"]), mask=mask),
                         lambda W, i: torch.cat(heads(W, cast(W, i["x"]), i["mask"])[:2], 2)),
        "heads_probs": (dict(x=f32(st["transform"]), mask=mask),
                        lambda W, i: torch.cat(heads(W, cast(W, i["x"]), i["mask"])[2:], 2)),
    }


# ---- measures ----------------------------------------------------------------------------------------------------------
def valid(t, mask):
    """The rows of the valid tokens, [n_valid, C]."""
    return t[mask != 0]


def gates(got, ref):
    """(rel RMS, max |d| / rms(ref)) over the whole tensor."""
    return di.gates(got.detach().cpu().contiguous(), ref.detach().cpu().contiguous())


def worst(acc, fig):
    return fig if acc is None else (max(acc[0], fig[0]), max(acc[1], fig[1]))


def gate(floor, factor=GATE_FACTOR):
    """factor x floor for a (rel, local) pair; neither floor is taken below half a float32 ulp."""
    return tuple(factor * max(float(v), HALF_ULP) for v in floor)


def fixture_gate(floor):
    return gate(floor, GATE_FACTOR + 1)


def within(fig, g):
    return fig[0] <= g[0] and fig[1] <= g[1]


# ---- the decisions of cli/frontend.py ------------------------------------------------------------------------------------
def toy_tables():
    """(token2id, polyphone2id, char2pinyins, pinyin2phones) of the toy lexicon, read as cli/frontend.py reads them."""
    def read_list(p):
        return {l.strip(): i for i, l in enumerate(open(p, encoding="utf-8"))}
    c2p = {}
    for l in open(os.path.join(TOY, "lexicon", "pinyin_dict.txt"), encoding="utf-8"):
        a = l.split()
        c2p[a[0]] = a[1].split(",")
    p2p = {}
    for l in open(os.path.join(TOY, "lexicon", "lexicon.txt"), encoding="utf-8"):
        a = l.split()
        p2p[a[0]] = a[1:]
    return (read_list(os.path.join(TOY, "vocab.txt")), read_list(os.path.join(TOY, "lexicon", "polyphone.txt")), c2p, p2p)


def decisions(text, phone_prob, prosody_prob, tables=None):
    """cli/frontend.py:61-86 on given probabilities of ONE text ([T, P], [T, R] arrays) -> the phoneme list."""
    token2id, poly2id, c2p, p2p = tables or toy_tables()
    tokens = ["[CLS]"] + list(text) + ["[SEP]"]
    pinyins = []
    for i in range(1, len(tokens) - 1):
        arr = c2p[tokens[i]]
        if len(arr) > 1:
            pp = [phone_prob[i][poly2id[p]] for p in arr]
            pinyins.append(arr[pp.index(max(pp))])
        else:
            pinyins.append(arr[0])
    pros = np.asarray(prosody_prob).argmax(axis=1).tolist()
    out = ["sil"]
    for i in range(len(pinyins)):
        out.extend(p2p[pinyins[i]])
        out.append("#{}".format(pros[i]))
    out[-1] = "#4"
    return out


def load_fixture(cname, lens):
    return np.load(os.path.join(GOLDEN, case_name(cname, lens) + ".npz"))


_REF = {}


def reference(cname, lens):
    """(ids, mask, float64 forward dict) of a fixture case, computed once per process and left unchanged."""
    key = (cname, tuple(lens))
    if key not in _REF:
        c = load_fixture(cname, lens)
        ids, mask = inputs(lens, int(c["input_seed"]))
        _REF[key] = (ids, mask, forward(weights(cname)[1], cname, ids, mask))
    return _REF[key]
