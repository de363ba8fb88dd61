"""Plain-torch restatement of the WavLM loss's network side -- the sinc resampler (a stand-in for
torchaudio.transforms.Resample at its defaults: torchaudio is not installed where these fixtures are made), transformers'
WavLMModel in the base architecture, the reference's WavLMDiscriminator (model/discriminators.py:452-498) and the three
loss terms of losses.py:63-153 -- with its stages, the two test configurations, the fixture shapes, the inputs, the error
measures and the injected defects.  No `transformers`.

Activations are token-major, [B, T, C].  Everything evaluates at the dtype of the weights it is given: float64 is the
oracle, float32 the floor's second opinion (the FIRST one is the reference itself, in the fixtures).

Gates (tests/frontend_oracle.py's convention).  The floor of a figure is the error of a float32 evaluation against the
float64 oracle on the same inputs, measured on the CPU when the fixtures are made (tests/golden/make_golden_wavlm.py) and
stored in the fixture as floor_<stage>: for the hidden states, the discriminator output and the losses the evaluation is
the reference's own float32 pass (transformers' WavLMModel inside the reference's WavLMLoss), for a stand-alone stage
torch's float32 kernels on the stage's input.  The device has to stay within GATE_FACTOR x floor of the float64 oracle;
against the reference's stored float32 values, themselves one floor from float64, within GATE_FACTOR + 1 floors.  Loss
scalars are gated on their relative error by the same rule.

Both configurations have num_buckets 16 and max_bucket_distance 12, so that the 18 frames of the recipe's slice already
reach the exact range (|rel| < 4), the log ramp (4 .. 11) AND the clamp (>= 12) of the relative position buckets; at the
real 320 / 800 only the exact range would be reached."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import frontend_oracle as fo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WSEED, DSEED = 20261, 20262
GATE_FACTOR = fo.GATE_FACTOR
SLM_SR = 16000

_COMMON = dict(conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], feat_extract_norm="group",
               feat_extract_activation="gelu", hidden_act="gelu", do_stable_layer_norm=False, conv_bias=False,
               add_adapter=False, layer_norm_eps=1e-5, num_buckets=16, max_bucket_distance=12, model_type="wavlm",
               hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, layerdrop=0.0,
               final_dropout=0.0, mask_time_prob=0.0, mask_feature_prob=0.0, vocab_size=32)
# transformers config.json dicts.  tiny: no dimension reaches a tile; wide: the real widths (32-row GEMM tiles, the 64-lane
# channel groups of the normalisation, heads of 64, positional groups of 48 channels under 128 taps)
HF_CONFIGS = {
    "tiny": dict(_COMMON, conv_dim=[32] * 7, hidden_size=48, num_attention_heads=4, intermediate_size=96,
                 num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4),
    "wide": dict(_COMMON, conv_dim=[512] * 7, hidden_size=768, num_attention_heads=12, intermediate_size=256,
                 num_hidden_layers=1, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16),
}
INITIAL_CHANNEL = {"tiny": 8, "wide": 64}
CONFIGS = tuple(HF_CONFIGS)

# (rate, samples per row, rows): 401 samples after resampling, one frame; two frames; the recipe's slice (18 frames);
# identity resampling at the largest dropped tail (one frame) and one sample more (two); 33 frames, which cross the
# attention's 16-query tile and its 32-column GEMM half tile (4 rows x 33 = 132 columns also leave the 64-column tile
# ragged); 3:2 resampling (width 10); 65 frames, one key past the attention's 64-key chunk (its score loop, the
# re-staged keys and values and the softmax's second key per lane run a second time, on a chunk of ONE key); 130 frames, two
# full chunks and a tail of two (and a third 64-column GEMM tile per row)
SHAPES = ((22050, 552, 1), (22050, 1024, 3), (22050, 8192, 3), (16000, 719, 2), (16000, 720, 2), (16000, 10640, 2),
          (24000, 2048, 2), (16000, 20880, 2), (16000, 41680, 1))
FAULTS = ("conv_tap", "unbiased_var", "pos_shift", "rel_sign", "ramp_clamp", "gate_one", "own_table", "disc_order")
# the figure a fault must move: the last hidden state, or the discriminator's output
FAULT_STAGE = {f: ("disc" if f == "disc_order" else "hidden") for f in FAULTS}


def slm_layers(cname):
    return HF_CONFIGS[cname]["num_hidden_layers"] + 1


def faults(cname):
    """The defects that exist in a config: one layer has no second layer to give a table of its own."""
    return tuple(f for f in FAULTS if f != "own_table" or HF_CONFIGS[cname]["num_hidden_layers"] > 1)


def case_name(cname, shape):
    return f"wavlm_{cname}_r{shape[0]}_b{shape[2]}x{shape[1]}"


def case_seed(shape):
    return 9000 + shape[0] % 1000 + 7 * shape[1] + shape[2]


_W = {}


def weights(cname):
    """((WavLM float32 state_dict, float64), (discriminator float32 state_dict, float64)), made once per process."""
    if cname not in _W:
        from wetts_amd import synth
        sd = synth.make_wavlm_state_dict(HF_CONFIGS[cname], WSEED)
        dd = synth.make_wavlm_discriminator_state_dict(HF_CONFIGS[cname]["hidden_size"], slm_layers(cname),
                                                       INITIAL_CHANNEL[cname], DSEED)
        _W[cname] = ((sd, {k: v.double() for k, v in sd.items()}), (dd, {k: v.double() for k, v in dd.items()}))
    return _W[cname]


def inputs(shape, seed):
    """(wav, y_rec) float32 [rows, samples]: a few sinusoids under noise, and the same with a perturbation -- a
    generated waveform is close to the real one, not independent of it."""
    rate, L, B = shape
    g = torch.Generator().manual_seed(int(seed))
    t = torch.arange(L, dtype=torch.float64)[None, :] / rate
    f = 80.0 + 3000.0 * torch.rand(B, 3, generator=g, dtype=torch.float64)
    a = 0.1 + 0.2 * torch.rand(B, 3, generator=g, dtype=torch.float64)
    wav = sum(a[:, i:i + 1] * torch.sin(2 * math.pi * f[:, i:i + 1] * t) for i in range(3))
    wav = wav + 0.05 * torch.randn(B, L, generator=g, dtype=torch.float64)
    rec = 0.9 * wav + 0.08 * torch.randn(B, L, generator=g, dtype=torch.float64)
    return wav.float(), rec.float()


# ---- the resampler -----------------------------------------------------------------------------------------------------
def resample_kernel(orig_freq, new_freq, width_taps=6, rolloff=0.99):
    """-> (float32 kernel [new, 2 width + orig], width, orig, new): sinc(pi t) cos^2(pi t / 12) base / orig at
    t = (-j / new + (i - width) / orig) base clamped to +-6, in float64, rounded once."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * rolloff
    width = math.ceil(width_taps * o / base)
    i = (torch.arange(2 * width + o, dtype=torch.float64) - width) / o
    j = -torch.arange(n, dtype=torch.float64) / n
    t = ((j[:, None] + i[None, :]) * base).clamp(-width_taps, width_taps)
    sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(math.pi * t) / (math.pi * t + (t == 0)))
    return (sinc * torch.cos(math.pi * t / (2 * width_taps)) ** 2 * (base / o)).float(), width, o, n


def resample(x, orig_freq, new_freq, dtype=torch.float64):
    """x [..., L] -> [..., ceil(new L / orig)] at `dtype`: zero-pad by (width, width + orig), frames of 2 width + orig
    samples at stride orig against the kernel, the `new` outputs of a frame interleaved, cropped."""
    if int(orig_freq) == int(new_freq):
        return x.to(dtype)
    k, width, o, n = resample_kernel(orig_freq, new_freq)
    shape = x.shape
    x = F.pad(x.to(dtype).reshape(-1, shape[-1]), (width, width + o))
    y = F.conv1d(x[:, None], k.to(dtype=dtype, device=x.device)[:, None], stride=o)
    y = y.transpose(1, 2).reshape(x.shape[0], -1)[:, :-(-n * shape[-1] // o)]
    return y.reshape(*shape[:-1], y.shape[-1])


class ResampleStandIn:
    """torchaudio.transforms.Resample's surface for the reference's WavLMLoss where torchaudio is not installed."""

    def __init__(self, orig_freq=16000, new_freq=16000, **kw):
        self.orig_freq, self.new_freq = orig_freq, new_freq

    def __call__(self, waveform):
        return resample(waveform, self.orig_freq, self.new_freq, waveform.dtype)

    def to(self, *a, **k):
        return self


# ---- WavLM ---------------------------------------------------------------------------------------------------------------
def frames(cname, L):
    for k, s in zip(HF_CONFIGS[cname]["conv_kernel"], HF_CONFIGS[cname]["conv_stride"]):
        L = (L - k) // s + 1 if L >= k else 0
    return L


def conv0_norm(W, cname, x, fault=None):
    """x [B, L] -> gelu(group norm over time per channel (conv 0 (x))) [B, T0, C]."""
    c = HF_CONFIGS[cname]
    y = F.conv1d(x[:, None], W["feature_extractor.conv_layers.0.conv.weight"], stride=c["conv_stride"][0])
    mean = y.mean(2, keepdim=True)
    var = y.var(2, keepdim=True, unbiased=fault == "unbiased_var")
    y = (y - mean) / torch.sqrt(var + 1e-5)
    y = y * W["feature_extractor.conv_layers.0.layer_norm.weight"][None, :, None] + \
        W["feature_extractor.conv_layers.0.layer_norm.bias"][None, :, None]
    return F.gelu(y).transpose(1, 2)


def conv(W, cname, i, x, fault=None):
    """Conv layer i >= 1 and GELU on x [B, Tin, C] -> [B, Tout, C]."""
    w = W[f"feature_extractor.conv_layers.{i}.conv.weight"]
    if fault == "conv_tap" and i == 1:
        w = w.clone()
        w[:, :, -1] = 0
    return F.gelu(F.conv1d(x.transpose(1, 2), w, stride=HF_CONFIGS[cname]["conv_stride"][i])).transpose(1, 2)


def features(W, cname, x, fault=None):
    h = conv0_norm(W, cname, x, fault)
    for i in range(1, len(HF_CONFIGS[cname]["conv_dim"])):
        h = conv(W, cname, i, h, fault)
    return h


def project(W, x):
    n = F.layer_norm(x, (x.shape[-1],), W["feature_projection.layer_norm.weight"], W["feature_projection.layer_norm.bias"], 1e-5)
    return F.linear(n, W["feature_projection.projection.weight"], W["feature_projection.projection.bias"])


def pos_conv_weight(W):
    g = W["encoder.pos_conv_embed.conv.parametrizations.weight.original0"]
    v = W["encoder.pos_conv_embed.conv.parametrizations.weight.original1"]
    return v * (g / torch.linalg.vector_norm(v, ord=2, dim=(0, 1), keepdim=True))


def pos_conv(W, cname, x, fault=None):
    """gelu(grouped conv, padding k / 2, the last column of an even kernel dropped) on x [B, T, H] -> [B, T, H]."""
    c = HF_CONFIGS[cname]
    k = c["num_conv_pos_embeddings"]
    y = F.conv1d(x.transpose(1, 2), pos_conv_weight(W), W["encoder.pos_conv_embed.conv.bias"], padding=k // 2,
                 groups=c["num_conv_pos_embedding_groups"])
    if k % 2 == 0:
        y = y[:, :, 1:] if fault == "pos_shift" else y[:, :, :-1]
    return F.gelu(y).transpose(1, 2)


def buckets(cname, T, fault=None):
    """[T, T] int64: the bucket of key j - query i (T5's bidirectional rule, float32 log ramp)."""
    c = HF_CONFIGS[cname]
    nb = c["num_buckets"] // 2
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    rel = i - j if fault == "rel_sign" else j - i
    out = (rel > 0).long() * nb
    p = rel.abs()
    max_exact = nb // 2
    large = torch.log(p.float() / max_exact) / math.log(c["max_bucket_distance"] / max_exact) * (nb - max_exact)
    large = (max_exact + large).long().clamp(max=nb - 1)
    if fault == "ramp_clamp":
        large = torch.full_like(large, nb - 1)
    return out + torch.where(p < max_exact, p, large)


def gate(W, cname, layer, x, fault=None):
    """x [B, T, H] -> [B, heads, T]: a (b const - 1) + 2 with a, b the sigmoids of the two half sums of
    gru_rel_pos_linear(x viewed as heads)."""
    heads = HF_CONFIGS[cname]["num_attention_heads"]
    B, T, H = x.shape
    p = f"encoder.layers.{layer}.attention."
    xh = x.reshape(B, T, heads, H // heads).transpose(1, 2)
    pr = F.linear(xh, W[p + "gru_rel_pos_linear.weight"], W[p + "gru_rel_pos_linear.bias"]).reshape(B, heads, T, 2, 4).sum(-1)
    a, b = torch.sigmoid(pr).unbind(-1)
    g = a * (b * W[p + "gru_rel_pos_const"].reshape(1, heads, 1) - 1.0) + 2.0
    return torch.ones_like(g) if fault == "gate_one" else g


def attention(W, cname, layer, x, qkv, fault=None):
    """qkv [B, T, 3 H] (q | k | v) and the layer's input x -> [B, T, H]: softmax(q k^T / sqrt(dk) + gate bias) v with
    bias[h, i, j] = layer 0's rel_attn_embed[bucket(j - i), h]."""
    heads = HF_CONFIGS[cname]["num_attention_heads"]
    B, T, H3 = qkv.shape
    H = H3 // 3
    dk = H // heads
    q, k, v = (t.reshape(B, T, heads, dk).transpose(1, 2) for t in qkv.split(H, dim=2))
    emb = W["encoder.layers.0.attention.rel_attn_embed.weight"]
    bias = emb[buckets(cname, T, fault)].permute(2, 0, 1)
    if fault == "own_table" and layer > 0:
        bias = torch.zeros_like(bias)
    s = q @ k.transpose(2, 3) / math.sqrt(dk) + gate(W, cname, layer, x, fault)[:, :, :, None] * bias[None]
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, H)


def qkv_proj(W, layer, x):
    p = f"encoder.layers.{layer}.attention."
    w = torch.cat([W[p + f"{n}_proj.weight"] for n in "qkv"], 0)
    b = torch.cat([W[p + f"{n}_proj.bias"] for n in "qkv"], 0)
    return F.linear(x, w, b)


def layer(W, cname, i, x, fault=None):
    p = f"encoder.layers.{i}."
    H = x.shape[-1]
    a = attention(W, cname, i, x, qkv_proj(W, i, x), fault)
    a = F.linear(a, W[p + "attention.out_proj.weight"], W[p + "attention.out_proj.bias"])
    h = F.layer_norm(x + a, (H,), W[p + "layer_norm.weight"], W[p + "layer_norm.bias"], 1e-5)
    f = F.gelu(F.linear(h, W[p + "feed_forward.intermediate_dense.weight"], W[p + "feed_forward.intermediate_dense.bias"]))
    f = F.linear(f, W[p + "feed_forward.output_dense.weight"], W[p + "feed_forward.output_dense.bias"])
    return F.layer_norm(h + f, (H,), W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], 1e-5)


def encoder_input(W, cname, proj, fault=None):
    H = proj.shape[-1]
    return F.layer_norm(proj + pos_conv(W, cname, proj, fault), (H,), W["encoder.layer_norm.weight"],
                        W["encoder.layer_norm.bias"], 1e-5)


def hidden_states(W, cname, x, fault=None):
    """x [B, L] at the WavLM rate -> list of num_hidden_layers + 1 tensors [B, T, H]."""
    h = encoder_input(W, cname, project(W, features(W, cname, x, fault)), fault)
    out = [h]
    for i in range(HF_CONFIGS[cname]["num_hidden_layers"]):
        h = layer(W, cname, i, h, fault)
        out.append(h)
    return out


# ---- the discriminator and the losses ----------------------------------------------------------------------------------
def _wn(D, name):
    v = D[name + ".weight_v"]
    return v * (D[name + ".weight_g"] / torch.linalg.vector_norm(v, ord=2, dim=(1, 2), keepdim=True))


def disc_pre(D, hidden, fault=None):
    """hidden: list of [R, T, H] -> [R, T, c0]; input channel layer * H + c (c * layers + layer under `disc_order`)."""
    x = torch.stack(hidden, dim=1).transpose(-1, -2)  # [R, layers, H, T]
    if fault == "disc_order":
        x = x.transpose(1, 2)
    return F.conv1d(x.flatten(1, 2), _wn(D, "pre"), D["pre.bias"]).transpose(1, 2)


def disc_convs(D, pre):
    """pre [R, T, c0] -> [R, T]."""
    x = pre.transpose(1, 2)
    for i in range(3):
        x = F.leaky_relu(F.conv1d(x, _wn(D, f"convs.{i}"), D[f"convs.{i}.bias"], padding=2), 0.1)
    return F.conv1d(x, _wn(D, "conv_post"), D["conv_post.bias"], padding=1).flatten(1, -1)


def disc(D, hidden, fault=None):
    return disc_convs(D, disc_pre(D, hidden, fault))


def losses(hidden, d, B):
    """(loss_lm, loss_lm_gen, loss_slm) and their per-utterance [B] forms from the 2B-row hidden states and d [2B, T]."""
    lm = sum((h[:B] - h[B:]).abs().mean() for h in hidden)
    lm_pu = sum((h[:B] - h[B:]).abs().flatten(1).mean(1) for h in hidden)
    gen, gen_pu = ((1 - d[B:]) ** 2).mean(), ((1 - d[B:]) ** 2).mean(1)
    slm = ((1 - d[:B]) ** 2).mean() + (d[B:] ** 2).mean()
    slm_pu = ((1 - d[:B]) ** 2).mean(1) + (d[B:] ** 2).mean(1)
    return dict(loss_lm=lm, loss_lm_gen=gen, loss_slm=slm, loss_lm_per_utt=lm_pu, loss_lm_gen_per_utt=gen_pu,
                loss_slm_per_utt=slm_pu)


def forward(cname, shape, wav, rec, dtype=torch.float64, fault=None):
    """Everything of one case at `dtype` -> dict: resampled [2B, L'], hidden (list of [2B, T, H]), pre, d [2B, T] and
    the losses.  Rows: wav's, then rec's."""
    (sd, W64), (dd, D64) = weights(cname)
    W, D = (W64, D64) if dtype == torch.float64 else (sd, dd)
    x = resample(torch.cat([wav, rec], 0), shape[0], SLM_SR, dtype)
    hidden = hidden_states(W, cname, x, fault)
    pre = disc_pre(D, hidden, fault)
    d = disc_convs(D, pre)
    out = dict(resampled=x, hidden=hidden, pre=pre, d=d)
    out.update(losses(hidden, d, wav.shape[0]))
    return out


STAGES = ("resample", "conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "project", "pos_conv", "attention",
          "layer", "disc_pre", "disc_convs", "reduce_lm", "reduce_lm_gen", "reduce_slm")


def stage_cases(cname, shape, wav, rec):
    """The inputs of every stand-alone stage, taken from the float64 forward pass and rounded to float32 (what the
    device entry receives), and the function that evaluates the stage on them at W's dtype:
    {stage: (dict of float32 inputs, fn(W, D, inputs) -> tensor)}."""
    (sd, W64), (dd, D64) = weights(cname)
    f32 = lambda t: t.to(torch.float32)  # noqa: E731
    cast = lambda W, t: t.to(W["encoder.layer_norm.weight"].dtype)  # noqa: E731
    both = torch.cat([wav, rec], 0)
    x = resample(both, shape[0], SLM_SR)
    feats = [conv0_norm(W64, cname, x)]
    for i in range(1, 7):
        feats.append(conv(W64, cname, i, feats[-1]))
    proj = project(W64, feats[-1])
    h0 = encoder_input(W64, cname, proj)
    hidden = hidden_states(W64, cname, x)
    pre = disc_pre(D64, hidden)
    out = {
        "resample": (dict(x=both), lambda W, D, i: resample(i["x"], shape[0], SLM_SR, cast(W, i["x"]).dtype)),
        "conv0": (dict(x=f32(x)), lambda W, D, i: conv0_norm(W, cname, cast(W, i["x"]))),
        "project": (dict(x=f32(feats[-1])), lambda W, D, i: project(W, cast(W, i["x"]))),
        "pos_conv": (dict(x=f32(proj)), lambda W, D, i: pos_conv(W, cname, cast(W, i["x"]))),
        "attention": (dict(x=f32(h0), qkv=f32(qkv_proj(W64, 0, h0))),
                      lambda W, D, i: attention(W, cname, 0, cast(W, i["x"]), cast(W, i["qkv"]))),
        "layer": (dict(x=f32(h0)), lambda W, D, i: layer(W, cname, 0, cast(W, i["x"]))),
        "disc_pre": (dict(hidden=[f32(h) for h in hidden]), lambda W, D, i: disc_pre(D, [cast(W, h) for h in i["hidden"]])),
        "disc_convs": (dict(pre=f32(pre)), lambda W, D, i: disc_convs(D, cast(W, i["pre"]))),
    }
    # the reductions alone, on given hidden states and discriminator outputs: the total, then the B per-utterance values
    d64 = disc_convs(D64, pre)
    B = wav.shape[0]

    def reduce(key):
        def fn(W, D, i):
            r = losses([cast(W, h) for h in i["hidden"]], cast(W, i["d"]), B)
            return torch.cat([r[key].reshape(1), r[key + "_per_utt"]])
        return (dict(hidden=[f32(h) for h in hidden], d=f32(d64)), fn)
    out.update(reduce_lm=reduce("loss_lm"), reduce_lm_gen=reduce("loss_lm_gen"), reduce_slm=reduce("loss_slm"))
    for n in range(1, 7):
        out[f"conv{n}"] = (dict(x=f32(feats[n - 1])), (lambda n: lambda W, D, i: conv(W, cname, n, cast(W, i["x"])))(n))
    return out


# ---- measures ------------------------------------------------------------------------------------------------------------
gates, worst, gate_of, fixture_gate, within = fo.gates, fo.worst, fo.gate, fo.fixture_gate, fo.within


def rel_err(got, ref):
    """(|got - ref| / |ref|, the same): a scalar's figure in the (rel, local) pair form of the tensor gates."""
    e = abs(float(got) - float(ref)) / max(abs(float(ref)), 1e-30)
    return e, e


def load_fixture(cname, shape):
    return np.load(os.path.join(GOLDEN, case_name(cname, shape) + ".npz"))


_REF = {}


def reference(cname, shape):
    """(wav, rec, float64 forward dict) of a fixture case, computed once per process and left unchanged."""
    key = (cname, tuple(shape))
    if key not in _REF:
        c = load_fixture(cname, shape)
        wav, rec = inputs(shape, int(c["input_seed"]))
        _REF[key] = (wav, rec, forward(cname, shape, wav, rec))
    return _REF[key]
