"""Seeded synthetic checkpoints (there is no network for real ones).

Produces a state_dict keyed and shaped exactly like the reference's `G_*.pth["model"]`
(old-style weight-norm pairs `weight_g`/`weight_v` on dec.ups / dec.resblocks / flow WN layers,
SURVEY.md §5 "Checkpoint / resume") so that
  * tests/golden/make_golden.py can load it into the *reference* SynthesizerTrn unchanged, and
  * wetts_amd.checkpoint.pack_blob exercises the real fold + repack path.
Layers the reference zero-initialises (flow `post`, ConvFlow `proj`) get non-zero values so the
couplings / splines are not identities.  The duration heads are biased to ~6 frames per phoneme
(SURVEY.md §8d "duration pinning"): SDP via its ElementwiseAffine, DP via proj.bias = log 6.
"""
import math
import re

import torch

from . import checkpoint

_WN_PATTERNS = [
    re.compile(r"^dec\.ups\.\d+\.weight$"),
    re.compile(r"^dec\.resblocks\.\d+\.convs[12]?\.\d+\.weight$"),
    re.compile(r"^flow\.flows\.\d+\.enc\.(in_layers|res_skip_layers)\.\d+\.weight$"),
    re.compile(r"^flow\.flows\.\d+\.enc\.cond_layer\.weight$"),
]


def is_weight_normed(name):
    return any(p.match(name) for p in _WN_PATTERNS)


def _std_for(name, shape, cfg):
    """Effective weight std chosen so activations stay O(1) through ~70 conv layers."""
    if name.endswith("emb.weight"):
        return cfg.hidden_channels ** -0.5
    if name == "emb_g.weight":
        return 1.0
    if "emb_rel_" in name:
        return shape[-1] ** -0.5
    if name.startswith("dec.ups."):
        cin, _, k = shape
        i = int(name.split(".")[2])
        u = cfg.upsample_rates[i]
        return 1.0 / math.sqrt(cin * k / u)
    if name.startswith("dec.resblocks."):
        return 0.5 / math.sqrt(shape[1] * shape[2])
    if name == "dec.conv_post.weight":
        return 0.7 / math.sqrt(shape[1] * shape[2])
    if name.endswith(".scale"):  # ConvNeXtLayer.scale: the reference initialises it to 1/num_layers
        return 0.0
    if name == "dec.out_conv.weight":  # log-magnitude / phase head: keep exp() well below its clamp
        return 0.5 / math.sqrt(shape[1])
    if name.endswith("cond.weight") or name.endswith("cond_layer.weight"):
        return 0.3 / math.sqrt(shape[1])
    if name.endswith("post.weight"):
        return 0.3 / math.sqrt(shape[1])
    if name == "enc_p.proj.weight":
        return 0.3 / math.sqrt(shape[1])
    if name == "dp.proj.weight" and shape[0] == 1:
        return 0.1 / math.sqrt(shape[1])
    if "convs_sep" in name:
        return 1.0 / math.sqrt(shape[2])
    fan_in = shape[1] * (shape[2] if len(shape) > 2 else 1)
    return 1.0 / math.sqrt(fan_in)


def make_state_dict(cfg, seed=0):
    """Reference-keyed float32 state_dict for `cfg` (wetts_config_t), deterministic in `seed`."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, _, _, shape in checkpoint.blob_layout(cfg):
        def rn(*s):
            return torch.randn(*s, generator=g, dtype=torch.float32)
        if name.endswith(".gamma"):
            sd[name] = 1.0 + 0.1 * rn(*shape)
        elif name.endswith(".beta") or name.endswith(".bias"):
            sd[name] = 0.05 * rn(*shape)
        elif name.endswith(".scale"):
            sd[name] = (1.0 / max(1, cfg.vocos_num_layers)) * (1.0 + 0.2 * rn(*shape))
        elif name == "dp.flows.0.m":
            sd[name] = 0.1 * rn(*shape)
        elif name == "dp.flows.0.logs":
            sd[name] = 0.1 * rn(*shape)
        else:
            w = rn(*shape) * _std_for(name, shape, cfg)
            if is_weight_normed(name):
                dims = tuple(range(1, w.dim()))
                norm = torch.linalg.vector_norm(w, ord=2, dim=dims, keepdim=True)
                gain = norm * (1.0 + 0.05 * rn(shape[0], *([1] * (w.dim() - 1))))
                base = name[:-len("weight")]
                sd[base + "weight_g"] = gain
                sd[base + "weight_v"] = w
            else:
                sd[name] = w
    # duration pinning: ~6 frames / phoneme
    if cfg.use_sdp:
        # reverse EA: logw = (z0 - m0) * exp(-logs0) = 0.1*z0 + log 6
        sd["dp.flows.0.logs"][0, 0] = math.log(10.0)
        sd["dp.flows.0.m"][0, 0] = -10.0 * math.log(6.0)
    else:
        sd["dp.proj.bias"][0] = math.log(6.0)
    return sd


_POSTERIOR_WN = re.compile(r"^enc_q\.enc\.(in_layers\.\d+|res_skip_layers\.\d+|cond_layer)\.weight$")


def make_posterior_state_dict(cfg, spec_channels, seed=0):
    """Reference-keyed `enc_q.*` tensors (PosteriorEncoder, encoders.py:60-99) for `cfg`, deterministic in `seed`, from
    a generator of their own (make_state_dict's stream, and so every stored blob checksum, is untouched).  The WN layers
    carry weight-norm pairs like a reference checkpoint (modules.py:35,49,58).  The pre conv is scaled for linear
    spectrogram input (magnitudes of up to a few hundred for a loud harmonic at n_fft 1024) and the projection for
    log-scales of a few tenths, so the posterior sample is O(1)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, _, _, shape in checkpoint.posterior_layout(cfg, spec_channels):
        w = torch.randn(*shape, generator=g, dtype=torch.float32)
        if name.endswith(".bias"):
            sd[name] = 0.05 * w
            continue
        if name == "enc_q.pre.weight":
            w = w * (0.05 / math.sqrt(shape[1]))
        elif name == "enc_q.proj.weight":
            w = w * (0.3 / math.sqrt(shape[1]))
        elif name.endswith("cond_layer.weight"):
            w = w * (0.3 / math.sqrt(shape[1]))
        elif ".res_skip_layers." in name:
            w = w * (0.5 / math.sqrt(shape[1]))
        else:
            w = w * (1.0 / math.sqrt(shape[1] * shape[2]))
        if _POSTERIOR_WN.match(name):
            dims = tuple(range(1, w.dim()))
            norm = torch.linalg.vector_norm(w, ord=2, dim=dims, keepdim=True)
            gain = norm * (1.0 + 0.05 * torch.randn(shape[0], *([1] * (w.dim() - 1)), generator=g))
            base = name[:-len("weight")]
            sd[base + "weight_g"] = gain
            sd[base + "weight_v"] = w
        else:
            sd[name] = w
    return sd


def make_duration_state_dict(cfg, seed=0):
    """Reference-keyed tensors of the duration posterior's blob (checkpoint.duration_layout: `dp.flows.1.*`,
    `dp.post_*`; StochasticDurationPredictor, duration_predictors.py:176-195) for `cfg`, deterministic in `seed`, from a
    generator of their own (make_state_dict's stream, and so every stored blob checksum, is untouched).  Values as
    make_state_dict gives the main ConvFlows: the `proj` the reference zero-initialises is non-zero, so no spline is
    the identity.  Empty for a DurationPredictor model."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, _, _, shape in checkpoint.duration_layout(cfg):
        w = torch.randn(*shape, generator=g, dtype=torch.float32)
        if name.endswith(".gamma"):
            sd[name] = 1.0 + 0.1 * w
        elif name.endswith(".beta") or name.endswith(".bias"):
            sd[name] = 0.05 * w
        elif name.endswith(".m") or name.endswith(".logs"):  # post_flows.0: ElementwiseAffine
            sd[name] = 0.1 * w
        else:
            sd[name] = w * _std_for(name, shape, cfg)
    return sd


def make_discriminator_state_dict(seed=0):
    """Reference-keyed state_dict of MultiPeriodDiscriminator (discriminators.py:228-239) with old-style weight-norm
    pairs on every conv, as a `D_*.pth` holds them, deterministic in `seed` from a generator of its own.  Weights are
    randn * sqrt(2 / fan_in) with fan_in = (Cin / groups) * k, biases 0.05 * randn: activations stay O(1) through all
    seven layers (the reference's default init gives outputs of rms ~ 0.014 that are almost all bias, on which a parity
    test would test nothing)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, _, _, shape in checkpoint.disc_layout():
        base, kind = name.rsplit(".", 1)
        if kind == "bias":
            sd[name] = 0.05 * torch.randn(*shape, generator=g, dtype=torch.float32)
            continue
        fan_in = shape[1] * shape[2]
        w = torch.randn(*shape, generator=g, dtype=torch.float32) * math.sqrt(2.0 / fan_in)
        norm = torch.linalg.vector_norm(w, ord=2, dim=tuple(range(1, w.dim())), keepdim=True)
        sd[base + ".weight_g"] = norm * (1.0 + 0.05 * torch.randn(shape[0], *([1] * (w.dim() - 1)), generator=g))
        sd[base + ".weight_v"] = w
    return sd


def make_mrd_state_dict(seed=0):
    """Reference-keyed state_dict of MultiPeriodMultiResolutionDiscriminator (discriminators.py:256-268) with old-style
    weight-norm pairs on every conv, deterministic in `seed` from a generator of its own; values as
    make_discriminator_state_dict gives them (fan_in = Cin * kh * kw for the Conv2d stacks)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, _, _, shape in checkpoint.mrd_layout():
        base, kind = name.rsplit(".", 1)
        if kind == "bias":
            sd[name] = 0.05 * torch.randn(*shape, generator=g, dtype=torch.float32)
            continue
        fan_in = shape[1] * shape[2] * shape[3]
        w = torch.randn(*shape, generator=g, dtype=torch.float32) * math.sqrt(2.0 / fan_in)
        norm = torch.linalg.vector_norm(w, ord=2, dim=tuple(range(1, w.dim())), keepdim=True)
        sd[base + ".weight_g"] = norm * (1.0 + 0.05 * torch.randn(shape[0], *([1] * (w.dim() - 1)), generator=g))
        sd[base + ".weight_v"] = w
    return sd


def make_duration_discriminator_state_dict(version, seed=0, in_channels=192, filter_channels=192, kernel_size=3):
    """Reference-keyed state_dict of DurationDiscriminatorV1 (version 1) or V2 (version 2) (discriminators.py:287-449) as
    a `DUR_*.pth` holds it, deterministic in `seed` from a generator of its own.  Weights randn * fan_in ** -0.5, biases
    0.05 * randn, gamma = 1 + 0.1 * randn, beta = 0.1 * randn: with unit-variance inputs the probabilities stay away from
    0 and 1, so a parity test measures something.  Version 1 carries the `pre_out_norm_*` tensors its class constructs
    and never reads."""
    if version not in (1, 2):
        raise ValueError(f"version must be 1 or 2, got {version!r}")
    g = torch.Generator().manual_seed(int(seed))
    F_, K = int(filter_channels), int(kernel_size)
    sd = {}

    def conv(name, cout, cin, k):
        sd[name + ".weight"] = torch.randn(cout, cin, k, generator=g, dtype=torch.float32) * float(cin * k) ** -0.5
        sd[name + ".bias"] = 0.05 * torch.randn(cout, generator=g, dtype=torch.float32)

    def norm(name):
        sd[name + ".gamma"] = 1.0 + 0.1 * torch.randn(F_, generator=g, dtype=torch.float32)
        sd[name + ".beta"] = 0.1 * torch.randn(F_, generator=g, dtype=torch.float32)

    conv("conv_1", F_, int(in_channels), K)
    if version == 2:
        norm("norm_1")
    conv("conv_2", F_, F_, K)
    if version == 2:
        norm("norm_2")
    conv("dur_proj", F_, 1, 1)
    conv("pre_out_conv_1", F_, 2 * F_, K)
    norm("pre_out_norm_1")
    conv("pre_out_conv_2", F_, F_, K)
    norm("pre_out_norm_2")
    sd["output_layer.0.weight"] = torch.randn(1, F_, generator=g, dtype=torch.float32) * float(F_) ** -0.5
    sd["output_layer.0.bias"] = 0.05 * torch.randn(1, generator=g, dtype=torch.float32)
    return sd


def make_frontend_state_dict(cfg, seed=0):
    """Reference-keyed state_dict of the frontend (frontend/model.py:21-73) as frontend/train.py:215 saves it, for a
    frontend config dict (wetts_frontend_config_t's fields), deterministic in `seed` from a generator of its own; plain
    torch, no `transformers`.  Embeddings randn (their sum is normalised at once), Linear weights randn * fan_in ** -0.5,
    biases 0.05 * randn, LayerNorm weights 1 + 0.1 * randn and biases 0.1 * randn: every LayerNorm output has unit scale,
    so both classifiers' logits are O(1) and the probabilities stay away from 0 and 1.  Carries bert.pooler.* and
    bert.embeddings.position_ids, which the model constructs and the frontend never reads."""
    g = torch.Generator().manual_seed(int(seed))
    d = int(cfg["hidden_size"])
    sd = {}

    def lin(name, out, inp):
        sd[name + ".weight"] = torch.randn(out, inp, generator=g, dtype=torch.float32) * float(inp) ** -0.5
        sd[name + ".bias"] = 0.05 * torch.randn(out, generator=g, dtype=torch.float32)

    def norm(name):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(d, generator=g, dtype=torch.float32)
        sd[name + ".bias"] = 0.1 * torch.randn(d, generator=g, dtype=torch.float32)

    for name, rows in (("word", "vocab_size"), ("position", "max_position_embeddings"), ("token_type", "type_vocab_size")):
        sd[f"bert.embeddings.{name}_embeddings.weight"] = torch.randn(int(cfg[rows]), d, generator=g, dtype=torch.float32)
    sd["bert.embeddings.position_ids"] = torch.arange(int(cfg["max_position_embeddings"])).unsqueeze(0)
    norm("bert.embeddings.LayerNorm")
    for i in range(int(cfg["num_layers"])):
        p = f"bert.encoder.layer.{i}."
        for n in ("query", "key", "value"):
            lin(p + "attention.self." + n, d, d)
        lin(p + "attention.output.dense", d, d)
        norm(p + "attention.output.LayerNorm")
        lin(p + "intermediate.dense", int(cfg["intermediate_size"]), d)
        lin(p + "output.dense", d, int(cfg["intermediate_size"]))
        norm(p + "output.LayerNorm")
    lin("bert.pooler.dense", d, d)
    sd["transform.self_attn.in_proj_weight"] = torch.randn(3 * d, d, generator=g, dtype=torch.float32) * float(d) ** -0.5
    sd["transform.self_attn.in_proj_bias"] = 0.05 * torch.randn(3 * d, generator=g, dtype=torch.float32)
    lin("transform.self_attn.out_proj", d, d)
    lin("transform.linear1", int(cfg["transform_ff"]), d)
    lin("transform.linear2", d, int(cfg["transform_ff"]))
    norm("transform.norm1")
    norm("transform.norm2")
    lin("phone_classifier", int(cfg["num_polyphones"]), d)
    lin("prosody_classifier", int(cfg["num_prosody"]), d)
    return sd


def blob_checksum(blob):
    """Order-sensitive fingerprint of a float32 blob (guards golden fixtures against RNG drift)."""
    b = blob.detach().to(torch.float64)
    idx = torch.arange(1, b.numel() + 1, dtype=torch.float64)
    return float((b * torch.cos(idx * 0.37)).sum())


def make_wavlm_state_dict(config, seed=0):
    """transformers-keyed state_dict of a WavLMModel in the base architecture for a WavLM config dict (config.json's
    keys), deterministic in `seed` from a generator of its own; plain torch, no `transformers`.  Conv and Linear weights
    randn * sqrt(gain / fan_in) (gain 2 in front of a GELU), biases 0.05 * randn, norm weights 1 + 0.1 * randn and biases
    0.1 * randn, the positional conv as its weight-norm parametrisation (`original0` [1, 1, k], `original1`), the
    relative position table randn and gru_rel_pos_const 1 + 0.3 * randn: the bias and its gate move the attention
    logits by O(1), so a parity test sees them.  Carries masked_spec_embed, which the model constructs and never reads
    in evaluation."""
    g = torch.Generator().manual_seed(int(seed))
    c = config
    d, heads, ff = int(c["hidden_size"]), int(c["num_attention_heads"]), int(c["intermediate_size"])
    dims, kernels = [int(v) for v in c["conv_dim"]], [int(v) for v in c["conv_kernel"]]
    sd = {}

    def randn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float32)

    def lin(name, out, inp, gain=1.0):
        sd[name + ".weight"] = randn(out, inp) * math.sqrt(gain / inp)
        sd[name + ".bias"] = 0.05 * randn(out)

    def norm(name, n):
        sd[name + ".weight"] = 1.0 + 0.1 * randn(n)
        sd[name + ".bias"] = 0.1 * randn(n)

    sd["masked_spec_embed"] = randn(d)
    for i, (co, k) in enumerate(zip(dims, kernels)):
        ci = 1 if i == 0 else dims[i - 1]
        sd[f"feature_extractor.conv_layers.{i}.conv.weight"] = randn(co, ci, k) * math.sqrt(2.0 / (ci * k))
    norm("feature_extractor.conv_layers.0.layer_norm", dims[0])
    norm("feature_projection.layer_norm", dims[-1])
    lin("feature_projection.projection", d, dims[-1])
    pk, cg = int(c["num_conv_pos_embeddings"]), d // int(c["num_conv_pos_embedding_groups"])
    v = randn(d, cg, pk) * math.sqrt(2.0 / (cg * min(pk, 16)))
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = (
        torch.linalg.vector_norm(v, ord=2, dim=(0, 1), keepdim=True) * (1.0 + 0.05 * randn(1, 1, pk)))
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = v
    sd["encoder.pos_conv_embed.conv.bias"] = 0.05 * randn(d)
    norm("encoder.layer_norm", d)
    for i in range(int(c["num_hidden_layers"])):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            lin(p + "attention." + n, d, d)
        lin(p + "attention.gru_rel_pos_linear", 8, d // heads)
        sd[p + "attention.gru_rel_pos_const"] = 1.0 + 0.3 * randn(1, heads, 1, 1)
        if i == 0:
            sd[p + "attention.rel_attn_embed.weight"] = randn(int(c["num_buckets"]), heads)
        norm(p + "layer_norm", d)
        lin(p + "feed_forward.intermediate_dense", ff, d, 2.0)
        lin(p + "feed_forward.output_dense", d, ff)
        norm(p + "final_layer_norm", d)
    return sd


def make_wavlm_discriminator_state_dict(slm_hidden=768, slm_layers=13, initial_channel=64, seed=0):
    """Reference-keyed state_dict of WavLMDiscriminator (discriminators.py:452-485) with old-style weight-norm pairs on
    every conv, deterministic in `seed` from a generator of its own; values as make_discriminator_state_dict gives them
    (`pre`, which no activation follows, at gain 1)."""
    g = torch.Generator().manual_seed(int(seed))
    c0 = int(initial_channel)
    sd = {}
    for name, co, ci, k, gain in (("pre", c0, int(slm_hidden) * int(slm_layers), 1, 1.0), ("convs.0", 2 * c0, c0, 5, 2.0),
                                  ("convs.1", 4 * c0, 2 * c0, 5, 2.0), ("convs.2", 4 * c0, 4 * c0, 5, 2.0),
                                  ("conv_post", 1, 4 * c0, 3, 1.0)):
        w = torch.randn(co, ci, k, generator=g, dtype=torch.float32) * math.sqrt(gain / (ci * k))
        norm = torch.linalg.vector_norm(w, ord=2, dim=(1, 2), keepdim=True)
        sd[name + ".weight_g"] = norm * (1.0 + 0.05 * torch.randn(co, 1, 1, generator=g))
        sd[name + ".weight_v"] = w
        sd[name + ".bias"] = 0.05 * torch.randn(co, generator=g, dtype=torch.float32)
    return sd
