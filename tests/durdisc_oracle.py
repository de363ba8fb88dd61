"""Shared by tests/test_cpu_durdisc.py, tests/test_gpu_durdisc.py and tests/golden/make_golden_durdisc.py: the VITS2
duration discriminators (model/discriminators.py:287-449) and their adversarial losses (losses.py:17-42 as train.py:441-453,
481-495 calls them) restated on F.conv1d at the dtype of the weights, independent of the device code.

forward(W, version, x, x_mask, dur_r, dur_hat) -> the five stages over which the device is gated (STAGES): the two trunk
maps [B, F, Tx], the two head maps over 2B rows (dur_r's rows first; version 2: after ReLU + LayerNorm, before the next
mask) and the probabilities [2B, Tx].  losses(prob, mask, version) -> the reference's scalars for the class in use --
version 1 returns two tensors, so the reference's zip walks their batch rows: B terms, each a mean over one utterance's Tx
padded positions, summed; version 2 returns two one-element lists: one term over B * Tx -- and the masked per-utterance
means.

The gates.  Stages: `rel = rms(d) / rms(ref)` and `local = max|d| / rms(ref)` over a whole stage, d = device - float64
oracle.  Scalars: |d| / ref (every term of these sums is non-negative).  FLOOR holds the worst figure of the oracle at
float32 against the oracle at float64 over SHAPES, per version; the gates are GATE_FACTOR (4, the project's convention) x
the floor.  `fault` injects the faults of the gate-sensitivity tests."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import decoder_input as di, encoder_input as ei
from wetts_amd import synth

WSEED = 31
GATE_FACTOR = ei.GATE_FACTOR
CHANNELS, KERNEL = 192, 3  # train.py:144-160: (hidden_channels, hidden_channels, 3, 0.1)
EPS = 1e-5
STAGES = ("conv_1", "conv_2", "pre_out_conv_1", "pre_out_conv_2", "prob")
VERSIONS = (1, 2)
_RAGGED16 = (7, 31, 1, 19, 30, 12, 31, 2, 25, 16, 9, 28, 3, 31, 22, 14)
# (B, Tx, lens): both neighbours of every tap are padding | a small ragged batch | a 64-column tile straddles a row join,
# a one-phoneme row | an empty row, a tile holding three rows' ends | columns (496, 992 in the head) not a multiple of 64
SHAPES = ((1, 1, (1,)), (2, 5, (5, 2)), (3, 65, (65, 1, 40)), (5, 129, (129, 0, 1, 64, 100)), (16, 31, _RAGGED16))
FIXTURE_SHAPES = SHAPES[:4]
FAULTS = ("drop_tap", "no_mask_before_pre_out_conv_1", "no_mask_after_norm", "relu_after_norm", "unbiased_variance",
          "norm_over_time", "swap_durations")
# the stage a fault first touches, and the versions it exists in
FAULT_STAGE = dict(drop_tap="conv_2", no_mask_before_pre_out_conv_1="pre_out_conv_1", no_mask_after_norm="conv_2",
                   relu_after_norm="conv_1", unbiased_variance="conv_1", norm_over_time="conv_1", swap_durations="prob")
FAULT_VERSIONS = dict(drop_tap=(1, 2), no_mask_before_pre_out_conv_1=(1, 2), no_mask_after_norm=(2,),
                      relu_after_norm=(2,), unbiased_variance=(2,), norm_over_time=(2,), swap_durations=(1, 2))


def weights(version, seed=WSEED):
    """(reference-keyed float32 state dict, the same widened to float64)."""
    sd = synth.make_duration_discriminator_state_dict(version, seed, CHANNELS, CHANNELS, KERNEL)
    return sd, {k: v.to(torch.float64) for k, v in sd.items()}


def case_seed(B, Tx):
    return 9000 + 17 * B + Tx


# log(w + 1e-6) for the integer durations 0..19 from the scalar double-precision log, rounded to float32 once: the
# vectorised float32 log of torch's CPU kernels differs between processors in the last bit, and the fixtures' input
# digests must not
_LOG_W = torch.tensor([math.log(k + 1e-6) for k in range(20)], dtype=torch.float64).to(torch.float32)


def inputs(B, Tx, lens, seed, channels=CHANNELS):
    """(hidden_x [B, C, Tx] -- deliberately NOT pre-masked --, x_mask [B, 1, Tx], dur_r, dur_hat [B, 1, Tx]) float32:
    dur_r = log(w + 1e-6) * mask for integer durations w, as models.py:201 forms logw_; dur_hat a noisy copy."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, channels, Tx, generator=g)
    mask = (torch.arange(Tx)[None, :] < torch.tensor(lens)[:, None]).to(torch.float32).unsqueeze(1)
    w = torch.randint(1, 20, (B, 1, Tx), generator=g)
    dur_r = _LOG_W[w] * mask
    dur_hat = (dur_r + 0.5 * torch.randn(B, 1, Tx, generator=g)) * mask
    return x, mask, dur_r, dur_hat


def _norm(W, name, x, fault):
    """normalization.py:16-19: F.layer_norm over the channels (biased variance, eps 1e-5)."""
    if fault == "norm_over_time" and name == "norm_1":
        m, v = x.mean(2, keepdim=True), x.var(2, unbiased=False, keepdim=True)
    else:
        m, v = x.mean(1, keepdim=True), x.var(1, unbiased=(fault == "unbiased_variance" and name == "norm_1"), keepdim=True)
    return (x - m) / torch.sqrt(v + EPS) * W[name + ".gamma"][None, :, None] + W[name + ".beta"][None, :, None]


def _conv(W, name, x, version, norm, fault):
    w = W[name + ".weight"]
    if fault == "drop_tap" and name == "conv_2":
        w = w.clone()
        w[:, :, 2] = 0
    x = F.conv1d(x, w, W[name + ".bias"], 1, w.shape[2] // 2)
    if version == 2:
        if fault == "relu_after_norm" and name == "conv_1":
            return torch.relu(_norm(W, norm, x, fault))
        x = _norm(W, norm, torch.relu(x), fault)
    return x


def forward(W, version, x, x_mask, dur_r, dur_hat, fault=None):
    """{stage: tensor} at the dtype of W (discriminators.py:334-369 / 418-449)."""
    dt = W["conv_1.bias"].dtype
    x, m, dur_r, dur_hat = (t.to(dt) for t in (x, x_mask, dur_r, dur_hat))
    if fault == "swap_durations":
        dur_r, dur_hat = dur_hat, dur_r
    B = x.shape[0]
    t1 = _conv(W, "conv_1", x * m, version, "norm_1", fault)
    t2 = _conv(W, "conv_2", t1 if fault == "no_mask_after_norm" else t1 * m, version, "norm_2", fault)
    m2 = torch.cat([m, m], 0)
    dur = F.conv1d(torch.cat([dur_r, dur_hat], 0), W["dur_proj.weight"], W["dur_proj.bias"])
    h = torch.cat([torch.cat([t2, t2], 0), dur], 1)
    h1 = _conv(W, "pre_out_conv_1", h if fault == "no_mask_before_pre_out_conv_1" else h * m2, version, "pre_out_norm_1",
               fault)
    h2 = _conv(W, "pre_out_conv_2", h1 * m2, version, "pre_out_norm_2", fault)
    z = F.linear((h2 * m2).transpose(1, 2), W["output_layer.0.weight"], W["output_layer.0.bias"])
    return {"conv_1": t1, "conv_2": t2, "pre_out_conv_1": h1, "pre_out_conv_2": h2, "prob": torch.sigmoid(z)[:, :, 0]}


def reference_form(prob, version):
    """What the class's forward returns: [prob_r, prob_g] (version 1) or [[prob_r], [prob_g]] (version 2), [B, Tx, 1]."""
    B = prob.shape[0] // 2
    r, g = prob[:B].unsqueeze(2), prob[B:].unsqueeze(2)
    return [r, g] if version == 1 else [[r], [g]]


SCALARS = ("disc", "disc_r", "disc_g", "gen", "gen_terms", "disc_per_utt", "gen_per_utt")


def losses(prob, x_mask, version, one_mean=False):
    """losses.py:17-42 over reference_form(prob) as train.py calls them -> dict of tensors at prob's dtype: disc, disc_r,
    disc_g, gen, gen_terms (B terms for version 1, one for version 2; `one_mean`: the fault of forming version 1's as one
    mean), and disc_per_utt / gen_per_utt [B], each utterance's mean over its own phonemes (NaN without any)."""
    B = prob.shape[0] // 2
    r, g = prob[:B], prob[B:]
    m = x_mask.reshape(B, -1).to(prob.dtype)
    if version == 1 and not one_mean:
        dr, dg, gn = ((1 - r) ** 2).mean(1), (g ** 2).mean(1), ((1 - g) ** 2).mean(1)
    else:
        dr, dg, gn = ((1 - r) ** 2).mean().reshape(1), (g ** 2).mean().reshape(1), ((1 - g) ** 2).mean().reshape(1)
    n = m.sum(1)
    return dict(disc=(dr + dg).sum(), disc_r=dr, disc_g=dg, gen=gn.sum(), gen_terms=gn,
                disc_per_utt=((((1 - r) ** 2) + g ** 2) * m).sum(1) / n, gen_per_utt=(((1 - g) ** 2) * m).sum(1) / n)


def gates(got, ref):
    return di.gates(got, ref)


def scalar_err(got, ref):
    """max |got - ref| / ref over the entries (every term of these sums is non-negative).  An entry that is NaN in the
    reference (an utterance without phonemes) must be NaN in `got` and is left out of the maximum."""
    got = torch.as_tensor(got).double().reshape(-1)
    ref = torch.as_tensor(ref).double().reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert bool((torch.isnan(got) == nan).all()), (got, ref)
    if bool(nan.all()):
        return 0.0
    return float(((got[~nan] - ref[~nan]).abs() / ref[~nan].clamp_min(1e-300)).max())


def measure(st, ls, ref_st, ref_ls):
    """{stage: (rel, local), scalar: figure} of (stages, losses) against the float64 (stages, losses)."""
    out = {s: gates(st[s].detach().cpu().contiguous(), ref_st[s].contiguous()) for s in STAGES}
    for s in SCALARS:
        out[s] = scalar_err(ls[s].detach().cpu(), ref_ls[s])
    return out


def worst(acc, m):
    if acc is None:
        return dict(m)
    for s in STAGES:
        acc[s] = (max(acc[s][0], m[s][0]), max(acc[s][1], m[s][1]))
    for s in SCALARS:
        acc[s] = max(acc[s], m[s])
    return acc


_REF = {}


def reference(version, B, Tx, lens):
    """((x, x_mask, dur_r, dur_hat), float64 stages, float64 losses) of a case, computed once per process and left
    unchanged."""
    key = (version, B, Tx)
    if key not in _REF:
        inp = inputs(B, Tx, lens, case_seed(B, Tx))
        st = forward(weights(version)[1], version, *inp)
        _REF[key] = (inp, st, losses(st["prob"], inp[1], version))
    return _REF[key]


def floor(version, shapes=SHAPES):
    """Worst figures of the float32 oracle against the float64 oracle over `shapes`."""
    W32 = weights(version)[0]
    acc = None
    for B, Tx, lens in shapes:
        inp, rs, rl = reference(version, B, Tx, lens)
        st = forward(W32, version, *inp)
        acc = worst(acc, measure(st, losses(st["prob"], inp[1], version), rs, rl))
    return acc


HALF_ULP = 2.0 ** -24  # the worst relative rounding error of one float32 value


def gate(version, stage, factor=GATE_FACTOR):
    """4 x floor: a stage's (rel, local) or a scalar's figure.  A scalar's floor is one float32 number's distance from
    float64, measured on five cases: where it came out below half an ulp -- the error a correctly rounded float32 result
    may have -- half an ulp is taken, a figure of the number format and not of a lucky draw."""
    if stage in STAGES:
        return tuple(factor * v for v in FLOOR[version][stage])
    return factor * max(FLOOR[version][stage], HALF_ULP)


def fixture_gate(version, stage):
    """Against the reference's stored float32 values, which are themselves one floor away from float64: 4 + 1 floors."""
    return gate(version, stage, GATE_FACTOR + 1)


def check(version, m, where=""):
    """Asserts measurement `m` against the gates; returns the worst multiple of a gate (1 = at the gate)."""
    top = 0.0
    for s in STAGES:
        g = gate(version, s)
        top = max(top, m[s][0] / g[0], m[s][1] / g[1])
        assert m[s][0] <= g[0] and m[s][1] <= g[1], \
            f"{where} {s}: rel {m[s][0]:.3e} (gate {g[0]:.3e}) local {m[s][1]:.3e} (gate {g[1]:.3e})"
    for s in SCALARS:
        top = max(top, m[s] / gate(version, s))
        assert m[s] <= gate(version, s), f"{where} {s}: {m[s]:.3e} (gate {gate(version, s):.3e})"
    return top


# Worst figures of oracle-at-float32 against oracle-at-float64 over SHAPES (weights WSEED, inputs case_seed), measured on
# one CPU (torch CPU kernels): (rel, local) per stage, |d| / ref for the scalars.
FLOOR = {
    1: dict(conv_1=(1.41e-07, 1.3e-06), conv_2=(2e-07, 1.56e-06), pre_out_conv_1=(1.7e-07, 1.36e-06),
            pre_out_conv_2=(2.3e-07, 1.77e-06), prob=(9.72e-08, 4.84e-07), disc=1.4e-07, disc_r=1.85e-07, disc_g=1.66e-07,
            gen=6.51e-08, gen_terms=1.79e-07, disc_per_utt=2.24e-07, gen_per_utt=5.45e-07),
    2: dict(conv_1=(1.62e-07, 1.45e-06), conv_2=(2.52e-07, 1.97e-06), pre_out_conv_1=(2.24e-07, 2.06e-06),
            pre_out_conv_2=(3.26e-07, 2.89e-06), prob=(2.04e-07, 7.24e-07), disc=1.3e-07, disc_r=1.47e-07, disc_g=3.16e-07,
            gen=1.17e-07, gen_terms=1.17e-07, disc_per_utt=1.52e-07, gen_per_utt=2.12e-07),
}
