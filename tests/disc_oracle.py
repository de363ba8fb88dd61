"""Shared by tests/test_cpu_disc.py, tests/test_gpu_disc.py and tests/golden/make_golden_disc.py: MultiPeriodDiscriminator
(model/discriminators.py:21-124,228-254) and the three adversarial losses (losses.py:6-42) restated on F.conv1d at the
dtype of the weights, independent of the device code.  A period stack runs on the [rows = R * p][C][H] layout (row
(b, w) is x[b, h * p + w]), where every (k,1) Conv2d is a Conv1d; maps are handed out in the reference's shapes.

forward(W, y, y_hat) -> the 37 feature maps over the 2B utterances (real first), index 0..6 DiscriminatorS, then six per
period; the last map of a stack is its conv_post output.  losses(maps, B) -> the scalars of the three loss functions,
their per-layer / per-discriminator terms and their per-utterance forms.

The gates.  Tensors: `rel = rms(d) / rms(ref)` and `local = max|d| / rms(ref)` over a whole map, d = device - float64
oracle.  Scalars: |d| / (sum of the absolute terms) -- every term of these sums is non-negative, so that is |d| / ref.
FLOOR holds the worst figure of the oracle at float32 against the oracle at float64 over SHAPES; the gates are
GATE_FACTOR (4, the project's convention) x the floor.  `fault` injects the faults of the gate-sensitivity tests."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import decoder_input as di, encoder_input as ei
from wetts_amd import checkpoint, synth

PERIODS = (2, 3, 5, 7, 11)
SLOPE = 0.1
WSEED = 29
GATE_FACTOR = ei.GATE_FACTOR
N_MAPS = 37
# (B, T): H falls to 1 inside the stacks (12: period 11 reflects 10 samples); several ragged tiles, only 2, 5, 7 divide;
# every period divides (no reflect pad), H = 210 for p = 11; the segment every recipe trains at
SHAPES = ((1, 12), (2, 64), (2, 700), (3, 2310), (2, 8192))
FIXTURE_SHAPES = SHAPES[:4]
# (stride, pad, groups) of DiscriminatorS's six convs; the period stacks: stride 3 (last: 1), pad 2
S_SPEC = ((1, 7, 1), (4, 20, 4), (4, 20, 16), (4, 20, 64), (4, 20, 256), (1, 2, 1))
FAULTS = ("drop_tap", "zero_pad", "stride_phase", "group_swap", "slope")
# the map a fault first touches (index into the 37)
FAULT_STAGE = dict(drop_tap=7 + 6 * 2 + 2, zero_pad=7 + 6 * 1, stride_phase=7 + 6 * 3 + 1, group_swap=2, slope=0)


def weights(seed=WSEED):
    """(reference-keyed state dict with weight-norm pairs, folded float32 weights, the same widened to float64)."""
    sd = synth.make_discriminator_state_dict(seed)
    W32 = checkpoint.fold_weight_norm(sd)
    return sd, W32, {k: v.to(torch.float64) for k, v in W32.items()}


def inputs(B, T, seed):
    """(y, y_hat) [B, 1, T] float32: a recording-like signal and a noisy copy (so |r - g| is neither zero nor O(r))."""
    g = torch.Generator().manual_seed(seed)
    y = 0.5 * torch.randn(B, 1, T, generator=g)
    return y, y + 0.2 * torch.randn(B, 1, T, generator=g)


def case_seed(B, T):
    return 7000 + 13 * B + T


def map_index(d, layer):
    return layer if d == 0 else 7 + 6 * (d - 1) + layer


def stack_s(W, x, fault=None):
    """DiscriminatorS on x [R, 1, T] -> its seven maps [R, C, T']."""
    slope = 0.01 if fault == "slope" else SLOPE
    maps = []
    for m, (stride, pad, groups) in enumerate(S_SPEC):
        w = W[f"discriminators.0.convs.{m}.weight"]
        if fault == "group_swap" and m == 2:  # group 0 reads group 1's channels and the other way round
            x = torch.cat([x[:, 4:8], x[:, 0:4], x[:, 8:]], 1)
        x = F.leaky_relu(F.conv1d(x, w, W[f"discriminators.0.convs.{m}.bias"], stride, pad, 1, groups), slope)
        maps.append(x)
    maps.append(F.conv1d(x, W["discriminators.0.conv_post.weight"], W["discriminators.0.conv_post.bias"], 1, 1))
    return maps


def stack_p(W, d, x, fault=None):
    """DiscriminatorP(PERIODS[d - 1]) on x [R, 1, T] -> its six maps in the reference's shapes [R, C, H, p]."""
    p = PERIODS[d - 1]
    slope = 0.01 if fault == "slope" else SLOPE
    R, _, T = x.shape
    if T % p:
        n_pad = p - T % p
        x = F.pad(x, (0, n_pad)) if fault == "zero_pad" else F.pad(x, (0, n_pad), "reflect")
    H = x.shape[2] // p
    x = x.view(R, H, p).permute(0, 2, 1).reshape(R * p, 1, H)
    maps = []
    for m in range(5):
        w = W[f"discriminators.{d}.convs.{m}.weight"][..., 0]
        if fault == "drop_tap" and d == 3 and m == 2:
            w = w.clone()
            w[:, :, 3] = 0
        stride = 3 if m < 4 else 1
        if fault == "stride_phase" and d == 4 and m == 1:  # the windows start one sample late
            x = F.conv1d(F.pad(x, (1, 3)), w, W[f"discriminators.{d}.convs.{m}.bias"], stride, 0)[:, :, :(x.shape[2] - 1) // 3 + 1]
        else:
            x = F.conv1d(x, w, W[f"discriminators.{d}.convs.{m}.bias"], stride, 2)
        x = F.leaky_relu(x, slope)
        maps.append(x)
    maps.append(F.conv1d(x, W[f"discriminators.{d}.conv_post.weight"][..., 0], W[f"discriminators.{d}.conv_post.bias"], 1, 1))
    return [m.view(R, p, m.shape[1], m.shape[2]).permute(0, 2, 3, 1) for m in maps]


def forward(W, y, y_hat, fault=None):
    """The 37 maps over cat(y, y_hat) [2B, 1, T] at the dtype of W."""
    dt = W["discriminators.0.conv_post.bias"].dtype
    x = torch.cat([y, y_hat], 0).to(dt)
    maps = stack_s(W, x, fault)
    for d in range(1, 6):
        maps += stack_p(W, d, x, fault)
    return maps


def reference_form(maps, B):
    """(y_d_rs, y_d_gs, fmap_rs, fmap_gs) as discriminators.py:241-254 returns them."""
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
    for d in range(6):
        ms = maps[map_index(d, 0):map_index(d, 0) + (7 if d == 0 else 6)]
        fmap_rs.append([m[:B] for m in ms])
        fmap_gs.append([m[B:] for m in ms])
        y_d_rs.append(ms[-1][:B].reshape(B, -1))
        y_d_gs.append(ms[-1][B:].reshape(B, -1))
    return y_d_rs, y_d_gs, fmap_rs, fmap_gs


def losses(maps, B):
    """losses.py:6-42 on the 37 maps [2B, ...] -> dict of tensors at the maps' dtype: layer_means [37] (mean |r - g|),
    fm, fm_per_utt [B], disc_r / disc_g / gen_terms [6], disc, gen, disc_per_utt / gen_per_utt [B]."""
    def per(t):  # mean over each utterance's own elements -> [B]
        return t.reshape(B, -1).mean(1)
    l1 = torch.stack([per((m[:B] - m[B:]).abs()) for m in maps])  # [37, B]
    posts = [maps[map_index(d, 6 if d == 0 else 5)] for d in range(6)]
    r = torch.stack([per((1 - m[:B]) ** 2) for m in posts])  # [6, B]
    g = torch.stack([per(m[B:] ** 2) for m in posts])
    gen = torch.stack([per((1 - m[B:]) ** 2) for m in posts])
    return dict(layer_means=l1.mean(1), fm=2 * l1.mean(1).sum(), fm_per_utt=2 * l1.sum(0),
                disc_r=r.mean(1), disc_g=g.mean(1), disc=(r.mean(1) + g.mean(1)).sum(), disc_per_utt=(r + g).sum(0),
                gen_terms=gen.mean(1), gen=gen.mean(1).sum(), gen_per_utt=gen.sum(0))


SCALARS = ("layer_means", "fm", "fm_per_utt", "disc_r", "disc_g", "disc", "disc_per_utt", "gen_terms", "gen", "gen_per_utt")


def gates(got, ref):
    return di.gates(got, ref)


def scalar_err(got, ref):
    """max |got - ref| / ref over the entries: every term of these sums is non-negative, so the sum of the absolute
    terms is the reference value itself."""
    got = torch.as_tensor(got).double().reshape(-1)
    ref = torch.as_tensor(ref).double().reshape(-1)
    return float(((got - ref).abs() / ref.clamp_min(1e-300)).max())


def measure(maps, ls, ref_maps, ref_ls):
    """{"maps": [(rel, local)] * 37, scalar name: figure} of (maps, losses) against the float64 (maps, losses)."""
    out = dict(maps=[gates(a.cpu().contiguous(), r.contiguous()) for a, r in zip(maps, ref_maps)])
    for s in SCALARS:
        out[s] = scalar_err(ls[s].cpu(), ref_ls[s])
    return out


def worst(acc, m):
    """Folds measurement `m` into the running worst `acc` (or starts it)."""
    if acc is None:
        return dict(m, maps=[tuple(v) for v in m["maps"]])
    acc["maps"] = [(max(a[0], b[0]), max(a[1], b[1])) for a, b in zip(acc["maps"], m["maps"])]
    for s in SCALARS:
        acc[s] = max(acc[s], m[s])
    return acc


_REF = {}


def reference(B, T):
    """(y, y_hat, float64 maps, float64 losses) of case (B, T), computed once per process and left unchanged."""
    if (B, T) not in _REF:
        y, y_hat = inputs(B, T, case_seed(B, T))
        maps = forward(weights()[2], y, y_hat)
        _REF[(B, T)] = (y, y_hat, maps, losses(maps, B))
    return _REF[(B, T)]


def floor(shapes=SHAPES):
    """Worst figures of the float32 oracle against the float64 oracle over `shapes`."""
    _, W32, _ = weights()
    acc = None
    for B, T in shapes:
        y, y_hat, rm, rl = reference(B, T)
        maps = forward(W32, y, y_hat)
        acc = worst(acc, measure(maps, losses(maps, B), rm, rl))
    return acc


HALF_ULP = 2.0 ** -24  # the worst relative rounding error of one float32 value


def gate(stage, factor=GATE_FACTOR):
    """4 x floor: stage = a map index (-> (rel, local)) or a scalar's name.  A scalar's floor is one float32 number's
    distance from float64, measured on five cases: where it came out below half an ulp -- the error a correctly rounded
    float32 result may have -- half an ulp is taken, a figure of the number format and not of a lucky draw."""
    if isinstance(stage, int):
        return tuple(factor * v for v in FLOOR["maps"][stage])
    return factor * max(FLOOR[stage], HALF_ULP)


def fixture_gate(stage):
    """Against the reference's stored float32 values, which are themselves one floor away from float64: 4 + 1 floors."""
    return gate(stage, GATE_FACTOR + 1)


def check(m, where=""):
    """Asserts measurement `m` against the gates; returns the worst multiple of a gate (1 = at the gate)."""
    top = 0.0
    for i, (rel, loc) in enumerate(m["maps"]):
        g = gate(i)
        top = max(top, rel / g[0], loc / g[1])
        assert rel <= g[0] and loc <= g[1], f"{where} map {i}: rel {rel:.3e} (gate {g[0]:.3e}) local {loc:.3e} (gate {g[1]:.3e})"
    for s in SCALARS:
        top = max(top, m[s] / gate(s))
        assert m[s] <= gate(s), f"{where} {s}: {m[s]:.3e} (gate {gate(s):.3e})"
    return top


# Worst figures of oracle-at-float32 against oracle-at-float64 over SHAPES (weights WSEED, inputs case_seed), measured on
# one CPU (torch CPU kernels): (rel, local) per map, |d| / ref for the scalars.
FLOOR = dict(
    maps=[(7.66e-08, 1.56e-06), (2.46e-07, 4.35e-06), (3.23e-07, 4.97e-06), (3.93e-07, 8.82e-06), (4.54e-07, 7.67e-06), (5.02e-07, 3.23e-06), (8.59e-07, 2.25e-06), (4.99e-08, 8.96e-07), (1.72e-07, 2.46e-06), (2.47e-07, 2.28e-06), (3.15e-07, 3.02e-06), (3.91e-07, 3.39e-06), (1.25e-06, 2.12e-06), (5.92e-08, 1.07e-06), (1.68e-07, 2.22e-06), (2.41e-07, 2.28e-06), (3.16e-07, 2.54e-06), (3.8e-07, 2.93e-06), (6.75e-07, 2.72e-06), (4.82e-08, 9.11e-07), (1.83e-07, 2.54e-06), (2.47e-07, 2.02e-06), (3.14e-07, 2.48e-06), (3.87e-07, 2.91e-06), (4.53e-07, 1.47e-06), (4.96e-08, 1.11e-06), (1.69e-07, 2.77e-06), (2.4e-07, 2.26e-06), (3.08e-07, 2.42e-06), (3.84e-07, 2.97e-06), (4.44e-07, 1.1e-06), (5.17e-08, 1.32e-06), (1.78e-07, 2.54e-06), (2.51e-07, 2.36e-06), (3.17e-07, 2.73e-06), (3.86e-07, 2.95e-06), (6.67e-07, 2.25e-06)],
    layer_means=0.000102, fm=4.71e-08, fm_per_utt=5.28e-08, disc_r=1.34e-07, disc_g=1.17e-06, disc=4.16e-08, disc_per_utt=8.76e-08, gen_terms=2.71e-07, gen=8.67e-08, gen_per_utt=1.19e-07)
