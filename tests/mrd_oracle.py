"""Shared by tests/test_cpu_mrd.py, tests/test_gpu_mrd.py and tests/golden/make_golden_mrd.py:
MultiPeriodMultiResolutionDiscriminator (model/discriminators.py:127-225,256-283) and the three adversarial losses
(losses.py:6-42) restated at the dtype of the weights, independent of the device code.  DiscriminatorR is written on
F.conv2d; its STFT is a frame matrix times the window-folded DFT basis -- the arithmetic the device chose (DESIGN.md §8:
a GEMM against an f32-rounded basis sits near 7e-7 of float64 where an f32 FFT sits near 1e-7, so the float32 floor has
to be that of the GEMM or the 4 x gate would test the FFT).  The basis is built in float64 and rounded to the oracle's
dtype; test_cpu_mrd checks the float64 form against torch.stft once.  The period stacks are disc_oracle.stack_p.

forward(W, y, y_hat) -> (the 93 maps over the 2B utterances (real first), stages): maps 21 r + 4 b + (l - 1) are layers
1..4 of band b of resolution r, 21 r + 20 its conv_post, 63 + 6 d + m the period stacks; stages = {"norm": the normalised
audio [2B, T], "spec0".."spec2": the complex spectrograms [2B, 2, frames, bins]}.

Gates as in disc_oracle: rel / local per tensor, |d| / ref per scalar, FLOOR = the float32 oracle against the float64
oracle over SHAPES, gate = GATE_FACTOR x floor (scalars: x max(floor, half an f32 ulp))."""
import math

import torch
import torch.nn.functional as F

from tests import disc_oracle as do
from wetts_amd import checkpoint, synth

WINDOWS = (2048, 1024, 512)
BANDS = ((0.0, 0.1), (0.1, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0))
PERIODS = do.PERIODS
SLOPE = 0.1
WSEED = 31
GATE_FACTOR = do.GATE_FACTOR
HALF_ULP = do.HALF_ULP
N_MAPS = 93
R_MAPS = 21
TILE = 128  # the band conv's column tile (kMrdN in csrc/mrd.hip)
# (B, T): the shortest legal length; ragged everywhere; every period divides (the fixtures); the recipe's training segment;
# and EDGE.  A band's end-to-end column count is rows * frames * F'.  At T = 2177 the 2048 window has 5 frames, and the
# layer-1 outputs of its bands 0 and 1 are 51 and 77 wide: one row has 255 = 2 * 128 - 1 and 385 = 3 * 128 + 1 columns
# (the stand-alone layer entries run that), the forward pass of one pair, whose 2B rows make every count even, 510 and
# 770: two short of and two past a multiple of the tile, the closest an even count comes.
FIXTURE_SHAPES = ((1, 1025), (2, 1536), (3, 2310))
EDGE = (1, 2177)
SHAPES = FIXTURE_SHAPES + ((2, 8192), EDGE)
FAULTS = ("drop_ftap", "drop_ttap", "stride_phase", "bands_contiguous", "post_band_pad", "swap_reim", "skip_dc", "sym_hann")


def map_index(d, k):
    """Index of map k of discriminator d (0..2: DiscriminatorR, k = 4 * band + layer - 1, 20 = conv_post; 3..7: period
    stacks, k = layer)."""
    return R_MAPS * d + k if d < 3 else 3 * R_MAPS + 6 * (d - 3) + k


POSTS = tuple(map_index(d, 20 if d < 3 else 5) for d in range(8))
# the stage a fault first touches: a map index or a stage name
FAULT_STAGE = dict(drop_ftap=map_index(1, 4 * 2 + 0), drop_ttap=map_index(0, 4 * 1 + 1), stride_phase=map_index(2, 4 * 3 + 0),
                   bands_contiguous=map_index(0, 4 * 1 + 0), post_band_pad=map_index(0, 20), swap_reim="spec1", skip_dc="norm",
                   sym_hann="spec2")


def band_edges(w):
    """discriminators.py:155-156, the reference's own expression."""
    n_fft = w // 2 + 1
    return [(int(b[0] * n_fft), int(b[1] * n_fft)) for b in BANDS]


def frames(w, T):
    return 1 + T // int(w * 0.25)


def conv_width(F_in, layer):
    """Width after band layer `layer` (0..4): kernel 9 / pad 4 / stride 1 or 2, last: kernel 3 / pad 1."""
    k, s = ((9, 1), (9, 2), (9, 2), (9, 2), (3, 1))[layer]
    return (F_in + 2 * (k // 2) - k) // s + 1


def band_widths(w):
    """[band][0..5]: the width of each band before layer 0 and after every layer."""
    out = []
    for lo, hi in band_edges(w):
        ws = [hi - lo]
        for l in range(5):
            ws.append(conv_width(ws[-1], l))
        out.append(ws)
    return out


def weights(seed=WSEED):
    """(reference-keyed state dict with weight-norm pairs, folded float32 weights, the same widened to float64)."""
    sd = synth.make_mrd_state_dict(seed)
    W32 = checkpoint.fold_weight_norm(sd)
    return sd, W32, {k: v.to(torch.float64) for k, v in W32.items()}


def inputs(B, T, seed):
    """(y, y_hat) [B, 1, T] float32: a recording-like signal with a DC offset (so its removal matters) and a noisy copy."""
    g = torch.Generator().manual_seed(seed)
    y = 0.5 * torch.randn(B, 1, T, generator=g) + 0.05
    return y, y + 0.2 * torch.randn(B, 1, T, generator=g)


def case_seed(B, T):
    return 9000 + 13 * B + T


_BASIS = {}


def dft_basis(w, dtype, symmetric=False):
    """(cos [w, bins], -sin [w, bins]) folded with the Hann window (periodic, as torch.hann_window's default), built in
    float64 with k * n reduced mod w before the trig call, rounded once to `dtype`."""
    key = (w, dtype, symmetric)
    if key not in _BASIS:
        n = torch.arange(w, dtype=torch.float64)
        win = 0.5 - 0.5 * torch.cos(2 * math.pi * n / (w - 1 if symmetric else w))
        k = torch.arange(w // 2 + 1, dtype=torch.int64)
        ang = 2 * math.pi * ((torch.arange(w, dtype=torch.int64)[:, None] * k[None, :]) % w).to(torch.float64) / w
        _BASIS[key] = ((win[:, None] * torch.cos(ang)).to(dtype), (-win[:, None] * torch.sin(ang)).to(dtype))
    return _BASIS[key]


def normalize(x, fault=None):
    """discriminators.py:190-193 on x [R, T]."""
    if fault != "skip_dc":
        x = x - x.mean(dim=-1, keepdim=True)
    return 0.8 * x / (x.abs().max(dim=-1, keepdim=True)[0] + 1e-9)


def spectrogram(x, w, fault=None):
    """Spectrogram(n_fft=w, hop=w // 4, win=w, power=None) of x [R, T], view_as_real, transpose(1, 3) ->
    [R, 2, frames, bins]."""
    hop = w // 4
    xp = F.pad(x[:, None], (w // 2, w // 2), "reflect")[:, 0]
    fr = xp.unfold(1, w, hop)  # [R, frames, w]
    c, s = dft_basis(w, x.dtype, symmetric=fault == "sym_hann")
    re, im = fr @ c, fr @ s
    if fault == "swap_reim":
        re, im = im, re
    return torch.stack([re, im], 1)


def stack_r(W, r, x, fault=None):
    """DiscriminatorR(WINDOWS[r]) on x [R, 1, T] -> (its 21 maps, normalised audio, spectrogram)."""
    w = WINDOWS[r]
    norm = normalize(x[:, 0], fault)
    spec = spectrogram(norm, w, fault if (fault, r) in (("swap_reim", 1), ("sym_hann", 2)) else None)
    maps, last = [], []
    pre = f"discriminators.{r}.band_convs"
    for b, (lo, hi) in enumerate(band_edges(w)):
        h = spec[..., lo:hi]
        for l in range(5):
            wt, bias = W[f"{pre}.{b}.{l}.weight"], W[f"{pre}.{b}.{l}.bias"]
            kf, sf = (3, 1) if l == 4 else (9, 1 if l == 0 else 2)
            if fault == "drop_ftap" and (r, b, l) == (1, 2, 1):
                wt = wt.clone()
                wt[:, :, :, 3] = 0
            if fault == "drop_ttap" and (r, b, l) == (0, 1, 2):
                wt = wt.clone()
                wt[:, :, 0, :] = 0
            if fault == "stride_phase" and (r, b, l) == (2, 3, 1):  # the windows start one bin late
                h = F.conv2d(F.pad(h, (3, 5, 1, 1)), wt, bias, (1, sf), 0)
            elif fault == "bands_contiguous" and r == 0 and l == 0:  # a neighbour's bins in place of the zero pad
                h = F.conv2d(spec, wt, bias, 1, (1, 4))[..., lo:hi]
            else:
                h = F.conv2d(h, wt, bias, (1, sf), (1, kf // 2))
            h = F.leaky_relu(h, SLOPE)
            if l > 0:
                maps.append(h)
        last.append(h)
    pw, pb = W[f"discriminators.{r}.conv_post.weight"], W[f"discriminators.{r}.conv_post.bias"]
    if fault == "post_band_pad" and r == 0:  # zero pad at every band join
        maps.append(torch.cat([F.conv2d(h, pw, pb, 1, 1) for h in last], -1))
    else:
        maps.append(F.conv2d(torch.cat(last, -1), pw, pb, 1, 1))
    return maps, norm, spec


def period_weights(W):
    """The period stacks' tensors keyed as disc_oracle.stack_p expects them (discriminators.1..5)."""
    out = {}
    for k, v in W.items():
        d = int(k.split(".")[1])
        if d >= 3:
            out[k.replace(f"discriminators.{d}.", f"discriminators.{d - 2}.", 1)] = v
    return out


def forward(W, y, y_hat, fault=None):
    dt = W["discriminators.0.conv_post.bias"].dtype
    x = torch.cat([y, y_hat], 0).to(dt)
    maps, stages = [], {}
    for r in range(3):
        m, norm, spec = stack_r(W, r, x, fault)
        maps += m
        stages["norm"] = norm
        stages[f"spec{r}"] = spec
    Wp = period_weights(W)
    for d in range(1, 6):
        maps += do.stack_p(Wp, d, x)
    return maps, stages


STAGES = ("norm", "spec0", "spec1", "spec2")


def reference_form(maps, B):
    """(y_d_rs, y_d_gs, fmap_rs, fmap_gs) as discriminators.py:270-283 returns them."""
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
    for d in range(8):
        ms = maps[map_index(d, 0):map_index(d, 0) + (R_MAPS if d < 3 else 6)]
        fmap_rs.append([m[:B] for m in ms])
        fmap_gs.append([m[B:] for m in ms])
        y_d_rs.append(ms[-1][:B] if d < 3 else ms[-1][:B].reshape(B, -1))
        y_d_gs.append(ms[-1][B:] if d < 3 else ms[-1][B:].reshape(B, -1))
    return y_d_rs, y_d_gs, fmap_rs, fmap_gs


def losses(maps, B):
    """losses.py:6-42 on the 93 maps [2B, ...]: as disc_oracle.losses, eight discriminators."""
    def per(t):
        return t.reshape(B, -1).mean(1)
    l1 = torch.stack([per((m[:B] - m[B:]).abs()) for m in maps])
    posts = [maps[i] for i in POSTS]
    r = torch.stack([per((1 - m[:B]) ** 2) for m in posts])
    g = torch.stack([per(m[B:] ** 2) for m in posts])
    gen = torch.stack([per((1 - m[B:]) ** 2) for m in posts])
    return dict(layer_means=l1.mean(1), fm=2 * l1.mean(1).sum(), fm_per_utt=2 * l1.sum(0),
                disc_r=r.mean(1), disc_g=g.mean(1), disc=(r.mean(1) + g.mean(1)).sum(), disc_per_utt=(r + g).sum(0),
                gen_terms=gen.mean(1), gen=gen.mean(1).sum(), gen_per_utt=gen.sum(0))


SCALARS = do.SCALARS
gates = do.gates
scalar_err = do.scalar_err


def measure(maps, stages, ls, ref_maps, ref_stages, ref_ls):
    """{"maps": [(rel, local)] * 93, stage: (rel, local), scalar: figure} against the float64 values.  `stages` / `ls`
    may be None (not measured)."""
    out = dict(maps=[gates(a.cpu().contiguous(), r.contiguous()) for a, r in zip(maps, ref_maps)])
    for s in STAGES:
        if stages is not None:
            out[s] = gates(stages[s].cpu().contiguous(), ref_stages[s].contiguous())
    for s in SCALARS:
        if ls is not None:
            out[s] = scalar_err(ls[s].cpu(), ref_ls[s])
    return out


def worst(acc, m):
    if acc is None:
        return dict(m, maps=[tuple(v) for v in m["maps"]])
    acc["maps"] = [(max(a[0], b[0]), max(a[1], b[1])) for a, b in zip(acc["maps"], m["maps"])]
    for s in STAGES:
        acc[s] = (max(acc[s][0], m[s][0]), max(acc[s][1], m[s][1]))
    for s in SCALARS:
        acc[s] = max(acc[s], m[s])
    return acc


_REF = {}


def reference(B, T):
    """(y, y_hat, float64 maps, float64 stages, float64 losses) of case (B, T), computed once per process."""
    if (B, T) not in _REF:
        y, y_hat = inputs(B, T, case_seed(B, T))
        maps, stages = forward(weights()[2], y, y_hat)
        _REF[(B, T)] = (y, y_hat, maps, stages, losses(maps, B))
    return _REF[(B, T)]


def floor(shapes=SHAPES):
    """Worst figures of the float32 oracle against the float64 oracle over `shapes`."""
    _, W32, _ = weights()
    acc = None
    for B, T in shapes:
        y, y_hat, rm, rs, rl = reference(B, T)
        maps, stages = forward(W32, y, y_hat)
        acc = worst(acc, measure(maps, stages, losses(maps, B), rm, rs, rl))
    return acc


def gate(stage, factor=GATE_FACTOR):
    """4 x floor: stage = a map index or a stage name (-> (rel, local)), or a scalar's name."""
    if isinstance(stage, int):
        return tuple(factor * v for v in FLOOR["maps"][stage])
    if stage in STAGES:
        return tuple(factor * v for v in FLOOR[stage])
    return factor * max(FLOOR[stage], HALF_ULP)


def fixture_gate(stage):
    """Against the reference's stored float32 values, themselves one floor away from float64: 4 + 1 floors."""
    return gate(stage, GATE_FACTOR + 1)


def check(m, where=""):
    """Asserts measurement `m` against the gates; returns the worst multiple of a gate (1 = at the gate)."""
    top = 0.0
    for i, (rel, loc) in enumerate(m["maps"]):
        g = gate(i)
        top = max(top, rel / g[0], loc / g[1])
        assert rel <= g[0] and loc <= g[1], f"{where} map {i}: rel {rel:.3e} (gate {g[0]:.3e}) local {loc:.3e} (gate {g[1]:.3e})"
    for s in STAGES:
        if s in m:
            g = gate(s)
            top = max(top, m[s][0] / g[0], m[s][1] / g[1])
            assert m[s][0] <= g[0] and m[s][1] <= g[1], f"{where} {s}: {m[s]} (gate {g})"
    for s in SCALARS:
        if s in m:
            top = max(top, m[s] / gate(s))
            assert m[s] <= gate(s), f"{where} {s}: {m[s]:.3e} (gate {gate(s):.3e})"
    return top


def edge_case(rows, T):
    """(one short, one past): whether some (resolution, band, layer)'s end-to-end column count rows * frames * F' is
    TILE - 1 and some other's 1 modulo TILE."""
    short = past = False
    for w in WINDOWS:
        for ws in band_widths(w):
            for l in range(1, 6):
                n = rows * frames(w, T) * ws[l]
                short |= n % TILE == TILE - 1
                past |= n % TILE == 1
    return short, past


# Worst figures of oracle-at-float32 against oracle-at-float64 over SHAPES (weights WSEED, inputs case_seed), measured on
# one CPU (torch CPU kernels): (rel, local) per map and stage, |d| / ref for the scalars.
FLOOR = dict(
    maps=[(5.21e-07, 5.09e-06), (6.39e-07, 6.36e-06), (7.8e-07, 5.67e-06), (7.97e-07, 6.62e-06), (4.88e-07, 6.12e-06), (5.67e-07, 5.08e-06), (6.74e-07, 5.35e-06), (7.14e-07, 6.43e-06), (5.35e-07, 7.32e-06), (6.31e-07, 5.43e-06), (6.9e-07, 5.9e-06), (9.57e-07, 9.94e-06), (5.28e-07, 6.09e-06), (6.49e-07, 6.1e-06), (7.88e-07, 7.54e-06), (7.91e-07, 6.05e-06), (5.05e-07, 5.9e-06), (5.64e-07, 5.09e-06), (6.55e-07, 6.5e-06), (6.62e-07, 4.84e-06), (9.92e-07, 5.12e-06), (4.94e-07, 6.06e-06), (6.34e-07, 5.88e-06), (6.61e-07, 5.34e-06), (6.97e-07, 5.09e-06), (4.89e-07, 5.06e-06), (5.96e-07, 5.45e-06), (7.19e-07, 5.71e-06), (7.49e-07, 5.37e-06), (5.21e-07, 7.46e-06), (6.41e-07, 5.28e-06), (7.34e-07, 6.31e-06), (8.55e-07, 6.01e-06), (5.16e-07, 5.43e-06), (7e-07, 6.65e-06), (7.65e-07, 6.27e-06), (7.59e-07, 5.61e-06), (5.78e-07, 6.08e-06), (6.77e-07, 5.67e-06), (7.81e-07, 5.92e-06), (8.13e-07, 5.8e-06), (9.88e-07, 5.2e-06), (4.91e-07, 5.65e-06), (6.23e-07, 5.38e-06), (6.69e-07, 4.63e-06), (6.61e-07, 4.32e-06), (4.83e-07, 5.22e-06), (6.54e-07, 6.62e-06), (6.56e-07, 4.82e-06), (6.29e-07, 5.43e-06), (4.67e-07, 5.97e-06), (5.58e-07, 4.49e-06), (7.22e-07, 5.91e-06), (7.71e-07, 6.51e-06), (4.92e-07, 5.72e-06), (6.66e-07, 6.78e-06), (7.28e-07, 5.74e-06), (7.19e-07, 5.43e-06), (5.04e-07, 6.65e-06), (6.31e-07, 6.14e-06), (7.09e-07, 6.65e-06), (8.09e-07, 6.48e-06), (6.63e-07, 4.73e-06), (5.03e-08, 9.46e-07), (1.64e-07, 2.74e-06), (2.33e-07, 2.07e-06), (2.99e-07, 2.48e-06), (3.67e-07, 2.82e-06), (7.13e-07, 2.27e-06), (5.07e-08, 1.04e-06), (1.75e-07, 2.69e-06), (2.49e-07, 2.16e-06), (3.16e-07, 2.39e-06), (3.82e-07, 3e-06), (5.14e-07, 1.33e-06), (5.25e-08, 1.03e-06), (1.67e-07, 2.9e-06), (2.37e-07, 2.1e-06), (3.01e-07, 2.55e-06), (3.63e-07, 2.95e-06), (8.14e-07, 2.22e-06), (5.25e-08, 1.07e-06), (1.78e-07, 2.74e-06), (2.51e-07, 2.77e-06), (3.13e-07, 2.73e-06), (3.75e-07, 3.1e-06), (5.73e-07, 2.65e-06), (5.16e-08, 1.07e-06), (1.73e-07, 2.95e-06), (2.41e-07, 2.06e-06), (3.02e-07, 2.84e-06), (3.79e-07, 2.91e-06), (6.33e-07, 1.93e-06)],
    norm=(6.84e-08, 5.03e-07), spec0=(3.54e-07, 3.34e-06), spec1=(3.32e-07, 2.72e-06), spec2=(2.94e-07, 3.29e-06),
    layer_means=8.55e-07, fm=1.52e-07, fm_per_utt=1.62e-07, disc_r=1.92e-07, disc_g=7.38e-07, disc=7.33e-08, disc_per_utt=1.12e-07, gen_terms=3.05e-07, gen=1.11e-07, gen_per_utt=9.54e-08)
