"""Shared by tests/test_cpu_decoder_gate.py and tests/test_gpu_decoder_oracle.py: the decoder-only models, inputs, the
two gates of a decode against the float64 oracle, their committed values, and the tile geometry of the fused f32
ResBlock kernels restated in Python (for choosing lengths; no kernel reads it).

The gates.  `rel = rms(d) / rms(ref)` and `local = max|d| / rms(ref)` over the whole audio tensor, d = audio - float64
oracle.  FLOOR[config] is the worst (rel, local) of the oracle run at float32 against the same oracle at float64 over
every (B, L) of the GPU sweep (SHAPES[config], both iSTFT heads for the Vocos configs): the honest cost of f32 arithmetic
for this operation on the reference side.  REL_GATE / LOCAL_GATE are 4 x that floor: the MFMA tiles and the K-split small
kernel sum K in another order than the CPU conv, and the floor is the worst of a few dozen draws of a random walk, not a
bound.  tests/test_cpu_decoder_gate.py recomputes the floor of the cheap configs and holds the constants to 2 .. 8 x
it, and proves that the local gate sees a dropped tap, a lost halo column and a lost bias span by a factor >= 10."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import util
from wetts_amd import checkpoint, config, synth

N_VOCAB, N_SPK, WSEED = 40, 3, 81
AUDIO_ABS = 1e-4  # the whole-tensor abs RMS gate of the infer() sweeps, kept as a third assert
GATE_FACTOR = 4.0

HIFIGAN = ("tiny", "tiny_dp", "tiny_oddrate", "v2", "v1", "v3", "stress48k")
VOCOS = ("tiny_vocos", "vits2_vocos_v1")
CONFIGS = HIFIGAN + VOCOS

_SMALL_B, _SMALL_L = (1, 2, 3, 5), (1, 2, 3, 4, 5, 7, 8, 13, 21, 37, 50)
_BIG_B, _BIG_L = (1, 2, 3), (1, 2, 3, 5, 13, 37)


def _grid(Bs, Ls, extra=()):
    """Every B at every L <= 5 (the short end whole), then every longer L once with B cycling downwards from the
    largest (the long end trimmed to what a few seconds of float64 oracle allow), plus `extra` (B, L) pairs."""
    short = [(B, L) for L in Ls if L <= 5 for B in Bs]
    rest = [L for L in Ls if L > 5]
    long_ = [(Bs[len(Bs) - 1 - i % len(Bs)], L) for i, L in enumerate(rest)]
    return tuple(short + long_) + tuple(extra)


# (B, L) per config.  The extras end a fused kernel's last tile exactly on a seam, or leave it narrower than its halo,
# where no length of the set does (see tests/test_gpu_decoder_oracle.py's docstring).
SHAPES = {
    "tiny": _grid(_SMALL_B, _SMALL_L, extra=((1, 181), (1, 190), (1, 191))),
    "tiny_dp": _grid(_SMALL_B, _SMALL_L),
    "tiny_oddrate": _grid(_SMALL_B, _SMALL_L, extra=((1, 102), (1, 306))),
    "v2": _grid(_SMALL_B, _SMALL_L),
    "tiny_vocos": _grid(_SMALL_B, _SMALL_L[1:]),  # nn.ReflectionPad1d([1, 0]) needs two frames
    "vits2_vocos_v1": _grid(_BIG_B, _BIG_L[1:]),
    "v1": _grid(_BIG_B, _BIG_L, extra=((1, 53),)),
    "v3": _grid(_BIG_B, _BIG_L),
    "stress48k": _grid(_BIG_B, _BIG_L),
}
BIG_SHAPE = (32, 64)  # v1 / v3: the size at which the default dispatch picks the fused forms and the big conv tiles
LENGTHS = {k: tuple(sorted({L for _, L in v})) for k, v in SHAPES.items()}

# Worst (rel, local) of oracle-at-float32 against oracle-at-float64 over SHAPES[config] (seed = 1000 + index), measured
# on one CPU (torch CPU kernels); the gates are GATE_FACTOR x these.
FLOOR = {
    "tiny": (5.78e-07, 2.43e-06),
    "tiny_dp": (6.49e-07, 2.35e-06),
    "tiny_oddrate": (4.65e-07, 1.84e-06),
    "v2": (5.81e-07, 3.04e-06),
    "v1": (7.72e-07, 3.57e-06),
    "v3": (3.01e-07, 1.42e-06),
    "stress48k": (5.31e-07, 2.46e-06),
    "tiny_vocos": (5.49e-07, 2.19e-06),  # worst of the torch.istft and the OnnxSTFT.inverse head
    "vits2_vocos_v1": (6.20e-07, 2.92e-06),
}
# Raised factors.  vits2_vocos_v1: the tiled conv kernel (form "tiled", small_max_tiles=0) measured on an MI355X a
# worst rel of 3.49e-6 = 5.6 x floor and a worst local of 1.34e-5 = 4.6 x floor over the sweep; where it first crossed
# 4 x (B = 1, L = 2, torch.istft head: rel 3.05e-6, local 1.10e-5) max|d| was 3.6 x rms(d) over 512 samples: the error of
# K = 1536 sums taken in MFMA order, spread evenly, no locality (the default form of the config: 3.9e-7 / 1.8e-6).
# 6 x keeps the local gate (1.75e-5) under one tenth of the smallest defect effect of tests/test_cpu_decoder_gate.py
# (0.1 x 6.6e-4).
FACTOR = dict({k: GATE_FACTOR for k in FLOOR}, vits2_vocos_v1=6.0)
REL_GATE = {k: FACTOR[k] * v[0] for k, v in FLOOR.items()}
LOCAL_GATE = {k: FACTOR[k] * v[1] for k, v in FLOOR.items()}


def vo():
    from oracle import vits_oracle
    return vits_oracle


def model_cfg(mname):
    return config.make_config(dict(config.MODEL_CONFIGS[mname]), N_VOCAB, N_SPK)


def weights(mname, wseed=WSEED):
    """(cfg struct, state dict, cfg dict, folded float32 weights, the same widened to float64): the float32 checkpoint is
    folded in float32 -- what the library packs -- and widened, so both oracles and the device hold the same numbers."""
    cfg = model_cfg(mname)
    sd = synth.make_state_dict(cfg, wseed)
    W32 = checkpoint.fold_weight_norm(sd)
    W64 = {k: v.to(torch.float64) for k, v in W32.items()}
    return cfg, sd, util.cfg_dict(cfg), W32, W64


def inputs(W, B, L, seed):
    """z ~ N(0, 1) [B, 192, L] and a speaker embedding g [B, gin, 1] (rows of the checkpoint's table), float32."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 192, L, generator=gen)
    sid = torch.randint(0, N_SPK, (B,), generator=gen)
    g = F.embedding(sid, W["emb_g.weight"].float()).unsqueeze(-1)
    return z, g


def oracle(W, cd, z, g, is_onnx=None):
    """vits_oracle.decoder at the dtype of W; `is_onnx` overrides the config's iSTFT head."""
    d = W["emb_g.weight"].dtype
    if is_onnx is not None:
        cd = dict(cd, is_onnx=int(is_onnx))
    with torch.no_grad():
        return vo().decoder(W, cd, z.to(d), g.to(d))


def gates(got, ref):
    """(rel RMS, max |d| / rms(ref)) over the whole tensor."""
    a, r = got.double().numpy(), ref.double().numpy()
    assert a.shape == r.shape, (a.shape, r.shape)
    scale = max(util.rms(r), 1e-30)
    return util.rms(a - r) / scale, float(np.abs(a - r).max()) / scale


def heads(mname):
    """The iSTFT heads a config is swept under: both for Vocos, the config's own (no effect) for HiFi-GAN."""
    return (False, True) if mname in VOCOS else (None,)


def floor(mname, shapes=None):
    """Worst (rel, local) of the float32 oracle against the float64 oracle over `shapes` (default: SHAPES[mname])."""
    cfg, sd, cd, W32, W64 = weights(mname)
    worst = [0.0, 0.0]
    for i, (B, L) in enumerate(SHAPES[mname]):
        if shapes is not None and (B, L) not in shapes:
            continue
        z, g = inputs(W32, B, L, 1000 + i)
        for head in heads(mname):
            rel, loc = gates(oracle(W32, cd, z, g, head), oracle(W64, cd, z, g, head))
            worst = [max(worst[0], rel), max(worst[1], loc)]
    return tuple(worst)


# ---- tile geometry of the fused f32 ResBlock kernels (csrc/resblock32.hip, csrc/resblock_chain32.hip) ------------------
def chain_geometry(k, dils):
    """(S, Mmin) of resblock_chain32.hip:chain_geometry: columns a chain of (c1, c2) pairs loses per side, widest tap."""
    hk, s, m = (k - 1) // 2, 0, 0
    for p, d in enumerate(dils):
        s += (hk * d if p > 0 else 0) + hk
        m = max(m, hk * d, hk)
    return s, m


def chain_ntc(C, Mmin):
    """Computed columns per tile of the chain kernel: 32 * nb * (4 / (C / 32)), nb = 3 at C = 32 where three blocks of the
    narrower tile fit the LDS (chain_nb), else 4."""
    nb = 4
    if C == 32 and 3 * C * ((32 * 3 * 4 + 2 * Mmin + 4 + 3) & ~3) * 4 <= 160 * 1024:
        nb = 3
    return 32 * nb * (4 // (C // 32))


FORCED_TUNE = "fuse_min_blocks=0,fuse2_waste_pct=100,chain_whole_pct=100,chain_whole_maxc=128,small_max_tiles=0"
# whole-ResBlock launches off: every pair the chain kernel takes runs as a one-pair launch, also below 128 tiles
PAIRS_TUNE = "fuse_min_blocks=0,fuse2_waste_pct=100,chain_whole_pct=0,small_max_tiles=0"


def fused_launches(mname, B, L, form):
    """The fused-kernel launches of one f32 decode of [B, 192, L]: a restatement of run_hifigan's choice per ResBlock
    (model.hip) and of the `*_supported` predicates, under FORCED_TUNE (form "forced"), PAIRS_TUNE ("pairs") or the defaults ("default").  One dict per launch:
    kernel ("chain_whole" / "chain_pair": resblock_chain32_kernel, "pair32": resblock_pair32, "rb2_chain":
    resblock2_chain32), C, k, dil, nto (output columns per tile), halo (columns of the tile lost), T (stage length).
    For choosing lengths and for the docstrings; no kernel reads it."""
    m = config.MODEL_CONFIGS[mname]
    forced = form != "default"
    min_blocks = 0 if forced else 128
    whole_pct, whole_maxc = {"forced": (100, 128), "pairs": (0, 64), "default": (15, 64)}[form]
    out, ch, T = [], m["upsample_initial_channel"], L
    for u in m["upsample_rates"]:
        ch, T = ch // 2, T * u
        if ch not in (32, 64, 128):
            continue
        ntc_pair = 128 * (4 // (ch // 32))
        for k, dils in zip(m["resblock_kernel_sizes"], m["resblock_dilation_sizes"]):
            def put(kernel, dil, ntc, nto):
                out.append(dict(kernel=kernel, C=ch, k=k, dil=tuple(dil), nto=nto, halo=ntc - nto, T=T))
            tiles = lambda nto: -(-T // nto) * B
            if str(m["resblock"]) != "1":
                d1, d2 = dils[:2]
                lost = (k - 1) * d2
                pct = 100 if forced else (20 if ch <= 32 else 10)
                if (k - 1) * max(d1, d2) <= 64 and lost * 100 <= pct * ntc_pair and \
                        ch * ((ntc_pair + (k - 1) * max(d1, d2) + 3) & ~3) * 4 <= 160 * 1024 and \
                        tiles(ntc_pair - lost) >= min_blocks:
                    put("rb2_chain", (d1, d2), ntc_pair, ntc_pair - lost)
                continue
            S, Mmin = chain_geometry(k, dils)
            ntc = chain_ntc(ch, Mmin)
            lds_ok = lambda ntc_, M: ch * ((ntc_ + 2 * M + 4 + 3) & ~3) * 4 <= 80 * 1024
            if ch <= whole_maxc and T % 4 == 0 and Mmin <= 28 and ntc - 2 * S > 0 and \
                    2 * S * 100 <= whole_pct * ntc and lds_ok(ntc, Mmin) and tiles(ntc - 2 * S) >= min_blocks:
                put("chain_whole", dils, ntc, ntc - 2 * S)
                continue
            for d in dils:
                enough = tiles(ntc_pair - (k - 1)) >= min_blocks
                S, Mmin = chain_geometry(k, [d])
                ntc = chain_ntc(ch, Mmin)
                if T % 4 == 0 and (ch <= 32 or k <= 3) and Mmin <= 28 and lds_ok(ntc, Mmin) and enough:
                    put("chain_pair", (d,), ntc, ntc - 2 * S)
                elif (k - 1) * d <= 64 and ch * ((ntc_pair + (k - 1) * d + 3) & ~3) * 4 <= 160 * 1024 and \
                        not (ch >= 128 and k >= 11) and (ch <= 32 or k <= 3) and enough:
                    put("pair32", (d,), ntc_pair, ntc_pair - (k - 1))
    return out


def last_tiles(mname, shapes, form="forced"):
    """{(kernel, C, k, dil): sorted set of (T mod nto) over `shapes`}: the widths of the last tile (0: it ends exactly
    on a seam), with the tile's nto and halo."""
    acc = {}
    for B, L in shapes:
        for r in fused_launches(mname, B, L, form):
            key = (r["kernel"], r["C"], r["k"], r["dil"])
            e = acc.setdefault(key, dict(nto=r["nto"], halo=r["halo"], rems=set(), multi=False))
            e["rems"].add(r["T"] % r["nto"])
            e["multi"] |= r["T"] > r["nto"]
    return acc
