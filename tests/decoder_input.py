"""Shared by tests/test_cpu_decoder_gate.py and tests/test_gpu_decoder_oracle.py: the decoder-only models, inputs, the
two gates of a decode against the float64 oracle, their committed values, and the tile geometry of the fused f32
ResBlock kernels restated in Python (for choosing lengths; no kernel reads it).

The gates.  `rel = rms(d) / rms(ref)` and `local = max|d| / rms(ref)` over the whole audio tensor, d = audio - float64
oracle.  FLOOR[config] is the worst (rel, local) of the oracle run at float32 against the same oracle at float64 over
every (B, L) of the GPU sweep (SHAPES[config], both iSTFT heads for the Vocos configs): the honest cost of f32 arithmetic
for this operation on the reference side.  REL_GATE / LOCAL_GATE are 4 x that floor: the MFMA tiles and the K-split small
kernel sum K in another order than the CPU conv, and the floor is the worst of a few dozen draws of a random walk, not a
bound.  tests/test_cpu_decoder_gate.py recomputes the floor of the cheap configs and holds the constants to 2 .. 8 x
it, and proves that the local gate sees a dropped tap, a lost halo column and a lost bias span by a factor >= 10.

The Vocos seam sweep has a second family of the same things, leaving the first as it is: SEAM_CONFIGS (the two Vocos
configs plus four coverage configs kept here as dicts, COVERAGE), SEAM_SHAPES (frame counts around the 62-column seams of
convnext_dwln_kernel at every junk width of the padded rows), WIDE_SHAPES (vits2_vocos_v1 at B = 32 where pw_schedule
gives pw_gemm_kernel blocks of several passes), SEAM_FLOOR / SEAM_FACTOR / SEAM_REL_GATE / SEAM_LOCAL_GATE measured over
those shapes at their own seeds, and the head's geometry restated: dwln_tiles (tiles of the fused depthwise conv +
LayerNorm), vocos_launches (launch_conv_small's take rule, pw_gemm_eligible and pw_schedule with the CU count as an
argument: kernel, S, upb, pass widths and last unit per conv), pw_patterns and wide_claims (what a list of cases reaches)."""
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


# ---- the Vocos seam sweep: a second family of shapes, floors and gates (SHAPES / FLOOR / FACTOR above stay as they are) ---
def _vocos_variant(channels, h_channels, n_fft, hop):
    return dict(config.MODEL_CONFIGS["tiny_vocos"], vocos_channels=channels, vocos_h_channels=h_channels,
                vocos_out_channels=n_fft + 2, vocos_num_layers=2,
                vocos_istft_config=dict(n_fft=n_fft, hop_length=hop, win_length=n_fft, center=True))


# Coverage configs of the seam sweep (two ConvNeXt layers, small n_fft: a float64 decode costs milliseconds).  They live
# here and not in config.MODEL_CONFIGS, which other tests enumerate.  What each is for:
#   vocos_c256  C = 256: convnext_dwln_kernel<16> and layernorm_reg_kernel<16>; h = 272 = 17 chunks of 16 (an odd number
#               of chunks in pw_conv2's reduction); n_fft / hop = 2
#   vocos_c96   C = 96 = 6 x 16, which k_convnext_dwln refuses: the k_dwconv + k_layernorm fallback; h = 176 = 11 chunks;
#               n_fft / hop = 8
#   vocos_c80   C = 80, no multiple of 32: pw_gemm_eligible refuses the residual conv (pw_conv2) and conv_mfma_kernel
#               runs it with `res`; the fallback again (80 / 16 = 5); pw_conv1's reduction is 5 chunks; hop 24 does not
#               divide n_fft 64
#   vocos_n78   n_fft = 78: n_fft + 2 = 80 rows are whole chunks, k_rows_padded pads nothing; n_fft / hop = 3
COVERAGE = {
    "vocos_c256": _vocos_variant(256, 272, 64, 32),
    "vocos_c96": _vocos_variant(96, 176, 64, 8),
    "vocos_c80": _vocos_variant(80, 160, 64, 24),
    "vocos_n78": _vocos_variant(64, 160, 78, 26),
}
SEAM_CONFIGS = ("tiny_vocos", "vocos_c256", "vocos_c96", "vocos_c80", "vocos_n78", "vits2_vocos_v1")

# Frames F = L + 1 per config (row stride Fs = (F + 3) & ~3; convnext_dwln_kernel works in tiles of 62 columns of Fs):
#   60 .. 66    the first seam 61 | 62 at all four junk widths Fs - F: 60 (one tile, 0 junk), 61 (Fs 64: the second tile
#               holds columns 62, 63, junk only, 3 junk), 62 (F on the seam, second tile junk only, 2 junk), 63 (second tile:
#               ONE valid column and one junk column), 64 (two valid, 0 junk), 65 (Fs 68, 3 junk), 66 (2 junk)
#   122 .. 126  the second seam 123 | 124 likewise: 124 = 2 x 62 ends on it, 125 (Fs 128) leaves one valid column + 3 junk
#   187         beyond the third seam 185 | 186: a fourth tile of one valid column and one junk column
_SEAM_F_FULL = (60, 61, 62, 63, 64, 65, 66, 122, 123, 124, 125, 126, 187)
_SEAM_F_SHORT = (61, 62, 63, 64, 124, 187)  # every junk width each side of the first seam, the second seam, four tiles
_SEAM_F_BIG = (61, 62, 63, 64, 124)  # vits2_vocos_v1: what a few seconds of float64 oracle allow


def _seam_grid(Bs, Fs_):
    """(B, L) with B cycling through `Bs` by index."""
    return tuple((Bs[i % len(Bs)], F_ - 1) for i, F_ in enumerate(Fs_))


SEAM_SHAPES = {
    "tiny_vocos": _seam_grid(_SMALL_B, _SEAM_F_FULL),
    "vocos_c256": _seam_grid(_SMALL_B, _SEAM_F_FULL),
    "vocos_c96": _seam_grid(_SMALL_B, _SEAM_F_SHORT),
    "vocos_c80": _seam_grid(_SMALL_B, _SEAM_F_SHORT),
    "vocos_n78": _seam_grid(_SMALL_B, _SEAM_F_SHORT),
    "vits2_vocos_v1": _seam_grid(_BIG_B, _SEAM_F_BIG),
}
# vits2_vocos_v1 at the default dispatch, one utterance repeated B times, then B distinct ones: the (B, L) at which
# pw_schedule (256 CUs) gives pw_gemm_kernel blocks of several passes (see vocos_launches; asserted in
# tests/test_cpu_decoder_gate.py:test_wide_cases_reach_every_pass_pattern_of_pw_gemm).  The smallest L per pattern.
#   32 x 128  Fs 132, 5 units, last of 4 columns: pw1 upb 3 = passes (2, 1) and (2): widths 2 and 1 in one block, S = 2
#   32 x 192  Fs 196, 7 units: pw1 upb 4 = one 4-unit pass, then (2, 1); in / pw2 / iSTFT upb 2 with S = 4
#   32 x 479  Fs 480 = 15 full units: pw1 upb 8 = (4, 4) and (4, 2, 1); in / out / iSTFT upb 4; pw2 (residual init) upb 2
#   32 x 671  Fs 672 = 21 full units: pw1 upb 11 = (4, 4, 2, 1); pw2 upb 4 with the residual init; iSTFT upb 7 = (4, 2, 1)
WIDE_CONFIG = "vits2_vocos_v1"
WIDE_SHAPES = ((32, 128), (32, 192), (32, 479), (32, 671))
SEAM_SEED, WIDE_SEED = 2000, 3000  # seed = base + index into SEAM_SHAPES[config] / WIDE_SHAPES

# Worst (rel, local) of oracle-at-float32 against oracle-at-float64 over SEAM_SHAPES[config], both heads (seam_floor;
# vits2_vocos_v1: also over row 0 of every wide case), measured on one CPU.  Gates = SEAM_FACTOR x these: the project's
# 4, and the 6 of vits2_vocos_v1 for the reason written next to FACTOR (K = 1536 sums in MFMA order, spread evenly).
# Measured on an MI355X (profiles/vocos_seam_margins.txt): every 4 x config stays under 0.37 of its gates in both forms;
# vits2_vocos_v1 on pw_gemm_kernel (form tiled, and the wide cases at the default dispatch) reaches rel 3.3e-6 = 5.5 x
# floor = 0.92 of its gate and local 1.7e-5 = 4.3 x floor, max|d| about 5 x rms(d): the same evenly spread error as
# in the first sweep, at every pass pattern alike (32 x 128: 3.29e-6, 32 x 671: 3.27e-6), so no factor was raised.
SEAM_FLOOR = {
    "tiny_vocos": (4.71e-07, 2.98e-06),
    "vocos_c256": (5.85e-07, 3.72e-06),
    "vocos_c96": (6.09e-07, 3.27e-06),
    "vocos_c80": (4.67e-07, 2.28e-06),
    "vocos_n78": (4.52e-07, 2.79e-06),
    "vits2_vocos_v1": (5.98e-07, 3.96e-06),
}
SEAM_FACTOR = dict({k: GATE_FACTOR for k in SEAM_FLOOR}, vits2_vocos_v1=FACTOR["vits2_vocos_v1"])
SEAM_REL_GATE = {k: SEAM_FACTOR[k] * v[0] for k, v in SEAM_FLOOR.items()}
SEAM_LOCAL_GATE = {k: SEAM_FACTOR[k] * v[1] for k, v in SEAM_FLOOR.items()}


def model_dict(mname):
    """The model section of a config: a coverage config of this file, or an entry of config.MODEL_CONFIGS."""
    return dict(COVERAGE[mname] if mname in COVERAGE else config.MODEL_CONFIGS[mname])


def model_cfg(mname):
    return config.make_config(model_dict(mname), N_VOCAB, N_SPK)


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
    return (False, True) if mname in VOCOS or mname in COVERAGE else (None,)


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


def seam_floor(mname, wide=False):
    """Worst (rel, local) of the float32 oracle against the float64 oracle over SEAM_SHAPES[mname], both heads, at the
    seam sweep's own seeds; `wide`: also over row 0 of every wide case (WIDE_CONFIG only)."""
    cfg, sd, cd, W32, W64 = weights(mname)
    cases = [(B, L, SEAM_SEED + i, B) for i, (B, L) in enumerate(SEAM_SHAPES[mname])]
    if wide:
        assert mname == WIDE_CONFIG
        cases += [(B, L, WIDE_SEED + i, 1) for i, (B, L) in enumerate(WIDE_SHAPES)]
    worst = [0.0, 0.0]
    for B, L, seed, rows in cases:
        z, g = inputs(W32, B, L, seed)
        z, g = z[:rows], g[:rows]
        for head in heads(mname):
            rel, loc = gates(oracle(W32, cd, z, g, head), oracle(W64, cd, z, g, head))
            worst = [max(worst[0], rel), max(worst[1], loc)]
    return tuple(worst)


# ---- geometry of the Vocos head (run_vocos in csrc/model.hip) restated; for choosing lengths, no kernel reads it --------
def cdiv(a, b):
    return -(-a // b)


def vocos_frames(L):
    """(F, Fs): frames after nn.ReflectionPad1d([1, 0]) and the padded row stride of every [B][C][Fs] tensor."""
    return L + 1, (L + 1 + 3) & ~3


def dwln_tiles(C, L):
    """convnext_dwln_kernel over one row of Fs columns (kernels.hip): 62 output columns per block.  `inst`: the
    instantiation k_convnext_dwln picks (PER = C / 16 in {4, 16, 32}), None: it refuses and run_vocos falls back to
    k_dwconv + k_layernorm (no tiles there; the same figures are kept so that the lengths can be judged alike).
    `last_cols` / `last_valid`: stored / valid (< F) columns of the last tile; `junk` = Fs - F."""
    F_, Fs = vocos_frames(L)
    tiles = cdiv(Fs, 62)
    inst = C // 16 if C % 16 == 0 and C // 16 in (4, 16, 32) else None
    return dict(inst=inst, tiles=tiles, last_cols=Fs - 62 * (tiles - 1), last_valid=max(0, F_ - 62 * (tiles - 1)),
                junk=Fs - F_, F=F_, Fs=Fs)


def pw_schedule(strips, U, K, cus, slots=4):
    """gemm_pw.hip:pw_schedule: (S blocks per strip, upb 32-column units per block) from the CU count."""
    best, bestS = 1e30, 1
    for S in range(1, U + 1):
        upb = cdiv(U, S)
        if S > 1 and cdiv(U, S - 1) == upb:
            continue
        blocks = strips * cdiv(U, upb)
        per_cu = cdiv(blocks, cus)
        npass = upb // 4 + (1 if upb % 4 >= 2 else 0) + (upb % 4 & 1)
        block_cost = float(upb) * K + npass * (0.12 * K + 96.0)
        block_cost += (2.0 * K * 0.08 if upb % 4 >= 2 else 0.0) + (1.0 * K * 0.20 if upb % 4 & 1 else 0.0)
        resident = min(per_cu, slots)
        eff = 1.0 if resident >= 3 else 0.85 if resident == 2 else 0.6
        cost = float(per_cu) * block_cost / eff
        if cost < best * 0.999:
            best, bestS = cost, cdiv(U, upb)
    return bestS, cdiv(U, bestS)


def pw_passes(U, S, upb):
    """The pass widths (4 / 2 / 1 units) of each of the S blocks of a strip, as pw_gemm_kernel walks them."""
    out = []
    for part in range(S):
        u, u1, ws = part * upb, min(part * upb + upb, U), []
        while u < u1:
            w = 4 if u1 - u >= 4 else 2 if u1 - u >= 2 else 1
            ws.append(w)
            u += w
        out.append(tuple(ws))
    return tuple(out)


def vocos_launches(mname, B, L, form, cus=256):
    """The five kinds of conv launch of one Vocos decode of [B, 192, L] (in, pw1, pw2, out, istft; pw1 / pw2 once per
    layer, all layers alike), form "default" (small_max_tiles = 256) or "tiled" (0): a restatement of launch_conv's
    order -- launch_conv_small's take rule, then pw_gemm_eligible, else conv_mfma_kernel -- and of pw_schedule.  One
    dict per conv: kernel ("small" / "pw_gemm" / "tiled"), M, K (the reduction in whole 16-channel chunks), N = Fs,
    and for pw_gemm: S, upb, passes (per block of a strip), U, last_unit (stored columns of the last 32-column unit)
    and last_valid (those of them in front of F)."""
    m = model_dict(mname)
    VC, VH, NF = m["vocos_channels"], m["vocos_h_channels"], m["vocos_istft_config"]["n_fft"]
    VO = NF + 2
    F_, Fs = vocos_frames(L)
    small_max = 256 if form == "default" else 0
    out = []
    for name, M, Cin, res, padded in (("in", VC, m["inter_channels"], False, False), ("pw1", VH, VC, False, False),
                                      ("pw2", VC, VH, True, False), ("out", VO, VC, False, False),
                                      ("istft", NF, VO, False, True)):
        nchunks = cdiv(Cin, 16)
        r = dict(conv=name, M=M, K=nchunks * 16, N=Fs)
        tiles64 = cdiv(M, 64) * cdiv(Fs, 64) * B
        eligible = not (res and M % 32) and (Cin % 16 == 0 or padded) and Cin >= 32 and M * Fs * 4 < 2 ** 31 and \
            nchunks * 16 * Fs * 4 < 2 ** 31  # (Fs % 4 == 0 and 256-byte aligned workspace tensors: the other terms hold)
        if 0 < tiles64 <= small_max and nchunks >= 2:
            r["kernel"] = "small"
        elif eligible:
            U = cdiv(Fs, 32)
            S, upb = pw_schedule(B * cdiv(M, 128), U, nchunks * 16, cus)
            r.update(kernel="pw_gemm", U=U, S=S, upb=upb, passes=pw_passes(U, S, upb), last_unit=Fs - 32 * (U - 1),
                     last_valid=F_ - 32 * (U - 1))
        else:
            r["kernel"] = "tiled"
        out.append(r)
    return out


def pw_patterns(cases, form, cus=256):
    """What the pw_gemm launches of `cases` [(config, B, L)] reach: {conv: dict(widths, mixed, upb, split, partial,
    full)} -- pass widths seen, a block of >= 2 passes of different width, the largest upb, S > 1 with upb > 1, a last
    unit of fewer than 32 columns, a full last unit."""
    acc = {}
    for mname, B, L in cases:
        for r in vocos_launches(mname, B, L, form, cus):
            if r["kernel"] != "pw_gemm":
                continue
            e = acc.setdefault(r["conv"], dict(widths=set(), mixed=False, upb=0, split=False, partial=False, full=False))
            for blk in r["passes"]:
                e["widths"] |= set(blk)
                e["mixed"] |= len(set(blk)) >= 2
            e["upb"] = max(e["upb"], r["upb"])
            e["split"] |= r["S"] > 1 and r["upb"] > 1
            e["partial"] |= r["last_unit"] < 32
            e["full"] |= r["last_unit"] == 32
    return acc


def wide_claims(cus):
    """What the wide cases must reach on pw_gemm_kernel at the default dispatch with `cus` compute units: (patterns,
    the claims that do NOT hold).  The CPU tier asserts them at 256 CUs, the GPU tier at the device's own count."""
    pat = pw_patterns([(WIDE_CONFIG, B, L) for B, L in WIDE_SHAPES], "default", cus)
    every = set().union(*(e["widths"] for e in pat.values())) if pat else set()
    claims = {
        "every conv (in, pw1, pw2, out, istft) runs on pw_gemm_kernel": set(pat) == {"in", "pw1", "pw2", "out", "istft"},
        "pass widths 1, 2 and 4": every == {1, 2, 4},
        "a block of passes of different width": any(e["mixed"] for e in pat.values()),
        "upb >= 8": any(e["upb"] >= 8 for e in pat.values()),
        "S > 1 together with upb > 1": any(e["split"] for e in pat.values()),
        "a last unit of fewer than 32 columns": any(e["partial"] for e in pat.values()),
        "a full last unit": any(e["full"] for e in pat.values()),
        "a pass wider than one unit on the residual conv pw2": pat.get("pw2", {}).get("upb", 0) > 1,
        "a pass wider than one unit on the padded-K iSTFT conv": pat.get("istft", {}).get("upb", 0) > 1,
    }
    return pat, [k for k, ok in claims.items() if not ok]


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
