"""Shared by tests/test_cpu_encoder_gate.py and tests/test_gpu_encoder_oracle.py: the models, inputs, stages and gates of
the front half of infer() -- text encoder (embedding, relative-position attention, FFN convs, layer norms, proj) and
the duration predictor (SDP reverse with its spline inverse, or DP) -- against the float64 oracle, and the dispatch of
attention.hip:k_rel_attention restated in Python (for choosing shapes; no kernel reads it).

Stages (stages()): x_enc [B, H, Tx], m_p / logs_p [B, inter, Tx] (the prior statistics per phoneme, `stats` of the
device call, before length regulation), x_mask, logw [B, 1, Tx], w_ceil, y_lengths.

The gates.  `rel = rms(d) / rms(ref)` and `local = max|d| / rms(ref)` over a whole stage tensor, padded columns included,
d = device - float64 oracle.  FLOOR[config][stage] is the worst (rel, local) of the oracle run at float32 against the
same oracle at float64 over SHAPES[config]: the honest cost of f32 arithmetic for this operation on the reference side.
REL_GATE / LOCAL_GATE are FACTOR x that floor (4 x, the project's convention: the kernels sum in another order than the
CPU matmul and conv, and the floor is the worst of a few dozen draws, not a bound).  tests/test_cpu_encoder_gate.py
recomputes the floor of the cheap configs, holds the constants to 2 .. 8 x it, and proves that the local gate of x_enc
sees one lost band term, a masked last key and a key dropped from the softmax sum by a factor >= 10."""
import torch
import torch.nn.functional as F

from tests import decoder_input as di
from wetts_amd import config

N_VOCAB, N_SPK, WSEED = di.N_VOCAB, di.N_SPK, di.WSEED
GATE_FACTOR = 4.0
NOISE_SCALE_W, TAIL_NOISE_SCALE_W = 0.8, 3.0  # 3.0 sends spline inputs beyond +-5, into the linear tails
WINDOW = 4  # attentions.Encoder's window_size, and the pre_conv2 flows'

SDP = ("tiny", "tiny_preconv2_spk", "v1")
CONFIGS = ("tiny", "tiny_dp", "tiny_preconv2_spk", "v1")
GATED = ("x_enc", "m_p", "logs_p", "logw")

# Tx: the band wider than the sequence | the 32-query strips and 32-key tiles | both staging branches of the small
# kernel and its largest LDS footprint | the first lengths of the matrix-core path (the last 128-key block of the
# scores grid holds 1, 2, 31, 32, 33 keys) | the third 128-key block, and a length that is no multiple of anything
LENGTHS = (1, 2, 3, 4, 5, 8, 9, 10, 31, 32, 33, 63, 64, 65, 95, 96, 97, 100, 125, 126, 127, 128, 129, 130, 159, 160,
           161, 255, 256, 257, 300)
_V1_LENGTHS = (1, 5, 33, 64, 97, 126, 128, 129, 161, 257)  # six layers, filter_channels 768: a trimmed list
_BS = (1, 2, 3, 5)


def _shapes(lengths, tail):
    out = [(_BS[i % len(_BS)], Tx, NOISE_SCALE_W) for i, Tx in enumerate(lengths)]
    return tuple(out + ([tail] if tail else []))


# (B, Tx, noise_scale_w) per config; the last case of an SDP model draws the spline's linear tails
SHAPES = {
    "tiny": _shapes(LENGTHS, (3, 65, TAIL_NOISE_SCALE_W)),
    "tiny_dp": _shapes(LENGTHS, None),
    "tiny_preconv2_spk": _shapes(LENGTHS, (3, 65, TAIL_NOISE_SCALE_W)),
    "v1": _shapes(_V1_LENGTHS, (2, 33, TAIL_NOISE_SCALE_W)),
}

def _gate(i):
    return {m: {s: FACTOR[m] * v[i] for s, v in FLOOR[m].items()} for m in FLOOR}


# Worst (rel, local) per stage of oracle-at-float32 against oracle-at-float64 over SHAPES[config] (seed = 2000 + index),
# measured on one CPU (torch CPU kernels); the gates are FACTOR x these.
FLOOR = {
    "tiny": dict(x_enc=(4.34e-07, 2.72e-06), m_p=(4.92e-07, 3.78e-06), logs_p=(5.24e-07, 3.96e-06),
                 logw=(1.06e-07, 1.16e-06)),
    "tiny_dp": dict(x_enc=(4.34e-07, 2.72e-06), m_p=(4.92e-07, 3.78e-06), logs_p=(5.24e-07, 3.96e-06),
                    logw=(4.10e-07, 1.59e-06)),
    "tiny_preconv2_spk": dict(x_enc=(4.15e-07, 2.79e-06), m_p=(4.61e-07, 3.67e-06), logs_p=(4.55e-07, 4.31e-06),
                              logw=(1.05e-07, 7.00e-07)),
    "v1": dict(x_enc=(5.34e-07, 4.04e-06), m_p=(5.79e-07, 4.13e-06), logs_p=(6.30e-07, 5.16e-06),
               logw=(1.78e-07, 1.06e-06)),
}
# The float32 oracle's ceil(exp(logw)) differed from the float64 oracle's on none of the 4990 / 4891 / 4990 / 1482 valid
# phonemes of these sweeps.
# Measured on an MI355X (profiles/r08_encoder_oracle_gates.txt), worst over every form of a config, as a multiple of
# the floor: x_enc / m_p / logs_p rel 0.6 - 0.8 x and local 0.5 - 0.85 x over the sweeps, 1.2 x / 1.3 x at 32 x 129;
# logw rel up to 2.1 x (tiny, dds_fused=0) and local up to 2.3 x (tiny_preconv2_spk: 1.64e-6, max|d| = 19 x rms(d), a
# single phoneme).  No form needs a raised factor.
FACTOR = {k: GATE_FACTOR for k in FLOOR}
REL_GATE, LOCAL_GATE = _gate(0), _gate(1)


def weights(mname):
    return di.weights(mname)


def lengths_of(B, Tx, gen):
    """Ragged x_lengths of a [B, Tx] batch: a row of Tx, a row of 1, a row 1 past a multiple of 32 (the largest such
    length below Tx; with Tx < 34 the length-1 row is that row and the third is drawn), the others drawn from 1 .. Tx;
    rotated so that the full row is not always row 0."""
    if B == 1:
        return torch.tensor([Tx])
    rows = [Tx, 1]
    if B > 2:
        rows.append(32 * ((Tx - 2) // 32) + 1 if Tx >= 34 else int(torch.randint(1, Tx + 1, (1,), generator=gen)))
    while len(rows) < B:
        rows.append(int(torch.randint(1, Tx + 1, (1,), generator=gen)))
    k = Tx % B
    return torch.tensor(rows[k:] + rows[:k])


def inputs(B, Tx, seed):
    """(ids [B, Tx], x_lengths [B], sid [B], eps_w [B, 2, Tx] ~ N(0, 1))."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, N_VOCAB, (B, Tx), generator=gen)
    xl = lengths_of(B, Tx, gen)
    sid = torch.randint(0, N_SPK, (B,), generator=gen)
    eps_w = torch.randn(B, 2, Tx, generator=gen)
    return x, xl, sid, eps_w


def stages(W, cd, x, xl, sid, eps_w, noise_scale_w=NOISE_SCALE_W, length_scale=1.0):
    """The front half of vits_oracle.infer at the dtype of W."""
    vo, d = di.vo(), W["enc_p.emb.weight"].dtype
    with torch.no_grad():
        g = F.embedding(sid, W["emb_g.weight"]).unsqueeze(-1) if cd["n_speakers"] > 0 else None
        x_enc, m_p, logs_p, x_mask = vo.text_encoder(W, cd, x, xl, g)
        if cd["use_sdp"]:
            logw = vo.sdp_reverse(W, cd, x_enc, x_mask, g, eps_w.to(d), noise_scale_w)
        else:
            logw = vo.dp_forward(W, cd, x_enc, x_mask, g)
        w_ceil, y_lengths = vo.durations_to_lengths(logw, x_mask, length_scale)
        w = torch.exp(logw) * x_mask * length_scale
    return dict(x_enc=x_enc, m_p=m_p, logs_p=logs_p, x_mask=x_mask, logw=logw, w=w, w_ceil=w_ceil, y_lengths=y_lengths)


def gates(got, ref):
    return di.gates(got, ref)


def floor(mname, shapes=None):
    """{stage: worst (rel, local)} of the float32 oracle against the float64 oracle over SHAPES[mname] (or the subset
    `shapes`), and the number of valid w_ceil entries on which the two differ."""
    cfg, sd, cd, W32, W64 = weights(mname)
    worst, flips, n = {s: [0.0, 0.0] for s in GATED}, 0, 0
    for i, (B, Tx, nsw) in enumerate(SHAPES[mname]):
        if shapes is not None and (B, Tx, nsw) not in shapes:
            continue
        x, xl, sid, eps_w = inputs(B, Tx, 2000 + i)
        a, r = stages(W32, cd, x, xl, sid, eps_w, nsw), stages(W64, cd, x, xl, sid, eps_w, nsw)
        for s in GATED:
            rel, loc = gates(a[s], r[s])
            worst[s] = [max(worst[s][0], rel), max(worst[s][1], loc)]
        flips += int((a["w_ceil"].double() != r["w_ceil"]).sum())
        n += int(r["x_mask"].sum())
    return {s: tuple(v) for s, v in worst.items()}, flips, n


# ---- the dispatch of attention.hip:k_rel_attention --------------------------------------------------------------------
def small_layout(T, dk, window=WINDOW):
    """attention.hip:attn_small_layout -> (Tp, Tk, SS, lds bytes)."""
    nrel = 2 * window + 1
    Tp = (T + 3) & ~3
    Tk = Tp + ((nrel + 3) & ~3)
    SS = Tk + (0 if (Tk >> 2) & 1 else 4)
    return Tp, Tk, SS, (dk * 32 + 2 * dk * Tk + 32 * SS + 32 * 36) * 4


def attention_form(window, T, dk, small_max_t=128, large_lds=True):
    """The kernels k_rel_attention launches for one attention of T positions: "small" (attn_small_kernel), "flash"
    (attn_transpose_v + attn_flash), "mfma_windowed" (attn_relk, attn_scores_mfma with the band epilogue, attn_softmax,
    attn_transpose_v, attn_pv_mfma, attn_relv_add), "mfma_plain" (the same without the two relative kernels; window-less
    heads wider than 48 channels, which no config of the reference has) or "scalar" (attn_scores, attn_softmax,
    attn_pv).  `window` < 0 or None: no relative terms.  `large_lds`: whether the device grants the > 64 KiB opt-in."""
    window = -1 if window is None else window
    if window >= 0 and T <= min(small_max_t, 128):
        lds = small_layout(T, dk, window)[3]
        if lds <= 150 * 1024 and (lds <= 64 * 1024 or large_lds):
            return "small"
    if window < 0 or T >= 64:
        if window < 0 and dk <= 48:
            return "flash"
        return "mfma_windowed" if window >= 0 else "mfma_plain"
    return "scalar"


def small_staging(T):
    """Which staging branch attn_small_kernel takes for k and v: 16-byte pieces when T is a multiple of 4."""
    return "vec16" if T % 4 == 0 else "scalar"


def encoder_attention(mname):
    """(window, dk) of the text encoder's attention."""
    m = config.MODEL_CONFIGS[mname]
    return WINDOW, m["hidden_channels"] // m["n_heads"]


def flow_attention(mname):
    """(window, dk) of the attention inside a transformer flow: pre_conv2 runs a windowed encoder over all
    hidden_channels, every other type a window-less one over half of them; two heads either way (model.hip)."""
    m = config.MODEL_CONFIGS[mname]
    if not m.get("use_transformer_flows"):
        return None
    if m.get("transformer_flow_type") == "pre_conv2":
        return WINDOW, m["hidden_channels"] // 2
    return -1, m["hidden_channels"] // 4


def flash_tiles(T):
    """(32-key tiles of wave 0 of attn_flash_kernel, keys in the sequence's last tile): the four waves of a block walk
    the keys in strides of 128."""
    return len(range(0, T, 128)), T - 32 * ((T - 1) // 32)
