"""The numerics spec of the text frontend's 16-bit mode (csrc/frontend16.hip, FrontendModel.set_dtype), as code.

With bf16 or f16 set, each of the six Linears of a layer (q, k, v packed as one, attention output, feed-forward in and
out; the BERT layers and `transform`) reads BOTH operands rounded to the type, round to nearest even; products are exact
and accumulation is in f32, in an order that is the kernel's choice; bias, GELU (erf form), ReLU and the residual add are
f32 epilogues.  Everything else -- embeddings, LayerNorms, attention on the f32 qkv, the residual stream, both
classifiers, the softmaxes -- is tests/frontend_oracle.py's arithmetic unchanged.  Where a rounded value is stored is
free: rounding at the producer's store and at the consumer's load give the same bits.

`forward16` is frontend_oracle.forward with those Linears replaced by F.linear(q(x), q(W), b) at the dtype of the weights
it is given: float64 weights give the spec's oracle, float32 weights a CPU realisation of it (`split8`: a second one that
sums K as fe_linear_kernel's block does).  (A float64 activation passes through float32 on its way to the type, as
torch converts it; that differs from the direct rounding only at a tie closer than 2^-24 relative, far inside every
figure measured here.  The per-launch references below receive float32 inputs, which the conversion rounds once.)

Gates.
 * End to end the gate is 3 x D per output and measure, D = the (rel RMS, local) figure of forward16(float64 weights)
   against the full float64 model frontend_oracle.forward: the mode's own precision loss.  Not a floor against the
   spec's own float64 evaluation: one operand rounding that falls the other way perturbs everything downstream by ~1e-4
   and flips roundings wholesale in later layers, so two faithful realisations differ by about half the precision loss
   itself (measured 2e-3 against D = 4e-3 at bf16, bimodal per case; tests/conv16_oracle.py records the same for the
   decoder).  score()'s two losses are held to the same relative gate against the float64 model's losses:
   |loss - loss64| / |loss64| <= 3 x D_rel of the head's logits.
 * Per launch, against float64 ON THE ROUNDED OPERANDS (`linear_ref`): gate 1, per element, |got - y| <= (K + 4) 2^-24 S
   (S = the same Linear on absolute values + |bias| + |residual|: conv16_oracle.gate's f32-accumulation term) for the
   bias, ReLU and residual epilogues; gate 2, for all four, (rel, local) <= GATE_FACTOR x the figures of torch's
   float32 evaluation of the same launch on the same rounded operands."""
import torch
import torch.nn.functional as F

from tests import frontend_oracle as fo

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
PRECISION = {"bf16": 1, "f16": 2}
EPILOGUES = ("linear_bias", "linear_gelu", "linear_relu", "linear_residual")  # WETTS_FRONTEND_EPI_* 0 .. 3, stage names
U32 = 2.0 ** -24
E2E_FACTOR = 3.0
# the token tile of each kernel form of wetts_frontend_linear16 (1 = K split, 2 / 3 = tiled GEMM)
FORM_TILE = {1: 64, 2: 64, 3: 128}
EDGE_KM = ((8, 4), (24, 36), (312, 312), (1200, 312), (768, 100))
# end-to-end defects the 3 x D gate must see; tanh_gelu and eps_1e-5 lie inside the mode's precision loss
SEEN_FAULTS = ("no_position", "swap_qk", "no_residual", "softmax_axis", "pad_key", "transform_12_heads")


def q(t, dtype):
    """Round to nearest even to `dtype`, widened back to t's own dtype."""
    return t.to(dtype).to(t.dtype)


def linear16(x, w, b, dtype):
    return F.linear(q(x, dtype), q(w, dtype), b)


def split8(x, w, b):
    """F.linear(x, w, b) with K summed in 8 interleaved chunks (chunk j: the 8-element steps j, j + 8, ..) whose partial
    sums are added pairwise, ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)), then the bias: a K-split block's order."""
    K = x.shape[-1]
    pad = -K % 64
    xs = F.pad(x, (0, pad)).reshape(*x.shape[:-1], -1, 8, 8)
    ws = F.pad(w, (0, pad)).reshape(w.shape[0], -1, 8, 8)
    p = [F.linear(xs[..., :, j, :].reshape(*x.shape[:-1], -1), ws[:, :, j, :].reshape(w.shape[0], -1)) for j in range(8)]
    y = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))
    return y if b is None else y + b


def linear16_split8(x, w, b, dtype):
    return split8(q(x, dtype), q(w, dtype), b)


def _block16(W, names, h, mask, heads, act, eps, lin, fault=None, qk_fault=None):
    """frontend_oracle.block with its four Linears through `lin`."""
    wqkv, bqkv, out, n1, l1, l2, n2 = names
    a = fo.attention(lin(h, wqkv, bqkv), mask, heads, qk_fault if qk_fault else fault)
    a = lin(a, W[out + ".weight"], W[out + ".bias"])
    h = fo.layer_norm(a if fault == "no_residual" else a + h, W[n1 + ".weight"], W[n1 + ".bias"], eps)
    f = act(lin(h, W[l1 + ".weight"], W[l1 + ".bias"]))
    f = lin(f, W[l2 + ".weight"], W[l2 + ".bias"])
    return fo.layer_norm(f + h, W[n2 + ".weight"], W[n2 + ".bias"], eps)


def forward16(W, cname, ids, mask, dtype, tt=None, fault=None, linear=linear16):
    """frontend_oracle.forward in the 16-bit mode: the four outputs (and `transform`) at W's dtype.  `linear`:
    linear16 (torch's summation order) or linear16_split8."""
    c = fo.config(cname)
    tt = torch.zeros_like(ids) if tt is None else tt
    eps = 1e-5 if fault == "eps_1e-5" else c["layer_norm_eps"]
    common = fault if fault in ("pad_key", "no_residual") else None
    lin = lambda x, w, b: linear(x, w, b, dtype)  # noqa: E731
    h = fo.embed(W, ids, tt, eps, fault)
    for i in range(c["num_layers"]):
        h = _block16(W, fo.bert_block_names(W, i), h, mask, c["num_heads"], lambda x: fo.gelu(x, fault), eps, lin, common)
    th = 12 if fault == "transform_12_heads" else c["transform_heads"]
    h = _block16(W, fo.transform_names(W), h, mask, th, F.relu, 1e-5, lin, common, "swap_qk" if fault == "swap_qk" else None)
    out = {"transform": h}
    out["phone_logits"], out["prosody_logits"], out["phone_prob"], out["prosody_prob"] = \
        fo.heads(W, h, mask, 1 if fault == "softmax_axis" else -1)
    return out


# ---- end to end: D and the 3 x D gate -------------------------------------------------------------------------------------
_D = {}


def precision_loss(cname, lens, tname):
    """(D, ids, mask, float64 model's forward dict): D = {output: (rel, local)} of forward16(float64 weights) against
    the full float64 model at the valid tokens of a fixture case.  Computed once per process and left unchanged."""
    key = (cname, tuple(lens), tname)
    if key not in _D:
        ids, mask, st64 = fo.reference(cname, lens)
        s16 = forward16(fo.weights(cname)[1], cname, ids, mask, DTYPES[tname])
        _D[key] = {k: fo.gates(fo.valid(s16[k], mask), fo.valid(st64[k], mask)) for k in fo.OUTPUTS}
    ids, mask, st64 = fo.reference(cname, lens)
    return _D[key], ids, mask, st64


def e2e_multiples(got, st64, mask, D):
    """{output: (rel / D_rel, local / D_local)} of `got` (dict of [B, T, .] tensors) against the float64 model."""
    out = {}
    for k in fo.OUTPUTS:
        fig = fo.gates(fo.valid(got[k].detach().cpu(), mask), fo.valid(st64[k], mask))
        out[k] = (fig[0] / max(D[k][0], fo.HALF_ULP), fig[1] / max(D[k][1], fo.HALF_ULP))
    return out


def e2e_worst(mult):
    return max(max(v) for v in mult.values())


# ---- one launch ---------------------------------------------------------------------------------------------------------
def _epilogue(y, epi):
    if epi == 1:
        return F.gelu(y)
    return F.relu(y) if epi == 2 else y


def linear_ref(x, w, b, res, dtype, epi):
    """(y, S, K) of one launch in float64 on the rounded operands.  x [N, K], w [M, K], b [M], res [N, M] or None, all
    float32 as the device entry receives them; epi 0 .. 3.  S bounds the magnitude of what is summed per element."""
    xq, wq = q(x, dtype).double(), q(w, dtype).double()
    y = F.linear(xq, wq, b.double())
    S = F.linear(xq.abs(), wq.abs(), b.double().abs())
    if epi == 3:
        y, S = y + res.double(), S + res.double().abs()
    return _epilogue(y, epi), S, x.shape[1]


def linear_f32(x, w, b, res, dtype, epi, linear=F.linear):
    """torch's float32 evaluation of the launch on the same rounded operands: gate 2's floor, and (with split8) a clean
    realisation."""
    y = linear(q(x, dtype), q(w, dtype), b)
    if epi == 3:
        y = y + res
    return _epilogue(y, epi)


def launch_reference(x, w, b, res, dtype, epi):
    """What launch_multiples needs of a launch, computed once where several kernel forms run it: (y, S, K, gate 2)."""
    y, S, K = linear_ref(x, w, b, res, dtype, epi)
    return y, S, K, fo.gate(fo.gates(linear_f32(x, w, b, res, dtype, epi), y))


def launch_multiples(got, x, w, b, res, dtype, epi, ref=None):
    """(m1, m2): the worst multiple of gate 1 over the elements (None for GELU, which gate 1 does not cover) and the worst
    multiple of gate 2 over (rel, local).  A launch passes with both <= 1."""
    y, S, K, g2 = ref if ref is not None else launch_reference(x, w, b, res, dtype, epi)
    got = got.detach().cpu().reshape(y.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    m1 = None if epi == 1 else float(((got.double() - y).abs() / ((K + 4) * U32 * S).clamp_min(1e-300)).max())
    fig = fo.gates(got, y)
    return m1, max(fig[0] / g2[0], fig[1] / g2[1])


def launch_ok(m):
    return (m[0] is None or m[0] <= 1.0) and m[1] <= 1.0


def random_launch(N, K, M, seed):
    """Seeded float32 (x, w, b, res) of a launch: activations of unit scale, weights of 1 / sqrt(K)."""
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn(N, K, generator=g)
    w = torch.randn(M, K, generator=g) / K ** 0.5
    return x, w, 0.1 * torch.randn(M, generator=g), torch.randn(N, M, generator=g)


def edge_tokens(tile):
    return (1, tile - 1, tile, tile + 1, 2 * tile + 3)


# ---- the stage cases of frontend_oracle as launches ----------------------------------------------------------------------
_STAGE = {}


def stage_launches(cname, lens):
    """{stage: (x [N, K], w [M, K], b [M], res [N, M] or None)} float32, from frontend_oracle.stage_cases; once per process."""
    key = (cname, tuple(lens))
    if key not in _STAGE:
        ids, mask, _ = fo.reference(cname, lens)
        sd = fo.weights(cname)[0]
        out = {}
        for stage, (i, _) in fo.stage_cases(cname, ids, mask).items():
            if stage not in EPILOGUES:
                continue
            if stage == "linear_bias":
                w, b = (torch.cat([sd[f"bert.encoder.layer.0.attention.self.{n}.{p}"] for n in ("query", "key", "value")], 0)
                        for p in ("weight", "bias"))
            else:
                w, b = sd[i["name"] + ".weight"], sd[i["name"] + ".bias"]
            x = i["x"].reshape(-1, i["x"].shape[-1]).contiguous()
            res = i["res"].reshape(-1, i["res"].shape[-1]).contiguous() if "res" in i else None
            out[stage] = (x, w.contiguous(), b.contiguous(), res)
        _STAGE[key] = out
    return _STAGE[key]
