"""GPU tier: the front half of infer() -- the text encoder (embedding, relative-position attention, FFN convs, layer
norms, proj) and the duration predictors (SDP reverse: dds_fused.hip or layer by layer, spline inverse; DP) -- against
the float64 oracle (oracle/vits_oracle.py: text_encoder, sdp_reverse, dp_forward, durations_to_lengths) under a
local-error gate.  Every stage of every call -- x_enc, m_p, logs_p (the prior statistics per phoneme) and logw -- is
held to rel = rms(d) / rms(ref) <= REL_GATE[config][stage] and local = max|d| / rms(ref) <= LOCAL_GATE[config][stage]
over the whole tensor: one wrong attention column, band term or last key does not hide in 192 channels and a whole
utterance.  The gates are 4 x the error of the float32 oracle against the float64 oracle on the same inputs
(tests/encoder_input.py; calibrated, and shown to see one lost band term by >= 10 x, in
tests/test_cpu_encoder_gate.py).  x_mask must be equal, every stage exactly zero behind x_lengths, and w_ceil and
y_lengths equal except where the float64 duration lies within 1e-5 of an integer (at most 0.5 % of a sweep).
Every kernel form is compared with the oracle, never with another form.

Forms (WETTS_TUNE is read at create, so a form is a model):
  default        the product dispatch: attn_small_kernel up to Tx = 128 (16-byte staging when Tx is a multiple of 4,
                 scalar staging otherwise; the 142,336-byte LDS opt-in at Tx = 128, dk = 96), the matrix-core path
                 (attn_relk, attn_scores_mfma with the band epilogue, attn_softmax, attn_transpose_v, attn_pv_mfma
                 over three 32-row d-blocks, attn_relv_add) from Tx = 129; dds_fused mode 1 (small calls)
  general        attn_small_max_t=0: what a device that refuses the large-LDS opt-in runs -- the scalar kernels
                 (attn_scores, attn_softmax, attn_pv) below Tx = 64, the matrix-core path from 64
  dds_layerwise  dds_fused=0: every DDSConv of the SDP layer by layer (SDP models)
  dds_fused64    dds_fused=2: every DDSConv in one launch at any size, 64-column tiles (SDP models)
tests/test_cpu_encoder_gate.py asserts what SHAPES reaches of each form.  Not covered here or anywhere: the window-less
three-kernel path for heads wider than 48 channels (attention_form "mfma_plain"), which no config the reference can
construct reaches; the graphed encoder's length buckets and the 16-bit flow have tests of their own."""
import os

import numpy as np
import pytest
import torch

from tests import encoder_input as ei
from tests import util
from wetts_amd import SynthesizerTrn, config

pytestmark = pytest.mark.gpu

FORMS = {"default": None, "general": "attn_small_max_t=0", "dds_layerwise": "dds_fused=0", "dds_fused64": "dds_fused=2"}
SWEEP = [(m, f) for m in ei.CONFIGS for f in FORMS if m in ei.SDP or not f.startswith("dds_")]
NOISE_SCALE, NEAR_INTEGER, MAX_LEFT_OUT = 0.667, 1e-5, 0.005


def _net(mname, form="default"):
    cfg, sd, cd, W32, W64 = ei.weights(mname)
    net = SynthesizerTrn(ei.N_VOCAB, 513, 32, n_speakers=ei.N_SPK, **config.MODEL_CONFIGS[mname])
    if FORMS[form] is not None:
        os.environ["WETTS_TUNE"] = FORMS[form]
    try:
        net.load_state_dict(sd).to("cuda")  # (a per-model setting, read at create)
    finally:
        os.environ.pop("WETTS_TUNE", None)
    return net, cd, W64


_REFS = {}


def _refs(mname):
    """[(B, Tx, noise_scale_w, inputs, float64 oracle stages)] over SHAPES[mname]: computed once, shared by every form."""
    if mname not in _REFS:
        cfg, sd, cd, W32, W64 = ei.weights(mname)
        out = []
        for i, (B, Tx, nsw) in enumerate(ei.SHAPES[mname]):
            ins = ei.inputs(B, Tx, 2000 + i)  # the inputs the floor was measured on
            out.append((B, Tx, nsw, ins, ei.stages(W64, cd, *ins, nsw)))
        _REFS[mname] = out
    return _REFS[mname]


def _gpu(net, x, xl, sid, eps_w, nsw):
    st = net._encode(x.cuda(), xl.cuda(), sid.cuda(), NOISE_SCALE, 1.0, nsw, eps_w.cuda(), None)
    torch.cuda.synchronize()
    I = net.inter_channels
    out = dict(x_enc=st["x_enc"], m_p=st["stats"][:, :I], logs_p=st["stats"][:, I:], x_mask=st["x_mask"].unsqueeze(1),
               logw=st["logw"].unsqueeze(1), w_ceil=st["w_ceil"].unsqueeze(1), y_lengths=st["y_lengths"])
    return {k: v.detach().cpu() for k, v in out.items()}


def _check_stages(tag, mname, got, ref, worst, rows=None):
    """Mask, the two gates and the zeros of one call; `rows`: the batch rows of `got` that `ref` holds.  The failure
    names the stage, the shape, and the row and column of the largest error."""
    if rows is not None:
        got = {k: v[rows] for k, v in got.items()}
    assert torch.equal(got["x_mask"].double(), ref["x_mask"]), (tag, "x_mask")
    pad = ref["x_mask"] == 0
    for s in ei.GATED:
        g, r = got[s], ref[s]
        assert g.shape == r.shape, (tag, s, g.shape, r.shape)
        assert bool(torch.isfinite(g).all()), (tag, s, "not finite")
        assert bool((g[pad.expand_as(g)] == 0).all()), (tag, s, "not zero behind x_lengths")
        rel, loc = ei.gates(g, r)
        w = worst.setdefault(s, [0.0, 0.0, 0.0])
        d = (g.double() - r).abs()
        spread = float(d.max()) / max(util.rms(d.numpy()), 1e-300)
        if loc > w[1]:
            w[2] = spread
        w[0], w[1] = max(w[0], rel), max(w[1], loc)
        at = np.unravel_index(int(d.argmax()), d.shape)
        msg = (tag, s, f"rel {rel:.3g} (gate {ei.REL_GATE[mname][s]:.3g})",
               f"local {loc:.3g} (gate {ei.LOCAL_GATE[mname][s]:.3g})", f"max|d| / rms(d) {spread:.2f}",
               f"max |d| at row {at[0]} channel {at[1]} column {at[2]} of {g.shape[-1]}")
        assert rel <= ei.REL_GATE[mname][s] and loc <= ei.LOCAL_GATE[mname][s], msg


def _check_durations(tag, got, ref, tally):
    """w_ceil and y_lengths equal to the oracle's; an entry whose float64 duration lies within 1e-5 * max(1, w) of an
    integer may differ, and then its row's y_lengths is not compared.  tally = [left out, valid entries]."""
    w = ref["w"]
    near = (w - torch.round(w)).abs() <= NEAR_INTEGER * torch.clamp_min(w, 1.0)
    differ = got["w_ceil"].double() != ref["w_ceil"]
    bad = differ & ~near
    assert not bool(bad.any()), (tag, "w_ceil", [(int(b), int(t), float(w[b, 0, t]), float(got["w_ceil"][b, 0, t]))
                                                 for b, _, t in bad.nonzero()[:8]])
    rows_ok = ~differ.flatten(1).any(1)
    assert torch.equal(got["y_lengths"][rows_ok], ref["y_lengths"][rows_ok]), (tag, "y_lengths")
    tally[0] += int(differ.sum())
    tally[1] += int(ref["x_mask"].sum())


def _report(tag, mname, worst, tally=None):
    fig = {s: (float(f"{w[0]:.3g}"), float(f"{w[1]:.3g}"), float(f"{w[2]:.2f}")) for s, w in worst.items()}
    gate = {s: (float(f"{ei.REL_GATE[mname][s]:.3g}"), float(f"{ei.LOCAL_GATE[mname][s]:.3g}")) for s in ei.GATED}
    print(f"{tag}: worst (rel RMS, max|d|/rms, max|d|/rms(d) there) = {fig}; gates {gate}; floor {ei.FLOOR[mname]}"
          + (f"; durations left out {tally[0]} of {tally[1]}" if tally else ""))


# ---- the sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,form", SWEEP)
def test_encoder_sweep_matches_float64_oracle(mname, form):
    net, cd, W64 = _net(mname, form)
    worst, tally = {}, [0, 0]
    for B, Tx, nsw, ins, ref in _refs(mname):
        got = _gpu(net, *ins, nsw)
        _check_stages((mname, form, B, Tx, nsw), mname, got, ref, worst)
        _check_durations((mname, form, B, Tx, nsw), got, ref, tally)
    _report(f"{mname} {form} sweep ({len(ei.SHAPES[mname])} cases)", mname, worst, tally)
    assert tally[0] <= MAX_LEFT_OUT * tally[1], tally


# ---- batch and head indexing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tx", [129, 64])
@pytest.mark.parametrize("form", ["default", "general"])
def test_batch_of_32_rows_are_independent_and_match_the_oracle(form, Tx):
    """B = 32 (64 attention heads per launch): the front half has no cross-batch term, so one utterance repeated 32
    times must give 32 bit-equal rows (every block of every grid against its neighbours), and one float64 oracle row pins
    them all.  Then 32 different ragged utterances, rows 0 and 31 against the oracle of those two rows alone."""
    B, mname = 32, "tiny"
    net, cd, W64 = _net(mname, form)
    x, xl, sid, eps_w = ei.inputs(B, Tx, 31337 + Tx)
    worst = {}
    rep = [t[:1].expand(B, *t.shape[1:]).contiguous() for t in (x, xl, sid, eps_w)]
    rep[1] = torch.full((B,), Tx)
    same = _gpu(net, *rep, ei.NOISE_SCALE_W)
    for s in ei.GATED + ("w_ceil", "y_lengths"):
        rows = [b for b in range(1, B) if not torch.equal(same[s][b], same[s][0])]
        assert not rows, f"{s}: rows {rows} differ from row 0 of a repeated utterance"
    ref0 = ei.stages(W64, cd, *(t[:1] for t in rep), ei.NOISE_SCALE_W)
    _check_stages((mname, form, "repeated", Tx), mname, same, ref0, worst, rows=[0])
    ends = [0, B - 1]
    diff = _gpu(net, x, xl, sid, eps_w, ei.NOISE_SCALE_W)
    ref = ei.stages(W64, cd, x[ends], xl[ends], sid[ends], eps_w[ends], ei.NOISE_SCALE_W)
    _check_stages((mname, form, "distinct", Tx, xl[ends].tolist()), mname, diff, ref, worst, rows=ends)
    _check_durations((mname, form, "distinct", Tx), {k: v[ends] for k, v in diff.items()}, ref, [0, 0])
    _report(f"{mname} {form} {B} x {Tx}", mname, worst)


# ---- padding invariance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "general"])
@pytest.mark.parametrize("B,Tx", [(3, 33), (2, 129)])
def test_ids_behind_x_lengths_change_nothing(form, B, Tx):
    """Other valid ids behind x_lengths: every stage bit-identical on the valid columns and zero behind them."""
    net, cd, W64 = _net("tiny", form)
    x, xl, sid, eps_w = ei.inputs(B, Tx, 555 + Tx)
    valid = torch.arange(Tx)[None, :] < xl[:, None]
    assert int((~valid).sum()) > 0
    other = torch.randint(0, ei.N_VOCAB, (B, Tx), generator=torch.Generator().manual_seed(556))
    x2 = torch.where(valid, x, other)
    assert not torch.equal(x, x2)
    a, b = _gpu(net, x, xl, sid, eps_w, ei.NOISE_SCALE_W), _gpu(net, x2, xl, sid, eps_w, ei.NOISE_SCALE_W)
    for s in ei.GATED + ("w_ceil",):
        v = valid.unsqueeze(1).expand_as(a[s])
        assert torch.equal(a[s][v], b[s][v]), s
        assert bool((a[s][~v] == 0).all()) and bool((b[s][~v] == 0).all()), s
    assert torch.equal(a["y_lengths"], b["y_lengths"]) and torch.equal(a["x_mask"], b["x_mask"])
