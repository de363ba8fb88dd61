"""GPU tier: the f32 decoder (HiFi-GAN ResBlock1 / ResBlock2 generators and the Vocos head) against the float64 oracle
(oracle/vits_oracle.py: decoder) under a local-error gate.  Every decode is held to three asserts over the whole audio
tensor: rel = rms(d) / rms(ref) <= REL_GATE[config], local = max|d| / rms(ref) <= LOCAL_GATE[config] (one wrong tile
seam, dropped tap or last sample does not hide in a whole-tensor RMS) and the abs RMS <= 1e-4 of the infer() sweeps.
The gates are 4 x the error of the float32 oracle against the float64 oracle on the same inputs (6 x for
vits2_vocos_v1, whose tiled form measured an evenly spread 4.9 x; tests/decoder_input.py:FACTOR; calibrated, and shown to see a dropped tap, a lost halo column and a lost bias span by >= 10 x,
in tests/test_cpu_decoder_gate.py).  Every kernel form is compared with the oracle, never with another form.

Forms (WETTS_TUNE is read at create, so a form is a model):
  default         the product dispatch: at these sizes the small-launch conv schedule, three-stream fork
  forced_fused    FORCED_TUNE (test_fused_resblock_pair_bit_identical's string): every ResBlock1 the chain kernel
                  supports as ONE launch (C = 32 and 64: k = 3, 7, 11; C = 128: k = 3), ResBlock2 chains fused
                  (k = 3, 5; k = 7 at dilation 12 exceeds the staging span), pair32 where the stage length is no
                  multiple of 4 (tiny_oddrate), everything else conv by conv on the tiled kernel
  forced_unfused  the same string with fused=False: every conv its own tiled launch
  pairs           PAIRS_TUNE: whole-ResBlock launches off, so the chain kernel runs (c1, c2) pairs -- every pair at
                  C = 32, k = 3 pairs at C = 64 / 128 -- a form FORCED_TUNE never reaches because whole chains win
  tiled           small_max_tiles=0 alone: the tiled conv kernel at small shapes, default fusion thresholds
  serial          serial=True: no stream fork, grouped launches
The Vocos configs have no ResBlocks: they run default and tiled, each under both iSTFT heads (set_is_onnx).

Last tiles (output columns per tile `nto`, T mod nto over SHAPES; tests/decoder_input.py:last_tiles restates the
geometry, tests/test_cpu_decoder_gate.py asserts the narrow / seam / multi-tile coverage per kernel):
  chain kernel, whole ResBlock1 (forced_fused), nto = 32 nb (4 / (C / 32)) - 2 S, S = 11 / 33 / 55 for k = 3 / 7 / 11:
    v1 (T = 64 L, 128 L, 256 L; L = 1, 2, 3, 5, 13, 37, 53)
      C = 128 k = 3, nto 106: 64, 22, 86, 2 (narrower than the 22-column halo), 90, 36, and 0 at L = 53 (32 tiles)
      C = 64, nto 234 / 190 / 146: e.g. k = 7: 128, 66, 4 (narrow), 70, 144, 176
      C = 32, nto 362 / 318 / 402: e.g. k = 7: 256, 194, 132, 8 (narrow), 148, 250
    v2 (C = 64 at 8 L, C = 32 at 64 L), stress48k (C = 64 at 256 L, C = 32 at 512 L): other remainders of the same tiles
    tiny (C = 32 at 4 L): one partial tile up to L = 50; L = 181: 724 = 2 x 362, exactly on the k = 3 seam
  chain kernel, one pair (pairs), nto = ntc - (k - 1): C = 128 k = 3: 126; C = 64 k = 3: 254; C = 32: 382 / 378 / 374
    (502 for k = 11 at dilation 5, whose margins need the 4-block tile)
    tiny L = 190: 760 = 2 x 378 + 4, narrower than the k = 7 halo of 6; L = 191: 764 = 2 x 382, on the k = 3 seam
    v1: 2 .. 116 of 126 at C = 128 (up to 19 tiles), 4 .. 304 of 382 at C = 32 (up to 36 tiles)
  pair32 (resblock32.hip; tiny_oddrate, C = 32 at 5 L when 5 L is no multiple of 4), nto = 512 - (k - 1):
    L = 102: 510 = the whole k = 3 tile, and 506 + 4 for k = 7 (narrower than its halo of 6); L = 306: 1530 = 3 x 510
    (L = 4, 8: 5 L is a multiple of 4 and the chain kernel takes the stage -- the `len % 4` guards)
  ResBlock2 chain (v3, forced_fused), nto = 128 (4 / (C / 32)) - (k - 1) d2:
    C = 128 at 8 L: k = 3, nto 124: 8 .. 104; k = 5, nto 104: 8, 16 (narrower than the halo of 24), 24, 40, 0 at
    L = 13 (on the seam), 88; C = 64 at 64 L (nto 252 / 232) and C = 32 at 256 L (nto 508 / 488): up to 41 tiles
The default dispatch takes these forms by itself only from 128 tiles up (the 128 x 128 conv tile from 1024):
test_default_dispatch_at_the_size_of_the_big_forms reaches them with one utterance repeated 32 times."""
import os

import numpy as np
import pytest
import torch

from tests import decoder_input as di
from tests import util
from wetts_amd import SynthesizerTrn, config

pytestmark = pytest.mark.gpu

FORMS = {  # name: (WETTS_TUNE at create, fused, serial)
    "default": (None, True, False),
    "forced_fused": (di.FORCED_TUNE, True, False),
    "forced_unfused": (di.FORCED_TUNE, False, False),
    "pairs": (di.PAIRS_TUNE, True, False),
    "tiled": ("small_max_tiles=0", True, False),
    "serial": (None, True, True),
}
SWEEP = [(m, f) for m in di.HIFIGAN for f in FORMS] + [(m, f) for m in di.VOCOS for f in ("default", "tiled")]


def _net(mname, form="default"):
    tune, fused, serial = FORMS[form]
    cfg, sd, cd, W32, W64 = di.weights(mname)
    net = SynthesizerTrn(di.N_VOCAB, 513, 32, n_speakers=di.N_SPK, **config.MODEL_CONFIGS[mname])
    if tune is not None:
        os.environ["WETTS_TUNE"] = tune
    try:
        net.load_state_dict(sd).to("cuda")  # (a per-model setting, read at create)
    finally:
        os.environ.pop("WETTS_TUNE", None)
    net.set_decoder_dtype(torch.float32, fused=fused, serial=serial)
    return net, cd, W32, W64


_REFS = {}


def _refs(mname):
    """[(B, L, z, g, {head: float64 oracle audio})] over SHAPES[mname]: computed once, shared by every form."""
    if mname not in _REFS:
        cfg, sd, cd, W32, W64 = di.weights(mname)
        out = []
        for i, (B, L) in enumerate(di.SHAPES[mname]):
            z, g = di.inputs(W32, B, L, 1000 + i)  # the inputs the floor was measured on
            out.append((B, L, z, g, {h: di.oracle(W64, cd, z, g, h) for h in di.heads(mname)}))
        _REFS[mname] = out
    return _REFS[mname]


def _check(tag, mname, got, ref, worst):
    """The three asserts of one decode; the failure names where the largest error sits."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), tag
    rel, loc = di.gates(got, ref)
    err = util.rms((got.double() - ref).numpy())
    worst[0], worst[1], worst[2] = max(worst[0], rel), max(worst[1], loc), max(worst[2], err)
    d = (got.double() - ref).abs()
    at = np.unravel_index(int(d.argmax()), d.shape)
    msg = (tag, f"rel {rel:.3g} (gate {di.REL_GATE[mname]:.3g})", f"local {loc:.3g} (gate {di.LOCAL_GATE[mname]:.3g})",
           f"abs rms {err:.3g}", f"max|d| / rms(d) {float(d.max()) / max(util.rms(d.numpy()), 1e-300):.2f}",
           f"max |d| at row {at[0]} sample {at[-1]} of {got.shape[-1]}")
    assert rel <= di.REL_GATE[mname] and loc <= di.LOCAL_GATE[mname] and err <= di.AUDIO_ABS, msg


def _report(tag, mname, worst):
    print(f"{tag}: worst (rel RMS, max|d|/rms, abs RMS) = ({worst[0]:.3g}, {worst[1]:.3g}, {worst[2]:.3g}); gates "
          f"({di.REL_GATE[mname]:.3g}, {di.LOCAL_GATE[mname]:.3g}, {di.AUDIO_ABS:g}); floor {di.FLOOR[mname]}")


# ---- 2. the sweep ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,form", SWEEP)
def test_decoder_sweep_matches_float64_oracle(mname, form):
    net, cd, W32, W64 = _net(mname, form)
    worst = [0.0, 0.0, 0.0]
    for B, L, z, g, refs in _refs(mname):
        zc, gc = z.cuda(), g[:, :, 0].cuda()
        for head, ref in refs.items():
            if head is not None:
                net.set_is_onnx(head)
            _check((mname, form, B, L, head), mname, net.hifigan(zc, gc), ref, worst)
    _report(f"{mname} {form} sweep ({len(di.SHAPES[mname])} shapes)", mname, worst)


# ---- strides and mask through _decode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,form,B,W,L,lengths", [("tiny", "default", 3, 41, 37, [37, 1, 20]),
                                                      ("tiny", "forced_fused", 3, 41, 37, [37, 1, 20]),
                                                      ("v1", "default", 2, 16, 13, [13, 6]),
                                                      ("v1", "forced_fused", 2, 16, 13, [13, 6])])
def test_decode_reads_strided_and_masked_z_in_place(mname, form, B, W, L, lengths):
    """_decode(z, g, y_mask, L) = dec((z * y_mask)[:, :, :L], g): z wider than L (row stride W), a ragged y_mask, and a
    time-major z (channel stride 1), each against the oracle on the materialised input and, bit for bit, against the
    contiguous call."""
    net, cd, W32, W64 = _net(mname, form)
    z, g = di.inputs(W32, B, W, 4242)
    y_mask = (torch.arange(W)[None, :] < torch.tensor(lengths)[:, None]).float().unsqueeze(1)
    zin = (z * y_mask)[:, :, :L].contiguous()
    ref = di.oracle(W64, cd, zin, g)
    gc = g[:, :, 0].cuda()
    worst = [0.0, 0.0, 0.0]
    plain = net._decode(zin.cuda(), gc, None, L)
    _check((mname, "contiguous"), mname, plain, ref, worst)
    in_place = net._decode(z.cuda(), gc, y_mask.cuda(), L)
    _check((mname, "wide + mask"), mname, in_place, ref, worst)
    assert torch.equal(in_place, plain)
    tm = (z * y_mask).transpose(1, 2).contiguous().cuda().transpose(1, 2)  # [B, 192, W] with strides (192 W, 1, 192)
    assert tm.stride(1) == 1 and tm.stride(2) == 192
    time_major = net._decode(tm, gc, None, L)
    _check((mname, "time-major"), mname, time_major, ref, worst)
    assert torch.equal(time_major, plain)
    _report(f"{mname} {form} strided / masked decode", mname, worst)


# ---- 3. the default dispatch where it picks the big forms by itself -------------------------------------------------
@pytest.mark.parametrize("mname", ["v1", "v3"])
def test_default_dispatch_at_the_size_of_the_big_forms(mname):
    """B = 32, L = 64: >= 128 tiles for the fused kernels (v1: whole chains at C = 32 / 64 k = 3, chain pairs at C = 32
    and for k = 3 at C = 128; v3: ResBlock2 chains), 1024 tiles of 128 x 128 at the C = 128 stage.  The decoder has no
    cross-batch term: one utterance repeated 32 times must give 32 bit-equal rows (every block of every grid against
    its neighbours), and one float64 oracle row pins them all.  Then 32 different utterances, rows 0 and 31."""
    B, L = di.BIG_SHAPE
    net, cd, W32, W64 = _net(mname)
    z, g = di.inputs(W32, B, L, 31337)
    worst = [0.0, 0.0, 0.0]
    zr, gr = z[:1].expand(B, -1, -1).contiguous(), g[:1].expand(B, -1, -1).contiguous()
    same = net.hifigan(zr.cuda(), gr[:, :, 0].cuda()).cpu()
    ref0 = di.oracle(W64, cd, z[:1], g[:1])
    rows = [b for b in range(1, B) if not torch.equal(same[b], same[0])]
    assert not rows, f"rows {rows} differ from row 0 of a repeated utterance"
    _check((mname, "repeated", 0), mname, same[:1], ref0, worst)
    diff = net.hifigan(z.cuda(), g[:, :, 0].cuda()).cpu()
    _check((mname, "distinct", 0), mname, diff[:1], ref0, worst)
    _check((mname, "distinct", B - 1), mname, diff[B - 1:], di.oracle(W64, cd, z[B - 1:], g[B - 1:]), worst)
    _report(f"{mname} default dispatch at {B} x {L}", mname, worst)


# ---- 4. ragged decode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,form,lengths", [
    # hop 15, last stage on 32- and 64-column conv tiles: 63, 64 and 65 frames end 15 samples before, on and 15 after
    # the seam at sample 960
    ("tiny_oddrate", "default", [63, 64, 65, 1]),
    ("tiny_oddrate", "forced_fused", [63, 64, 65, 1]),
    # hop 256: every utterance ends on a conv-tile seam of every stage; forced_fused: the chain kernel with lens at
    # C = 32 / 64 / 128, whose seams (362, 234, 106 ...) no frame count meets: 7 and 8 frames straddle sample 5 x 362
    ("v1", "default", [6, 7, 8, 1]),
    ("v1", "forced_fused", [6, 7, 8, 1]),
])
def test_ragged_decode_rows_match_float64_oracle_alone(mname, form, lengths):
    """_decode(..., y_lengths=): row b under both gates against the oracle of z[b:b+1, :, :len_b] alone, and exactly zero
    behind len_b * hop."""
    net, cd, W32, W64 = _net(mname, form)
    assert net.ragged_supported()
    B, L = len(lengths), max(lengths)
    z, g = di.inputs(W32, B, L, 777)
    out = net._decode(z.cuda(), g[:, :, 0].cuda(), None, L, y_lengths=torch.tensor(lengths, device="cuda")).cpu()
    hop = net.hop_length
    assert out.shape == (B, 1, L * hop)
    worst = [0.0, 0.0, 0.0]
    for b, n in enumerate(lengths):
        assert bool((out[b, :, n * hop:] == 0).all()), (b, n)
        _check((mname, form, "row", b, n), mname, out[b:b + 1, :, :n * hop],
               di.oracle(W64, cd, z[b:b + 1, :, :n], g[b:b + 1]), worst)
    _report(f"{mname} {form} ragged {lengths}", mname, worst)
