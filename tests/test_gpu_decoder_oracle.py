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
test_default_dispatch_at_the_size_of_the_big_forms reaches them with one utterance repeated 32 times.

The Vocos seam sweep (section 5; run_vocos in csrc/model.hip).  SHAPES stops at L = 50 (row stride Fs <= 52): one tile
of the fused depthwise conv + LayerNorm, one 32-column unit per block of the pointwise GEMM, n_fft / hop = 4 only.  A
second family of shapes, with floors and gates of its own (tests/decoder_input.py: SEAM_SHAPES, WIDE_SHAPES, SEAM_FLOOR;
4 x floor, 6 x for vits2_vocos_v1 as above), holds the head to the float64 oracle where those kernels have edges.
F = L + 1 frames, Fs = (F + 3) & ~3, junk = Fs - F columns ride along behind every row:
  convnext_dwln_kernel, tiles of 62 columns of Fs (lanes 0 / 63 are the halo), seams 61 | 62, 123 | 124, 185 | 186:
    F = 60  one tile, no junk                      F = 61  Fs 64: the second tile is columns 62, 63, junk only (3 junk)
    F = 62  F on the seam, second tile junk only   F = 63  second tile = ONE valid column + one junk column
    F = 64  two valid columns, no junk             F = 65, 66  Fs 68: 3 and 2 junk columns in a second tile of 6
    F = 122 .. 126  the same at the second seam (124 = 2 x 62 ends on it; 125: one valid column + 3 junk in tile 3)
    F = 187  a fourth tile of one valid column and one junk column
    <4>: tiny_vocos, vocos_n78; <16> (and layernorm_reg_kernel<16>): vocos_c256; <32>: vits2_vocos_v1 at F = 61 .. 64 and
    124, and over 3, 4, 8 and 11 tiles in the wide cases; the k_dwconv + k_layernorm fallback: vocos_c96, vocos_c80
  convs (forms default: conv_small_kernel for every conv; tiled: pw_gemm_kernel, one unit per block, last units of 4 .. 32
    columns): reductions of 5 (vocos_c80 pw1 / out, vocos_n78 iSTFT), 11 (vocos_c96 pw2) and 17 chunks (vocos_c256 pw2);
    vocos_c80's residual conv (M = 80) is refused by pw_gemm_eligible and runs on conv_mfma_kernel with `res`;
    k_rows_padded pads 66 -> 80 and 1026 -> 1040 rows, and nothing for vocos_n78 (80 rows)
  iSTFT (istft_ola_kernel, envelope, OnnxSTFT basis scale): n_fft / hop = 2 (vocos_c256), 3 (vocos_n78: 78 / 26), 4, 8
    (vocos_c96) and hop 24 against n_fft 64 (vocos_c80), both heads each
  pw_gemm_kernel passes (vits2_vocos_v1, default dispatch, B = 32; pw_schedule at 256 CUs, recomputed with the device's
    count -- the tests fail, naming it, if the patterns differ there):
    L = 128  pw1 upb 3 = passes (2, 1) | (2), last unit of 4 columns      L = 192  pw1 upb 4 = (4) | (2, 1); in, pw2, iSTFT (2)
    L = 479  Fs 480, full last unit: pw1 upb 8 = (4, 4) | (4, 2, 1); in, out, iSTFT upb 4 = (4) .. (2, 1); pw2 upb 2
    L = 671  Fs 672: pw1 upb 11 = (4, 4, 2, 1) | (4, 4, 2); pw2 (residual init) and in / out upb 4; iSTFT upb 7 = (4, 2, 1)
tests/test_cpu_decoder_gate.py asserts this coverage from the restated geometry and that SHAPES reaches none of it.
With WETTS_VOCOS_SEAM_MARGINS set the worst multiple of each gate per (config, form) goes to that file
(profiles/vocos_seam_margins.txt).  Not covered: pw_gemm_kernel's <32, 4> / <32, 2> stage shapes (micro-benchmark
variants only, no product dispatch); nothing else of the head is left out: a ragged (y_lengths) decode is a HiFi-GAN
form (ragged_supported()), and win_length != n_fft is refused at create."""
import os

import numpy as np
import pytest
import torch

from tests import decoder_input as di
from tests import util
from wetts_amd import SynthesizerTrn

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
    net = SynthesizerTrn(di.N_VOCAB, 513, 32, n_speakers=di.N_SPK, **di.model_dict(mname))
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


def _check(tag, mname, got, ref, worst, gate=None):
    """The three asserts of one decode; the failure names where the largest error sits.  `gate`: (rel, local) where
    they are not REL_GATE / LOCAL_GATE of the config (the Vocos seam sweep has gates of its own)."""
    rel_gate, loc_gate = gate or (di.REL_GATE[mname], di.LOCAL_GATE[mname])
    got = got.detach().cpu()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), tag
    rel, loc = di.gates(got, ref)
    err = util.rms((got.double() - ref).numpy())
    worst[0], worst[1], worst[2] = max(worst[0], rel), max(worst[1], loc), max(worst[2], err)
    d = (got.double() - ref).abs()
    at = np.unravel_index(int(d.argmax()), d.shape)
    msg = (tag, f"rel {rel:.3g} (gate {rel_gate:.3g})", f"local {loc:.3g} (gate {loc_gate:.3g})",
           f"abs rms {err:.3g}", f"max|d| / rms(d) {float(d.max()) / max(util.rms(d.numpy()), 1e-300):.2f}",
           f"max |d| at row {at[0]} sample {at[-1]} of {got.shape[-1]}")
    assert rel <= rel_gate and loc <= loc_gate and err <= di.AUDIO_ABS, msg


def _report(tag, mname, worst, gate=None, floor=None):
    rel_gate, loc_gate = gate or (di.REL_GATE[mname], di.LOCAL_GATE[mname])
    print(f"{tag}: worst (rel RMS, max|d|/rms, abs RMS) = ({worst[0]:.3g}, {worst[1]:.3g}, {worst[2]:.3g}); gates "
          f"({rel_gate:.3g}, {loc_gate:.3g}, {di.AUDIO_ABS:g}); floor {floor or di.FLOOR[mname]}")


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


# ======================================================================================================================
# 5. The Vocos head across tile seams, GEMM passes and hops (see the module docstring: "The Vocos seam sweep")
# ======================================================================================================================
_MARGINS = {}  # (config, form) -> worst [rel / gate, local / gate, abs RMS / 1e-4] over the Vocos seam tests


def _seam_gate(mname):
    return di.SEAM_REL_GATE[mname], di.SEAM_LOCAL_GATE[mname]


def _margin(mname, form, worst):
    g = _seam_gate(mname)
    m = _MARGINS.setdefault((mname, form), [0.0, 0.0, 0.0])
    for i, v in enumerate((worst[0] / g[0], worst[1] / g[1], worst[2] / di.AUDIO_ABS)):
        m[i] = max(m[i], v)


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    out = os.environ.get("WETTS_VOCOS_SEAM_MARGINS")  # the GPU run that records profiles/vocos_seam_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst multiple of each gate per (config, form) over the Vocos seam tests of "
                    "tests/test_gpu_decoder_oracle.py (1 = at the gate)\n"
                    "gates: rel RMS and max|d| / rms(ref) = SEAM_FACTOR x SEAM_FLOOR (tests/decoder_input.py), abs RMS 1e-4\n"
                    "config form: rel / gate, local / gate, abs RMS / 1e-4   [factor, gates]\n")
            for (m, form) in sorted(_MARGINS):
                v, g = _MARGINS[m, form], _seam_gate(m)
                f.write(f"{m} {form}: {v[0]:.3f}, {v[1]:.3f}, {v[2]:.4f}   [{di.SEAM_FACTOR[m]:g} x floor, "
                        f"{g[0]:.3g}, {g[1]:.3g}]\n")


_SEAM_REFS = {}


def _seam_refs(mname):
    """[(B, L, z, g, {head: float64 oracle audio})] over SEAM_SHAPES[mname]: computed once, shared by both forms."""
    if mname not in _SEAM_REFS:
        cfg, sd, cd, W32, W64 = di.weights(mname)
        out = []
        for i, (B, L) in enumerate(di.SEAM_SHAPES[mname]):
            z, g = di.inputs(W32, B, L, di.SEAM_SEED + i)  # the inputs the seam floor was measured on
            out.append((B, L, z, g, {h: di.oracle(W64, cd, z, g, h) for h in di.heads(mname)}))
        _SEAM_REFS[mname] = out
    return _SEAM_REFS[mname]


@pytest.mark.parametrize("mname,form", [(m, f) for m in di.SEAM_CONFIGS for f in ("default", "tiled")])
def test_vocos_seam_sweep_matches_float64_oracle(mname, form):
    """Every (B, L) of SEAM_SHAPES[config] under both iSTFT heads against the float64 oracle, under the seam gates."""
    net, cd, W32, W64 = _net(mname, form)
    worst = [0.0, 0.0, 0.0]
    for B, L, z, g, refs in _seam_refs(mname):
        zc, gc = z.cuda(), g[:, :, 0].cuda()
        for head, ref in refs.items():
            net.set_is_onnx(head)
            _check((mname, form, B, L, "F", L + 1, "onnx head" if head else "torch.istft head"), mname,
                   net.hifigan(zc, gc), ref, worst, _seam_gate(mname))
    _margin(mname, form, worst)
    _report(f"{mname} {form} seam sweep ({len(di.SEAM_SHAPES[mname])} shapes)", mname, worst, _seam_gate(mname),
            di.SEAM_FLOOR[mname])


def _device_claims():
    """The coverage claims of the wide cases recomputed with the CU count of THIS device (pw_schedule reads it)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pat, missing = di.wide_claims(cus)
    assert not missing, (f"with the {cus} compute units of this device pw_schedule gives the wide cases "
                         f"{di.WIDE_SHAPES} other pass patterns than with 256; not reached: {missing}", pat)
    return cus


def test_wide_cases_reach_the_pass_patterns_on_this_device():
    cus = _device_claims()
    for B, L in di.WIDE_SHAPES:
        print(cus, (B, L), [(r["conv"], r["S"], r["upb"], sorted(set(r["passes"])), r["last_unit"])
                            for r in di.vocos_launches(di.WIDE_CONFIG, B, L, "default", cus)])


@pytest.mark.parametrize("case", range(len(di.WIDE_SHAPES)))
def test_vocos_default_dispatch_at_the_sizes_of_the_wide_gemm_passes(case):
    """vits2_vocos_v1, B = 32 at the default dispatch: every conv of the head on pw_gemm_kernel with blocks of several
    passes (the patterns per (B, L): tests/decoder_input.py:WIDE_SHAPES).  One utterance repeated B times must give B
    bit-equal rows (every block of every strip against its neighbours), and one float64 oracle row pins them all; then
    B distinct utterances, rows 0 and B - 1 against the oracle of those rows alone."""
    _device_claims()
    mname, (B, L) = di.WIDE_CONFIG, di.WIDE_SHAPES[case]
    net, cd, W32, W64 = _net(mname)
    z, g = di.inputs(W32, B, L, di.WIDE_SEED + case)
    gate, worst = _seam_gate(mname), [0.0, 0.0, 0.0]
    zr, gr = z[:1].expand(B, -1, -1).contiguous(), g[:1].expand(B, -1, -1).contiguous()
    same = net.hifigan(zr.cuda(), gr[:, :, 0].cuda()).cpu()
    diff = net.hifigan(z.cuda(), g[:, :, 0].cuda()).cpu()
    rows = [b for b in range(1, B) if not torch.equal(same[b], same[0])]
    assert not rows, f"rows {rows} differ from row 0 of a repeated utterance"
    ref0 = di.oracle(W64, cd, z[:1], g[:1])
    _check((mname, B, L, "repeated", 0), mname, same[:1], ref0, worst, gate)
    _check((mname, B, L, "distinct", 0), mname, diff[:1], ref0, worst, gate)
    _check((mname, B, L, "distinct", B - 1), mname, diff[B - 1:], di.oracle(W64, cd, z[B - 1:], g[B - 1:]), worst, gate)
    _margin(mname, "default wide", worst)
    _report(f"{mname} default dispatch at {B} x {L}", mname, worst, gate, di.SEAM_FLOOR[mname])


@pytest.mark.parametrize("form", ["default", "tiled"])
def test_vocos_decode_reads_strided_and_masked_z_in_place_at_a_seam(form):
    """tiny_vocos, L = 62 (F = 63: the second tile of the fused depthwise conv + LayerNorm holds one valid column and
    one junk column) through _decode: z wider than L (row stride 70), a ragged y_mask, and a time-major z, each against
    the oracle on the materialised input and, bit for bit, against the contiguous call."""
    mname, B, W, L, lengths = "tiny_vocos", 3, 70, 62, [62, 2, 31]
    net, cd, W32, W64 = _net(mname, form)
    z, g = di.inputs(W32, B, W, 4243)
    y_mask = (torch.arange(W)[None, :] < torch.tensor(lengths)[:, None]).float().unsqueeze(1)
    zin = (z * y_mask)[:, :, :L].contiguous()
    ref = di.oracle(W64, cd, zin, g)
    gc = g[:, :, 0].cuda()
    gate, worst = _seam_gate(mname), [0.0, 0.0, 0.0]
    plain = net._decode(zin.cuda(), gc, None, L)
    _check((mname, form, "contiguous"), mname, plain, ref, worst, gate)
    in_place = net._decode(z.cuda(), gc, y_mask.cuda(), L)
    _check((mname, form, "wide + mask"), mname, in_place, ref, worst, gate)
    assert torch.equal(in_place, plain)
    tm = (z * y_mask).transpose(1, 2).contiguous().cuda().transpose(1, 2)  # [B, 192, W] with strides (192 W, 1, 192)
    assert tm.stride(1) == 1 and tm.stride(2) == 192
    time_major = net._decode(tm, gc, None, L)
    _check((mname, form, "time-major"), mname, time_major, ref, worst, gate)
    assert torch.equal(time_major, plain)
    _margin(mname, form + " strided", worst)
    _report(f"{mname} {form} strided / masked decode at a seam", mname, worst, gate, di.SEAM_FLOOR[mname])
