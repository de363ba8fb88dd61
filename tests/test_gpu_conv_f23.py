"""The F(2,3) minimal-filtering form of the f32 MRF convs (conv_mfma.hip: conv_f23_body) on the device, against the
float64 oracle and against the direct kernels on the same inputs.

Two models per config (WETTS_TUNE is read at create), both with set_decoder_dtype(f32, fused=False) so that every
ResBlock pair runs as single convs:
    f23     conv_f23_min_tiles=0: the form wherever it is supported (v1: every conv of the C = 256 / 128 / 64 stages)
    direct  the form disabled: the parent's kernels, the yardstick
v1 at (B, L) up to (1, 53): every k / d at C = 256 .. 32, pair tiles of 32 / 64 pairs with seams from L = 37 (stage 2
is 2368 samples); tiny_oddrate: odd stage lengths (hop 15), unpaired last outputs.
Asserts: the form under the config's gates (tests/decoder_input.py); over each config's sweep its worst rel RMS <= the
direct form's and its worst max|d| / rms(ref) <= 1.5 x the direct form's (a maximum over a few thousand samples
fluctuates; the CPU emulation's worst ratio was 0.77); bit identity of serial / three-stream / grouped launches,
repeated calls, batch rows and ragged decodes under the forced knob.
With WETTS_CONV_F23_MARGINS set, both forms' figures go to that file (profiles/conv_f23_margins.txt)."""
import os

import pytest
import torch

from tests import decoder_input as di
from wetts_amd import SynthesizerTrn

pytestmark = pytest.mark.gpu

OFF = 2 ** 31 - 1
TUNE = {
    "f23": "conv_f23_min_tiles=0,small_max_tiles=0",
    "direct": f"conv_f23_min_tiles={OFF},small_max_tiles=0",
    # no fused ResBlock kernels although fused=True: the serial schedule then sends the single convs out in groups
    "f23_grouped": "conv_f23_min_tiles=0,small_max_tiles=0,fuse_min_blocks=1000000000,chain_whole_pct=0",
}
SHAPES = {
    "v1": ((1, 1), (2, 2), (3, 3), (1, 5), (2, 13), (1, 37), (1, 53)),
    "tiny_oddrate": tuple((1 + i % 3, L) for i, L in enumerate((1, 2, 3, 5, 7, 13, 63, 64, 65))),
}
RAGGED = {"tiny_oddrate": [63, 64, 65, 1], "v1": [6, 7, 8, 1]}
CASES = [(m, i) for m in SHAPES for i in range(len(SHAPES[m]))]

_NETS, _W, _FIG = {}, {}, {}


def _weights(mname):
    if mname not in _W:
        _W[mname] = di.weights(mname)
    return _W[mname]


def _net(mname, form, fused=False, serial=False):
    key = (mname, form)
    if key not in _NETS:
        cfg, sd, cd, W32, W64 = _weights(mname)
        net = SynthesizerTrn(di.N_VOCAB, 513, 32, n_speakers=di.N_SPK, **di.model_dict(mname))
        os.environ["WETTS_TUNE"] = TUNE[form]
        try:
            net.load_state_dict(sd).to("cuda")
        finally:
            os.environ.pop("WETTS_TUNE", None)
        _NETS[key] = net
    _NETS[key].set_decoder_dtype(torch.float32, fused=fused, serial=serial)
    return _NETS[key]


def _figures(mname, i):
    """{form: (rel RMS, max|d| / rms(ref), abs RMS)} of shape i against the float64 oracle, and the F(2,3) audio."""
    if (mname, i) not in _FIG:
        cfg, sd, cd, W32, W64 = _weights(mname)
        B, L = SHAPES[mname][i]
        z, g = di.inputs(W32, B, L, 5000 + i)
        ref = di.oracle(W64, cd, z, g)
        out = {}
        for form in ("f23", "direct"):
            got = _net(mname, form).hifigan(z.cuda(), g[:, :, 0].cuda()).cpu()
            assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (mname, form, B, L)
            rel, loc = di.gates(got, ref)
            out[form] = (rel, loc, float((got.double() - ref).pow(2).mean().sqrt()))
        _FIG[mname, i] = out
    return _FIG[mname, i]


@pytest.fixture(scope="module", autouse=True)
def _write_margins():
    yield
    path = os.environ.get("WETTS_CONV_F23_MARGINS")
    if path and _FIG:
        with open(path, "w") as f:
            f.write("f32 decoder, every ResBlock pair as single convs (fused=False, small_max_tiles=0), against the float64 oracle:\n"
                    "F(2,3) form (conv_f23_min_tiles=0) and direct form (disabled) on the same inputs (tests/test_gpu_conv_f23.py)\n"
                    "config B L: F23 rel RMS, max|d|/rms(ref), abs RMS | direct rel RMS, max|d|/rms(ref), abs RMS   [gates rel, local]\n")
            for (m, i) in sorted(_FIG):
                a, b = _FIG[m, i]["f23"], _FIG[m, i]["direct"]
                f.write(f"{m} {SHAPES[m][i][0]} {SHAPES[m][i][1]}: {a[0]:.3e}, {a[1]:.3e}, {a[2]:.3e} | {b[0]:.3e}, {b[1]:.3e}, "
                        f"{b[2]:.3e}   [{di.REL_GATE[m]:.3g}, {di.LOCAL_GATE[m]:.3g}]\n")
            for m in SHAPES:
                rows = [_FIG[m, i] for i in range(len(SHAPES[m])) if (m, i) in _FIG]
                if rows:
                    f.write(f"{m} worst over {len(rows)} shapes: F23 rel {max(r['f23'][0] for r in rows):.3e} local "
                            f"{max(r['f23'][1] for r in rows):.3e} | direct rel {max(r['direct'][0] for r in rows):.3e} local "
                            f"{max(r['direct'][1] for r in rows):.3e}\n")


@pytest.mark.parametrize("mname,i", CASES)
def test_f23_form_is_within_the_gates(mname, i):
    fig = _figures(mname, i)
    rel, loc, err = fig["f23"]
    print(f"{mname} {SHAPES[mname][i]}: F23 rel {rel:.3e} local {loc:.3e} abs {err:.3e} | direct rel {fig['direct'][0]:.3e} "
          f"local {fig['direct'][1]:.3e} abs {fig['direct'][2]:.3e}")
    assert rel <= di.REL_GATE[mname] and loc <= di.LOCAL_GATE[mname] and err <= di.AUDIO_ABS, (mname, SHAPES[mname][i], fig)


@pytest.mark.parametrize("mname", list(SHAPES))
def test_f23_form_is_no_worse_than_the_direct_form_over_the_sweep(mname):
    rows = [_figures(mname, i) for i in range(len(SHAPES[mname]))]
    rel_f, rel_d = max(r["f23"][0] for r in rows), max(r["direct"][0] for r in rows)
    loc_f, loc_d = max(r["f23"][1] for r in rows), max(r["direct"][1] for r in rows)
    print(f"{mname}: worst rel RMS F23 {rel_f:.3e} direct {rel_d:.3e}; worst max|d|/rms F23 {loc_f:.3e} direct {loc_d:.3e}")
    assert rel_f <= rel_d, (mname, rel_f, rel_d)
    assert loc_f <= 1.5 * loc_d, (mname, loc_f, loc_d)


@pytest.mark.parametrize("mname,B,L", [("v1", 3, 13), ("v1", 1, 53), ("tiny_oddrate", 3, 65)])
def test_f23_launch_forms_repeats_and_batch_rows_are_bit_identical(mname, B, L):
    cfg, sd, cd, W32, W64 = _weights(mname)
    z, g = di.inputs(W32, B, L, 6000 + L)
    zc, gc = z.cuda(), g[:, :, 0].cuda()
    forked = _net(mname, "f23", serial=False).hifigan(zc, gc).cpu()
    again = _net(mname, "f23", serial=False).hifigan(zc, gc).cpu()
    serial = _net(mname, "f23", serial=True).hifigan(zc, gc).cpu()
    grouped = _net(mname, "f23_grouped", fused=True, serial=True).hifigan(zc, gc).cpu()
    assert torch.equal(forked, again), "a second call differs"
    assert torch.equal(forked, serial), "serial and three-stream decodes differ"
    assert torch.equal(forked, grouped), "grouped and single launches differ"
    net = _net(mname, "f23")
    for b in range(B):
        alone = net.hifigan(zc[b:b + 1].contiguous(), gc[b:b + 1].contiguous()).cpu()
        assert torch.equal(alone[0], forked[b]), f"row {b} of the batch differs from the row decoded alone"
    # and the form is really taken where v1 supports it: the bits differ from the direct kernels'
    if mname == "v1":
        assert not torch.equal(forked, _net(mname, "direct").hifigan(zc, gc).cpu())


def _ragged(mname):
    lengths = RAGGED[mname]
    cfg, sd, cd, W32, W64 = _weights(mname)
    net = _net(mname, "f23")
    assert net.ragged_supported()
    B, L = len(lengths), max(lengths)
    z, g = di.inputs(W32, B, L, 777)
    zc, gc = z.cuda(), g[:, :, 0].cuda()
    out = net._decode(zc, gc, None, L, y_lengths=torch.tensor(lengths, device="cuda")).cpu()
    assert out.shape == (B, 1, L * net.hop_length)
    return net, lengths, zc, gc, out


@pytest.mark.parametrize("mname", list(RAGGED))
def test_f23_ragged_decode_equals_each_row_alone(mname):
    """Ragged rows against a plain decode of each row alone, bit for bit, and zero behind each end.  (This also holds
    conv_post to it: k_conv_post_tanh sends small ragged launches to conv_post_tanh_small_kernel like small dense ones;
    with the ragged launches on conv_post_tanh_kernel's channel-major sum 85 % of the samples differed by an ulp.)"""
    net, lengths, zc, gc, out = _ragged(mname)
    hop, bad = net.hop_length, []
    for b, n in enumerate(lengths):
        assert bool((out[b, :, n * hop:] == 0).all()), (b, n)
        alone = net.hifigan(zc[b:b + 1, :, :n].contiguous(), gc[b:b + 1].contiguous()).cpu()
        ne = int((out[b, :, :n * hop] != alone[0]).sum())
        print(f"{mname} ragged row {b} ({n} frames): {ne} of {n * hop} samples differ from the row alone, max |d| "
              f"{float((out[b, :, :n * hop] - alone[0]).abs().max()):.3g}")
        if ne:
            bad.append((b, n, ne))
    assert not bad, f"ragged rows differ from the rows decoded alone: (row, frames, samples) {bad}"


def test_f23_ragged_rows_equal_the_row_alone_through_the_ragged_entry():
    """v1 (every conv of the C = 256 / 128 / 64 stages in F(2,3) form): row b of a ragged batch equals the same row as a
    ragged batch of one, bit for bit -- the pairing and the ends do not depend on the other rows."""
    net, lengths, zc, gc, out = _ragged("v1")
    hop = net.hop_length
    for b, n in enumerate(lengths):
        one = net._decode(zc[b:b + 1, :, :n].contiguous(), gc[b:b + 1].contiguous(), None, n,
                          y_lengths=torch.tensor([n], device="cuda")).cpu()
        assert torch.equal(out[b, :, :n * hop], one[0]), f"ragged row {b} ({n} frames) depends on the batch"
