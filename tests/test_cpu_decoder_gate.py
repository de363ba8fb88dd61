"""CPU tier: the two gates that tests/test_gpu_decoder_oracle.py holds the f32 decoder to (tests/decoder_input.py:
REL_GATE, LOCAL_GATE = 4 x the worst error of the float32 oracle against the float64 oracle over the GPU sweep's shapes)
are calibrated and proven here, without a GPU.

* The committed floors cannot drift silently: the floor of two cheap configs is recomputed and the committed gates
  must lie within 2 .. 8 x it.
* The local gate sees the defects it exists for.  Three defective float64 oracles (vits_oracle.conv1d wrapped by name)
  -- (a) the last output column of the last conv of the last stage computed without its right-most in-range tap, (b)
  one interior input column (position 118) of a mid-stage convs1 read as zero: a lost halo column, (c) one output
  channel of the conv that feeds conv_post without its bias over 32 columns -- must each move `local` to >= 10 x
  LOCAL_GATE[config], while the whole-tensor abs RMS that gated the decoder before stays under its 1e-4 (printed).
* The lengths of the GPU sweep put a last tile narrower than its halo, and one that ends exactly on a seam, in front of
  every fused f32 ResBlock kernel (the tile geometry restated in tests/decoder_input.py)."""
import pytest
import torch

from tests import decoder_input as di
from tests import util


# ---- the floor ---------------------------------------------------------------------------------------------------
def test_every_swept_config_has_a_committed_floor_and_gate():
    assert set(di.FLOOR) == set(di.CONFIGS) == set(di.SHAPES)
    for m in di.CONFIGS:
        assert 2.0 <= di.FACTOR[m] <= 8.0 and (di.FACTOR[m] == di.GATE_FACTOR or m == "vits2_vocos_v1")
        assert di.REL_GATE[m] == di.FACTOR[m] * di.FLOOR[m][0] and di.LOCAL_GATE[m] == di.FACTOR[m] * di.FLOOR[m][1]
        # a gate that the old whole-tensor abs RMS gate (1e-4 at an audio RMS of 0.12 .. 0.36) would not have implied
        assert di.REL_GATE[m] < 1e-5 and di.LOCAL_GATE[m] < 1e-4, m


@pytest.mark.parametrize("mname", ["tiny", "v2"])
def test_committed_gates_are_2_to_8_times_the_recomputed_floor(mname):
    """float32 oracle against float64 oracle on the sweep's own inputs (same seeds), every (B, L) of SHAPES[mname]."""
    rel, loc = di.floor(mname)
    print(f"{mname}: recomputed floor rel {rel:.3g} local {loc:.3g}; committed floor {di.FLOOR[mname]}, gates "
          f"rel {di.REL_GATE[mname]:.3g} ({di.REL_GATE[mname] / rel:.2f} x) local {di.LOCAL_GATE[mname]:.3g} "
          f"({di.LOCAL_GATE[mname] / loc:.2f} x)")
    assert 2.0 * rel <= di.REL_GATE[mname] <= 8.0 * rel
    assert 2.0 * loc <= di.LOCAL_GATE[mname] <= 8.0 * loc


# ---- sensitivity -------------------------------------------------------------------------------------------------
# (B, L) of the sensitivity runs: 4 L (tiny, tiny_dp) / 5 L (tiny_oddrate) / 64 L (the others) samples at the middle
# stage, so that column 118 exists and is interior
SENS_SHAPE = {"tiny": (2, 50), "tiny_dp": (2, 50), "tiny_oddrate": (2, 50), "v2": (2, 13), "v1": (2, 13), "v3": (2, 13),
              "stress48k": (2, 5)}
HALO_COLUMN, BIAS_ROW, BIAS_SPAN = 118, 5, (64, 96)


def _conv_names(cd):
    """(the last conv of the last stage -- the last conv in front of conv_post --, a convs1 of the middle stage)."""
    nk, ns = len(cd["resblock_kernel_sizes"]), len(cd["upsample_rates"])
    rb1 = str(cd["resblock"]) == "1"
    last = f"dec.resblocks.{ns * nk - 1}." + ("convs2.2" if rb1 else "convs.1")
    mid_stage = (ns - 1) // 2  # v1: the C = 128 stage; tiny: its C = 32 stage
    mid = f"dec.resblocks.{mid_stage * nk + 1}." + ("convs1.1" if rb1 else "convs.1")
    return last, mid


def _defective_conv1d(real, defect, cd):
    last, mid = _conv_names(cd)
    hit = []

    def conv1d(W, name, x, dilation=1, padding=0, groups=1):
        if defect == "halo" and name == mid:
            assert x.shape[-1] > HALO_COLUMN + 32, "column 118 must be interior"
            x = x.clone()
            x[:, :, HALO_COLUMN] = 0.0  # one staged column never arrived
            hit.append(name)
        y = real(W, name, x, dilation=dilation, padding=padding, groups=groups)
        if name == last and defect == "tap":
            # the last output column reads taps at T - 1 + (j - hk) * dilation: the centre tap j = hk is the right-most
            # one inside the sequence
            w = W[name + ".weight"]
            y = y.clone()
            y[:, :, -1] -= torch.einsum("oc,bc->bo", w[:, :, w.shape[-1] // 2], x[:, :, -1])
            hit.append(name)
        if name == last and defect == "bias":
            y = y.clone()
            y[:, BIAS_ROW, BIAS_SPAN[0]:BIAS_SPAN[1]] -= W[name + ".bias"][BIAS_ROW]
            hit.append(name)
        return y
    return conv1d, hit


_CLEAN = {}


def _clean(mname):
    """The float64 oracle of the sensitivity shape, once per config."""
    if mname not in _CLEAN:
        cfg, sd, cd, W32, W64 = di.weights(mname)
        z, g = di.inputs(W32, *SENS_SHAPE[mname], seed=77)
        _CLEAN[mname] = (cd, W64, z, g, di.oracle(W64, cd, z, g))
    return _CLEAN[mname]


@pytest.mark.parametrize("defect", ["tap", "halo", "bias"])
@pytest.mark.parametrize("mname", di.HIFIGAN)
def test_local_gate_sees_the_defect(mname, defect, monkeypatch):
    cd, W64, z, g, ref = _clean(mname)
    fake, hit = _defective_conv1d(di.vo().conv1d, defect, cd)
    monkeypatch.setattr(di.vo(), "conv1d", fake)
    bad = di.oracle(W64, cd, z, g)
    monkeypatch.undo()
    assert len(hit) == 1, hit
    rel, loc = di.gates(bad, ref)
    abs_rms = util.rms((bad - ref).numpy())
    print(f"{mname} {SENS_SHAPE[mname]} defect {defect} in {hit[0]}: local {loc:.3g} = {loc / di.LOCAL_GATE[mname]:.0f} x "
          f"LOCAL_GATE ({di.LOCAL_GATE[mname]:.3g}); rel {rel:.3g} = {rel / di.REL_GATE[mname]:.1f} x REL_GATE; abs RMS "
          f"{abs_rms:.3g} = {di.AUDIO_ABS / max(abs_rms, 1e-300):.1f} x under the 1e-4 gate")
    assert loc >= 10.0 * di.LOCAL_GATE[mname]


# ---- the sweep's lengths against the tile geometry ---------------------------------------------------------------------
def test_sweep_lengths_reach_narrow_and_seam_exact_last_tiles_of_every_fused_kernel():
    """Per fused kernel, over the configs and forms of the GPU sweep: at least one decode leaves a last tile narrower
    than the tile's halo (columns it computes and discards), at least one ends exactly on a seam (T a multiple of the
    tile's output width), and at least one spans several tiles."""
    seen = {}
    for mname in di.HIFIGAN:
        for form in ("forced", "pairs"):
            for (kernel, C, k, dil), e in di.last_tiles(mname, di.SHAPES[mname], form).items():
                s = seen.setdefault("chain" if kernel.startswith("chain") else kernel, dict(narrow=0, seam=0, multi=0))
                s["narrow"] += any(0 < r < e["halo"] for r in e["rems"])
                s["seam"] += 0 in e["rems"]
                s["multi"] += e["multi"]
    print(seen)
    assert set(seen) == {"chain", "pair32", "rb2_chain"}
    for kernel, s in seen.items():
        assert s["narrow"] and s["seam"] and s["multi"], (kernel, s)
    # the default dispatch reaches the fused forms by itself only at the repeated-utterance size
    big = {k[0] for m in ("v1", "v3") for k in di.last_tiles(m, [di.BIG_SHAPE], "default")}
    assert big == {"chain_whole", "chain_pair", "rb2_chain"}
    assert not any(di.fused_launches(m, B, L, "default") for m in di.HIFIGAN for B, L in di.SHAPES[m])
