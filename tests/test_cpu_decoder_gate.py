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
  every fused f32 ResBlock kernel (the tile geometry restated in tests/decoder_input.py).

The Vocos seam sweep (second half of this file; SEAM_* / WIDE_SHAPES of tests/decoder_input.py) gets the same three:
* its floors are recomputed for the five cheap configs (which also shows that torch.istft accepts every hop ratio of
  the coverage configs) and the committed gates held to 2 .. 8 x them;
* six defects in the float64 oracle (vits_oracle's `F`, `conv1d` and `torch` names wrapped) at (B, L) = (2, 70), each
  >= 10 x SEAM_LOCAL_GATE[config]: column 62 of the last layer's depthwise conv without its left tap (lane 0 of the
  second tile), for all channels and for the PER channels of one wave; the right tap of the last valid column reading
  a value where the zero padding starts (junk from behind F); the last valid column of the last pw_conv2 without its
  last 16-channel chunk; the last frame left out of the overlap-add over the final hop samples; column 0 of the
  reflection pad from z[..., 0].  Measured 860 x (vits2_vocos_v1, the chunk: rel RMS 6.6e-4 and abs RMS 1.4e-5, both
  under the old whole-tensor gates 2e-3 / 1e-4; its one-wave tap defect is under both too) to 470000 x;
* coverage from the restated geometry at 256 CUs: per instantiation of convnext_dwln_kernel and for the fallback a last
  tile of one valid column, one of junk only, F on a seam, several tiles and all four junk widths; which kernel every
  conv takes per config and form; and for the wide cases pass widths 1 / 2 / 4, mixed blocks, upb >= 8, split strips,
  partial and full last units on pw_gemm_kernel -- none of which the old sweep reaches (asserted)."""
import pytest
import torch

from tests import decoder_input as di
from tests import util
from wetts_amd import config


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


# ======================================================================================================================
# The Vocos seam sweep (tests/decoder_input.py: SEAM_SHAPES, WIDE_SHAPES, SEAM_FLOOR, SEAM_*_GATE)
# ======================================================================================================================
def test_every_seam_config_has_a_committed_floor_and_gate_of_its_own():
    assert set(di.SEAM_FLOOR) == set(di.SEAM_CONFIGS) == set(di.SEAM_SHAPES)
    assert not set(di.COVERAGE) & set(config.MODEL_CONFIGS)  # the coverage configs stay out of the table others enumerate
    for m in di.SEAM_CONFIGS:
        assert di.SEAM_FACTOR[m] == (6.0 if m == "vits2_vocos_v1" else di.GATE_FACTOR)
        assert di.SEAM_REL_GATE[m] == di.SEAM_FACTOR[m] * di.SEAM_FLOOR[m][0]
        assert di.SEAM_LOCAL_GATE[m] == di.SEAM_FACTOR[m] * di.SEAM_FLOOR[m][1]
        assert 0 < di.SEAM_REL_GATE[m] < 1e-5 and 0 < di.SEAM_LOCAL_GATE[m] < 1e-4, m
        di.model_cfg(m)  # make_config takes it
        for B, L in di.SEAM_SHAPES[m]:
            assert L >= 2 and 1 <= B <= (3 if m == "vits2_vocos_v1" else 5)


@pytest.mark.parametrize("mname", [m for m in di.SEAM_CONFIGS if m != "vits2_vocos_v1"])
def test_committed_seam_gates_are_2_to_8_times_the_recomputed_floor(mname):
    """float32 oracle against float64 oracle on the seam sweep's own inputs, every (B, L) of SEAM_SHAPES[mname], both
    heads.  torch.istft runs for every config here: it asserts that the window envelope stays above 1e-11, so the hop
    ratios 2, 8, 64 / 24 and 78 / 26 are ones the reference accepts."""
    rel, loc = di.seam_floor(mname)
    print(f"{mname}: recomputed seam floor rel {rel:.3g} local {loc:.3g}; committed floor {di.SEAM_FLOOR[mname]}, gates "
          f"rel {di.SEAM_REL_GATE[mname]:.3g} ({di.SEAM_REL_GATE[mname] / rel:.2f} x) local "
          f"{di.SEAM_LOCAL_GATE[mname]:.3g} ({di.SEAM_LOCAL_GATE[mname] / loc:.2f} x)")
    assert 2.0 * rel <= di.SEAM_REL_GATE[mname] <= 8.0 * rel
    assert 2.0 * loc <= di.SEAM_LOCAL_GATE[mname] <= 8.0 * loc


# ---- sensitivity of the seam gates -------------------------------------------------------------------------------------
VOCOS_SENS_SHAPE = (2, 70)  # F = 71 frames: column 62 (the first column of the fused kernel's second tile) is interior
SEAM_COLUMN, WAVE = 62, 3  # the single-wave defect: channels WAVE * PER .. of convnext_dwln_kernel<PER>
VOCOS_DEFECTS = ("dw_left_tap", "dw_left_tap_one_wave", "dw_right_tap_reads_junk", "pw2_last_chunk", "ola_last_frame",
                 "reflect_pad")
OLD_REL = 2e-3  # the whole-tensor rel RMS gate of test_vocos_b16x128_oracle_spot_check_and_stream (with abs RMS 1e-4)


class _Patched:
    """A module seen through a few replaced attributes (the oracle's `F` / `torch` names, wrapped by name)."""

    def __init__(self, real, **over):
        self._real = real
        self.__dict__.update(over)

    def __getattr__(self, k):
        return getattr(self._real, k)


def _defective_vocos(monkeypatch, defect, cd, n_layers, per):
    """Patches oracle/vits_oracle.py so that vocos() computes with one defect; returns the list the hits are logged to.
      dw_left_tap              column 62 of the last layer's depthwise conv without its left tap (a tile's halo lane 0
                               that never arrived), all channels
      dw_left_tap_one_wave     the same for the PER consecutive channels one wave of convnext_dwln_kernel<PER> owns
      dw_right_tap_reads_junk  the right tap of the last valid column reads a non-zero value (the column's own) where
                               the zero padding starts: junk from behind F leaking in
      pw2_last_chunk           the last valid column of the last pw_conv2 without its last 16-channel chunk
      ola_last_frame           the last frame left out of the overlap-add over the final hop samples (envelope kept)
      reflect_pad              column 0 of the reflection pad taken from z[..., 0] instead of z[..., 1]"""
    vo, hit, seen = di.vo(), [], [0]
    real_F, real_conv1d, real_istft = vo.F, vo.conv1d, torch.istft

    def f_conv1d(x, w, b=None, *a, **kw):
        y = real_F.conv1d(x, w, b, *a, **kw)
        if kw.get("groups", 1) == x.shape[1] > 1:  # a depthwise conv: layer `seen[0]`
            layer, seen[0] = seen[0], seen[0] + 1
            if layer == n_layers - 1 and defect.startswith("dw_"):
                y = y.clone()
                if defect == "dw_right_tap_reads_junk":
                    y[:, :, -1] += w[:, 0, 2] * x[:, :, -1]
                else:
                    ch = slice(WAVE * per, (WAVE + 1) * per) if defect.endswith("one_wave") else slice(None)
                    assert x.shape[-1] > SEAM_COLUMN + 2
                    y[:, ch, SEAM_COLUMN] -= w[ch, 0, 0] * x[:, ch, SEAM_COLUMN - 1]
                hit.append(f"dw_conv {layer}")
        return y

    def f_pad(x, pad, mode="constant", value=None):
        y = real_F.pad(x, pad, mode=mode, value=value)
        if mode == "reflect" and defect == "reflect_pad":
            y = y.clone()
            y[..., 0] = x[..., 0]
            hit.append("reflection pad")
        return y

    def conv1d(W, name, x, dilation=1, padding=0, groups=1):
        y = real_conv1d(W, name, x, dilation=dilation, padding=padding, groups=groups)
        if defect == "pw2_last_chunk" and name == f"dec.layers.{n_layers - 1}.pw_conv2":
            w = W[name + ".weight"]
            y = y.clone()
            y[:, :, -1] -= torch.einsum("oc,bc->bo", w[:, -16:, 0], x[:, -16:, -1])
            hit.append(name)
        return y

    def istft(spec, n_fft, hop, win, window, **kw):
        y = real_istft(spec, n_fft, hop, win, window=window, **kw)
        if defect == "ola_last_frame":
            assert hop <= n_fft // 2
            nfr = spec.shape[-1]
            last = torch.fft.irfft(spec[..., -1], n=n_fft, dim=-1) * window  # the last frame, windowed: [B, n_fft]
            env = torch.zeros(n_fft + hop * (nfr - 1), dtype=window.dtype)
            for f in range(nfr):
                env[f * hop:f * hop + n_fft] += window * window
            end = n_fft // 2 + hop * (nfr - 1)  # the trimmed audio is [n_fft / 2, end) of the overlap-add buffer
            y = y.clone()
            y[:, -hop:] -= last[:, n_fft // 2 - hop:n_fft // 2] / env[end - hop:end]
            hit.append("overlap-add")
        return y

    monkeypatch.setattr(vo, "F", _Patched(real_F, conv1d=f_conv1d, pad=f_pad))
    monkeypatch.setattr(vo, "conv1d", conv1d)
    monkeypatch.setattr(vo, "torch", _Patched(vo.torch, istft=istft))
    return hit


_VCLEAN = {}


def _vclean(mname):
    if mname not in _VCLEAN:
        cfg, sd, cd, W32, W64 = di.weights(mname)
        z, g = di.inputs(W32, *VOCOS_SENS_SHAPE, seed=78)
        _VCLEAN[mname] = (cd, W64, z, g, di.oracle(W64, cd, z, g))
    return _VCLEAN[mname]


# the factor each defect must reach over the local gate of its config: the issue's 10, everywhere
SENS_FACTOR = 10.0


@pytest.mark.parametrize("defect", VOCOS_DEFECTS)
@pytest.mark.parametrize("mname", di.SEAM_CONFIGS)
def test_seam_local_gate_sees_the_vocos_defect(mname, defect, monkeypatch):
    """Each defect, applied to the float64 oracle, moves `local` to >= 10 x SEAM_LOCAL_GATE[config]: the GPU sweep's
    assert would fail on a kernel that computed it.  What the whole-tensor gates of the full-size test (abs RMS 1e-4,
    rel RMS 2e-3) would have seen is printed."""
    cd, W64, z, g, ref = _vclean(mname)
    md = di.model_dict(mname)
    C = md["vocos_channels"]
    per = di.dwln_tiles(C, VOCOS_SENS_SHAPE[1])["inst"] or C // 16  # the fallback has no waves: the same share of C
    hit = _defective_vocos(monkeypatch, defect, cd, md["vocos_num_layers"], per)
    bad = di.oracle(W64, cd, z, g)
    monkeypatch.undo()
    assert len(hit) == 1, hit
    rel, loc = di.gates(bad, ref)
    abs_rms = util.rms((bad - ref).numpy())
    gate = di.SEAM_LOCAL_GATE[mname]
    print(f"{mname} {VOCOS_SENS_SHAPE} defect {defect} in {hit[0]}: local {loc:.3g} = {loc / gate:.0f} x SEAM_LOCAL_GATE "
          f"({gate:.3g}); rel {rel:.3g} = {rel / di.SEAM_REL_GATE[mname]:.1f} x SEAM_REL_GATE; old whole-tensor gates: abs "
          f"RMS {abs_rms:.3g} ({'seen' if abs_rms > di.AUDIO_ABS else 'not seen'} by 1e-4), rel RMS {rel:.3g} "
          f"({'seen' if rel > OLD_REL else 'not seen'} by 2e-3)")
    assert loc >= SENS_FACTOR * gate


# ---- the sweep's lengths against the geometry of the Vocos head -----------------------------------------------------------
CUS = 256  # the CU count of an MI355X, fixed here; the GPU tier recomputes the claims with the device's own


def _dwln_coverage(shapes_of):
    """{instantiation (4 / 16 / 32 / "fallback"): dict(one_valid, junk_only, seam, multi, junk widths at a seam)}."""
    acc = {}
    for m in shapes_of:
        C = di.model_dict(m)["vocos_channels"]
        for B, L in shapes_of[m]:
            t = di.dwln_tiles(C, L)
            e = acc.setdefault(t["inst"] or "fallback", dict(one_valid=0, junk_only=0, seam=0, multi=0, junk=set(),
                                                             last=set()))
            e["one_valid"] += t["tiles"] > 1 and t["last_valid"] == 1
            e["junk_only"] += t["tiles"] > 1 and t["last_valid"] == 0
            e["seam"] += t["F"] % 62 == 0
            e["multi"] += t["tiles"] > 1
            e["last"].add((t["last_valid"], t["last_cols"]))
            if abs(t["F"] - 62 * round(t["F"] / 62)) <= 3:  # F within 3 columns of a seam
                e["junk"].add(t["junk"])
    return acc


def test_seam_sweep_reaches_every_edge_of_the_fused_dwconv_layernorm_kernel():
    """Per instantiation of convnext_dwln_kernel (<4>: tiny_vocos / vocos_n78, <16>: vocos_c256, <32>: vits2_vocos_v1)
    and for the k_dwconv + k_layernorm fallback (vocos_c96, vocos_c80): a last tile of one valid column, a last tile of
    junk only, a decode that ends exactly on a seam, a multi-tile decode, and all four junk widths at a seam.  The old
    sweep (SHAPES, Fs <= 52) has one tile everywhere and no <16> or fallback config."""
    new = _dwln_coverage({m: di.SEAM_SHAPES[m] for m in di.SEAM_CONFIGS})
    for inst, e in sorted(new.items(), key=str):
        print(f"dwln {inst}: one-valid-column last tiles {e['one_valid']}, junk-only {e['junk_only']}, F on a seam "
              f"{e['seam']}, multi-tile {e['multi']}, junk widths at a seam {sorted(e['junk'])}, (valid, stored) columns "
              f"of the last tile {sorted(e['last'])}")
    assert set(new) == {4, 16, 32, "fallback"}
    for inst, e in new.items():
        assert e["one_valid"] and e["junk_only"] and e["seam"] and e["multi"], (inst, e)
        assert e["junk"] == {0, 1, 2, 3}, (inst, e)
    old = _dwln_coverage({m: di.SHAPES[m] for m in di.VOCOS})
    assert set(old) == {4, 32}
    assert not any(e["multi"] or e["seam"] or e["one_valid"] or e["junk_only"] for e in old.values())
    # the wide cases run <32> over 3, 4, 8 and 11 tiles
    assert sorted(di.dwln_tiles(512, L)["tiles"] for _, L in di.WIDE_SHAPES) == [3, 4, 8, 11]


def test_seam_configs_reach_the_other_conv_paths():
    """Which kernel each conv of the head takes (restated launch_conv order), per config and form: the small-launch
    kernel for everything at the default dispatch; at small_max_tiles=0 pw_gemm_kernel for every conv except the
    residual conv of vocos_c80 (M = 80 is no multiple of 32: conv_mfma_kernel with `res`).  Odd chunk counts in the
    reductions: 17 (vocos_c256 pw2), 11 (vocos_c96 pw2), 5 (vocos_c80 pw1, out; vocos_n78's iSTFT: 80 rows, nothing
    padded); the padded iSTFT reductions 66 -> 80 and 1026 -> 1040."""
    table = {}
    for m in di.SEAM_CONFIGS:
        for form in ("default", "tiled"):
            for B, L in di.SEAM_SHAPES[m]:
                for r in di.vocos_launches(m, B, L, form, CUS):
                    table.setdefault((m, form, r["conv"]), set()).add((r["kernel"], r["K"]))
    for k in sorted(table):
        print(k, sorted(table[k]))
    for (m, form, conv), v in table.items():
        kernels = {k for k, _ in v}
        if form == "default":
            assert kernels == {"small"}, (m, conv, v)
        else:
            assert kernels == ({"tiled"} if (m, conv) == ("vocos_c80", "pw2") else {"pw_gemm"}), (m, conv, v)
    K = {(m, conv): next(iter(v))[1] for (m, form, conv), v in table.items() if form == "tiled"}
    assert K["vocos_c256", "pw2"] == 17 * 16 and K["vocos_c96", "pw2"] == 11 * 16 and K["vocos_c80", "pw1"] == 5 * 16
    assert K["vocos_n78", "istft"] == 80 and K["tiny_vocos", "istft"] == 80 and K["vits2_vocos_v1", "istft"] == 1040
    ratios = {m: (di.model_dict(m)["vocos_istft_config"]["n_fft"], di.model_dict(m)["vocos_istft_config"]["hop_length"])
              for m in di.SEAM_CONFIGS}
    assert {n / h for n, h in ratios.values()} >= {2.0, 3.0, 4.0, 8.0} and any(n % h for n, h in ratios.values())
    assert any((n + 2) % 16 == 0 for n, h in ratios.values())


def test_wide_cases_reach_every_pass_pattern_of_pw_gemm():
    """pw_schedule restated with 256 CUs: the wide cases (vits2_vocos_v1, B = 32, default dispatch) reach pass widths 1,
    2 and 4, blocks of several passes of different width, upb >= 8, strips split over blocks of upb > 1, a partial and
    a full last unit -- on pw1 (GELU epilogue, K = 512, 12 m-tiles), pw2 (K = 1536, residual accumulator init), in,
    out and the padded-K iSTFT GEMM (1026 -> 1040 rows).  The old sweep and the seam sweep reach upb = 1 only."""
    pat, missing = di.wide_claims(CUS)
    for conv, e in pat.items():
        print(f"pw_gemm {conv}: pass widths {sorted(e['widths'])}, mixed-width block {e['mixed']}, largest upb {e['upb']}, "
              f"S > 1 with upb > 1 {e['split']}, partial last unit {e['partial']}, full last unit {e['full']}")
    for B, L in di.WIDE_SHAPES:
        print((B, L), [(r["conv"], r["S"], r["upb"], sorted(set(r["passes"])), r["last_unit"])
                       for r in di.vocos_launches(di.WIDE_CONFIG, B, L, "default", CUS)])
    assert not missing, missing
    assert pat["pw1"]["upb"] >= 11 and pat["pw1"]["widths"] == {1, 2, 4} and pat["pw1"]["mixed"]
    for cases in ([(m, B, L) for m in di.VOCOS for B, L in di.SHAPES[m]],
                  [(m, B, L) for m in di.SEAM_CONFIGS for B, L in di.SEAM_SHAPES[m]]):
        assert di.pw_patterns(cases, "default", CUS) == {}  # the small-launch kernel takes everything
        for conv, e in di.pw_patterns(cases, "tiled", CUS).items():
            assert e["widths"] == {1} and e["upb"] == 1 and not e["mixed"] and not e["split"], (conv, e)
