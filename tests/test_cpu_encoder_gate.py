"""CPU tier: the gates that tests/test_gpu_encoder_oracle.py holds the text encoder and the duration predictors to
(tests/encoder_input.py: REL_GATE, LOCAL_GATE = 4 x the worst error of the float32 oracle against the float64 oracle
over the GPU sweep's shapes) are calibrated and proven here, without a GPU.

* The committed floors cannot drift silently: the floor of the two cheap configs is recomputed and the committed gates
  must lie within 2 .. 8 x it.
* The local gate of x_enc sees the defects it exists for.  Four defective float32 attentions (a copy of
  vits_oracle.rel_attention with one term changed, in the last encoder layer, one batch row, at Tx = 129) -- one query
  without one relative-key band term, one query without one relative-value term, the last key masked, the key at T - 1
  left out of the softmax sum -- must each move `local` of x_enc to >= 10 x its gate.
* The lengths of the GPU sweeps put every kernel form of attention.hip, and every edge of a form that a length decides,
  in front of the float64 oracle (the dispatch restated in tests/encoder_input.py:attention_form)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import encoder_input as ei


# ---- the floor ---------------------------------------------------------------------------------------------------
def test_every_swept_config_has_a_committed_floor_and_gate():
    assert set(ei.FLOOR) == set(ei.CONFIGS) == set(ei.SHAPES) == set(ei.FACTOR)
    for m in ei.CONFIGS:
        assert set(ei.FLOOR[m]) == set(ei.GATED)
        assert 2.0 <= ei.FACTOR[m] <= 8.0
        for s in ei.GATED:
            assert ei.REL_GATE[m][s] == ei.FACTOR[m] * ei.FLOOR[m][s][0]
            assert ei.LOCAL_GATE[m][s] == ei.FACTOR[m] * ei.FLOOR[m][s][1]
            # far under what the whole-utterance audio gates (1e-4 / 1e-3 RMS) imply for a stage
            assert ei.REL_GATE[m][s] < 1e-5 and ei.LOCAL_GATE[m][s] < 1e-4, (m, s)
        # every multi-row batch: a full row, a row of 1, a row 1 past a multiple of 32
        for i, (B, Tx, nsw) in enumerate(ei.SHAPES[m]):
            xl = ei.inputs(B, Tx, 2000 + i)[1].tolist()
            assert len(xl) == B and max(xl) == Tx and min(xl) >= 1
            if B > 1:
                assert 1 in xl and any(n % 32 == 1 for n in xl)
            if B > 2 and Tx >= 34:
                assert any(n % 32 == 1 and n > 1 for n in xl)
        assert (m in ei.SDP) == any(nsw == ei.TAIL_NOISE_SCALE_W for _, _, nsw in ei.SHAPES[m])


@pytest.mark.parametrize("mname", ["tiny", "tiny_dp"])
def test_committed_gates_are_2_to_8_times_the_recomputed_floor(mname):
    """float32 oracle against float64 oracle on the sweep's own inputs (same seeds), every case of SHAPES[mname]; no
    ceil(w) differs between the two."""
    fl, flips, n = ei.floor(mname)
    for s in ei.GATED:
        rel, loc = fl[s]
        print(f"{mname} {s}: recomputed floor rel {rel:.3g} local {loc:.3g}; committed {ei.FLOOR[mname][s]}, gates rel "
              f"{ei.REL_GATE[mname][s]:.3g} ({ei.REL_GATE[mname][s] / rel:.2f} x) local {ei.LOCAL_GATE[mname][s]:.3g} "
              f"({ei.LOCAL_GATE[mname][s] / loc:.2f} x)")
        assert 2.0 * rel <= ei.REL_GATE[mname][s] <= 8.0 * rel, s
        assert 2.0 * loc <= ei.LOCAL_GATE[mname][s] <= 8.0 * loc, s
    print(f"{mname}: {flips} of {n} durations differ between the float32 and the float64 oracle")
    assert flips == 0


# ---- sensitivity -------------------------------------------------------------------------------------------------
SENS_B, SENS_TX, SENS_QUERY, SENS_R, SENS_HEAD = 2, 129, 64, 2, 0
DEFECTS = ("rel_key_term", "rel_value_term", "last_key_masked", "last_key_not_in_sum")


def _defective_attention(real, defect, layer, row):
    """vits_oracle.rel_attention with one defect in encoder layer `layer`, batch row `row`, head SENS_HEAD."""
    hit = []

    def rel_attention(W, pre, x, attn_mask, n_heads, window):
        if pre != layer:
            return real(W, pre, x, attn_mask, n_heads, window)
        hit.append(pre)
        conv = ei.di.vo().conv1d
        q, k, v = (conv(W, pre + n, x) for n in (".conv_q", ".conv_k", ".conv_v"))
        b, d, t = q.shape
        dk = d // n_heads
        q, k, v = (a.view(b, n_heads, dk, t).transpose(2, 3) for a in (q, k, v))
        qs = q / math.sqrt(dk)
        scores = torch.matmul(qs, k.transpose(-2, -1))
        Ek, Ev = W[pre + ".emb_rel_k"][0], W[pre + ".emb_rel_v"][0]
        rel = torch.matmul(qs, Ek.t())
        idx = torch.arange(t)
        for r in range(-window, window + 1):
            i = idx[(idx + r >= 0) & (idx + r < t)]
            keep = torch.ones(b, n_heads, i.numel(), dtype=x.dtype)
            if defect == "rel_key_term" and r == SENS_R:
                keep[row, SENS_HEAD, int((i == SENS_QUERY).nonzero())] = 0.0
            scores[:, :, i, i + r] += rel[:, :, i, r + window] * keep
        scores = scores.masked_fill(attn_mask == 0, -1e4)
        if defect == "last_key_masked":
            scores[row, SENS_HEAD, :, t - 1] = -1e4
        if defect == "last_key_not_in_sum":
            e = torch.exp(scores - scores.max(dim=-1, keepdim=True).values)
            z = e.sum(-1, keepdim=True)
            z[row, SENS_HEAD] -= e[row, SENS_HEAD, :, t - 1:]
            p = e / z
        else:
            p = F.softmax(scores, dim=-1)
        out = torch.matmul(p, v)
        for r in range(-window, window + 1):
            i = idx[(idx + r >= 0) & (idx + r < t)]
            keep = torch.ones(b, n_heads, i.numel(), 1, dtype=x.dtype)
            if defect == "rel_value_term" and r == SENS_R:
                keep[row, SENS_HEAD, int((i == SENS_QUERY).nonzero())] = 0.0
            out[:, :, i, :] += p[:, :, i, i + r].unsqueeze(-1) * Ev[r + window] * keep
        out = out.transpose(2, 3).contiguous().view(b, d, t)
        return conv(W, pre + ".conv_o", out)
    return rel_attention, hit


_SENS = {}


def _sens():
    """Inputs, the clean float64 x_enc and the clean float32 x_enc of the sensitivity shape, once."""
    if not _SENS:
        cfg, sd, cd, W32, W64 = ei.weights("tiny")
        x, xl, sid, eps_w = ei.inputs(SENS_B, SENS_TX, 77)
        row = int(xl.argmax())
        assert int(xl[row]) == SENS_TX
        _SENS.update(cd=cd, W32=W32, ins=(x, xl, sid, eps_w), row=row,
                     ref=ei.stages(W64, cd, x, xl, sid, eps_w)["x_enc"], clean=ei.stages(W32, cd, x, xl, sid, eps_w)["x_enc"])
    return _SENS


def test_defect_free_copy_of_the_attention_is_the_oracle(monkeypatch):
    """The copy the defects are injected into computes what vits_oracle.rel_attention computes (to float32 rounding: the
    band terms enter in the same order), so a defect's effect is the defect's."""
    s = _sens()
    layer = f"enc_p.encoder.attn_layers.{s['cd']['n_layers'] - 1}"
    fake, hit = _defective_attention(ei.di.vo().rel_attention, None, layer, s["row"])
    monkeypatch.setattr(ei.di.vo(), "rel_attention", fake)
    same = ei.stages(s["W32"], s["cd"], *s["ins"])["x_enc"]
    monkeypatch.undo()
    assert len(hit) == 1
    rel, loc = ei.gates(same, s["clean"])
    print(f"defect-free copy against the float32 oracle: rel {rel:.3g} local {loc:.3g}")
    assert loc <= ei.FLOOR["tiny"]["x_enc"][1]


@pytest.mark.parametrize("defect", DEFECTS)
def test_local_gate_of_x_enc_sees_the_defect(defect, monkeypatch):
    s = _sens()
    layer = f"enc_p.encoder.attn_layers.{s['cd']['n_layers'] - 1}"
    fake, hit = _defective_attention(ei.di.vo().rel_attention, defect, layer, s["row"])
    monkeypatch.setattr(ei.di.vo(), "rel_attention", fake)
    bad = ei.stages(s["W32"], s["cd"], *s["ins"])["x_enc"]
    monkeypatch.undo()
    assert len(hit) == 1, hit
    rel, loc = ei.gates(bad, s["ref"])
    gate = ei.LOCAL_GATE["tiny"]["x_enc"]
    print(f"tiny ({SENS_B}, {SENS_TX}) defect {defect} in {layer}: local {loc:.3g} = {loc / gate:.0f} x LOCAL_GATE "
          f"({gate:.3g}); rel {rel:.3g} = {rel / ei.REL_GATE['tiny']['x_enc']:.1f} x REL_GATE")
    assert loc >= 10.0 * gate
    # every local gate of x_enc, raised factors included, stays under a tenth of the defect
    assert all(ei.LOCAL_GATE[m]["x_enc"] <= 0.1 * loc for m in ei.CONFIGS)


# ---- the sweeps' lengths against the dispatch ----------------------------------------------------------------------
def _enc_forms(mname, small_max_t):
    w, dk = ei.encoder_attention(mname)
    acc = {}
    for T in sorted({Tx for _, Tx, _ in ei.SHAPES[mname]}):
        acc.setdefault(ei.attention_form(w, T, dk, small_max_t), []).append(T)
    return acc


@pytest.mark.parametrize("mname", ["tiny", "tiny_dp", "tiny_preconv2_spk"])
def test_encoder_sweep_reaches_every_windowed_form_and_edge(mname):
    w, dk = ei.encoder_attention(mname)
    assert (w, dk) == (4, 96)
    default, general = _enc_forms(mname, 128), _enc_forms(mname, 0)
    print(mname, "default", default, "attn_small_max_t=0", general)
    # the one-launch kernel: both staging branches, both row-stride paddings, several 32-query strips, T = 128
    small = default["small"]
    assert max(small) == 128 and set(default) == {"small", "mfma_windowed"}
    assert ei.small_layout(128, dk)[3] == 142336 > 64 * 1024  # its largest footprint: the large-LDS opt-in
    for branch in ("vec16", "scalar"):
        assert len([T for T in small if ei.small_staging(T) == branch]) >= 3, branch
    for pad in (0, 4):
        assert len([T for T in small if ei.small_layout(T, dk)[2] - ei.small_layout(T, dk)[1] == pad]) >= 3, pad
    assert len([T for T in small if T > 32]) >= 3 and len([T for T in small if T % 32 not in (0, 1)]) >= 3
    assert len([T for T in small if T <= 2 * w]) >= 3  # the band wider than the sequence
    # the matrix-core path of the default dispatch: the last 128-key block narrower than, equal to and one past 32
    long_ = default["mfma_windowed"]
    assert min(long_) == 129 and len(long_) >= 3
    rems = {T % 128 for T in long_}
    assert any(0 < r < 32 for r in rems) and 32 in rems and 33 in rems and 0 in rems
    # under attn_small_max_t=0: the scalar kernels below 64, the matrix-core path from 64 to 128
    assert set(general) == {"scalar", "mfma_windowed"}
    assert len(general["scalar"]) >= 3 and max(general["scalar"]) == 63
    assert len([T for T in general["mfma_windowed"] if T <= 128]) >= 3 and min(general["mfma_windowed"]) == 64
    # a device that refuses the opt-in falls to the same kernels the knob reaches
    assert ei.attention_form(w, 128, dk, 128, large_lds=False) == "mfma_windowed"


def test_v1_sweep_reaches_every_windowed_form():
    default, general = _enc_forms("v1", 128), _enc_forms("v1", 0)
    print("v1 default", default, "attn_small_max_t=0", general)
    assert len(default["small"]) >= 3 and 128 in default["small"] and len(default["mfma_windowed"]) >= 3
    assert {ei.small_staging(T) for T in default["small"]} == {"vec16", "scalar"}
    assert len(general["scalar"]) >= 3 and len([T for T in general["mfma_windowed"] if T <= 128]) >= 3


def test_flow_sweep_reaches_flash_tiles_and_the_wide_windowed_path():
    """tests/test_gpu_vc_oracle.py's tile-edge list: attn_flash_kernel (dk = 48) with one, two and five or more key tiles
    per wave and a partial last tile; the windowed matrix-core path at dk = 96 (three 32-row d-blocks of
    attn_pv_mfma_kernel); and, under attn_small_max_t=0, the scalar kernels and that path below 129."""
    from tests import test_gpu_vc_oracle as vc
    lengths = sorted({Ty for _, Ty, _ in vc.TILE_SHAPES})
    for B, Ty, yl in vc.TILE_SHAPES:
        assert len(yl) == B and max(yl) == Ty and (B == 1 or 1 in yl) and (B < 3 or any(n % 32 == 1 and n > 1 for n in yl))
    forms = {}
    for m in vc.TF_MODELS:
        w, dk = ei.flow_attention(m)
        forms[m] = {T: ei.attention_form(w, T, dk) for T in lengths}
    print(forms)
    flash = [m for m in vc.TF_MODELS if set(forms[m].values()) == {"flash"}]
    assert sorted(flash) == sorted(["vits2_v1", "tiny_mono_post", "tiny_mono_inter", "tiny_vits2_vocos"])
    assert all(ei.flow_attention(m) == (-1, 48) for m in flash)
    tiles = {ei.flash_tiles(T)[0] for T in lengths}
    assert 1 in tiles and 2 in tiles and max(tiles) >= 5
    assert any(ei.flash_tiles(T)[1] < 32 for T in lengths) and any(ei.flash_tiles(T)[1] == 32 for T in lengths)
    assert ei.flow_attention("tiny_preconv2_spk") == (4, 96)
    wide = forms["tiny_preconv2_spk"]
    assert len([T for T in lengths if wide[T] == "mfma_windowed"]) >= 3 and len([T for T in lengths if wide[T] == "small"]) >= 3
    assert ("tiny_preconv2_spk", "attn_small_max_t=0") in vc.TILE_SWEEP
    general = {T: ei.attention_form(4, T, 96, 0) for T in lengths}
    assert len([T for T in lengths if general[T] == "scalar"]) >= 3
    assert len([T for T in lengths if general[T] == "mfma_windowed" and T <= 128]) >= 3


def test_every_kernel_of_attention_hip_is_reached_by_an_oracle_compared_case():
    """Form -> kernels, and the forms the two GPU sweeps reach.  Left uncovered, by the issue's own scope: "mfma_plain",
    the window-less three-kernel path for heads wider than 48 channels, which no config of the reference has (its
    kernels all run in "mfma_windowed")."""
    kernels = {
        "small": {"attn_small_kernel"},
        "flash": {"attn_transpose_v_kernel", "attn_flash_kernel"},
        "mfma_windowed": {"attn_relk_kernel", "attn_scores_mfma_kernel", "attn_softmax_kernel", "attn_transpose_v_kernel",
                          "attn_pv_mfma_kernel", "attn_relv_add_kernel"},
        "scalar": {"attn_scores_kernel", "attn_softmax_kernel", "attn_pv_kernel"},
    }
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wetts_amd", "csrc",
                            "attention.hip")).read()
    defined = set(re.findall(r"void\s+(attn_\w+_kernel)\s*\(", src))
    reached = set(_enc_forms("tiny", 128)) | set(_enc_forms("tiny", 0))
    from tests import test_gpu_vc_oracle as vc
    for m in vc.TF_MODELS:
        w, dk = ei.flow_attention(m)
        reached |= {ei.attention_form(w, Ty, dk) for _, Ty, _ in vc.TILE_SHAPES}
    assert reached == set(kernels)
    assert set().union(*kernels.values()) == defined, defined
