"""CPU tier of the duration loss (SynthesizerTrn.duration_loss): the oracle of tests/duration_oracle.py pinned to the
reference's fixtures (tests/golden/dur_*.npz, made by make_golden_dur.py), the committed floors recomputed, proof that
the gates see the defects they exist for, the extra blob's layout against the reference module's own keys, and the
argument validation that needs no device."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import align_oracle as ao, duration_oracle as do, encoder_input as ei, util
from wetts_amd import SynthesizerTrn, _lib, checkpoint, config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "dur_*.npz")))
SPEC = ao.SPEC


def fixture_model(c):
    """(cfg struct, state dict with the duration tensors, cfg dict) of a dur_* fixture, both checksums asserted."""
    cfg = config.make_config(dict(config.MODEL_CONFIGS[str(c["model"])]), int(c["n_vocab"]), int(c["n_speakers"]))
    sd = synth.make_state_dict(cfg, int(c["weight_seed"]))
    dsd = synth.make_duration_state_dict(cfg, int(c["duration_seed"]))
    for blob, key in ((checkpoint.pack_blob(cfg, sd), "blob_checksum"),
                      (checkpoint.pack_duration_blob(cfg, dsd) if dsd else None, "duration_checksum")):
        if blob is not None:
            assert abs(synth.blob_checksum(blob) - float(c[key])) <= 1e-6 * max(1.0, abs(float(c[key]))), key
    return cfg, dict(sd, **dsd), util.cfg_dict(cfg)


def fixture_inputs(c):
    xls = [int(v) for v in c["x_lengths"]]
    x = torch.from_numpy(ao.align_tokens(int(c["token_seed"]), int(c["n_vocab"]), xls))
    return (x, torch.tensor(xls), torch.from_numpy(c["sid"]), torch.from_numpy(c["w"]).unsqueeze(1),
            torch.from_numpy(c["e_q"]), torch.from_numpy(c["eps_w"]))


# ---- 1. the oracle against the reference ------------------------------------------------------------------------------
def test_fixtures_exist_for_every_alignment_case():
    assert len(FIXTURES) == 9 and "dur_tiny_dp_b2" in FIXTURES and "dur_aishell3_b4x600" in FIXTURES
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 64 << 10


@pytest.mark.parametrize("name", FIXTURES)
def test_float32_oracle_reproduces_the_reference_fixture(name):
    """l_length within FIXTURE_GATE x abs_total / sum(x_mask) of the live reference's value (the float64 oracle too), logw
    within the logw gates of tests/encoder_input.py, logw_ to float32 rounding of one log."""
    c = util.load_case(name)
    cfg, sd, cd = fixture_model(c)
    W32 = checkpoint.fold_weight_norm(sd)
    W64 = {k: v.double() for k, v in W32.items()}
    inp = fixture_inputs(c)
    a, r = do.stages(W32, cd, *inp), do.stages(W64, cd, *inp)
    scale = torch.from_numpy(c["abs_total"]) / float(r["x_mask"].sum())
    assert np.allclose(r["abs_total"].numpy(), c["abs_total"], rtol=1e-9)
    for tag, st in (("float32", a), ("float64", r)):
        err = do.scalar_err(st["l_length"], torch.from_numpy(c["l_length"]), scale)
        print(f"{name}: {tag} oracle l_length {st['l_length'].tolist()} reference {c['l_length'].tolist()} "
              f"|d| / scale {err:.3g} (gate {do.FIXTURE_GATE:.3g})")
        assert err <= do.FIXTURE_GATE
    rel, loc = do.gates(a["logw"], torch.from_numpy(c["logw"]))
    m = do.logw_gate_model(str(c["model"]))
    print(f"{name}: logw rel {rel:.3g} local {loc:.3g}")
    assert rel <= ei.REL_GATE[m]["logw"] and loc <= ei.LOCAL_GATE[m]["logw"]
    assert np.abs(a["logw_"].numpy() - c["logw_"]).max() <= 4 * 2.0 ** -24 * np.abs(c["logw_"]).max()


# ---- 2. the floor ----------------------------------------------------------------------------------------------------
def test_every_swept_config_has_a_committed_floor():
    assert set(do.FLOOR) == set(do.SDP) and set(do.SHAPES) == set(do.SDP) | set(do.DP)
    for m in do.SDP:
        assert set(do.FLOOR[m]) == set(do.VARIANTS)
        for v in do.VARIANTS:
            assert set(do.FLOOR[m][v]) == set(do.TENSORS) | set(do.SCALARS)
        assert do.SHAPES[m][-1][2] == 3.0  # the case that sends the posterior flows' inputs past +-5
    assert do.GATE_FACTOR == ei.GATE_FACTOR == 4.0
    for m in do.SHAPES:  # every multi-row batch: a full row and a row of 1
        for i, (B, Tx, sc) in enumerate(do.SHAPES[m]):
            x, xl, sid, w, e_q, eps_w = do.inputs(B, Tx, 3000 + i, sc)
            assert max(xl.tolist()) == Tx and (B == 1 or 1 in xl.tolist())
            full = w[int(torch.argmax(xl)), 0].tolist()
            assert full[:3] == [0.0, 300.0, 1.0][:Tx]
            assert float((w[:, 0] * (torch.arange(Tx)[None] >= xl[:, None])).abs().sum()) == 0.0


@pytest.mark.parametrize("variant", do.VARIANTS)
@pytest.mark.parametrize("mname", ["tiny", "tiny_preconv2_spk"])
def test_committed_gates_are_2_to_8_times_the_recomputed_floor(mname, variant):
    fl = do.floor(mname, variant)
    for s in do.TENSORS + do.SCALARS:
        got, gate = fl[s], do.gate(mname, variant, s)
        print(f"{mname} {variant} {s}: recomputed floor {got}; committed {do.FLOOR[mname][variant][s]}; gate {gate}")
        for f, g in zip(got if isinstance(got, tuple) else (got,), gate if isinstance(gate, tuple) else (gate,)):
            assert 2.0 * f <= g <= 8.0 * f, (s, f, g)


def test_dp_floor_is_the_committed_one():
    worst, wl = do.dp_floor()
    print("tiny_dp rows:", worst, "logw_:", wl, "committed", do.DP_FLOOR)
    assert 2.0 * worst <= do.GATE_FACTOR * do.DP_FLOOR[0] <= 8.0 * worst
    assert 2.0 * wl[1] <= do.GATE_FACTOR * do.DP_FLOOR[1][1] <= 8.0 * wl[1]


# ---- 3. sensitivity --------------------------------------------------------------------------------------------------
SENS = (5, 65, 1.0)  # a case of the tiny sweep; its row 0 is the full row
FAULTS = {
    "one logabsdet dropped": ("drop_logabsdet", 1, 0, 7),
    "the neighbouring bin for one position": ("neighbour_bin", 1, 0, 7),
    "searchsorted on cumheights": "search_heights",
    "a Flip omitted": ("no_flip", 1),
    "dp.flows.1 skipped": "skip_flows1",
    "sign of logdet_tot_q flipped": "sign_q",
    "divisor per row": "row_divisor",
}


@pytest.mark.parametrize("what", sorted(FAULTS))
def test_the_gates_see_the_defect_by_a_factor_of_ten(what):
    """Each defect, in the float64 oracle on the unpinned tiny model, moves a gated quantity by >= 10 x its gate; the
    single-position ones are held to the local gate of nll_terms."""
    cfg, sd, cd, W32, W64 = do.weights("tiny", "unpinned")
    i = do.SHAPES["tiny"].index(SENS)
    inp = do.inputs(*SENS[:2], 3000 + i, SENS[2])
    good, bad = do.stages(W64, cd, *inp), do.stages(W64, cd, *inp, fault=FAULTS[what])
    assert int(inp[1][0]) > 7  # the position the single-position faults hit is a valid one
    m = do.measure(bad, good)
    ratios = {s: m[s][1] / do.gate("tiny", "unpinned", s)[1] for s in do.TENSORS}
    ratios.update({s: m[s] / do.gate("tiny", "unpinned", s) for s in do.SCALARS})
    ll = do.scalar_err(bad["l_length"], good["l_length"], good["abs_total"] / float(good["x_mask"].sum()))
    ratios["l_length"] = ll / (do.gate("tiny", "unpinned", "nll") + do.gate("tiny", "unpinned", "logq"))
    # a NaN (the log of a negative derivative in the wrong bin) fails every gate: the GPU tests assert `<=` and finiteness
    ratios = {k: (float("inf") if v != v else v) for k, v in ratios.items()}
    print(what, {k: round(v, 1) for k, v in ratios.items()})
    if what in ("one logabsdet dropped", "the neighbouring bin for one position"):
        assert ratios["nll_terms"] >= 10
    elif what == "divisor per row":
        assert ratios["l_length"] >= 10 and max(ratios[s] for s in do.TENSORS + do.SCALARS) == 0
    else:
        assert max(ratios.values()) >= 10


# ---- 4. no position sits on the clamp --------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", ["tiny", "tiny_preconv2_spk"])
def test_no_valid_position_is_within_1e_6_of_the_clamp(mname):
    """log(clamp_min(w - u, 1e-5)) has a kink at 1e-5: at float64 every valid w - u of every sweep case lies further
    than 1e-6 from it, so no position is ever left out of a comparison.  (v1: tests/test_gpu_duration.py asserts the
    same on the cases it runs.)"""
    for variant in do.VARIANTS:
        cfg, sd, cd, W32, W64 = do.weights(mname, variant)
        for i, (B, Tx, sc) in enumerate(do.SHAPES[mname]):
            r = do.stages(W64, cd, *do.inputs(B, Tx, 3000 + i, sc))
            valid = r["x_mask"][:, 0] > 0
            assert float((r["w_minus_u"][valid] - 1e-5).abs().min()) > 1e-6, (variant, B, Tx)


# ---- 5. - 8. the extra blob ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_duration_and_main_layout_cover_the_reference_modules_own_keys(name):
    c = util.load_case(name)
    cfg, sd, cd = fixture_model(c)
    ref = {str(k): tuple(int(v) for v in str(s).split(",")) for k, s in zip(c["key_names"], c["key_shapes"])}
    main = {n[3:]: shp for n, _, _, shp in checkpoint.blob_layout(cfg) if n.startswith("dp.")}
    dur = {n[3:]: shp for n, _, _, shp in checkpoint.duration_layout(cfg)}
    assert not set(main) & set(dur)
    if int(c["n_speakers"]) == 0:  # the reference builds dp.cond for gin_channels > 0 even without speakers
        ref = {k: v for k, v in ref.items() if not k.startswith("cond.")}
    assert dict(main, **dur) == ref
    assert bool(dur) == bool(cfg.use_sdp)
    end = 0
    for n, off, numel, shp in checkpoint.duration_layout(cfg):
        assert off >= end and off % 64 == 0 and numel == int(np.prod(shp))
        end = off + numel
    assert end <= checkpoint.duration_numel(cfg)


def _cfg(mname="tiny", n_spk=3):
    return config.make_config(dict(config.MODEL_CONFIGS[mname]), 40, n_spk)


def test_pack_duration_blob_names_the_missing_tensor_and_has_duration_is_false_for_todays_checkpoints():
    cfg = _cfg()
    sd = synth.make_state_dict(cfg, 1)
    dsd = synth.make_duration_state_dict(cfg, 2)
    assert not checkpoint.has_duration(cfg, sd)
    assert not checkpoint.has_duration(cfg, dict(sd, **synth.make_posterior_state_dict(cfg, SPEC, 3)))
    assert checkpoint.has_duration(cfg, dict(sd, **dsd))
    part = dict(dsd)
    del part["dp.post_flows.5.convs.norms_2.1.beta"]
    assert not checkpoint.has_duration(cfg, dict(sd, **part))
    with pytest.raises(KeyError, match=r"dp\.post_flows\.5\.convs\.norms_2\.1\.beta"):
        checkpoint.pack_duration_blob(cfg, part)
    bad = dict(dsd)
    bad["dp.post_pre.weight"] = torch.zeros(3, 1, 1)
    with pytest.raises(ValueError, match="dp.post_pre.weight"):
        checkpoint.pack_duration_blob(cfg, bad)
    blob = checkpoint.pack_duration_blob(cfg, dsd)
    assert blob.numel() == checkpoint.duration_numel(cfg) and blob.dtype == torch.float32
    dp = _cfg("tiny_dp")
    assert checkpoint.duration_layout(dp) == [] and synth.make_duration_state_dict(dp, 2) == {}
    assert not checkpoint.has_duration(dp, synth.make_state_dict(dp, 1))


def test_make_duration_state_dict_has_its_own_stream_and_no_identity_spline():
    cfg = _cfg()
    before = synth.make_state_dict(cfg, 5)
    dsd = synth.make_duration_state_dict(cfg, 5)
    after = synth.make_state_dict(cfg, 5)
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert not set(dsd) & set(before)
    again = synth.make_duration_state_dict(cfg, 5)
    assert all(torch.equal(dsd[k], again[k]) for k in dsd)
    for k, v in dsd.items():
        if k.endswith(".proj.weight") or k.endswith(".proj.bias"):
            assert float(v.abs().min()) > 0 or float(v.abs().mean()) > 1e-3, k


def test_state_dict_round_trip_carries_the_duration_tensors():
    cfg = _cfg()
    sd = dict(synth.make_state_dict(cfg, 1), **synth.make_duration_state_dict(cfg, 2))
    net = SynthesizerTrn(40, SPEC, 8, n_speakers=3, **config.MODEL_CONFIGS["tiny"]).load_state_dict(sd)
    out = net.state_dict()
    for k, v in synth.make_duration_state_dict(cfg, 2).items():
        assert torch.equal(out[k], v), k
    plain = SynthesizerTrn(40, SPEC, 8, n_speakers=3, **config.MODEL_CONFIGS["tiny"]).load_state_dict(
        synth.make_state_dict(cfg, 1))
    assert "dp.post_pre.weight" not in plain.state_dict()


# ---- 9. argument validation before any device work -------------------------------------------------------------------
def _net(mname="tiny", n_spk=3, with_duration=True):
    cfg = _cfg(mname, n_spk)
    sd = synth.make_state_dict(cfg, 1)
    if with_duration:
        sd = dict(sd, **synth.make_duration_state_dict(cfg, 2))
    return SynthesizerTrn(40, SPEC, 8, n_speakers=n_spk, **config.MODEL_CONFIGS[mname]).load_state_dict(sd)


def test_duration_loss_argument_validation_needs_no_device():
    net = _net()
    x, xl, sid = torch.zeros(2, 5, dtype=torch.long), torch.tensor([5, 3]), torch.tensor([0, 1])
    w = torch.ones(2, 1, 5)
    with pytest.raises(ValueError, match="x must be"):
        net.duration_loss(x[0], xl, w, sid)
    with pytest.raises(ValueError, match="x_lengths must be"):
        net.duration_loss(x, xl[:1], w, sid)
    for bad in (torch.ones(2, 1, 4), torch.ones(2, 2, 5), torch.ones(5), torch.ones(3, 5)):
        with pytest.raises(ValueError, match="w must be"):
            net.duration_loss(x, xl, bad, sid)
    with pytest.raises(ValueError, match="sid is required"):
        net.duration_loss(x, xl, w)
    with pytest.raises(ValueError, match="e_q must be"):
        net.duration_loss(x, xl, w, sid, e_q=torch.zeros(2, 2, 4))
    with pytest.raises(ValueError, match="eps_w must be"):
        net.duration_loss(x, xl, w, sid, eps_w=torch.zeros(2, 1, 5))
    with pytest.raises(ValueError, match="empty"):
        net.duration_loss(torch.zeros(0, 5, dtype=torch.long), torch.zeros(0, dtype=torch.long), torch.ones(0, 5), sid[:0])
    for kw in ({}, dict(e_q=torch.zeros(2, 2, 5)), dict(eps_w=torch.zeros(2, 2, 5))):
        for ww in (w, w[:, 0]):
            with pytest.raises(_lib.WettsError):  # valid arguments: the product path has no CPU fallback
                net.duration_loss(x, xl, ww, sid, **kw)
    with pytest.raises(_lib.WettsError):
        _net("tiny_dp").duration_loss(x, xl, w, sid)
    with pytest.raises(NotImplementedError):
        net.forward()
