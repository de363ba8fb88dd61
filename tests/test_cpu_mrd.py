"""CPU tier of MultiPeriodMultiResolutionDiscriminator: the blob layout against the reference's own state_dict, packing,
the host-side checks, band edges and frame counts against the reference's expressions, the float64 / float32 oracle of
tests/mrd_oracle.py against torch.stft, the live reference and its fixtures, and the sensitivity of the gates."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import ref_import
from tests import mrd_oracle as mo
from tests.test_cpu_disc import state_dict_digest
from wetts_amd import (MultiPeriodDiscriminator, MultiPeriodMultiResolutionDiscriminator, _lib, checkpoint, config,
                       discriminators, losses)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = mo.SHAPES[:2]  # the floor is recomputed on the two smallest shapes
_W = {}


def fixture_path(B, T):
    return os.path.join(ROOT, "tests", "golden", f"mrd_b{B}x{T}.npz")


def _weights():
    if not _W:
        _W["sd"], _W["W32"], _W["W64"] = mo.weights()
    return _W["sd"], _W["W32"], _W["W64"]


# ---- layout and packing ----------------------------------------------------------------------------------------------
def test_layout_is_the_fixed_architecture():
    lay = checkpoint.mrd_layout()
    assert len(lay) == 3 * 26 * 2 + 5 * 6 * 2 and len({n for n, *_ in lay}) == len(lay)
    end = 0
    for n, off, numel, shape in lay:
        assert off >= end and off % 64 == 0 and numel == int(np.prod(shape)), n
        end = off + numel
    assert checkpoint.mrd_numel() >= end
    shapes = dict((n, s) for n, _, _, s in lay)
    assert shapes["discriminators.0.band_convs.0.0.weight"] == (32, 2, 3, 9)
    assert shapes["discriminators.1.band_convs.4.2.weight"] == (32, 32, 3, 9)
    assert shapes["discriminators.2.band_convs.3.4.weight"] == (32, 32, 3, 3)
    assert shapes["discriminators.2.conv_post.weight"] == (1, 32, 3, 3)
    assert shapes["discriminators.7.convs.3.weight"] == (1024, 512, 5, 1)
    # the period stacks are MultiPeriodDiscriminator's, renumbered
    mpd = dict((n, s) for n, _, _, s in checkpoint.disc_layout())
    for d in range(1, 6):
        for n, s in mpd.items():
            if n.startswith(f"discriminators.{d}."):
                assert shapes[n.replace(f"discriminators.{d}.", f"discriminators.{d + 2}.", 1)] == s


@pytest.mark.skipif(not ref_import.available(), reason="the reference is not on this machine")
def test_layout_matches_a_live_reference_state_dict():
    from tests.golden.make_golden_mrd import import_reference
    MPMRD, _ = import_reference()
    ref = MPMRD(False).state_dict()
    folded = checkpoint.fold_weight_norm(ref)
    lay = checkpoint.mrd_layout()
    assert {n for n, *_ in lay} == set(folded)
    # natural order: the modules in the order the reference registers them
    assert [n[:-len(".weight")] for n, *_ in lay if n.endswith(".weight")] == \
        [k[:-len(".bias")] for k in ref if k.endswith(".bias")]
    for n, _, _, shape in lay:
        assert tuple(folded[n].shape) == shape, n


def test_packing_round_trips_and_both_spellings_fold_to_one_blob():
    sd, W32, _ = _weights()
    blob = checkpoint.pack_mrd_blob(sd)
    for n, off, numel, shape in checkpoint.mrd_layout():
        assert torch.equal(blob[off:off + numel].reshape(shape), W32[n]), n
    new = {}
    for k, v in sd.items():
        k = re.sub(r"\.weight_g$", ".parametrizations.weight.original0", k)
        new[re.sub(r"\.weight_v$", ".parametrizations.weight.original1", k)] = v
    assert set(new) != set(sd) and torch.equal(checkpoint.pack_mrd_blob(new), blob)
    assert torch.equal(checkpoint.pack_mrd_blob(W32), blob)  # already folded
    net = MultiPeriodMultiResolutionDiscriminator().load_state_dict(sd)
    back = net.state_dict()
    assert set(back) == set(W32) and all(torch.equal(back[k], W32[k]) for k in W32)
    short = dict(sd)
    del short["discriminators.1.band_convs.2.3.bias"]
    with pytest.raises(KeyError, match="discriminators.1.band_convs.2.3.bias"):
        checkpoint.pack_mrd_blob(short)
    bad = dict(sd)
    bad["discriminators.1.band_convs.2.3.bias"] = torch.zeros(3)
    with pytest.raises(ValueError):
        checkpoint.pack_mrd_blob(bad)
    emb = dict(sd)
    emb["discriminators.0.emb.weight"] = torch.zeros(4, 32)
    with pytest.raises(NotImplementedError, match="num_embeddings"):
        MultiPeriodMultiResolutionDiscriminator().load_state_dict(emb)


def test_synthetic_weights_keep_activations_of_order_one():
    _, W32, _ = _weights()
    y, y_hat = mo.inputs(1, 1300, 1)
    for i, m in enumerate(mo.forward(W32, y, y_hat)[0]):
        r = float(m.pow(2).mean().sqrt())
        assert 0.02 < r < 50, (i, r)


# ---- host checks -----------------------------------------------------------------------------------------------------
def test_host_side_checks_need_no_device():
    with pytest.raises(NotImplementedError, match="spectral"):
        MultiPeriodMultiResolutionDiscriminator(use_spectral_norm=True)
    net = MultiPeriodMultiResolutionDiscriminator()
    assert net.MIN_SAMPLES == 1025 and net.train(False) is net and net.eval() is net
    with pytest.raises(NotImplementedError):
        net.train()
    y = torch.zeros(2, 1, 2048)
    with pytest.raises(ValueError, match="HIP device"):
        net(y, y)
    with pytest.raises(ValueError, match="reflect pad of the 2048"):
        net(torch.zeros(2, 1, 1024), torch.zeros(2, 1, 1024))
    with pytest.raises(ValueError):
        net.to("cpu")
    with pytest.raises(RuntimeError, match="no weights"):
        net.state_dict()
    lib = _lib.load()
    assert lib.wetts_mrd_workspace_bytes(1, 1024) < 0 and lib.wetts_mrd_workspace_bytes(1, 1025) > 0
    with pytest.raises(ValueError, match="1 .. 128"):
        losses.feature_loss([[y] * 129], [[y] * 129])


def test_from_hparams_is_the_training_script_choice():
    hp = lambda **m: config.HParams(model=dict(use_spectral_norm=False, **m))  # noqa: E731
    assert type(discriminators.from_hparams(hp())) is MultiPeriodDiscriminator
    assert type(discriminators.from_hparams(hp(use_mrd_disc=False))) is MultiPeriodDiscriminator
    assert type(discriminators.from_hparams(hp(use_mrd_disc=True))) is MultiPeriodMultiResolutionDiscriminator


# ---- geometry --------------------------------------------------------------------------------------------------------
def test_band_edges_and_widths_are_the_reference_expressions():
    assert [hi - lo for lo, hi in mo.band_edges(2048)] == [102, 154, 256, 256, 257]
    assert [hi - lo for lo, hi in mo.band_edges(512)] == [25, 39, 64, 64, 65]
    lib = _lib.load()
    for r, w in enumerate(mo.WINDOWS):
        ws = mo.band_widths(w)
        assert mo.band_edges(w)[0][0] == 0 and mo.band_edges(w)[-1][1] == w // 2 + 1
        for b in range(5):
            for l in range(6):
                assert lib.wetts_mrd_band_width(r, b, l) == ws[b][l], (w, b, l)
    assert sum(v[5] for v in mo.band_widths(2048)) == 130 and sum(v[5] for v in mo.band_widths(512)) == 34


def test_fmap_shapes_are_the_oracles_for_every_frame_count():
    """Frame counts 1 + T // hop for T = 1025 .. 1025 + 2048 against torch.stft's own count and the library's shapes."""
    net = MultiPeriodMultiResolutionDiscriminator
    seen = set()
    for T in range(1025, 1025 + 2048 + 1):
        key = tuple(mo.frames(w, T) for w in mo.WINDOWS)
        if key in seen and T % 257:
            continue
        seen.add(key)
        shapes = net.fmap_shapes(1, T)
        assert len(shapes) == mo.N_MAPS
        for r, w in enumerate(mo.WINDOWS):
            fr = (T + 2 * (w // 2) - w) // (w // 4) + 1  # torch.stft, center=True
            assert fr == mo.frames(w, T)
            ws = mo.band_widths(w)
            for b in range(5):
                for l in range(1, 5):
                    assert shapes[mo.map_index(r, 4 * b + l - 1)] == (2, 32, fr, ws[b][l + 1]), (T, r, b, l)
            assert shapes[mo.map_index(r, 20)] == (2, 1, fr, sum(v[5] for v in ws))
    mpd = MultiPeriodDiscriminator.fmap_shapes(1, 2310)
    assert net.fmap_shapes(1, 2310)[63:] == mpd[7:]


def test_edge_shape_straddles_the_column_tile():
    B, T = mo.EDGE
    assert mo.edge_case(1, T) == (True, True)  # a row alone: one short of and one past a multiple of the tile
    counts = [2 * B * mo.frames(w, T) * ws[l] % mo.TILE for w in mo.WINDOWS for ws in mo.band_widths(w) for l in range(1, 6)]
    assert mo.TILE - 2 in counts and 2 in counts  # the forward pass: 2B rows make every count even


# ---- the oracle ------------------------------------------------------------------------------------------------------
def test_float64_oracle_stft_is_torch_stft():
    x = mo.normalize(mo.inputs(2, 3000, 3)[0][:, 0].double())
    for w in mo.WINDOWS:
        ref = torch.stft(x, w, w // 4, w, window=torch.hann_window(w, dtype=torch.float64), center=True, pad_mode="reflect",
                         normalized=False, onesided=True, return_complex=True)
        ref = torch.view_as_real(ref).transpose(1, 3)
        got = mo.spectrogram(x, w)
        assert got.shape == ref.shape == (2, 2, mo.frames(w, 3000), w // 2 + 1)
        assert float((got - ref).abs().max()) < 1e-11 * float(ref.abs().max())
        assert float(got[:, 1, :, 0].abs().max()) < 1e-11 and float(got[:, 1, :, -1].abs().max()) < 1e-11


@pytest.mark.parametrize("B,T", mo.FIXTURE_SHAPES)
def test_float64_oracle_reproduces_the_reference_fixture(B, T):
    """The regenerated weights' digest first; then what the reference computed at float32 against the float64 oracle,
    one floor (of the GEMM form, which bounds the FFT form's) away at most -- held to the fixture gate."""
    sd, _, _ = _weights()
    c = np.load(fixture_path(B, T))
    assert state_dict_digest(sd) == str(c["state_dict_sha256"]) and int(c["weight_seed"]) == mo.WSEED
    y, y_hat, maps, _, ls = mo.reference(B, T)
    assert np.array_equal(y.numpy(), c["y"]) and np.array_equal(y_hat.numpy(), c["y_hat"])
    y_d_rs, y_d_gs, fmap_rs, _ = mo.reference_form(maps, B)
    for d in range(8):
        g = mo.fixture_gate(mo.POSTS[d])
        for ref, nm in ((y_d_rs[d], f"y_d_r_{d}"), (y_d_gs[d], f"y_d_g_{d}")):
            assert tuple(ref.shape) == c[nm].shape, nm
            rel, loc = mo.gates(torch.from_numpy(c[nm]), ref.contiguous())
            assert rel <= g[0] and loc <= g[1], (nm, rel, loc, g)
    g = mo.fixture_gate(mo.map_index(2, 1))
    rel, loc = mo.gates(torch.from_numpy(c["fmap_r_2_1"]), fmap_rs[2][1].contiguous())
    assert rel <= g[0] and loc <= g[1], (rel, loc, g)
    for nm, key in (("layer_means", "layer_means"), ("loss_fm", "fm"), ("loss_disc", "disc"), ("losses_disc_r", "disc_r"),
                    ("losses_disc_g", "disc_g"), ("loss_gen", "gen"), ("losses_gen", "gen_terms")):
        assert mo.scalar_err(torch.from_numpy(np.asarray(c[nm])), ls[key]) <= mo.fixture_gate(key), nm


def test_committed_floor_is_the_measured_one():
    """The constants are the worst over all five shapes; recomputed over the two smallest they may only be smaller, and
    not by much: none above 2 x, most within 8 x."""
    now = mo.floor(SMALL)
    for i, (a, b) in enumerate(zip(now["maps"], mo.FLOOR["maps"])):
        assert a[0] <= 2 * b[0] and a[1] <= 2 * b[1], (i, a, b)
    for s in mo.STAGES:
        assert now[s][0] <= 2 * mo.FLOOR[s][0] and now[s][1] <= 2 * mo.FLOOR[s][1], (s, now[s], mo.FLOOR[s])
    for s in mo.SCALARS:
        assert now[s] <= 2 * mo.FLOOR[s], (s, now[s], mo.FLOOR[s])
    assert sum(8 * a[0] >= b[0] and 8 * a[1] >= b[1] for a, b in zip(now["maps"], mo.FLOOR["maps"])) >= 85
    assert all(8 * now[s][0] >= mo.FLOOR[s][0] for s in mo.STAGES)


@pytest.mark.parametrize("fault", mo.FAULTS)
def test_gates_see_the_faults(fault):
    """Each defect, injected into the float32 oracle, exceeds the gate of the stage it first touches."""
    _, W32, _ = _weights()
    B, T = 2, 1536
    y, y_hat, ref_maps, ref_stages, ref_ls = mo.reference(B, T)
    maps, stages = mo.forward(W32, y, y_hat, fault)
    cmaps, cstages = _W.setdefault("clean", mo.forward(W32, y, y_hat))
    i = mo.FAULT_STAGE[fault]
    pick = (lambda m, s: m[i]) if isinstance(i, int) else (lambda m, s: s[i])
    ref = pick(ref_maps, ref_stages).contiguous()
    rel, loc = mo.gates(pick(maps, stages).contiguous(), ref)
    g = mo.gate(i)
    assert rel > g[0] and loc > g[1], (fault, i, rel, loc, g)
    clean = mo.gates(pick(cmaps, cstages).contiguous(), ref)
    assert clean[0] <= g[0] and clean[1] <= g[1]
    with pytest.raises(AssertionError):
        mo.check(mo.measure(maps, stages, mo.losses(maps, B), ref_maps, ref_stages, ref_ls))
