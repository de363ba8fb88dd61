"""CPU tier of MultiPeriodDiscriminator: the blob layout against the reference's own state_dict, packing, the host-side
checks, the float64 / float32 oracle of tests/disc_oracle.py against the live reference and its fixtures, and the
sensitivity of the gates (a gate that a dropped tap passes would be vacuous)."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_import
from tests import disc_oracle as do
from wetts_amd import MultiPeriodDiscriminator, _lib, checkpoint, discriminators, losses, models, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = do.SHAPES[:4]  # the 8192-sample case is the GPU tier's
_W = {}


def fixture_path(B, T):
    return os.path.join(ROOT, "tests", "golden", f"disc_b{B}x{T}.npz")


def state_dict_digest(sd):
    """sha256 over the keys in order and each tensor's float32 bytes (tests/golden/make_golden_disc.py)."""
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().to(torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()


def _weights():
    if not _W:
        _W["sd"], _W["W32"], _W["W64"] = do.weights()
    return _W["sd"], _W["W32"], _W["W64"]


# ---- layout and packing ----------------------------------------------------------------------------------------------
def test_layout_is_the_fixed_architecture():
    lay = checkpoint.disc_layout()
    assert len(lay) == 74 and len({n for n, *_ in lay}) == 74
    end = 0
    for n, off, numel, shape in lay:
        assert off >= end and off % 64 == 0 and numel == int(np.prod(shape)), n
        end = off + numel
    assert checkpoint.disc_numel() >= end
    assert sum(numel for _, _, numel, _ in lay) == 46730118  # ~46.7 M floats
    shapes = dict((n, s) for n, _, _, s in lay)
    assert shapes["discriminators.0.convs.1.weight"] == (64, 4, 41)
    assert shapes["discriminators.5.convs.3.weight"] == (1024, 512, 5, 1)
    assert shapes["discriminators.3.conv_post.weight"] == (1, 1024, 3, 1)


@pytest.mark.skipif(not ref_import.available(), reason="the reference is not on this machine")
def test_layout_matches_a_live_reference_state_dict():
    from tests.golden.make_golden_disc import import_reference
    MPD, _ = import_reference()
    ref = MPD(False).state_dict()
    assert len(ref) == 111
    folded = checkpoint.fold_weight_norm(ref)
    lay = checkpoint.disc_layout()
    assert {n for n, *_ in lay} == set(folded)
    for n, _, _, shape in lay:
        assert tuple(folded[n].shape) == shape, n


def test_packing_round_trips_and_both_spellings_fold_to_one_blob():
    sd, W32, _ = _weights()
    assert len(sd) == 111
    blob = checkpoint.pack_disc_blob(sd)
    for n, off, numel, shape in checkpoint.disc_layout():
        assert torch.equal(blob[off:off + numel].reshape(shape), W32[n]), n
    new = {}
    for k, v in sd.items():
        k = re.sub(r"\.weight_g$", ".parametrizations.weight.original0", k)
        new[re.sub(r"\.weight_v$", ".parametrizations.weight.original1", k)] = v
    assert set(new) != set(sd) and torch.equal(checkpoint.pack_disc_blob(new), blob)
    assert torch.equal(checkpoint.pack_disc_blob(W32), blob)  # already folded
    net = MultiPeriodDiscriminator().load_state_dict(sd)
    back = net.state_dict()
    assert set(back) == set(W32) and all(torch.equal(back[k], W32[k]) for k in W32)
    short = dict(sd)
    del short["discriminators.4.convs.2.bias"]
    with pytest.raises(KeyError, match="discriminators.4.convs.2.bias"):
        checkpoint.pack_disc_blob(short)
    bad = dict(sd)
    bad["discriminators.4.convs.2.bias"] = torch.zeros(3)
    with pytest.raises(ValueError):
        checkpoint.pack_disc_blob(bad)


def test_load_checkpoint_reads_a_discriminator_file(tmp_path):
    sd, W32, _ = _weights()
    path = str(tmp_path / "D_7.pth")
    torch.save({"model": sd, "iteration": 7, "optimizer": None, "learning_rate": 2e-4}, path)
    net, _, lr, it = models.load_checkpoint(path, MultiPeriodDiscriminator())
    assert it == 7 and lr == 2e-4 and torch.equal(net.state_dict()["discriminators.2.convs.1.weight"],
                                                   W32["discriminators.2.convs.1.weight"])


def test_synthetic_weights_keep_activations_of_order_one():
    _, W32, _ = _weights()
    y, y_hat = do.inputs(2, 700, 1)
    for i, m in enumerate(do.forward(W32, y, y_hat)):
        r = float(m.pow(2).mean().sqrt())
        assert 0.05 < r < 20, (i, r)


# ---- host checks -----------------------------------------------------------------------------------------------------
def test_host_side_checks_need_no_device():
    with pytest.raises(NotImplementedError, match="spectral"):
        MultiPeriodDiscriminator(use_spectral_norm=True)
    net = MultiPeriodDiscriminator()
    y = torch.zeros(2, 1, 64)
    with pytest.raises(ValueError, match="HIP device"):
        net(y, y)
    with pytest.raises(ValueError, match=r"\[B, 1, T\]"):
        net(torch.zeros(2, 64), y)
    with pytest.raises(ValueError):
        net.to("cpu")
    with pytest.raises(RuntimeError, match="no weights"):
        net.state_dict()
    for fn, args in ((losses.feature_loss, ([[y]], [[y]])), (losses.discriminator_loss, ([y], [y])),
                     (losses.generator_loss, ([y],))):
        with pytest.raises(ValueError, match="HIP device"):
            fn(*args)
    with pytest.raises(ValueError):
        losses.discriminator_loss([y], [y, y])
    with pytest.raises(ValueError, match="go together"):
        losses.teacher_forced_losses(None, type("H", (), {"data": None})(), None, None, None, None, y=y)


def test_shortest_legal_length_is_what_reflect_padding_allows():
    """F.pad(..., "reflect") needs n_pad < T for every period that does not divide T."""
    def legal(T):
        try:
            for p in do.PERIODS:
                if T % p:
                    F.pad(torch.zeros(1, 1, T), (0, p - T % p), "reflect")
            return True
        except RuntimeError:
            return False
    assert [T for T in range(1, 122) if not legal(T)] == list(range(1, discriminators.MIN_SAMPLES))
    lib = _lib.load()
    assert lib.wetts_disc_forward(None, None, None, 1, 64, None, None) == -1  # null arguments: refused, no launch


def test_fmap_shapes_are_the_oracles():
    _, W32, _ = _weights()
    for B, T in ((1, 6), (1, 12), (2, 64), (2, 700)):
        y, y_hat = do.inputs(B, T, 3)
        maps = do.forward(W32, y, y_hat)
        for i, ((rows, C, H, p), m) in enumerate(zip(MultiPeriodDiscriminator.fmap_shapes(B, T), maps)):
            want = (2 * B, C, H) if i < 7 else (2 * B, C, H, p)
            assert tuple(m.shape) == want and rows == 2 * B * p, (B, T, i, tuple(m.shape), (rows, C, H, p))


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", do.FIXTURE_SHAPES)
def test_float32_oracle_reproduces_the_reference_fixture(B, T):
    """The regenerated weights' digest first; then the oracle at float32 against what the reference computed, under
    the gates (both are float32 evaluations of one function)."""
    sd, W32, _ = _weights()
    c = np.load(fixture_path(B, T))
    assert state_dict_digest(sd) == str(c["state_dict_sha256"]) and int(c["weight_seed"]) == do.WSEED
    y, y_hat = do.inputs(B, T, do.case_seed(B, T))
    assert np.array_equal(y.numpy(), c["y"]) and np.array_equal(y_hat.numpy(), c["y_hat"])
    maps = do.forward(W32, y, y_hat)
    y_d_rs, y_d_gs, fmap_rs, _ = do.reference_form(maps, B)
    for d in range(6):
        g = do.fixture_gate(do.map_index(d, 6 if d == 0 else 5))
        for got, nm in ((y_d_rs[d], f"y_d_r_{d}"), (y_d_gs[d], f"y_d_g_{d}")):
            rel, loc = do.gates(got.contiguous(), torch.from_numpy(c[nm]))
            assert rel <= g[0] and loc <= g[1], (nm, rel, loc, g)
    rel, loc = do.gates(fmap_rs[5][0].contiguous(), torch.from_numpy(c["fmap_r_5_0"]))
    assert rel <= do.fixture_gate(do.map_index(5, 0))[0] and loc <= do.fixture_gate(do.map_index(5, 0))[1]
    ls = do.losses(maps, B)
    for nm, key in (("layer_means", "layer_means"), ("loss_fm", "fm"), ("loss_disc", "disc"), ("losses_disc_r", "disc_r"),
                    ("losses_disc_g", "disc_g"), ("loss_gen", "gen"), ("losses_gen", "gen_terms")):
        assert do.scalar_err(ls[key], torch.from_numpy(np.asarray(c[nm]))) <= do.fixture_gate(key), nm


@pytest.mark.skipif(not ref_import.available(), reason="the reference is not on this machine")
def test_float32_oracle_equals_the_live_reference():
    from tests.golden.make_golden_disc import build_reference, run_reference
    sd, W32, _ = _weights()
    net, ref_losses = build_reference(sd)
    B, T = 2, 700
    y, y_hat = do.inputs(B, T, 11)
    ry_d_rs, ry_d_gs, rfr, rfg, _ = run_reference(net, ref_losses, y, y_hat)
    y_d_rs, y_d_gs, fr, fg = do.reference_form(do.forward(W32, y, y_hat), B)
    for d in range(6):
        assert tuple(y_d_rs[d].shape) == tuple(ry_d_rs[d].shape)
        for k, (a, r) in enumerate(zip(fr[d] + fg[d], rfr[d] + rfg[d])):
            assert tuple(a.shape) == tuple(r.shape), (d, k)
            g = do.gate(do.map_index(d, k % len(fr[d])))
            rel, loc = do.gates(a.contiguous(), r.contiguous())
            assert rel <= g[0] and loc <= g[1], (d, k, rel, loc, g)


def test_committed_floor_is_the_measured_one():
    """The constants are held to 1/2 .. 2 x of the floor recomputed here over the shapes the CPU tier can afford; the
    committed figure is the worst over all five shapes, so it may only be the larger."""
    now = do.floor(SMALL)
    for i, (a, b) in enumerate(zip(now["maps"], do.FLOOR["maps"])):
        assert a[0] <= 2 * b[0] and a[1] <= 2 * b[1], (i, a, b)
    for s in do.SCALARS:
        assert now[s] <= 2 * do.FLOOR[s], (s, now[s], do.FLOOR[s])
    assert sum(a[0] >= 0.5 * b[0] for a, b in zip(now["maps"], do.FLOOR["maps"])) >= 30


@pytest.mark.parametrize("fault", do.FAULTS)
def test_gates_see_the_faults(fault):
    """Each fault, applied to the float32 oracle, exceeds the gate of the map it first touches (and so would fail
    do.check) at a shape of the sweep."""
    _, W32, _ = _weights()
    B, T = 2, 700
    y, y_hat, ref_maps, ref_ls = do.reference(B, T)
    maps = do.forward(W32, y, y_hat, fault)
    i = do.FAULT_STAGE[fault]
    rel, loc = do.gates(maps[i].contiguous(), ref_maps[i].contiguous())
    g = do.gate(i)
    assert rel > g[0] and loc > g[1], (fault, i, rel, loc, g)
    clean = do.gates(do.forward(W32, y, y_hat)[i].contiguous(), ref_maps[i].contiguous())
    assert clean[0] <= g[0] and clean[1] <= g[1]
    with pytest.raises(AssertionError):
        do.check(do.measure(maps, do.losses(maps, B), ref_maps, ref_ls))
