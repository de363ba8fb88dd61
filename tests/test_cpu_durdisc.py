"""CPU tier of the VITS2 duration discriminators: the blob layout against the reference's own state_dict, packing, the
factory against train.py's three cases, the host-side checks, the float64 / float32 oracle of tests/durdisc_oracle.py
against the live reference and its fixtures, and the sensitivity of the gates (a gate that a dropped tap passes would be
vacuous)."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_import
from tests import durdisc_oracle as dd
from tests.test_cpu_disc import state_dict_digest
from wetts_amd import (DurationDiscriminatorV1, DurationDiscriminatorV2, _lib, checkpoint, config, discriminators,
                       duration_discriminator_from_hparams, losses, models, synth)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = (dd.CHANNELS, dd.CHANNELS, dd.KERNEL)


def fixture_path(version, B, Tx):
    return os.path.join(ROOT, "tests", "golden", f"durdisc_v{version}_b{B}x{Tx}.npz")


def _cls(version):
    return DurationDiscriminatorV1 if version == 1 else DurationDiscriminatorV2


# ---- layout and packing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", dd.VERSIONS)
def test_layout_and_pack_round_trip(version):
    lay = checkpoint.durdisc_layout(version, *CFG)
    assert len(lay) == (12 if version == 1 else 20) and len({n for n, *_ in lay}) == len(lay)
    end = 0
    for n, off, numel, shape in lay:
        assert off >= end and off % 64 == 0 and numel == int(np.prod(shape)), n
        end = off + numel
    assert checkpoint.durdisc_numel(version, *CFG) >= end
    shapes = dict((n, s) for n, _, _, s in lay)
    assert shapes["conv_1.weight"] == (192, 192, 3) and shapes["pre_out_conv_1.weight"] == (192, 384, 3)
    assert shapes["dur_proj.weight"] == (192, 1, 1) and shapes["output_layer.0.weight"] == (1, 192)
    assert shapes["output_layer.0.bias"] == (1,) and ("norm_2.gamma" in shapes) == (version == 2)
    sd = dd.weights(version)[0]
    blob = checkpoint.pack_durdisc_blob(version, *CFG, sd)
    for n, off, numel, shape in lay:
        assert torch.equal(blob[off:off + numel].reshape(shape), sd[n]), n
    net = _cls(version)(*CFG, 0.1).load_state_dict(sd)
    back = net.state_dict()
    assert set(back) == set(shapes) and all(torch.equal(back[k], sd[k]) for k in back)
    short = dict(sd)
    del short["pre_out_conv_2.bias"]
    with pytest.raises(KeyError, match="pre_out_conv_2.bias"):
        checkpoint.pack_durdisc_blob(version, *CFG, short)
    bad = dict(sd, **{"dur_proj.weight": torch.zeros(192)})
    with pytest.raises(ValueError):
        checkpoint.pack_durdisc_blob(version, *CFG, bad)


def test_v1_accepts_and_ignores_the_norms_it_never_reads():
    sd = dd.weights(1)[0]
    assert "pre_out_norm_1.gamma" in sd and "pre_out_norm_2.beta" in sd  # as a DUR_*.pth of the class holds them
    net = DurationDiscriminatorV1(*CFG, 0.1).load_state_dict(sd)
    assert not any("norm" in k for k in net.state_dict())
    other = dict(sd, **{"pre_out_norm_1.gamma": torch.full((192,), 7.0)})
    assert torch.equal(DurationDiscriminatorV1(*CFG, 0.1).load_state_dict(other)._blob, net._blob)
    without = {k: v for k, v in sd.items() if "norm" not in k}
    assert torch.equal(DurationDiscriminatorV1(*CFG, 0.1).load_state_dict(without)._blob, net._blob)


@pytest.mark.skipif(not ref_import.available(), reason="the reference is not on this machine")
@pytest.mark.parametrize("version", dd.VERSIONS)
def test_layout_matches_a_live_reference_state_dict(version):
    from tests.golden.make_golden_durdisc import import_reference
    ref = import_reference()[version - 1](*CFG, 0.1, gin_channels=0).state_dict()
    assert set(ref) == set(dd.weights(version)[0])  # the synthetic checkpoint has the class's own keys
    for n, _, _, shape in checkpoint.durdisc_layout(version, *CFG):
        assert tuple(ref[n].shape) == shape, n
    used = {n for n, *_ in checkpoint.durdisc_layout(version, *CFG)}
    assert set(ref) - used == ({"pre_out_norm_1.gamma", "pre_out_norm_1.beta", "pre_out_norm_2.gamma",
                                "pre_out_norm_2.beta"} if version == 1 else set())


def test_load_checkpoint_reads_a_duration_discriminator_file(tmp_path):
    sd = dd.weights(2)[0]
    path = str(tmp_path / "DUR_7.pth")
    torch.save({"model": sd, "iteration": 7, "optimizer": None, "learning_rate": 2e-4}, path)
    net, _, lr, it = models.load_checkpoint(path, DurationDiscriminatorV2(*CFG, 0.1))
    assert it == 7 and lr == 2e-4 and torch.equal(net.state_dict()["norm_1.beta"], sd["norm_1.beta"])


def test_synthetic_weights_are_deterministic_and_do_not_saturate_the_sigmoid():
    for version in dd.VERSIONS:
        a, b = (synth.make_duration_discriminator_state_dict(version, 3) for _ in range(2))
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
        for B, Tx, lens in dd.SHAPES[2:]:
            inp, st, _ = dd.reference(version, B, Tx, lens)
            p = st["prob"][torch.cat([inp[1][:, 0], inp[1][:, 0]], 0) > 0]
            assert float(((p > 0.05) & (p < 0.95)).double().mean()) >= 0.95, (version, B, Tx)
    with pytest.raises(ValueError):
        synth.make_duration_discriminator_state_dict(3)


# ---- the factory and the host checks ---------------------------------------------------------------------------------
def test_factory_mirrors_train_py():
    def hps(n_speakers=0, **model):
        return config.HParams(data=dict(n_speakers=n_speakers), model=dict(hidden_channels=192, gin_channels=256, **model))
    assert duration_discriminator_from_hparams(hps()) is None
    assert duration_discriminator_from_hparams(hps(use_duration_discriminator=False)) is None
    net = duration_discriminator_from_hparams(hps(use_duration_discriminator=True))
    assert type(net) is DurationDiscriminatorV1  # train.py:135-137: the default type is "dur_disc_1"
    assert (net.in_channels, net.filter_channels, net.kernel_size, net.p_dropout, net.gin_channels) == (192, 192, 3, 0.1, 0)
    net = duration_discriminator_from_hparams(hps(4, use_duration_discriminator=True, duration_discriminator_type="dur_disc_2"))
    assert type(net) is DurationDiscriminatorV2 and net.gin_channels == 256
    with pytest.raises(AssertionError):
        duration_discriminator_from_hparams(hps(use_duration_discriminator=True, duration_discriminator_type="dur_disc_3"))
    assert discriminators.AVAILABLE_DURATION_DISCRIMINATOR_TYPES == ("dur_disc_1", "dur_disc_2")


def test_host_side_checks_need_no_device():
    for bad in ((100, 192, 3), (192, 288, 3), (192, 192, 4), (192, 192, 9), (0, 192, 3)):
        with pytest.raises(ValueError, match="not supported"):  # no slow path: refused at create
            DurationDiscriminatorV1(*bad, 0.1)
    net = DurationDiscriminatorV2(*CFG, 0.1, gin_channels=256)
    assert net.eval() is net and net.train(False) is net
    with pytest.raises(NotImplementedError):
        net.train()
    with pytest.raises(ValueError):
        net.to("cpu")
    with pytest.raises(RuntimeError, match="no weights"):
        net.state_dict()
    x, m, dr, dh = dd.inputs(2, 5, (5, 2), 1)
    with pytest.raises(ValueError, match="HIP device"):
        net(x, m, dr, dh)
    with pytest.raises(ValueError, match=r"\[B, 192, Tx\]"):
        net(x[:, :32], m, dr, dh)
    with pytest.raises(ValueError, match="dur_hat"):
        net(x, m, dr, dh[:, :, :4])
    with pytest.raises(ValueError, match="with_duration"):
        losses.teacher_forced_losses(None, type("H", (), {"data": None})(), None, None, None, None, net_dur_disc=net)
    lib = _lib.load()
    assert lib.wetts_durdisc_forward(None, None, None, None, None, 1, 5, None, 0, None) == -1  # refused, no launch
    assert lib.wetts_durdisc_workspace_bytes(None, 1, 5) < 0 and lib.wetts_abi_version() == 12


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", dd.VERSIONS)
@pytest.mark.parametrize("B,Tx,lens", dd.FIXTURE_SHAPES)
def test_float32_oracle_reproduces_the_reference_fixture(version, B, Tx, lens):
    from tests.golden.make_golden_durdisc import inputs_digest
    sd = dd.weights(version)[0]
    c = np.load(fixture_path(version, B, Tx))
    assert state_dict_digest(sd) == str(c["state_dict_sha256"]) and int(c["weight_seed"]) == dd.WSEED
    inp = dd.inputs(B, Tx, lens, int(c["input_seed"]))
    assert int(c["input_seed"]) == dd.case_seed(B, Tx) and inputs_digest(inp) == str(c["inputs_sha256"])
    st = dd.forward(sd, version, *inp)
    form = dd.reference_form(st["prob"], version)
    g = dd.fixture_gate(version, "prob")
    for got, nm in ((form[0], "prob_r"), (form[1], "prob_g")):
        got = got if version == 1 else got[0]
        rel, loc = dd.gates(got.contiguous(), torch.from_numpy(c[nm]))
        assert rel <= g[0] and loc <= g[1], (nm, rel, loc, g)
    ls = dd.losses(st["prob"], inp[1], version)
    for nm, key in (("loss_dur_disc", "disc"), ("losses_dur_disc_r", "disc_r"), ("losses_dur_disc_g", "disc_g"),
                    ("loss_dur_gen", "gen"), ("losses_dur_gen", "gen_terms")):
        want = torch.from_numpy(np.asarray(c[nm]))
        assert want.numel() == ls[key].numel() == (1 if key in ("disc", "gen") or version == 2 else B), nm
        assert dd.scalar_err(ls[key], want) <= dd.fixture_gate(version, key), nm
    if version == 1 and B > 1:  # trap 1: the reference's zip walks the batch rows, B x the one-mean value
        one = dd.losses(st["prob"], inp[1], 1, one_mean=True)
        assert abs(float(c["loss_dur_disc"]) - B * float(one["disc"])) <= 1e-5 * float(c["loss_dur_disc"])


@pytest.mark.skipif(not ref_import.available(), reason="the reference is not on this machine")
@pytest.mark.parametrize("version", dd.VERSIONS)
def test_float32_oracle_equals_the_live_reference(version):
    from tests.golden.make_golden_durdisc import build_reference, run_reference
    sd = dd.weights(version)[0]
    net, ref_losses = build_reference(version, sd)
    B, Tx, lens = 4, 37, (37, 20, 1, 9)
    inp = dd.inputs(B, Tx, lens, 11)
    y_r, y_g, sc = run_reference(net, ref_losses, *inp)
    st = dd.forward(sd, version, *inp)
    form = dd.reference_form(st["prob"], version)
    assert type(form[0]) is type(y_r) and (version == 1 or len(y_r) == len(form[0]) == 1)
    g = dd.gate(version, "prob")
    for a, r in zip(form, (y_r, y_g)):
        a, r = (a, r) if version == 1 else (a[0], r[0])
        assert tuple(a.shape) == tuple(r.shape) == (B, Tx, 1)
        rel, loc = dd.gates(a.contiguous(), r.contiguous())
        assert rel <= g[0] and loc <= g[1], (rel, loc, g)
    assert len(sc["losses_dur_disc_r"]) == len(sc["losses_dur_gen"]) == (B if version == 1 else 1)


@pytest.mark.parametrize("version", dd.VERSIONS)
def test_committed_floor_is_the_measured_one(version):
    """The constants are held to at most 2 x the floor recomputed here, and most of them to at least half of it (the
    float32 CPU kernels of another processor round differently)."""
    now = dd.floor(version)
    for s in dd.STAGES:
        a, b = now[s], dd.FLOOR[version][s]
        assert a[0] <= 2 * b[0] and a[1] <= 2 * b[1], (s, a, b)
    assert sum(now[s][0] >= 0.5 * dd.FLOOR[version][s][0] for s in dd.STAGES) >= 3
    for s in dd.SCALARS:
        assert now[s] <= 2 * dd.FLOOR[version][s], (s, now[s], dd.FLOOR[version][s])


@pytest.mark.parametrize("fault", dd.FAULTS)
def test_gates_see_the_faults(fault):
    """Each fault, applied to the float32 oracle, exceeds the gate of the stage it first touches (and so fails dd.check)
    at a shape of the sweep; the clean float32 oracle passes there."""
    B, Tx, lens = dd.SHAPES[2]
    for version in dd.FAULT_VERSIONS[fault]:
        W32 = dd.weights(version)[0]
        inp, ref_st, ref_ls = dd.reference(version, B, Tx, lens)
        st = dd.forward(W32, version, *inp, fault=fault)
        s = dd.FAULT_STAGE[fault]
        rel, loc = dd.gates(st[s].contiguous(), ref_st[s].contiguous())
        g = dd.gate(version, s)
        assert rel > g[0] and loc > g[1], (fault, version, s, rel, loc, g)
        clean = dd.forward(W32, version, *inp)
        rel, loc = dd.gates(clean[s].contiguous(), ref_st[s].contiguous())
        assert rel <= g[0] and loc <= g[1]
        with pytest.raises(AssertionError):
            dd.check(version, dd.measure(st, dd.losses(st["prob"], inp[1], version), ref_st, ref_ls))
        dd.check(version, dd.measure(clean, dd.losses(clean["prob"], inp[1], version), ref_st, ref_ls))


def test_gates_see_a_v1_loss_formed_as_one_mean():
    B, Tx, lens = dd.SHAPES[2]
    inp, ref_st, ref_ls = dd.reference(1, B, Tx, lens)
    prob = dd.forward(dd.weights(1)[0], 1, *inp)["prob"]
    one = dd.losses(prob, inp[1], 1, one_mean=True)
    for s in ("disc", "gen"):
        assert dd.scalar_err(one[s], ref_ls[s]) > dd.gate(1, s), s  # off by the factor B
        assert dd.scalar_err(dd.losses(prob, inp[1], 1)[s], ref_ls[s]) <= dd.gate(1, s), s
    assert one["disc_r"].numel() == 1 and ref_ls["disc_r"].numel() == B
