"""GPU tier of DurationDiscriminatorV1 / V2 and their losses (csrc/duration_disc.hip): the reference's fixtures
(tests/golden/durdisc_*.npz), every stage and every scalar against the float64 oracle of tests/durdisc_oracle.py under the
gates defined there (4 x the float32 oracle's own distance from float64), the bit-exact conditions (a row alone, the
pairing, repeats, wetts_durdisc_layer on a cut-out row), the masked positions, the returned structures, and
teacher_forced_losses(net_dur_disc=).  The tile is 64 columns: the shapes of durdisc_oracle.SHAPES put row joins, a
one-phoneme row, an empty row and a ragged last tile inside it."""
import os

import numpy as np
import pytest
import torch

from tests import align_oracle as ao, durdisc_oracle as dd, util
from tests.golden.make_golden_durdisc import inputs_digest
from tests.test_cpu_disc import state_dict_digest
from tests.test_cpu_durdisc import fixture_path
from wetts_amd import (DurationDiscriminatorV1, DurationDiscriminatorV2, SynthesizerTrn, _lib, config, losses, synth)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPEC = ao.SPEC
_NET = {}
_MARGINS = {}
_KEYS = dict(disc="loss_dur_disc", disc_r="losses_dur_disc_r", disc_g="losses_dur_disc_g", gen="loss_dur_gen",
             gen_terms="losses_dur_gen", disc_per_utt="dur_disc_per_utt", gen_per_utt="dur_gen_per_utt")


@pytest.fixture(scope="module", autouse=True)
def _release_and_report():
    yield
    import gc
    _NET.clear()
    dd._REF.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = os.environ.get("WETTS_DURDISC_MARGINS")  # the GPU run that records profiles/durdisc_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst multiple of a gate per case (1 = at the gate; gate = 4 x floor), then the figures\n")
            for k in sorted(_MARGINS):
                f.write(f"{k}: {_MARGINS[k]}\n")


def _net(version):
    if version not in _NET:
        cls = DurationDiscriminatorV1 if version == 1 else DurationDiscriminatorV2
        _NET[version] = cls(dd.CHANNELS, dd.CHANNELS, dd.KERNEL, 0.1).load_state_dict(dd.weights(version)[0]).to(DEV)
    return _NET[version]


def _run(version, inp):
    """-> ({stage: device tensor}, {oracle scalar name: device tensor}) of one case."""
    net = _net(version)
    x, m, dr, dh = (t.to(DEV) for t in inp)
    st = dict(zip(dd.STAGES, net._run(x, m, dr, dh)))
    out = losses._duration_disc_losses(net, x, m, dr, dh)
    torch.cuda.synchronize()
    return st, {k: out[v] for k, v in _KEYS.items()}


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", dd.VERSIONS)
@pytest.mark.parametrize("B,Tx,lens", dd.FIXTURE_SHAPES)
def test_matches_reference_fixture(version, B, Tx, lens):
    """First the regenerated weights' and inputs' digests (a torch RNG change shows as that, not as a parity failure);
    then both probability tensors and the three losses with their term lists, as the reference's zip produced them."""
    c = np.load(fixture_path(version, B, Tx))
    assert state_dict_digest(dd.weights(version)[0]) == str(c["state_dict_sha256"])
    inp = dd.inputs(B, Tx, lens, int(c["input_seed"]))
    assert inputs_digest(inp) == str(c["inputs_sha256"]) and tuple(c["lens"]) == tuple(lens)
    st, ls = _run(version, inp)
    rows = {}
    g = dd.fixture_gate(version, "prob")
    for nm, got in (("prob_r", st["prob"][:B]), ("prob_g", st["prob"][B:])):
        rows[nm] = dd.gates(got.cpu().unsqueeze(2), torch.from_numpy(c[nm]))
        assert rows[nm][0] <= g[0] and rows[nm][1] <= g[1], (nm, rows[nm], g)
    for nm, key in (("loss_dur_disc", "disc"), ("losses_dur_disc_r", "disc_r"), ("losses_dur_disc_g", "disc_g"),
                    ("loss_dur_gen", "gen"), ("losses_dur_gen", "gen_terms")):
        want = torch.from_numpy(np.asarray(c[nm]))
        assert ls[key].numel() == want.numel() == (1 if key in ("disc", "gen") or version == 2 else B), nm
        rows[nm] = dd.scalar_err(ls[key].cpu(), want)
        assert rows[nm] <= dd.fixture_gate(version, key), (nm, rows[nm], dd.fixture_gate(version, key))
    print(f"durdisc fixture v{version} b{B}x{Tx}:", rows)


# ---- 2. every stage against the float64 oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("version", dd.VERSIONS)
@pytest.mark.parametrize("B,Tx,lens", dd.SHAPES)
def test_every_stage_against_float64_oracle(version, B, Tx, lens):
    inp, ref_st, ref_ls = dd.reference(version, B, Tx, lens)
    st, ls = _run(version, inp)
    m = dd.measure(st, ls, ref_st, ref_ls)
    fig = {k: (tuple(float(f"{a:.3g}") for a in v) if isinstance(v, tuple) else float(f"{v:.3g}")) for k, v in m.items()}
    print(f"durdisc v{version} b{B}x{Tx} vs float64:", fig)
    top = dd.check(version, m, f"v{version} b{B}x{Tx}")
    _MARGINS[f"v{version} b{B:02d}x{Tx:03d}"] = (round(top, 3), fig)


# (version, in_channels, filter_channels, kernel_size): the other forms of the kernel -- one, two (the second a zero-row
# tile: F / 32 odd), three and four 32-channel tiles per wave; 32, 8 and 4 input channels per chunk (k = 1, 5, 7);
# in_channels != filter_channels
OTHER_CONFIGS = ((1, 32, 32, 1), (2, 64, 96, 5), (1, 96, 160, 3), (2, 256, 256, 7))


@pytest.mark.parametrize("version,cin,F_,K", OTHER_CONFIGS)
def test_other_supported_configurations_against_float64_oracle(version, cin, F_, K):
    """The floors in durdisc_oracle.FLOOR belong to 192 channels and k = 3 (the length of the k sum sets them), so each
    configuration here is gated by 4 x ITS OWN floor: the float32 oracle against the float64 oracle on the same weights,
    the worst over the same two shapes the device then runs."""
    sd = synth.make_duration_discriminator_state_dict(version, 77, cin, F_, K)
    W64 = {k: v.to(torch.float64) for k, v in sd.items()}
    cls = DurationDiscriminatorV1 if version == 1 else DurationDiscriminatorV2
    net = cls(cin, F_, K, 0.1).load_state_dict(sd).to(DEV)
    cases = []
    for B, Tx, lens in dd.SHAPES[1:3]:
        inp = dd.inputs(B, Tx, lens, dd.case_seed(B, Tx) + K, channels=cin)
        cases.append((inp, dd.forward(W64, version, *inp), dd.forward(sd, version, *inp)))
    floor = {s: tuple(max(dd.gates(f32[s].contiguous(), ref[s].contiguous())[i] for _, ref, f32 in cases) for i in (0, 1))
             for s in dd.STAGES}
    top = 0.0
    for inp, ref, _ in cases:
        st = dict(zip(dd.STAGES, net._run(*(t.to(DEV) for t in inp))))
        torch.cuda.synchronize()
        fig = {s: dd.gates(st[s].cpu().contiguous(), ref[s].contiguous()) for s in dd.STAGES}
        print(f"durdisc v{version} {cin}->{F_} k{K} b{inp[0].shape[0]}x{inp[0].shape[2]}:", fig, "floor", floor)
        for s in dd.STAGES:
            assert fig[s][0] <= dd.GATE_FACTOR * floor[s][0] and fig[s][1] <= dd.GATE_FACTOR * floor[s][1], (s, fig[s], floor[s])
            top = max(top, fig[s][0] / floor[s][0] / dd.GATE_FACTOR, fig[s][1] / floor[s][1] / dd.GATE_FACTOR)
    _MARGINS[f"other v{version} {cin}->{F_} k{K}"] = (round(top, 3), floor)


# ---- 3. bit-exact conditions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", dd.VERSIONS)
def test_row_alone_pairing_and_repeats_are_bit_exact(version):
    B, Tx, lens = dd.SHAPES[3]
    inp = dd.inputs(B, Tx, lens, 4242)
    x, m, dr, dh = inp
    st, ls = _run(version, inp)
    st2, ls2 = _run(version, inp)
    for s in dd.STAGES:
        assert torch.equal(st[s], st2[s]), s
    for k in ls:
        assert torch.equal(torch.nan_to_num(ls[k], nan=-1.0), torch.nan_to_num(ls2[k], nan=-1.0)), k  # NaN: the empty row
    # the real half does not depend on what it is paired with
    st3, _ = _run(version, (x, m, dr, dr))
    for s in ("pre_out_conv_1", "pre_out_conv_2", "prob"):
        assert torch.equal(st3[s][:B], st[s][:B]) and torch.equal(st3[s][B:], st[s][:B]), s
    # a row alone, cut to its own length, equals the row in the padded batch at its own positions
    for b, n in enumerate(lens):
        if n == 0:
            continue
        st1, ls1 = _run(version, (x[b:b + 1, :, :n], m[b:b + 1, :, :n], dr[b:b + 1, :, :n], dh[b:b + 1, :, :n]))
        for s in ("conv_1", "conv_2"):
            assert torch.equal(st1[s][0], st[s][b, :, :n]), (b, s)
        for s in ("pre_out_conv_1", "pre_out_conv_2", "prob"):
            assert torch.equal(st1[s][0], st[s][b, ..., :n]) and torch.equal(st1[s][1], st[s][B + b, ..., :n]), (b, s)
        for k in ("disc_per_utt", "gen_per_utt"):
            assert torch.equal(ls1[k][0], ls[k][b]), (b, k)
    assert bool(torch.isnan(ls["disc_per_utt"][1])) and bool(torch.isnan(ls["gen_per_utt"][1]))  # the empty utterance


@pytest.mark.parametrize("version", dd.VERSIONS)
def test_layer_entry_on_a_cut_out_row_gives_the_batch_bits(version):
    B, Tx, lens = dd.SHAPES[2]
    inp = dd.inputs(B, Tx, lens, 4243)
    net = _net(version)
    x, m, dr, dh = (t.to(DEV).contiguous() for t in inp)
    t1, t2, h1, h2, prob = net._run(x, m, dr, dh)
    lib, h, s = _lib.load(), net._handle, _lib.current_stream_ptr()
    for b in range(B):
        mb = m[b:b + 1].contiguous()
        out = torch.empty_like(t1[b:b + 1])
        _lib.check(lib.wetts_durdisc_layer(h, 0, _lib.ptr(x[b:b + 1].contiguous()), _lib.ptr(mb), None, 1, 1, Tx,
                                           _lib.ptr(out), None, s), "layer 0")
        assert torch.equal(out, t1[b:b + 1]), b
        out = torch.empty_like(out)
        _lib.check(lib.wetts_durdisc_layer(h, 1, _lib.ptr(t1[b:b + 1].contiguous()), _lib.ptr(mb), None, 1, 1, Tx,
                                           _lib.ptr(out), None, s), "layer 1")
        assert torch.equal(out, t2[b:b + 1]), b
        for row, dur in ((b, dr), (B + b, dh)):
            out = torch.empty_like(out)
            _lib.check(lib.wetts_durdisc_layer(h, 2, _lib.ptr(t2[b:b + 1].contiguous()), _lib.ptr(mb),
                                               _lib.ptr(dur[b:b + 1].contiguous()), 1, 1, Tx, _lib.ptr(out), None, s),
                       "layer 2")
            assert torch.equal(out, h1[row:row + 1]), (b, row)
            out, p = torch.empty_like(out), torch.empty(1, Tx, device=DEV)
            _lib.check(lib.wetts_durdisc_layer(h, 3, _lib.ptr(h1[row:row + 1].contiguous()), _lib.ptr(mb), None, 1, 1,
                                               Tx, _lib.ptr(out), _lib.ptr(p), s), "layer 3")
            assert torch.equal(out, h2[row:row + 1]) and torch.equal(p, prob[row:row + 1]), (b, row)
    torch.cuda.synchronize()


# ---- 4. masked positions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", dd.VERSIONS)
def test_masked_positions_are_sigmoid_of_the_output_bias(version):
    """A masked position's features are multiplied by zero, so its probability is sigmoid(output bias): ONE bit pattern
    at every masked position of every row (the empty row included), and that value is the float64 sigmoid of the bias
    within 2 float32 ulps -- expf's 1 ulp and the correctly rounded addition and division behind it."""
    B, Tx, lens = dd.SHAPES[3]
    inp, _, _ = dd.reference(version, B, Tx, lens)
    st, _ = _run(version, inp)
    masked = torch.cat([inp[1][:, 0], inp[1][:, 0]], 0) == 0
    vals = st["prob"].cpu()[masked]
    assert vals.numel() == 2 * (B * Tx - sum(lens)) and len(torch.unique(vals.view(torch.int32))) == 1
    want = float(torch.sigmoid(dd.weights(version)[1]["output_layer.0.bias"])[0])
    assert abs(float(vals[0]) - want) <= 2 * float(np.spacing(np.float32(want)))
    assert not bool((st["prob"].cpu()[~masked].view(torch.int32) == vals.view(torch.int32)[0]).all())


# ---- 5. structures -----------------------------------------------------------------------------------------------------
def test_returned_structures_are_the_references():
    B, Tx, lens = dd.SHAPES[1]
    x, m, dr, dh = (t.to(DEV) for t in dd.inputs(B, Tx, lens, 5))
    out1 = _net(1)(x, m, dr, dh)
    assert isinstance(out1, list) and len(out1) == 2 and all(torch.is_tensor(t) and tuple(t.shape) == (B, Tx, 1) for t in out1)
    out2 = _net(2)(x, m, dr, dh, g=None)
    assert isinstance(out2, list) and len(out2) == 2
    assert all(isinstance(o, list) and len(o) == 1 and tuple(o[0].shape) == (B, Tx, 1) for o in out2)
    for r, g in (out1, (out2[0][0], out2[1][0])):  # slices of the call's one allocation
        assert r.untyped_storage().data_ptr() == g.untyped_storage().data_ptr()
    one = _net(2).forward_probability(x, m, dh)
    assert tuple(one.shape) == (B, Tx, 1) and torch.equal(one, out2[1][0])
    kept = [t.clone() for t in out1]
    _net(1)(x, m, dh, dr)  # another call does not touch what was returned
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out1, kept))
    for bad in ((x[:, :64], m, dr, dh), (x, m[:, :, :-1], dr, dh), (x, m, dr[:, 0], dh), (x.cpu(), m, dr, dh)):
        with pytest.raises(ValueError):
            _net(1)(*bad)


# ---- 6. teacher_forced_losses -----------------------------------------------------------------------------------------
def _recon_net(c):
    cfg, sd, psd = util.vc_case_model(c, SPEC)
    net = SynthesizerTrn(int(c["n_vocab"]), SPEC, 32, n_speakers=int(c["n_speakers"]), **config.MODEL_CONFIGS[str(c["model"])])
    return net.load_state_dict(dict(sd, **psd, **synth.make_duration_state_dict(cfg, 9))).to(DEV)


@pytest.mark.parametrize("name", ["recon_tiny_b3", "recon_vits2_v1_b2"])
def test_teacher_forced_losses_with_a_duration_discriminator(name):
    from tests import recon_oracle as ro
    c = ro.load_recon_case(name)
    if name not in _NET:
        _NET[name] = _recon_net(c)
    net = _NET[name]
    x, xl, spec, yl, sid, eps = (t.to(DEV) for t in ao.case_tensors(c))
    sid = sid if net.n_speakers > 0 else None
    B, Tx = x.shape
    if name in ro.MEL_CASES:
        hps = config.HParams(data=dict(ro.MEL, sampling_rate=int(c["sampling_rate_mel"])), model={},
                             train=dict(c_mel=45, c_kl=1.0))
    else:  # 8 samples per frame: an STFT that fits the 4-frame slice, the posterior input taken as the target "mel"
        hps = config.HParams(data=dict(filter_length=32, hop_length=int(net.hop_length), win_length=32,
                                       n_mel_channels=int(spec.shape[1]), mel_fmin=0.0, mel_fmax=None, sampling_rate=22050),
                             model=dict(use_mel_posterior_encoder=True), train=dict(c_mel=45, c_kl=1.0))
    gen = torch.Generator().manual_seed(83)
    e_q, eps_w = torch.randn(B, 2, Tx, generator=gen).to(DEV), torch.randn(B, 2, Tx, generator=gen).to(DEV)
    kw = dict(sid=sid, segment_size=int(c["segment"]), ids_slice=torch.from_numpy(c["ids_slice"]).to(DEV), eps_q=eps,
              with_duration=True, e_q=e_q, eps_w=eps_w)
    plain = {k: v.clone() for k, v in losses.teacher_forced_losses(net, hps, x, xl, spec, yl, **kw).items()}
    with pytest.raises(ValueError, match="with_duration"):
        losses.teacher_forced_losses(net, hps, x, xl, spec, yl, net_dur_disc=_net(1),
                                     **dict(kw, with_duration=False, e_q=None, eps_w=None))
    for version in dd.VERSIONS:
        out = losses.teacher_forced_losses(net, hps, x, xl, spec, yl, net_dur_disc=_net(version), **kw)
        assert set(out) == set(plain) | set(_KEYS.values())
        for k, v in plain.items():  # every pre-existing entry, bit for bit
            assert torch.equal(out[k], v), k
        st = net._last_duration
        x_enc, mask = net._last_recon["x_enc"].cpu(), st["x_mask"].cpu().reshape(B, 1, Tx)
        logw_, logw = st["logw_"].cpu().reshape(B, 1, Tx), st["logw"].cpu().reshape(B, 1, Tx)
        ref = dd.forward(dd.weights(version)[1], version, x_enc, mask, logw_, logw)
        ref_ls = dd.losses(ref["prob"], mask, version)
        fig = {}
        for s, k in _KEYS.items():
            assert out[k].numel() == ref_ls[s].numel(), (k, out[k].shape)
            fig[s] = dd.scalar_err(out[k].cpu(), ref_ls[s])
            assert fig[s] <= dd.gate(version, s), (name, version, s, fig[s], dd.gate(version, s))
        assert out["losses_dur_gen"].numel() == (B if version == 1 else 1) and tuple(out["dur_gen_per_utt"].shape) == (B,)
        print(f"durdisc teacher-forced {name} v{version}:", fig)
        _MARGINS[f"tf {name} v{version}"] = (round(max(fig[s] / dd.gate(version, s) for s in fig), 3), fig)
