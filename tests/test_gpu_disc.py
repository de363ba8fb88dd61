"""GPU tier of MultiPeriodDiscriminator and the adversarial losses (csrc/discriminator.hip): the reference's fixtures
(tests/golden/disc_*.npz), every feature map of every stack and every scalar against the float64 oracle of
tests/disc_oracle.py under the gates defined there (4 x the float32 oracle's own distance from float64), the bit-exact
conditions (a row alone, the pairing, repeats, the stand-alone layer entries), teacher_forced_losses(net_d=, y=), and the
shapes / ownership of what is returned.  Every kernel form is compared with the oracle, never with another form."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import disc_oracle as do
from tests.test_cpu_disc import fixture_path, state_dict_digest
from wetts_amd import MultiPeriodDiscriminator, _lib, losses

pytestmark = pytest.mark.gpu

DEV = "cuda"
_NET = {}
_MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_and_report():
    yield
    import gc
    _NET.clear()
    do._REF.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = os.environ.get("WETTS_DISC_MARGINS")  # the GPU run that records profiles/disc_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst multiple of a gate per case (1 = at the gate; gate = 4 x floor), then the figures\n")
            for k in sorted(_MARGINS):
                f.write(f"{k}: {_MARGINS[k]}\n")


def _net():
    if "net" not in _NET:
        sd = do.weights()[0]
        _NET["sd"] = sd
        _NET["net"] = MultiPeriodDiscriminator().load_state_dict(sd).to(DEV)
    return _NET["net"]


def _device_losses(y_d_rs, y_d_gs, fmap_rs, fmap_gs):
    """The three loss functions -> the dict disc_oracle.losses returns."""
    fm, layer_means, _, fm_pu = losses._feature(fmap_rs, fmap_gs)
    disc, r, g, disc_pu = losses.discriminator_loss(y_d_rs, y_d_gs, per_utterance=True)
    gen, gl, gen_pu = losses.generator_loss(y_d_gs, per_utterance=True)
    return dict(layer_means=layer_means, fm=fm[0], fm_per_utt=fm_pu, disc_r=r, disc_g=g, disc=disc, disc_per_utt=disc_pu,
                gen_terms=gl, gen=gen, gen_per_utt=gen_pu)


def _maps(fmap_rs, fmap_gs):
    """The 37 maps over 2B utterances (real first), as disc_oracle.forward orders them."""
    return [torch.cat([r, g], 0) for dr, dg in zip(fmap_rs, fmap_gs) for r, g in zip(dr, dg)]


def _run(y, y_hat):
    out = _net()(y.to(DEV), y_hat.to(DEV))
    ls = _device_losses(*out)
    torch.cuda.synchronize()
    return out, ls


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", do.FIXTURE_SHAPES)
def test_matches_reference_fixture(B, T):
    """First the regenerated weights' digest (a torch RNG change shows as that, not as a parity failure); then the twelve
    outputs, the stored feature map, the 37 per-layer means and every scalar loss within the gates."""
    c = np.load(fixture_path(B, T))
    net = _net()
    assert state_dict_digest(_NET["sd"]) == str(c["state_dict_sha256"])
    (y_d_rs, y_d_gs, fmap_rs, fmap_gs), ls = _run(torch.from_numpy(c["y"]), torch.from_numpy(c["y_hat"]))
    rows = {}
    for d in range(6):
        i = do.map_index(d, 6 if d == 0 else 5)
        for nm, got in ((f"y_d_r_{d}", y_d_rs[d]), (f"y_d_g_{d}", y_d_gs[d])):
            assert tuple(got.shape) == c[nm].shape
            rows[nm] = do.gates(got.cpu(), torch.from_numpy(c[nm]))
            assert rows[nm][0] <= do.fixture_gate(i)[0] and rows[nm][1] <= do.fixture_gate(i)[1], (nm, rows[nm], do.fixture_gate(i))
    rows["fmap_r_5_0"] = do.gates(fmap_rs[5][0].cpu().contiguous(), torch.from_numpy(c["fmap_r_5_0"]))
    g = do.fixture_gate(do.map_index(5, 0))
    assert rows["fmap_r_5_0"][0] <= g[0] and rows["fmap_r_5_0"][1] <= g[1], (rows["fmap_r_5_0"], g)
    for nm, key in (("layer_means", "layer_means"), ("loss_fm", "fm"), ("loss_disc", "disc"), ("losses_disc_r", "disc_r"),
                    ("losses_disc_g", "disc_g"), ("loss_gen", "gen"), ("losses_gen", "gen_terms")):
        rows[nm] = do.scalar_err(ls[key].cpu(), torch.from_numpy(np.asarray(c[nm])))
        assert rows[nm] <= do.fixture_gate(key), (nm, rows[nm], do.fixture_gate(key))
    print(f"disc fixture b{B}x{T}:", rows)


# ---- 2. every stage against the float64 oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", do.SHAPES)
def test_every_stage_against_float64_oracle(B, T):
    y, y_hat, ref_maps, ref_ls = do.reference(B, T)
    (y_d_rs, y_d_gs, fmap_rs, fmap_gs), ls = _run(y, y_hat)
    m = do.measure(_maps(fmap_rs, fmap_gs), ls, ref_maps, ref_ls)
    fig = {k: (v if k != "maps" else [(float(f"{a:.3g}"), float(f"{b:.3g}")) for a, b in v]) for k, v in m.items()}
    print(f"disc b{B}x{T} vs float64:", fig)
    top = do.check(m, f"b{B}x{T}")
    _MARGINS[f"b{B}x{T:05d}"] = (round(top, 3), fig)


# ---- 3. bit-exact conditions -------------------------------------------------------------------------------------------
def test_row_alone_pairing_and_repeats_are_bit_exact():
    B, T = 3, 700
    y, y_hat = do.inputs(B, T, 4242)
    net = _net()
    (rs, gs, frs, fgs), ls = _run(y, y_hat)
    (rs2, gs2, frs2, fgs2), ls2 = _run(y, y_hat)
    for a, b in zip(_maps(frs, fgs), _maps(frs2, fgs2)):
        assert torch.equal(a, b)
    for k in ls:
        assert torch.equal(ls[k], ls2[k]), k
    # the real half does not depend on what it is paired with
    (rs3, _, frs3, _), _ = _run(y, y)
    for d in range(6):
        assert torch.equal(rs[d], rs3[d])
        for a, b in zip(frs[d], frs3[d]):
            assert torch.equal(a, b)
    # a row alone equals the row in the batch: every map, every output, every per-utterance loss
    for b in range(B):
        (r1, g1, fr1, fg1), l1 = _run(y[b:b + 1], y_hat[b:b + 1])
        for d in range(6):
            assert torch.equal(r1[d][0], rs[d][b]) and torch.equal(g1[d][0], gs[d][b]), (b, d)
            for k, (a, c) in enumerate(zip(fr1[d] + fg1[d], frs[d] + fgs[d])):
                assert torch.equal(a[0], c[b]), (b, d, k)
        for k in ("fm_per_utt", "disc_per_utt", "gen_per_utt"):
            assert torch.equal(l1[k][0], ls[k][b]), (b, k)


def test_stand_alone_layer_entries_on_a_cut_out_row_give_the_batch_bits():
    B, T = 2, 700
    y, y_hat = do.inputs(B, T, 4243)
    net = _net()
    bufs, _ = net._run(y.to(DEV), y_hat.to(DEV))
    shapes = net.fmap_shapes(B, T)
    lib, h, s = _lib.load(), net._handle, _lib.current_stream_ptr()
    b = 1  # the second real utterance
    yb = y[b:b + 1].to(DEV).contiguous()
    # DiscriminatorS: grouped layers 0..4, the MFMA conv (layer 5), conv_post
    x, Tin = yb, T
    for m in range(5):
        out = torch.empty_like(bufs[m][b:b + 1])
        _lib.check(lib.wetts_disc_grouped_conv(h, m, _lib.ptr(x), 1, Tin, _lib.ptr(out), s), "grouped")
        assert torch.equal(out, bufs[m][b:b + 1]), m
        x, Tin = bufs[m][b:b + 1].contiguous(), shapes[m][2]
    out = torch.empty_like(bufs[5][b:b + 1])
    _lib.check(lib.wetts_disc_strided_conv(h, 0, 5, _lib.ptr(x), 1, Tin, _lib.ptr(out), s), "strided S")
    assert torch.equal(out, bufs[5][b:b + 1])
    out = torch.empty_like(bufs[6][b:b + 1])
    _lib.check(lib.wetts_disc_conv_post(h, 0, _lib.ptr(bufs[5][b:b + 1].contiguous()), 1, shapes[5][2], _lib.ptr(out), s), "post S")
    assert torch.equal(out, bufs[6][b:b + 1])
    # every period stack
    for d in range(1, 6):
        i0 = do.map_index(d, 0)
        p = do.PERIODS[d - 1]
        out = torch.empty_like(bufs[i0][b:b + 1])
        _lib.check(lib.wetts_disc_fold_conv0(h, d, _lib.ptr(yb), 1, T, _lib.ptr(out), s), "fold")
        assert torch.equal(out, bufs[i0][b:b + 1]), d
        for m in range(1, 5):
            x = bufs[i0 + m - 1][b:b + 1].contiguous()
            out = torch.empty_like(bufs[i0 + m][b:b + 1])
            _lib.check(lib.wetts_disc_strided_conv(h, d, m, _lib.ptr(x), p, shapes[i0 + m - 1][2], _lib.ptr(out), s), "strided")
            assert torch.equal(out, bufs[i0 + m][b:b + 1]), (d, m)
        x = bufs[i0 + 4][b:b + 1].contiguous()
        out = torch.empty_like(bufs[i0 + 5][b:b + 1])
        _lib.check(lib.wetts_disc_conv_post(h, d, _lib.ptr(x), 1, shapes[i0 + 4][2], _lib.ptr(out), s), "post")
        assert torch.equal(out, bufs[i0 + 5][b:b + 1]), d
    torch.cuda.synchronize()


# ---- 4. teacher_forced_losses -----------------------------------------------------------------------------------------
def test_teacher_forced_losses_with_a_discriminator():
    from tests import test_gpu_recon as tr
    from wetts_amd import commons
    from wetts_amd import config
    c = tr._case("recon_tiny_b3")
    net = tr._case_net(c)
    x, xl, spec, yl, sid, eps = tr._dev(c, net)
    # the tiny model makes 8 samples per frame, so a 4-frame slice is 32 samples: an STFT that fits it, and the posterior
    # input taken as the target "mel" itself (the mel terms only have to be the same with and without net_d here)
    hps = config.HParams(data=dict(filter_length=32, hop_length=int(net.hop_length), win_length=32,
                                   n_mel_channels=int(spec.shape[1]), mel_fmin=0.0, mel_fmax=None, sampling_rate=22050),
                         model=dict(use_mel_posterior_encoder=True), train=dict(c_mel=45, c_kl=1.0))
    seg = int(c["segment"])
    ids = torch.from_numpy(c["ids_slice"]).to(DEV)
    B, hop = x.shape[0], int(net.hop_length)
    wav = 0.3 * torch.randn(B, 1, int(spec.shape[2]) * hop, generator=torch.Generator().manual_seed(5)).to(DEV)
    kw = dict(sid=sid, segment_size=seg, ids_slice=ids, eps_q=eps)
    plain = losses.teacher_forced_losses(net, hps, x, xl, spec, yl, **kw)
    plain = {k: v.clone() for k, v in plain.items()}
    out = losses.teacher_forced_losses(net, hps, x, xl, spec, yl, net_d=_net(), y=wav, **kw)
    for k, v in plain.items():
        assert torch.equal(out[k], v), k
    y_slice = commons.slice_segments(wav, ids, seg, scale=hop)
    assert torch.equal(out["y_slice"], y_slice)
    y_d_r, y_d_g, fmap_r, fmap_g = _net()(y_slice, out["y_hat"])
    disc, r, g, disc_pu = losses.discriminator_loss(y_d_r, y_d_g, per_utterance=True)
    gen, gl, gen_pu = losses.generator_loss(y_d_g, per_utterance=True)
    fm, fm_pu = losses.feature_loss(fmap_r, fmap_g, per_utterance=True)
    for k, v in dict(loss_disc=disc, loss_gen=gen, loss_fm=fm, loss_disc_per_utt=disc_pu, loss_gen_per_utt=gen_pu,
                     loss_fm_per_utt=fm_pu, losses_disc_r=r, losses_disc_g=g, losses_gen=gl).items():
        assert torch.equal(out[k], v), k
        assert bool(torch.isfinite(v).all()) and float(v.reshape(-1)[0]) > 0, k
    assert tuple(out["losses_gen"].shape) == (6,) and tuple(out["loss_fm_per_utt"].shape) == (B,)
    with pytest.raises(ValueError):
        losses.teacher_forced_losses(net, hps, x, xl, spec, yl, net_d=_net(), **kw)


# ---- 5. shapes and ownership -------------------------------------------------------------------------------------------
def test_returned_views_have_the_reference_shapes_and_survive_a_second_call():
    B, T = 2, 700
    y, y_hat, ref_maps, _ = do.reference(B, T)
    ry_d_rs, ry_d_gs, rfr, rfg = do.reference_form(ref_maps, B)
    net = _net()
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = net(y.to(DEV), y_hat.to(DEV))
    assert len(y_d_rs) == len(y_d_gs) == len(fmap_rs) == len(fmap_gs) == 6
    for d in range(6):
        assert tuple(y_d_rs[d].shape) == tuple(ry_d_rs[d].shape) == tuple(y_d_gs[d].shape)
        assert [tuple(m.shape) for m in fmap_rs[d]] == [tuple(m.shape) for m in rfr[d]]
        assert [tuple(m.shape) for m in fmap_gs[d]] == [tuple(m.shape) for m in rfg[d]]
    torch.cuda.synchronize()
    kept = [m.clone() for d in fmap_rs + fmap_gs for m in d] + [t.clone() for t in y_d_rs + y_d_gs]
    net(torch.randn(3, 1, 900, device=DEV), torch.randn(3, 1, 900, device=DEV))  # another call, another shape
    net(y_hat.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    for a, b in zip([m for d in fmap_rs + fmap_gs for m in d] + y_d_rs + y_d_gs, kept):
        assert torch.equal(a, b)
    # a period stack's map is a view of torch-owned memory, not a copy: [2B, p, C, H] permuted
    assert not fmap_rs[3][1].is_contiguous() and fmap_rs[3][1].permute(0, 3, 1, 2).is_contiguous()


def test_host_checks_on_the_device():
    net = _net()
    y = torch.zeros(2, 1, 64, device=DEV)
    for bad in (torch.zeros(2, 64, device=DEV), torch.zeros(2, 2, 64, device=DEV), torch.zeros(2, 1, 65, device=DEV),
                torch.zeros(2, 1, 64)):
        with pytest.raises(ValueError):
            net(y, bad)
    with pytest.raises(ValueError):
        net(torch.zeros(1, 1, 5, device=DEV), torch.zeros(1, 1, 5, device=DEV))
    out = net(torch.zeros(1, 1, 6, device=DEV), torch.ones(1, 1, 6, device=DEV))  # the shortest legal length
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in out[0] + out[1])
