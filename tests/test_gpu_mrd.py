"""GPU tier of MultiPeriodMultiResolutionDiscriminator (csrc/mrd.hip, the complex STFT of csrc/stft.hip, the period
kernels of csrc/discriminator.hip) and of the adversarial losses over its 93 feature maps: the reference's fixtures
(tests/golden/mrd_*.npz), every map, the normalised audio, the three complex spectrograms and every scalar against the
float64 oracle of tests/mrd_oracle.py under the gates defined there, the bit-exact conditions (a row alone, the pairing,
the stand-alone stage entries, the period maps against MultiPeriodDiscriminator, a long loss list against its head),
teacher_forced_losses(net_d=MPMRD), and the argument errors."""
import os

import numpy as np
import pytest
import torch

from tests import mrd_oracle as mo
from tests.test_cpu_disc import state_dict_digest
from tests.test_cpu_mrd import fixture_path
from wetts_amd import MultiPeriodDiscriminator, MultiPeriodMultiResolutionDiscriminator, _lib, losses

pytestmark = pytest.mark.gpu

DEV = "cuda"
_NET = {}
_MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_and_report():
    yield
    import gc
    _NET.clear()
    mo._REF.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = os.environ.get("WETTS_MRD_MARGINS")  # the GPU run that records profiles/mrd_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst multiple of a gate per case (1 = at the gate; gate = 4 x floor), then the figures\n")
            for k in sorted(_MARGINS):
                f.write(f"{k}: {_MARGINS[k]}\n")


def _net():
    if "net" not in _NET:
        sd = mo.weights()[0]
        _NET["sd"] = sd
        _NET["net"] = MultiPeriodMultiResolutionDiscriminator().load_state_dict(sd).to(DEV)
    return _NET["net"]


def _device_losses(y_d_rs, y_d_gs, fmap_rs, fmap_gs):
    fm, layer_means, _, fm_pu = losses._feature(fmap_rs, fmap_gs)
    disc, r, g, disc_pu = losses.discriminator_loss(y_d_rs, y_d_gs, per_utterance=True)
    gen, gl, gen_pu = losses.generator_loss(y_d_gs, per_utterance=True)
    return dict(layer_means=layer_means, fm=fm[0], fm_per_utt=fm_pu, disc_r=r, disc_g=g, disc=disc, disc_per_utt=disc_pu,
                gen_terms=gl, gen=gen, gen_per_utt=gen_pu)


def _maps(fmap_rs, fmap_gs):
    return [torch.cat([r, g], 0) for dr, dg in zip(fmap_rs, fmap_gs) for r, g in zip(dr, dg)]


def _run(y, y_hat):
    out = _net()(y.to(DEV), y_hat.to(DEV))
    ls = _device_losses(*out)
    torch.cuda.synchronize()
    return out, ls


def _stages(x):
    """The stand-alone normalise and spectrogram entries on x [R, 1, T] -> mrd_oracle's stages (spectrograms transposed
    from the internal [R, 2, bins, frames] to the reference's [R, 2, frames, bins])."""
    net = _net()
    lib, s = _lib.load(), _lib.current_stream_ptr()
    x = x.to(DEV).to(torch.float32).contiguous()
    R, _, T = x.shape
    norm = torch.empty(R, T, device=DEV)
    _lib.check(lib.wetts_mrd_normalize(_lib.ptr(x), R, T, _lib.ptr(norm), s), "normalize")
    out = dict(norm=norm)
    for r, w in enumerate(mo.WINDOWS):
        spec = torch.empty(R, 2, w // 2 + 1, mo.frames(w, T), device=DEV)
        _lib.check(lib.wetts_mrd_spectrogram(net._handle, r, _lib.ptr(norm), R, T, _lib.ptr(spec), s), "spectrogram")
        out[f"spec{r}"] = spec.transpose(2, 3)
    torch.cuda.synchronize()
    return out


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", mo.FIXTURE_SHAPES)
def test_matches_reference_fixture(B, T):
    c = np.load(fixture_path(B, T))
    _net()
    assert state_dict_digest(_NET["sd"]) == str(c["state_dict_sha256"])
    (y_d_rs, y_d_gs, fmap_rs, fmap_gs), ls = _run(torch.from_numpy(c["y"]), torch.from_numpy(c["y_hat"]))
    rows = {}
    for d in range(8):
        g = mo.fixture_gate(mo.POSTS[d])
        for nm, got in ((f"y_d_r_{d}", y_d_rs[d]), (f"y_d_g_{d}", y_d_gs[d])):
            assert tuple(got.shape) == c[nm].shape
            rows[nm] = mo.gates(got.cpu().contiguous(), torch.from_numpy(c[nm]))
            assert rows[nm][0] <= g[0] and rows[nm][1] <= g[1], (nm, rows[nm], g)
    rows["fmap_r_2_1"] = mo.gates(fmap_rs[2][1].cpu().contiguous(), torch.from_numpy(c["fmap_r_2_1"]))
    g = mo.fixture_gate(mo.map_index(2, 1))
    assert rows["fmap_r_2_1"][0] <= g[0] and rows["fmap_r_2_1"][1] <= g[1], (rows["fmap_r_2_1"], g)
    for nm, key in (("layer_means", "layer_means"), ("loss_fm", "fm"), ("loss_disc", "disc"), ("losses_disc_r", "disc_r"),
                    ("losses_disc_g", "disc_g"), ("loss_gen", "gen"), ("losses_gen", "gen_terms")):
        rows[nm] = mo.scalar_err(ls[key].cpu(), torch.from_numpy(np.asarray(c[nm])))
        assert rows[nm] <= mo.fixture_gate(key), (nm, rows[nm], mo.fixture_gate(key))
    print(f"mrd fixture b{B}x{T}:", rows)


# ---- 2. every stage against the float64 oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", mo.SHAPES)
def test_every_stage_against_float64_oracle(B, T):
    y, y_hat, ref_maps, ref_stages, ref_ls = mo.reference(B, T)
    (y_d_rs, y_d_gs, fmap_rs, fmap_gs), ls = _run(y, y_hat)
    assert len(y_d_rs) == len(y_d_gs) == len(fmap_rs) == len(fmap_gs) == 8
    ry_d_rs, _, rfr, _ = mo.reference_form(ref_maps, B)
    for d in range(8):
        assert tuple(y_d_rs[d].shape) == tuple(ry_d_rs[d].shape) == tuple(y_d_gs[d].shape)
        assert [tuple(m.shape) for m in fmap_rs[d]] == [tuple(m.shape) for m in rfr[d]]
    stages = _stages(torch.cat([y, y_hat], 0))
    m = mo.measure(_maps(fmap_rs, fmap_gs), stages, ls, ref_maps, ref_stages, ref_ls)
    r3 = lambda v: float(f"{v:.3g}")  # noqa: E731
    fig = {k: ([(r3(a), r3(b)) for a, b in v] if k == "maps" else (tuple(r3(a) for a in v) if isinstance(v, tuple) else r3(v)))
           for k, v in m.items()}
    print(f"mrd b{B}x{T} vs float64:", fig)
    mult = dict(maps=max(max(a / mo.gate(i)[0], b / mo.gate(i)[1]) for i, (a, b) in enumerate(m["maps"])))
    for s in mo.STAGES:
        mult[s] = max(m[s][0] / mo.gate(s)[0], m[s][1] / mo.gate(s)[1])
    for s in mo.SCALARS:
        mult[s] = m[s] / mo.gate(s)
    print(f"mrd b{B}x{T} multiples of the gate:", {k: round(v, 3) for k, v in mult.items()})
    _MARGINS[f"b{B}x{T:05d}"] = ({k: round(v, 3) for k, v in mult.items()}, fig)
    mo.check(m, f"b{B}x{T}")


# ---- 3. bit-exact conditions -------------------------------------------------------------------------------------------
def test_row_alone_and_pairing_are_bit_exact():
    B, T = 3, 1300
    y, y_hat = mo.inputs(B, T, 4242)
    (rs, gs, frs, fgs), ls = _run(y, y_hat)
    y_other = mo.inputs(B, T, 77)[1]
    (rs3, _, frs3, _), _ = _run(y, y_other)  # the real half under another y_hat
    for d in range(8):
        assert torch.equal(rs[d], rs3[d])
        for a, b in zip(frs[d], frs3[d]):
            assert torch.equal(a, b)
    for b in range(B):
        (r1, g1, fr1, fg1), l1 = _run(y[b:b + 1], y_hat[b:b + 1])
        for d in range(8):
            assert torch.equal(r1[d][0], rs[d][b]) and torch.equal(g1[d][0], gs[d][b]), (b, d)
            for k, (a, c) in enumerate(zip(fr1[d] + fg1[d], frs[d] + fgs[d])):
                assert torch.equal(a[0], c[b]), (b, d, k)
        for k in ("fm_per_utt", "disc_per_utt", "gen_per_utt"):
            assert torch.equal(l1[k][0], ls[k][b]), (b, k)


def test_stand_alone_stage_entries_on_a_cut_out_row_give_the_batch_bits():
    """One row cut out of a batch through normalise, the three spectrograms, every band-conv layer and conv_post.  At
    EDGE's length one row's column counts are one short of and one past a multiple of the tile."""
    T = mo.EDGE[1]
    B = 2
    y, y_hat = mo.inputs(B, T, 4243)
    net = _net()
    bufs, _ = net._run(y.to(DEV), y_hat.to(DEV))
    lib, h, s = _lib.load(), net._handle, _lib.current_stream_ptr()
    both = torch.cat([y, y_hat], 0)
    whole = _stages(both)
    b = 2  # the first generated utterance
    one = _stages(both[b:b + 1])
    for k in mo.STAGES:
        assert torch.equal(one[k][0], whole[k][b]), k
    for r, w in enumerate(mo.WINDOWS):
        fr = mo.frames(w, T)
        ws = mo.band_widths(w)
        x = one[f"spec{r}"].transpose(2, 3).contiguous().reshape(-1)  # the internal layout
        for l in range(5):
            out = torch.empty(sum(32 * fr * v[l + 1] for v in ws), device=DEV)
            _lib.check(lib.wetts_mrd_band_conv(h, r, l, _lib.ptr(x), 1, fr, _lib.ptr(out), s), "band_conv")
            if l > 0:
                o = 0
                for bb in range(5):
                    n = 32 * fr * ws[bb][l + 1]
                    assert torch.equal(out[o:o + n], bufs[mo.map_index(r, 4 * bb + l - 1)][b].reshape(-1)), (r, l, bb)
                    o += n
            x = out
        post = torch.empty_like(bufs[mo.map_index(r, 20)][b:b + 1])
        _lib.check(lib.wetts_mrd_conv_post(h, r, _lib.ptr(x), 1, fr, _lib.ptr(post), s), "conv_post")
        assert torch.equal(post, bufs[mo.map_index(r, 20)][b:b + 1]), r
    torch.cuda.synchronize()


def test_period_maps_are_the_multi_period_discriminators():
    B, T = 2, 1300
    y, y_hat = mo.inputs(B, T, 4244)
    sd = mo.weights()[0]
    _net()
    psd = {k.replace(f"discriminators.{int(k.split('.')[1])}.", f"discriminators.{int(k.split('.')[1]) - 2}.", 1): v
           for k, v in sd.items() if int(k.split(".")[1]) >= 3}
    from wetts_amd import synth
    full = synth.make_discriminator_state_dict(3)
    full.update(psd)  # DiscriminatorS keeps its own weights; the five period stacks take the MPMRD's
    mpd = MultiPeriodDiscriminator().load_state_dict(full).to(DEV)
    a = _net()(y.to(DEV), y_hat.to(DEV))
    b = mpd(y.to(DEV), y_hat.to(DEV))
    torch.cuda.synchronize()
    for d in range(5):
        assert torch.equal(a[0][3 + d], b[0][1 + d]) and torch.equal(a[1][3 + d], b[1][1 + d]), d
        for k in range(6):
            assert torch.equal(a[2][3 + d][k], b[2][1 + d][k]) and torch.equal(a[3][3 + d][k], b[3][1 + d][k]), (d, k)


def test_feature_loss_over_93_maps_and_its_first_37_alone():
    B, T = mo.FIXTURE_SHAPES[1]
    y, y_hat, ref_maps, _, ref_ls = mo.reference(B, T)
    _, _, fmap_rs, fmap_gs = _net()(y.to(DEV), y_hat.to(DEV))
    total, item_a, _, per_utt = losses._feature(fmap_rs, fmap_gs)
    flat_r = [m for d in fmap_rs for m in d]
    flat_g = [m for d in fmap_gs for m in d]
    assert len(flat_r) == 93 and tuple(item_a.shape) == (93,)
    head = losses._disc_reduce(0, flat_r[:37], flat_g[:37], 2.0, "feature_loss")
    torch.cuda.synchronize()
    assert torch.equal(item_a[:37], head[1])
    assert mo.scalar_err(total.cpu(), ref_ls["fm"]) <= mo.gate("fm")
    assert mo.scalar_err(per_utt.cpu(), ref_ls["fm_per_utt"]) <= mo.gate("fm_per_utt")
    assert mo.scalar_err(item_a.cpu(), ref_ls["layer_means"]) <= mo.gate("layer_means")


# ---- 4. teacher_forced_losses -----------------------------------------------------------------------------------------
def test_teacher_forced_losses_with_the_mpmrd():
    """tiny_vits2_vocos makes 16 samples per frame: a 70-frame slice is 1120 samples, just above the shortest length."""
    from wetts_amd import SynthesizerTrn, commons, config, synth
    mname, n_vocab, n_spk, spec_ch = "tiny_vits2_vocos", 40, 3, 33
    cfg = config.make_config(dict(config.MODEL_CONFIGS[mname]), n_vocab, n_spk)
    net = SynthesizerTrn(n_vocab, spec_ch, 32, n_speakers=n_spk, **config.MODEL_CONFIGS[mname])
    net.load_state_dict(dict(synth.make_state_dict(cfg, 81), **synth.make_posterior_state_dict(cfg, spec_ch, 82))).to(DEV)
    hop = int(net.hop_length)
    B, Tx, Ty, seg = 2, 12, 90, 70
    assert seg * hop >= MultiPeriodMultiResolutionDiscriminator.MIN_SAMPLES
    g = torch.Generator().manual_seed(6)
    x = torch.randint(1, n_vocab, (B, Tx), generator=g).to(DEV)
    xl = torch.tensor([Tx, Tx - 3]).to(DEV)
    spec = (torch.rand(B, spec_ch, Ty, generator=g) + 0.1).to(DEV)
    yl = torch.tensor([Ty, Ty - 6]).to(DEV)
    sid = torch.tensor([0, 2]).to(DEV)
    ids = torch.tensor([3, 9]).to(DEV)
    eps = torch.randn(B, int(cfg.inter_channels), Ty, generator=g).to(DEV)
    wav = 0.3 * torch.randn(B, 1, Ty * hop, generator=g).to(DEV)
    hps = config.HParams(data=dict(filter_length=64, hop_length=hop, win_length=64, n_mel_channels=spec_ch, mel_fmin=0.0,
                                   mel_fmax=None, sampling_rate=24000),
                         model=dict(use_mel_posterior_encoder=True, use_mrd_disc=True, use_spectral_norm=False),
                         train=dict(c_mel=45, c_kl=1.0))
    kw = dict(sid=sid, segment_size=seg, ids_slice=ids, eps_q=eps)
    plain = losses.teacher_forced_losses(net, hps, x, xl, spec, yl, **kw)
    plain = {k: v.clone() for k, v in plain.items()}
    out = losses.teacher_forced_losses(net, hps, x, xl, spec, yl, net_d=_net(), y=wav, **kw)
    for k, v in plain.items():
        assert torch.equal(out[k], v), k
    y_slice = commons.slice_segments(wav, ids, seg, scale=hop)
    assert torch.equal(out["y_slice"], y_slice) and tuple(y_slice.shape) == (B, 1, seg * hop)
    y_d_r, y_d_g, fmap_r, fmap_g = _net()(y_slice, out["y_hat"])
    disc, r, gl_, disc_pu = losses.discriminator_loss(y_d_r, y_d_g, per_utterance=True)
    gen, gl, gen_pu = losses.generator_loss(y_d_g, per_utterance=True)
    fm, fm_pu = losses.feature_loss(fmap_r, fmap_g, per_utterance=True)
    for k, v in dict(loss_disc=disc, loss_gen=gen, loss_fm=fm, loss_disc_per_utt=disc_pu, loss_gen_per_utt=gen_pu,
                     loss_fm_per_utt=fm_pu, losses_disc_r=r, losses_disc_g=gl_, losses_gen=gl).items():
        assert torch.equal(out[k], v), k
        assert bool(torch.isfinite(v).all()) and float(v.reshape(-1)[0]) > 0, k
    assert tuple(out["losses_disc_r"].shape) == (8,) and tuple(out["losses_gen"].shape) == (8,)
    assert tuple(out["loss_fm_per_utt"].shape) == (B,)


# ---- 5. argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors_on_the_device():
    net = _net()
    y = torch.zeros(2, 1, 1300, device=DEV)
    for bad in (torch.zeros(2, 1300, device=DEV), torch.zeros(2, 2, 1300, device=DEV), torch.zeros(2, 1, 1301, device=DEV),
                torch.zeros(2, 1, 1300)):
        with pytest.raises(ValueError):
            net(y, bad)
    with pytest.raises(ValueError, match="reflect pad of the 2048"):
        net(torch.zeros(1, 1, 1024, device=DEV), torch.zeros(1, 1, 1024, device=DEV))
    with pytest.raises(RuntimeError, match="no weights"):
        MultiPeriodMultiResolutionDiscriminator().to(DEV)(y, y)
    emb = dict(_NET["sd"])
    emb["discriminators.1.emb.weight"] = torch.zeros(4, 32)
    with pytest.raises(NotImplementedError, match="num_embeddings"):
        MultiPeriodMultiResolutionDiscriminator().load_state_dict(emb)
    out = net(torch.zeros(1, 1, 1025, device=DEV), torch.ones(1, 1, 1025, device=DEV))  # the shortest legal length
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in out[0] + out[1])
