"""GPU tier of the WavLM loss (csrc/wavlm.hip; wetts_amd/wavlm.py, discriminators.WavLMDiscriminator, losses.WavLMLoss):
the reference's fixtures (tests/golden/wavlm_*.npz) end to end, every stand-alone stage against the float64 oracle of
tests/wavlm_oracle.py on the stage's own input under the gates defined there (4 x the float32 floor stored in the
fixtures; 4 + 1 floors against the reference's stored float32), the bit-exact conditions (a row alone, 2B rows against
two batches of B), WavLMLoss's four methods, teacher_forced_losses(wl=...) and the error paths.
Tiles: 64 GEMM columns in two halves of 32 and 32 GEMM rows, 16 queries and 64 keys per attention block, 64 channels
per normalisation block, 4 tokens per LayerNorm block.  wavlm_oracle.SHAPES put their edges inside: 33 frames x 4 rows
cross the 16-query tile, the 32-column half and the 64-column GEMM tile; 65 frames (one key in the attention's second
64-key chunk) and 130 frames (two full chunks and a tail of two) cross the key chunk, end to end and in the attention
and layer stage cases."""
import pytest
import torch

from tests import wavlm_oracle as wo
from wetts_amd import _lib, discriminators, losses, wavlm

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(c, s) for c in wo.CONFIGS for s in wo.SHAPES]
# 18 and 33 frames, the 3:2 rate, one frame, and the two shapes behind the attention's 64-key chunk (65 and 130 frames)
STAGE_SHAPES = (wo.SHAPES[2], wo.SHAPES[5], wo.SHAPES[6], wo.SHAPES[0], wo.SHAPES[7], wo.SHAPES[8])
_NET, _WL = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    import gc
    _NET.clear()
    _WL.clear()
    wo._REF.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _net(cname):
    if cname not in _NET:
        c = wo.HF_CONFIGS[cname]
        (sd, _), (dd, _) = wo.weights(cname)
        net = wavlm.WavLM(c).load_state_dict(sd).to(DEV)
        wd = discriminators.WavLMDiscriminator(c["hidden_size"], wo.slm_layers(cname), wo.INITIAL_CHANNEL[cname]) \
            .load_state_dict(dd).to(DEV)
        _NET[cname] = (net, wd)
    return _NET[cname]


def _wl(cname, rate):
    if (cname, rate) not in _WL:
        _WL[(cname, rate)] = losses.WavLMLoss(_net(cname)[0], _net(cname)[1], rate, wo.SLM_SR)
    return _WL[(cname, rate)]


def _figs(d):
    return {k: tuple(float(f"{x:.3g}") for x in v) for k, v in d.items()}


def _check(figs, c, tag, fixture=False):
    """Asserts {key: (rel, local)} against the gates of fixture `c` (prints every figure first)."""
    gate = wo.fixture_gate if fixture else wo.gate_of
    top = max(max(v[0] / gate(c["floor_" + k])[0], v[1] / gate(c["floor_" + k])[1]) for k, v in figs.items())
    print(tag, _figs(figs), "worst multiple of a gate", round(top, 3))
    for k, v in figs.items():
        g = gate(c["floor_" + k])
        assert wo.within(v, g), f"{tag} {k}: rel {v[0]:.3e} (gate {g[0]:.3e}) local {v[1]:.3e} (gate {g[1]:.3e})"


def _device_forward(cname, shape, wav, rec):
    """The device's counterpart of wavlm_oracle.forward: dict of CPU tensors."""
    wl = _wl(cname, shape[0])
    h = wl.hidden(wav.to(DEV), rec.to(DEV))
    d = wl.wd.on_hidden(h)
    both = torch.cat([wav, rec], 0).to(DEV)
    out = dict(resampled=wl.resample(both).cpu(), hidden=[t.cpu() for t in h.unbind(0)], d=d.cpu())
    out.update({k: v.cpu() for k, v in wl.all_terms(wav.to(DEV), rec.to(DEV)).items()})
    return out


# ---- 1. the fixtures, end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,shape", CASES)
def test_matches_reference_fixture_and_oracle(cname, shape):
    """Resampled audio, every hidden state, the discriminator's output and the three losses: within GATE_FACTOR floors
    of the float64 oracle, and within GATE_FACTOR + 1 of what the reference's own float32 pass stored."""
    c = wo.load_fixture(cname, shape)
    wav, rec, o = wo.reference(cname, shape)
    B = shape[2]
    got = _device_forward(cname, shape, wav, rec)
    assert got["hidden"][0].shape == o["hidden"][0].shape and len(got["hidden"]) == wo.slm_layers(cname)
    hid = None
    for a, r in zip(got["hidden"], o["hidden"]):
        hid = wo.worst(hid, wo.gates(a, r))
    figs = dict(resample=wo.gates(got["resampled"], o["resampled"]), hidden=hid, d=wo.gates(got["d"], o["d"]))
    for k in ("loss_lm", "loss_lm_gen", "loss_slm"):
        figs[k] = wo.rel_err(got[k], o[k])
    _check(figs, c, f"{wo.case_name(cname, shape)} oracle")
    for k in ("loss_lm", "loss_lm_gen", "loss_slm"):
        pu = wo.gates(got[k + "_per_utt"], o[k + "_per_utt"])
        g = wo.gate_of(c["floor_" + k + "_per_utt"])
        print(k + "_per_utt", pu)
        assert wo.within(pu, g), (k, pu, g)
    if "hidden" in c.files:
        rh = None
        for a, r in zip(got["hidden"], torch.from_numpy(c["hidden"])):
            rh = wo.worst(rh, wo.gates(a, r))
    else:
        rh = wo.gates(got["hidden"][-1][[0, B]], torch.from_numpy(c["hidden_last"]))
    rr = wo.gates(got["resampled"][:c["resampled"].shape[0]], torch.from_numpy(c["resampled"]))
    figs = dict(resample=rr, hidden=rh, d=wo.gates(got["d"], torch.from_numpy(c["d"])))
    for k in ("loss_lm", "loss_lm_gen", "loss_slm"):
        figs[k] = wo.rel_err(got[k], c[k])
    _check(figs, c, f"{wo.case_name(cname, shape)} reference", fixture=True)


# ---- 2. every stage alone -------------------------------------------------------------------------------------------------
def _run_stage(cname, stage, inp, shape):
    net, wd = _net(cname)
    lib, h, s = _lib.load(), net._handle, _lib.current_stream_ptr()
    c = wo.HF_CONFIGS[cname]
    H, heads = c["hidden_size"], c["num_attention_heads"]
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    new = lambda *shp: torch.empty(*shp, dtype=torch.float32, device=DEV)  # noqa: E731
    if stage == "resample":
        return wavlm.Resample(shape[0], wo.SLM_SR)(dev(inp["x"]))
    if stage == "conv0":
        x = dev(inp["x"])
        B, L = x.shape
        out = new(B, (L - c["conv_kernel"][0]) // c["conv_stride"][0] + 1, c["conv_dim"][0])
        _lib.check(lib.wetts_wavlm_conv0(h, _lib.ptr(x), L, B, L, _lib.ptr(out), s), stage)
        return out
    if stage.startswith("conv"):
        i = int(stage[4:])
        x = dev(inp["x"])
        B, Tin, _ = x.shape
        out = new(B, (Tin - c["conv_kernel"][i]) // c["conv_stride"][i] + 1, c["conv_dim"][i])
        _lib.check(lib.wetts_wavlm_conv(h, i, _lib.ptr(x), B, Tin, _lib.ptr(out), s), stage)
        return out
    if stage == "project":
        x = dev(inp["x"])
        B, T, Cl = x.shape
        normed, out = new(B, T, Cl), new(B, T, H)
        _lib.check(lib.wetts_wavlm_project(h, _lib.ptr(x), B * T, _lib.ptr(normed), _lib.ptr(out), s), stage)
        return out
    if stage == "pos_conv":
        x = dev(inp["x"])
        B, T, _ = x.shape
        out = new(B, T, H)
        _lib.check(lib.wetts_wavlm_pos_conv(h, _lib.ptr(x), B, T, _lib.ptr(out), s), stage)
        return out
    if stage == "attention":
        x, qkv = dev(inp["x"]), dev(inp["qkv"])
        B, T, _ = x.shape
        gate, out = new(B, T, heads), new(B, T, H)
        _lib.check(lib.wetts_wavlm_attention(h, 0, _lib.ptr(x), _lib.ptr(qkv), B, T, _lib.ptr(gate), _lib.ptr(out), s), stage)
        g64 = wo.gate(wo.weights(cname)[0][1], cname, 0, inp["x"].double()).transpose(1, 2)
        fig = wo.gates(gate.cpu(), g64)
        # at most 64 products per projection (6e-8 each of an O(1) sum: 4e-6), the sigmoids' slope is at most 1 / 4 and
        # the gate combines two of them with O(1) factors
        assert fig[1] <= 1e-5, ("gate", fig)
        return out
    if stage == "layer":
        x = dev(inp["x"])
        B, T, _ = x.shape
        ws = new(int(lib.wetts_wavlm_layer_workspace_bytes(h, B, T)) // 4)
        out = new(B, T, H)
        _lib.check(lib.wetts_wavlm_layer(h, 0, _lib.ptr(x), B, T, _lib.ptr(out), _lib.ptr(ws), s), stage)
        return out
    if stage == "disc_pre":
        hid = torch.stack([dev(t) for t in inp["hidden"]], 0).contiguous()
        _, R, T, _ = hid.shape
        out = new(R, T, wd.initial_channel)
        _lib.check(lib.wetts_wavlm_disc_pre(wd._handle, _lib.ptr(hid), R * T * H, R, T, _lib.ptr(out), s), stage)
        return out
    if stage.startswith("reduce_"):
        hid = torch.stack([dev(t) for t in inp["hidden"]], 0).contiguous()
        d = dev(inp["d"])
        B = d.shape[0] // 2
        if stage == "reduce_lm":  # the 13-item (here: layers + 1) call, split at B
            total, pu = _wl(cname, shape[0])._lm(hid, B)
        elif stage == "reduce_lm_gen":
            total, _, pu = losses.generator_loss([d[B:]], per_utterance=True)
        else:
            total, _, _, pu = losses.discriminator_loss([d[:B]], [d[B:]], per_utterance=True)
        return torch.cat([total.reshape(1), pu])
    assert stage == "disc_convs"
    pre = dev(inp["pre"])
    R, T, _ = pre.shape
    ws = new(int(lib.wetts_wavlm_disc_workspace_bytes(wd._handle, R, T)) // 4)
    out = new(R, T)
    _lib.check(lib.wetts_wavlm_disc_convs(wd._handle, _lib.ptr(pre), R, T, _lib.ptr(out), _lib.ptr(ws), s), stage)
    return out


@pytest.mark.parametrize("cname", wo.CONFIGS)
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_every_stage_alone_against_the_float64_oracle(cname, shape):
    """Resampler, conv 0 + norm, each strided conv, projection, positional conv, gate + attention, a whole layer, the
    discriminator's pre and its convs, and each of the three reductions (total and per-utterance values, on given hidden
    states and discriminator outputs): each on its own float32 input, against the float64 evaluation of that input."""
    c = wo.load_fixture(cname, shape)
    wav, rec, _ = wo.reference(cname, shape)
    (_, W64), (_, D64) = wo.weights(cname)
    figs = {}
    for stage, (inp, fn) in wo.stage_cases(cname, shape, wav, rec).items():
        got = _run_stage(cname, stage, inp, shape).cpu()
        figs[stage] = wo.gates(got, fn(W64, D64, inp))
    assert set(figs) == set(wo.STAGES)
    _check(figs, c, f"{wo.case_name(cname, shape)} stages")


# ---- 3. bit-exact conditions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", wo.CONFIGS)
def test_a_row_alone_and_the_2B_batch_equal_the_batch_bit_for_bit(cname):
    shape = wo.SHAPES[2]
    wav, rec, _ = wo.reference(cname, shape)
    wl = _wl(cname, shape[0])
    wav, rec = wav.to(DEV), rec.to(DEV)
    B = wav.shape[0]
    both = wl.hidden(wav, rec)
    d_both = wl.wd.on_hidden(both)
    real, gen = wl.hidden(wav), wl.hidden(rec)
    assert torch.equal(both[:, :B], real) and torch.equal(both[:, B:], gen)
    assert torch.equal(d_both[:B], wl.wd.on_hidden(real)) and torch.equal(d_both[B:], wl.discriminator_forward(rec))
    one = wl.hidden(wav[1:2])
    assert torch.equal(one[:, 0], real[:, 1])
    assert torch.equal(wl.discriminator_forward(wav[1:2])[0], d_both[1])
    assert torch.equal(wl.resample(wav[2:3]), wl.resample(wav)[2:3])
    # rows at any stride: an expanded row (stride 0), overlapping rows, a transposed tensor
    assert torch.equal(wl.resample(wav[1:2].expand(3, -1)), wl.resample(wav[1:2]).expand(3, -1))
    over = wav[0].as_strided((2, 4096), (100, 1))
    assert torch.equal(wl.resample(over), wl.resample(over.contiguous()))
    assert torch.equal(wl.resample(wav.t().contiguous().t()), wl.resample(wav))
    assert torch.equal(wl.hidden(wav[1:2].expand(2, -1))[:, 1], real[:, 1])
    assert torch.equal(wl.hidden(wav, rec), both)  # repeats
    # per-utterance losses of a row do not depend on the batch either
    full = wl.all_terms(wav, rec)
    solo = wl.all_terms(wav[1:2], rec[1:2])
    for k in ("loss_lm_per_utt", "loss_lm_gen_per_utt", "loss_slm_per_utt"):
        assert torch.equal(full[k][1:2], solo[k]), k
    # the stacked-tensor interface of the reference's class reads the same numbers
    x = torch.stack(list(real.unbind(0)), dim=1).transpose(-1, -2).flatten(1, 2)
    assert torch.equal(wl.wd(x), d_both[:B])


# ---- 4. WavLMLoss's four methods --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,shape", [(c, s) for c in wo.CONFIGS for s in (wo.SHAPES[0], wo.SHAPES[2], wo.SHAPES[5])])
def test_wavlm_loss_methods_match_the_reference(cname, shape):
    """__call__, generator, discriminator, discriminator_forward, on [B, L] and on [B, 1, L], B = 1 included (where the
    reference's own forward() fails): against the reference's stored float32 values, GATE_FACTOR + 1 floors."""
    c = wo.load_fixture(cname, shape)
    wav, rec, _ = wo.reference(cname, shape)
    wl = _wl(cname, shape[0])
    wav, rec = wav.to(DEV), rec.to(DEV)
    B = wav.shape[0]
    lm, lm_pu = wl(wav, rec, per_utterance=True)
    gen, gen_pu = wl.generator(rec, per_utterance=True)
    slm, slm_pu = wl.discriminator(wav, rec, per_utterance=True)
    d = wl.discriminator_forward(wav)
    figs = dict(loss_lm=wo.rel_err(lm, c["loss_lm"]), loss_lm_gen=wo.rel_err(gen, c["loss_lm_gen"]),
                loss_slm=wo.rel_err(slm, c["loss_slm"]), d=wo.gates(d.cpu(), torch.from_numpy(c["d"][:B])))
    _check(figs, c, f"{wo.case_name(cname, shape)} WavLMLoss", fixture=True)
    assert lm.dim() == 0 and tuple(lm_pu.shape) == (B,) and tuple(gen_pu.shape) == (B,) and tuple(slm_pu.shape) == (B,)
    assert tuple(d.shape) == (B, int(c["frames"]))
    assert torch.equal(wl(wav[:, None], rec[:, None]), lm) and torch.equal(wl.generator(rec[:, None]), gen)
    assert torch.equal(wl.discriminator(wav[:, None], rec[:, None]), slm) and torch.equal(wl.discriminator_forward(wav[:, None]), d)
    terms = wl.all_terms(wav, rec)
    assert torch.equal(terms["loss_lm"], lm) and torch.equal(terms["loss_lm_gen"], gen) and torch.equal(terms["loss_slm"], slm)
    assert torch.equal(terms["loss_lm_per_utt"], lm_pu) and torch.equal(terms["loss_slm_per_utt"], slm_pu)


# ---- 5. teacher_forced_losses(wl=...) ---------------------------------------------------------------------------------------
def test_teacher_forced_losses_adds_exactly_the_six_keys():
    """tiny_vits2_vocos makes 16 samples per frame: a 70-frame slice is 1120 samples at 24 kHz, 747 at 16 kHz, two WavLM
    frames.  With `wl` the call adds the six entries and leaves every other one bit-identical; `y` may come with `wl`
    alone."""
    from wetts_amd import SynthesizerTrn, commons, config, synth
    mname, n_vocab, n_spk, spec_ch = "tiny_vits2_vocos", 40, 3, 33
    cfg = config.make_config(dict(config.MODEL_CONFIGS[mname]), n_vocab, n_spk)
    net = SynthesizerTrn(n_vocab, spec_ch, 32, n_speakers=n_spk, **config.MODEL_CONFIGS[mname])
    net.load_state_dict(dict(synth.make_state_dict(cfg, 81), **synth.make_posterior_state_dict(cfg, spec_ch, 82))).to(DEV)
    hop = int(net.hop_length)
    B, Tx, Ty, seg = 2, 12, 90, 70
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
                         model=dict(use_mel_posterior_encoder=True, use_wd=True), train=dict(c_mel=45, c_kl=1.0))
    kw = dict(sid=sid, segment_size=seg, ids_slice=ids, eps_q=eps)
    wl = _wl("tiny", 24000)
    plain = losses.teacher_forced_losses(net, hps, x, xl, spec, yl, **kw)
    plain = {k: v.clone() for k, v in plain.items()}
    out = losses.teacher_forced_losses(net, hps, x, xl, spec, yl, y=wav, wl=wl, **kw)
    assert set(out) - set(plain) == {"loss_slm", "loss_lm", "loss_lm_gen", "loss_slm_per_utt", "loss_lm_per_utt",
                                     "loss_lm_gen_per_utt"} and set(plain) <= set(out)
    for k, v in plain.items():
        assert torch.equal(out[k], v), k
    y_slice = commons.slice_segments(wav, ids, seg, scale=hop)
    lm, lm_pu = wl(y_slice, out["y_hat"], per_utterance=True)
    gen, gen_pu = wl.generator(out["y_hat"], per_utterance=True)
    slm, slm_pu = wl.discriminator(y_slice, out["y_hat"], per_utterance=True)
    for k, v in dict(loss_lm=lm, loss_lm_gen=gen, loss_slm=slm, loss_lm_per_utt=lm_pu, loss_lm_gen_per_utt=gen_pu,
                     loss_slm_per_utt=slm_pu).items():
        assert torch.equal(out[k], v), k
        assert bool(torch.isfinite(v).all()) and float(v.reshape(-1)[0]) > 0, k
    assert out["loss_lm"].dim() == 0 and tuple(out["loss_lm_per_utt"].shape) == (B,)
    with pytest.raises(ValueError, match="wl needs y"):
        losses.teacher_forced_losses(net, hps, x, xl, spec, yl, wl=wl, **kw)
    with pytest.raises(ValueError, match="go together"):
        losses.teacher_forced_losses(net, hps, x, xl, spec, yl, y=wav, **kw)


# ---- 6. errors before any launch, then a clean call -----------------------------------------------------------------------
def test_errors_are_raised_before_any_launch_and_a_clean_call_follows():
    net, wd = _net("tiny")
    wl = _wl("tiny", 22050)
    lib, s = _lib.load(), _lib.current_stream_ptr()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="shorter than one frame"):
        net.hidden_states(torch.zeros(2, 399, device=DEV))
    with pytest.raises(ValueError, match="shorter than one WavLM frame"):
        wl(torch.zeros(2, 549, device=DEV), torch.zeros(2, 549, device=DEV))  # ceil(320 * 549 / 441) = 399 samples
    with pytest.raises(ValueError, match="at most 512"):
        net.hidden_states(torch.zeros(1, 400 + 320 * 512, device=DEV))
    with pytest.raises(ValueError, match=r"\[B, L\]"):
        net.hidden_states(torch.zeros(2, 1, 800, device=DEV))
    with pytest.raises(ValueError, match="one shape"):
        wl(torch.zeros(2, 800, device=DEV), torch.zeros(2, 801, device=DEV))
    with pytest.raises(ValueError, match="HIP device"):
        wl.generator(torch.zeros(2, 800))
    with pytest.raises(ValueError, match=r"\[B, 1, L\]"):
        wl.generator(torch.zeros(2, 2, 800, device=DEV))
    with pytest.raises(ValueError, match="hidden must be"):
        wd.on_hidden(torch.zeros(2, 2, 3, 48, device=DEV))
    with pytest.raises(ValueError, match="wd=None"):
        losses.WavLMLoss(net, None, 22050).generator(torch.zeros(2, 800, device=DEV))
    with pytest.raises(ValueError, match="expects"):
        losses.WavLMLoss(net, discriminators.WavLMDiscriminator(48, 4, 8), 22050)
    x = torch.zeros(2, 800, device=DEV)
    out = torch.zeros(3, 2, 2, 48, device=DEV)
    ws = torch.zeros(1 << 16, device=DEV)
    calls = (lambda: lib.wetts_wavlm_forward(net._handle, _lib.ptr(x), 800, 2, 399, _lib.ptr(out), _lib.ptr(ws), 1 << 18, s),
             lambda: lib.wetts_wavlm_forward(net._handle, _lib.ptr(x), 800, 2, 800, _lib.ptr(out), _lib.ptr(ws), 64, s),
             lambda: lib.wetts_wavlm_forward(net._handle, _lib.ptr(x), 700, 2, 800, _lib.ptr(out), _lib.ptr(ws), 1 << 18, s),
             lambda: lib.wetts_wavlm_forward(net._handle, None, 800, 2, 800, _lib.ptr(out), _lib.ptr(ws), 1 << 18, s),
             lambda: lib.wetts_wavlm_conv(net._handle, 7, _lib.ptr(x), 1, 10, _lib.ptr(out), s),
             lambda: lib.wetts_wavlm_conv(net._handle, 1, _lib.ptr(x), 1, 2, _lib.ptr(out), s),
             lambda: lib.wetts_wavlm_layer(net._handle, 2, _lib.ptr(x), 1, 2, _lib.ptr(out), _lib.ptr(ws), s),
             lambda: lib.wetts_wavlm_attention(net._handle, 0, _lib.ptr(x), _lib.ptr(x), 1, 513, _lib.ptr(ws), _lib.ptr(out), s),
             lambda: lib.wetts_wavlm_resample(_lib.ptr(x), 800, 2, 800, 441, 320, 9, _lib.ptr(ws), 459, _lib.ptr(ws), 2000,
                                              _lib.ptr(out), s),
             lambda: lib.wetts_wavlm_resample(_lib.ptr(x), 800, 2, 800, 441, 320, 9, _lib.ptr(ws), 464, _lib.ptr(ws), 800,
                                              _lib.ptr(out), s),
             lambda: lib.wetts_wavlm_disc_forward(wd._handle, _lib.ptr(out), 2 * 2 * 48, 0, 2, _lib.ptr(x), _lib.ptr(ws), s),
             lambda: lib.wetts_wavlm_disc_pre(wd._handle, _lib.ptr(out), 2 * 2 * 48 + 1, 2, 2, _lib.ptr(x), s))
    for i, call in enumerate(calls):
        assert call() == -1, (i, _lib.last_error())  # WETTS_E_INVALID
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(x.abs().sum()) == 0.0  # nothing ran
    wav, rec, o = wo.reference("tiny", wo.SHAPES[1])
    got = wl(wav.to(DEV), rec.to(DEV))
    assert wo.within(wo.rel_err(got, o["loss_lm"]), wo.gate_of(wo.load_fixture("tiny", wo.SHAPES[1])["floor_loss_lm"]))
