"""GPU tier of teacher-forced reconstruction: SynthesizerTrn.reconstruct, wetts_amd.commons / wetts_amd.losses and the
C entries of csrc/losses.hip against the reference's fixtures (tests/golden/recon_*.npz) and the float64 oracle
(tests/recon_oracle.py, pinned to those fixtures by tests/test_cpu_recon.py).

Gates.  Stage tensors: those of tests/test_gpu_align.py.  Audio of the slice: 1e-4 abs RMS, the gate
tests/test_gpu_voice_conversion.py applies to the same encoder-to-decoder chain.  Reductions against float64 on the
device's own tensors: |gpu - f64| <= 1e-5 * sum|terms| / divisor (a fixed-order f32 tree over N <= 2^20 terms errs by at
most about 20 eps = 1.2e-6 of sum|terms|; 1e-5 is the project's stage gate).  loss_kl against the reference's value:
5e-4 * mean|terms| (inputs gated at 1e-4 relative RMS, the term quadratic in z_p - m_p, exp(-2 logs_p) another factor
of two, 1e-5 for the reduction).  loss_mel against the reference's value: recon_oracle.MEL_GATE, 4x the worst relative
difference measured (profiles/recon_margins.txt) -- the log-mel clamp at 1e-5 gives no derivable bound.
"""
import numpy as np
import pytest
import torch

from tests import align_oracle as ao, recon_oracle as ro, util
from tests.test_gpu_vc_oracle import LOCAL, REL_RMS
from wetts_amd import SynthesizerTrn, _lib, commons, config, losses, synth

pytestmark = pytest.mark.gpu

SPEC = ao.SPEC
DEV = "cuda"
AUDIO_ABS_RMS = 1e-4     # tests/test_gpu_voice_conversion.py:81
AUDIO_16BIT_RMS = 2e-3   # tests/test_gpu_voice_conversion.py:161
REDUCTION = 1e-5
KL_VS_REFERENCE = 5e-4

_NETS = {}
_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    import gc
    _NETS.clear()
    _CASES.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _case(name):
    if name not in _CASES:
        _CASES[name] = ro.load_recon_case(name)
    return _CASES[name]


def _case_net(c):
    key = (str(c["model"]), int(c["n_vocab"]), int(c["n_speakers"]), int(c["weight_seed"]))
    if key not in _NETS:
        cfg, sd, psd = util.vc_case_model(c, SPEC)
        net = SynthesizerTrn(int(c["n_vocab"]), SPEC, 32, n_speakers=int(c["n_speakers"]),
                             **config.MODEL_CONFIGS[str(c["model"])])
        net.load_state_dict(dict(sd, **psd)).to(DEV)
        _NETS[key] = net
    return _NETS[key]


def _hps(sr, **model):
    return config.HParams(data=dict(ro.MEL, sampling_rate=int(sr)), model=model, train=dict(c_mel=45, c_kl=1.0))


def _dev(c, net):
    x, xl, y, yl, sid, eps = (t.to(DEV) for t in ao.case_tensors(c))
    return x, xl, y, yl, (sid if net.n_speakers > 0 else None), eps


def _gates(got, ref):
    a, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert a.shape == r.shape, (a.shape, r.shape)
    scale = max(util.rms(r), 1e-30)
    return util.rms(a - r) / scale, float(np.abs(a - r).max()) / scale


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ro.RECON_CASES)
def test_reconstruct_matches_reference_fixture(name):
    """With the fixture's u: ids_slice equal, z_slice bit-equal to indexing the call's own z, the audio of the slice
    within 1e-4 abs RMS of the reference's, stage tensors at test_gpu_align.py's gates, loss_kl within
    5e-4 * mean|terms| of the reference's and, for the hop-256 cases, loss_mel within MEL_GATE."""
    c = _case(name)
    net = _case_net(c)
    seg = int(c["segment"])
    x, xl, y, yl, sid, eps = _dev(c, net)
    B = x.shape[0]
    ids_drawn, short = ro.slice_ids(c["u"], c["y_lengths"], seg)
    # the u of the fixture through the kernel that turns it into ids
    z_probe = torch.zeros(B, 1, int(y.shape[2]), device=DEV)
    _, ids_u = commons.rand_slice_segments(z_probe, yl, seg, u=torch.from_numpy(c["u"]).to(DEV))
    assert np.array_equal(ids_u.cpu().numpy(), c["ids_slice"]) and np.array_equal(ids_drawn, c["ids_slice"])
    o, ids, attn, x_mask, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q) = net.reconstruct(
        x, xl, y, yl, sid=sid, segment_size=seg, ids_slice=ids_u, eps_q=eps)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), c["ids_slice"])
    assert tuple(o.shape) == c["o"].shape == (B, 1, seg * net.hop_length)
    z_host = z.cpu().numpy()
    z_slice = net._last_recon["z_slice"].cpu().numpy()
    assert np.array_equal(z_slice, ro.slice_segments(z_host, c["ids_slice"], seg))
    rows = {"audio_abs_rms": util.rms(o.cpu().numpy() - c["o"]), "z_slice": _gates(z_slice, c["z_slice"])}
    stride = int(c["sub_stride"]) if "sub_stride" in c else None
    got = dict(z=z, z_p=z_p, m_p=m_p, logs_p=logs_p, m_q=m_q, logs_q=logs_q)
    for k in ao.STAGES:
        a = got[k].cpu().numpy()
        rows[k] = _gates(a[..., ::stride], c[k + "_sub"]) if stride else _gates(a, c[k])
    assert np.array_equal(attn[:, 0].cpu().numpy().astype(np.uint8), c["attn"])
    assert np.array_equal(y_mask[:, 0].cpu().numpy(), c["y_mask"]) and np.array_equal(x_mask[:, 0].cpu().numpy(), c["x_mask"])
    kl = float(losses.kl_loss(z_p, logs_q, m_p, logs_p, y_mask).cpu())
    rows["loss_kl"] = (kl, float(c["loss_kl"]), abs(kl - float(c["loss_kl"])) / float(c["kl_abs_mean"]))
    if name in ro.MEL_CASES:
        out = losses.teacher_forced_losses(net, _hps(int(c["sampling_rate_mel"])), x, xl, y, yl, sid=sid, segment_size=seg,
                                           ids_slice=ids_u, eps_q=eps)
        torch.cuda.synchronize()
        assert torch.equal(out["y_hat"], o) and torch.equal(out["ids_slice"], ids)
        mel = float(out["mel"].cpu())
        rows["loss_mel"] = (mel, float(c["loss_mel"]), abs(mel - float(c["loss_mel"])) / float(c["loss_mel"]))
        rows["y_mel"] = _gates(out["y_mel"].cpu().numpy(), c["y_mel"])
        rows["y_hat_mel_abs_rms"] = util.rms(out["y_hat_mel"].cpu().numpy() - c["y_hat_mel"])
        assert float(out["loss_mel"].cpu()) == np.float32(mel) * np.float32(45) and float(out["loss_kl"].cpu()) == float(out["kl"].cpu())
        assert float(out["kl"].cpu()) == kl
    print(name, "reconstruct vs reference:", rows)
    for k in ao.STAGES:
        assert rows[k][0] <= REL_RMS and rows[k][1] <= LOCAL, (k, rows)
    assert rows["audio_abs_rms"] <= AUDIO_ABS_RMS, rows
    assert rows["loss_kl"][2] <= KL_VS_REFERENCE, rows
    if name in ro.MEL_CASES:
        assert rows["loss_mel"][2] <= ro.MEL_GATE, rows


# ---- 2. reductions against float64 on the device's own tensors ---------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_l1_loss_against_float64(B):
    gen = torch.Generator().manual_seed(21)
    for N in (1, 63, 64, 65, 255, 1025):
        a, b = torch.randn(B, N, generator=gen), torch.randn(B, N, generator=gen) * 3.0
        total, per = losses.l1_loss(a.to(DEV), b.to(DEV), per_utterance=True)
        want = ro.l1_loss(a.numpy(), b.numpy())  # sum|terms| / divisor is the loss itself
        err_t = abs(float(total.cpu()) - want["total"]) / want["total"]
        err_p = float(np.abs(per.cpu().numpy() - want["per_utt"]).max() / want["per_utt"].min())
        print(f"l1_loss B={B} N={N}: rel err total {err_t:.3g} per-utterance {err_p:.3g}")
        assert err_t <= REDUCTION and (np.abs(per.cpu().numpy() - want["per_utt"]) <= REDUCTION * want["per_utt"]).all()
    a3 = torch.randn(B, 5, 13, generator=gen)  # any shape behind the batch dimension
    got = losses.l1_loss(a3.to(DEV), torch.zeros_like(a3).to(DEV))
    assert abs(float(got.cpu()) - float(a3.double().abs().mean())) <= REDUCTION * float(a3.double().abs().mean())


@pytest.mark.parametrize("B", [1, 3])
def test_kl_loss_against_float64(B):
    gen = torch.Generator().manual_seed(22)
    I = 192
    for T in (1, 5, 64, 67):
        lens = [T, max(1, T // 2), 1][:B]
        mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float()
        z_p, m_p = torch.randn(B, I, T, generator=gen), torch.randn(B, I, T, generator=gen)
        logs_q, logs_p = 0.3 * torch.randn(B, I, T, generator=gen), 0.3 * torch.randn(B, I, T, generator=gen)
        total, per = losses.kl_loss(*(t.to(DEV) for t in (z_p, logs_q, m_p, logs_p)), mask.unsqueeze(1).to(DEV),
                                    per_utterance=True)
        want = ro.kl_loss(z_p.numpy(), logs_q.numpy(), m_p.numpy(), logs_p.numpy(), mask.numpy())
        err_t = abs(float(total.cpu()) - want["total"]) / want["abs_total"]
        err_p = np.abs(per.cpu().numpy() - want["per_utt"]) / want["abs_per_utt"]
        print(f"kl_loss B={B} T={T}: err / (sum|terms| / divisor) total {err_t:.3g} per-utterance {err_p.max():.3g}")
        assert err_t <= REDUCTION and (err_p <= REDUCTION).all()
        flat = losses.kl_loss(*(t.to(DEV) for t in (z_p, logs_q, m_p, logs_p)), mask.to(DEV))  # [B, T] mask
        assert torch.equal(flat, total)


def test_reductions_repeat_and_ignore_what_the_mask_hides():
    """Bit-reproducible from run to run; a row alone gives the per-utterance value it gives inside a padded batch, with
    NaN behind the lengths."""
    gen = torch.Generator().manual_seed(23)
    B, I, T = 3, 192, 300
    lens = [300, 131, 7]
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float().to(DEV)
    ts = [torch.randn(B, I, T, generator=gen).to(DEV) for _ in range(4)]
    total, per = losses.kl_loss(*ts, mask, per_utterance=True)
    total2, per2 = losses.kl_loss(*ts, mask, per_utterance=True)
    assert torch.equal(total, total2) and torch.equal(per, per2)
    hide = (mask == 0).unsqueeze(1).expand(B, I, T)
    dirty = [torch.where(hide, torch.full_like(t, float("nan")), t) for t in ts]
    total3, per3 = losses.kl_loss(*dirty, mask, per_utterance=True)
    assert torch.equal(total, total3) and torch.equal(per, per3)
    for b, n in enumerate(lens):
        _, one = losses.kl_loss(*(t[b:b + 1, :, :n].contiguous() for t in ts), mask[b:b + 1, :n].contiguous(),
                                per_utterance=True)
        assert torch.equal(one[0], per[b]), b
    a, bb = torch.randn(B, 999, generator=gen).to(DEV), torch.randn(B, 999, generator=gen).to(DEV)
    t1, p1 = losses.l1_loss(a, bb, per_utterance=True)
    t2, p2 = losses.l1_loss(a, bb, per_utterance=True)
    assert torch.equal(t1, t2) and torch.equal(p1, p2)
    for b in range(B):
        assert torch.equal(losses.l1_loss(a[b:b + 1], bb[b:b + 1], per_utterance=True)[1][0], p1[b])


# ---- 3. slice_segments against torch indexing on the host --------------------------------------------------------------
def test_slice_segments_sweep_is_bit_equal_to_indexing():
    """C in {1, 3, 192}, starts {0, 1, 2, 3, len - segment} (one per row), segment * scale in {1, 4, 45 = 3 x 15, 2048},
    contiguous input and a view whose base pointer is offset by one float: every alignment of base and start, with and
    without the 16-byte path."""
    gen = torch.Generator().manual_seed(24)
    B = 5
    for C in (1, 3, 192):
        for seg, scale in ((1, 1), (4, 1), (3, 15), (8, 256)):
            L = seg * scale
            for tail, off in ((3, 0), (3, 1), (4, 0), (4, 1)):  # row strides that are and are not multiples of 4 floats
                T = L + 5 * scale + tail
                frames = (T - L) // scale  # the largest id
                ids = torch.tensor([0, 1, 2, 3, frames])
                store = torch.randn(B * C * T + 1, generator=gen)
                x = store[off:off + B * C * T].view(B, C, T)
                xd = store.to(DEV)[off:off + B * C * T].view(B, C, T)
                assert xd.data_ptr() % 16 == 4 * off
                got = commons.slice_segments(xd, ids.to(DEV), seg, scale=scale)
                want = torch.stack([x[b, :, int(i) * scale:int(i) * scale + L] for b, i in enumerate(ids)])
                assert tuple(got.shape) == (B, C, L) and torch.equal(got.cpu(), want), (C, seg, scale, off)
    # a batch / channel stride that is no multiple of 4 floats (a time slice of a wider tensor), start aligned
    wide = torch.randn(2, 3, 21, generator=gen)
    got = commons.slice_segments(wide.to(DEV)[:, :, :18], torch.tensor([4, 8]).to(DEV), 8)
    assert torch.equal(got.cpu(), torch.stack([wide[0, :, 4:12], wide[1, :, 8:16]]))


def test_rand_slice_segments_draws_valid_ids_under_the_seed():
    x = torch.arange(4 * 2 * 50, dtype=torch.float32).view(4, 2, 50).to(DEV)
    lens = torch.tensor([50, 8, 9, 30]).to(DEV)
    torch.manual_seed(77)
    a, ia = commons.rand_slice_segments(x, lens, 8)
    b, ib = commons.rand_slice_segments(x, lens, 8)
    torch.manual_seed(77)
    c, ic = commons.rand_slice_segments(x, lens, 8)
    assert torch.equal(ia, ic) and torch.equal(a, c) and not torch.equal(ia, ib)
    for ids in (ia, ib):
        assert ((ids >= 0) & (ids <= lens - 8)).all() and ids[1] == 0
    assert torch.equal(a.cpu(), torch.stack([x[i, :, int(s):int(s) + 8] for i, s in enumerate(ia)]).cpu())
    torch.manual_seed(78)
    u = commons.rand(4096, DEV).cpu()
    assert u.min() >= 0 and u.max() < 1 and abs(float(u.mean()) - 0.5) < 0.03
    assert torch.equal(u * 16777216.0, (u * 16777216.0).round())  # 24-bit mantissas
    _, i0 = commons.rand_slice_segments(x, None, 8, u=torch.tensor([0.0, 0.5, 1.0 - 2.0 ** -24, 0.99]))
    assert i0.tolist() == [0, 21, 42, 42]


# ---- 4. behaviour ------------------------------------------------------------------------------------------------------
def test_reconstruct_is_seeded_and_successive_calls_differ():
    c = _case("recon_aishell3_b4x600")
    net = _case_net(c)
    x, xl, y, yl, sid, _ = _dev(c, net)

    def run(seed=None):
        if seed is not None:
            torch.manual_seed(seed)
        o, ids, *_ = net.reconstruct(x, xl, y, yl, sid=sid, segment_size=8)
        torch.cuda.synchronize()
        return o.clone(), ids.clone()

    o1, i1 = run(5)
    o2, i2 = run()
    o3, i3 = run(5)
    assert torch.equal(i1, i3) and torch.equal(o1, o3)
    assert not torch.equal(i1, i2)
    for ids in (i1, i2):
        assert ((ids >= 0) & (ids <= yl - 8)).all()


@pytest.mark.parametrize("name", ["recon_tiny_b3", "recon_vits2_v1_b2"])
def test_row_alone_scores_as_in_the_padded_batch(name):
    """A row run alone at its own (Tx, Ty), with the same eps_q rows and the same id, gives the audio slice and the
    per-utterance KL (and, for the hop-256 case, mel) values it gives in the padded batch, bit for bit -- the whole
    call, and the reductions alone on the batch's own stage tensors cut to the row."""
    c = _case(name)
    net = _case_net(c)
    seg = int(c["segment"])
    x, xl, y, yl, sid, eps = _dev(c, net)
    ids = torch.from_numpy(c["ids_slice"]).to(DEV)
    hps = _hps(int(c["sampling_rate_mel"])) if name in ro.MEL_CASES else None
    mel_per = None
    if hps is not None:
        mel_per = losses.teacher_forced_losses(net, hps, x, xl, y, yl, sid=sid, segment_size=seg, ids_slice=ids,
                                               eps_q=eps)["mel_per_utt"].clone()
    o, _, _, _, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q) = net.reconstruct(x, xl, y, yl, sid=sid, segment_size=seg,
                                                                            ids_slice=ids, eps_q=eps)
    _, per = losses.kl_loss(z_p, logs_q, m_p, logs_p, y_mask, per_utterance=True)
    for r in range(x.shape[0]):
        n, tx = int(yl[r]), int(xl[r])
        _, one = losses.kl_loss(*(t[r:r + 1, :, :n].contiguous() for t in (z_p, logs_q, m_p, logs_p)),
                                y_mask[r:r + 1, :, :n].contiguous(), per_utterance=True)
        assert torch.equal(one[0], per[r]), r  # identical inputs: the reduction order is the row's own
        args = (x[r:r + 1, :tx], xl[r:r + 1], y[r:r + 1, :, :n].contiguous(), yl[r:r + 1])
        kw = dict(sid=None if sid is None else sid[r:r + 1], segment_size=seg, ids_slice=ids[r:r + 1],
                  eps_q=eps[r:r + 1, :, :n].contiguous())
        o1, i1, *_ = net.reconstruct(*args, **kw)
        la = net._last_recon
        _, alone = losses.kl_loss(la["z_p"], la["logs_q"], la["m_p"], la["logs_p"], la["y_mask"], per_utterance=True)
        torch.cuda.synchronize()
        assert torch.equal(i1, ids[r:r + 1])
        assert torch.equal(o1[0], o[r]), r
        assert torch.equal(alone[0], per[r]), (r, float(alone[0].cpu()), float(per[r].cpu()))
        if hps is not None:
            mel_alone = losses.teacher_forced_losses(net, hps, *args, **kw)["mel_per_utt"]
            assert torch.equal(mel_alone[0], mel_per[r]), (r, float(mel_alone[0].cpu()), float(mel_per[r].cpu()))


def test_garbage_beyond_the_lengths_changes_nothing():
    c = _case("recon_tiny_b3")
    net = _case_net(c)
    seg = int(c["segment"])
    x, xl, y, yl, sid, eps = _dev(c, net)
    ids = torch.from_numpy(c["ids_slice"]).to(DEV)

    def run(x_, y_):
        o, i, attn, _, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q) = net.reconstruct(x_, xl, y_, yl, sid=sid, segment_size=seg,
                                                                                   ids_slice=ids, eps_q=eps)
        total, per = losses.kl_loss(z_p, logs_q, m_p, logs_p, y_mask, per_utterance=True)
        torch.cuda.synchronize()
        return [t.clone() for t in (o, i, attn, total, per)]

    clean = run(x, y)
    gen = torch.Generator().manual_seed(5)
    fv = (torch.arange(y.shape[2])[None, :] < yl.cpu()[:, None]).to(DEV)
    pv = (torch.arange(x.shape[1])[None, :] < xl.cpu()[:, None]).to(DEV)
    y2 = torch.where(fv.unsqueeze(1), y, (1e3 * torch.randn(y.shape, generator=gen).abs()).to(DEV))
    x2 = torch.where(pv, x, torch.randint(0, int(c["n_vocab"]), x.shape, generator=gen).to(DEV))
    assert not torch.equal(y2, y) and not torch.equal(x2, x)
    for a, b in zip(clean, run(x2, y2)):
        assert torch.equal(a, b)


def test_one_read_back_and_other_entry_points_unchanged(monkeypatch):
    """Exactly one host read-back per reconstruct() call; infer() and align() give the same bits before and after."""
    c = _case("recon_tiny_b3")
    net = _case_net(c)
    x, xl, y, yl, sid, eps = _dev(c, net)

    def others():
        torch.manual_seed(9)
        o, attn, _, (z, *_) = net.infer(x, xl, sid=sid, noise_scale=0.667, noise_scale_w=0.8)
        a_attn, w, _, _, (az, az_p, *_) = net.align(x, xl, y, yl, sid=sid, eps_q=eps)
        torch.cuda.synchronize()
        return [t.clone() for t in (o, attn, z, a_attn, w, az, az_p)]

    before = others()
    calls = {"cpu": 0}
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        calls["cpu"] += 1
        return real_cpu(self, *a, **k)

    real_item = torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    try:
        net.reconstruct(x, xl, y, yl, sid=sid, segment_size=4, eps_q=eps)
        net.reconstruct(x, xl, y, yl, sid=sid, segment_size=4)
    finally:
        monkeypatch.undo()
    assert calls["cpu"] == 2 and torch.Tensor.item is real_item
    for a, b in zip(before, others()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_decoder_on_the_slice(dtype):
    c = _case("recon_vits2_v1_b2")
    net = _case_net(c)
    seg = int(c["segment"])
    x, xl, y, yl, sid, eps = _dev(c, net)
    ids = torch.from_numpy(c["ids_slice"]).to(DEV)
    kw = dict(sid=sid, segment_size=seg, ids_slice=ids, eps_q=eps)
    o32 = net.reconstruct(x, xl, y, yl, **kw)[0].clone()
    try:
        net.set_decoder_dtype(dtype)
        o16 = net.reconstruct(x, xl, y, yl, **kw)[0].clone()
    finally:
        net.set_decoder_dtype(torch.float32)
    back = net.reconstruct(x, xl, y, yl, **kw)[0]
    torch.cuda.synchronize()
    d = util.rms((o16 - o32).cpu().numpy())
    print(f"reconstruct decoder {dtype}: abs RMS vs f32 {d:.3g}")
    assert 0 < d <= AUDIO_16BIT_RMS and torch.equal(back, o32)


def test_vocos_head_decodes_the_slice():
    """Both Vocos heads (torch.istft and OnnxSTFT.inverse) on the slice: the decoder entry on z_slice, bit for bit."""
    c = _case("recon_tiny_vocos_b2")
    net = _case_net(c)
    x, xl, y, yl, sid, eps = _dev(c, net)
    ids = torch.from_numpy(c["ids_slice"]).to(DEV)
    try:
        for onnx in (False, True):
            net.set_is_onnx(onnx)
            o = net.reconstruct(x, xl, y, yl, sid=sid, segment_size=4, ids_slice=ids, eps_q=eps)[0]
            want = net.hifigan(net._last_recon["z_slice"], net._last_recon["g"])
            torch.cuda.synchronize()
            assert torch.equal(o, want) and torch.isfinite(o).all()
            if not onnx:
                assert util.rms(o.cpu().numpy() - c["o"]) <= AUDIO_ABS_RMS
    finally:
        net.set_is_onnx(False)


def test_mel_posterior_model_losses_equal_the_pieces_composed_by_hand():
    """vits2_v1 built with a mel posterior encoder (spec_channels = n_mel_channels, use_mel_posterior_encoder): the
    target mel is `spec` itself; teacher_forced_losses equals reconstruct + slice + mel + the two reductions."""
    n_mel, n_vocab, n_spk, seg = 80, 64, 2, 8
    mname = "vits2_v1"
    cfg = config.make_config(dict(config.MODEL_CONFIGS[mname]), n_vocab, n_spk)
    sd = dict(synth.make_state_dict(cfg, 31), **synth.make_posterior_state_dict(cfg, n_mel, 32))
    net = SynthesizerTrn(n_vocab, n_mel, seg, n_speakers=n_spk, **config.MODEL_CONFIGS[mname]).load_state_dict(sd).to(DEV)
    gen = torch.Generator().manual_seed(33)
    xl, yl = torch.tensor([7, 5]), torch.tensor([26, 19])
    x = torch.randint(0, n_vocab, (2, 7), generator=gen).to(DEV)
    spec = (torch.randn(2, n_mel, 26, generator=gen) * 2.0 - 4.0) * (torch.arange(26)[None, None] < yl[:, None, None])
    spec, xl, yl, sid = spec.to(DEV), xl.to(DEV), yl.to(DEV), torch.tensor([1, 0]).to(DEV)
    eps = torch.randn(2, 192, 26, generator=gen).to(DEV)
    hps = _hps(config.SAMPLING_RATES[mname], use_mel_posterior_encoder=True)
    torch.manual_seed(3)
    out = losses.teacher_forced_losses(net, hps, x, xl, spec, yl, sid=sid, eps_q=eps)  # the constructor's segment
    torch.manual_seed(3)
    o, ids, _, _, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q) = net.reconstruct(x, xl, spec, yl, sid=sid, eps_q=eps)
    M = ro.MEL
    y_mel = commons.slice_segments(spec, ids, seg)
    from wetts_amd import mel_spectrogram_torch
    y_hat_mel = mel_spectrogram_torch(o[:, 0], M["filter_length"], n_mel, hps.data.sampling_rate, M["hop_length"],
                                      M["win_length"], M["mel_fmin"], M["mel_fmax"])
    mel, mel_per = losses.l1_loss(y_mel, y_hat_mel, per_utterance=True)
    kl, kl_per = losses.kl_loss(z_p, logs_q, m_p, logs_p, y_mask, per_utterance=True)
    torch.cuda.synchronize()
    assert torch.equal(out["ids_slice"], ids) and torch.equal(out["y_hat"], o) and tuple(o.shape) == (2, 1, seg * 256)
    assert torch.equal(out["y_mel"], y_mel) and torch.equal(out["y_hat_mel"], y_hat_mel)
    assert torch.equal(y_mel.cpu(), torch.stack([spec[b, :, int(i):int(i) + seg] for b, i in enumerate(ids)]).cpu())
    assert torch.equal(out["mel"], mel) and torch.equal(out["mel_per_utt"], mel_per)
    assert torch.equal(out["kl"], kl) and torch.equal(out["kl_per_utt"], kl_per)
    assert float(out["loss_mel"].cpu()) == float(np.float32(mel.cpu()) * np.float32(45)) and torch.equal(out["loss_kl"], kl)
    want = ro.l1_loss(y_mel.cpu().numpy(), y_hat_mel.cpu().numpy())
    assert abs(float(mel.cpu()) - want["total"]) <= REDUCTION * want["total"]
    with pytest.raises(ValueError, match="hop_length"):
        losses.teacher_forced_losses(net, config.HParams(data=dict(ro.MEL, hop_length=128, sampling_rate=22050), model={},
                                                         train=dict(c_mel=45, c_kl=1.0)), x, xl, spec, yl, sid=sid)


def test_short_row_and_bad_ids_raise_and_the_model_stays_usable():
    c = _case("recon_tiny_b3")
    net = _case_net(c)
    seg = int(c["segment"])
    x, xl, y, yl, sid, eps = _dev(c, net)
    ids = torch.from_numpy(c["ids_slice"]).to(DEV)
    kw = dict(sid=sid, segment_size=seg, ids_slice=ids, eps_q=eps)
    ref = net.reconstruct(x, xl, y, yl, **kw)[0].clone()
    short = yl.clone()
    short[1] = seg - 1  # a row shorter than the segment (still at least as long as its text?  no: see below)
    xs = xl.clone()
    xs[1] = seg - 1
    with pytest.raises(ValueError, match="shorter than the segment"):
        net.reconstruct(x, xs, y, short, sid=sid, segment_size=seg, eps_q=eps)
    assert net.last_status & _lib.STATUS_SEGMENT_LONGER
    bad = ids.clone()
    bad[2] = yl[2] - seg + 1  # one frame past the last valid start
    with pytest.raises(ValueError, match="ids_slice"):
        net.reconstruct(x, xl, y, yl, sid=sid, segment_size=seg, ids_slice=bad, eps_q=eps)
    neg = ids.clone()
    neg[0] = -1
    with pytest.raises(ValueError, match="ids_slice"):
        net.reconstruct(x, xl, y, yl, sid=sid, segment_size=seg, ids_slice=neg, eps_q=eps)
    with pytest.raises(ValueError, match="more phonemes than frames"):  # align()'s errors carry over
        net.reconstruct(x, xl, y, torch.tensor([37, 6, 29]).to(DEV), **kw)
    with pytest.raises(IndexError):
        net.reconstruct(x, xl, y, yl, sid=torch.tensor([0, 3, 1]).to(DEV), segment_size=seg, ids_slice=ids, eps_q=eps)
    with pytest.raises(ValueError, match="segment_size must be"):
        net.reconstruct(x, xl, y, yl, sid=sid, segment_size=int(y.shape[2]) + 1)
    again = net.reconstruct(x, xl, y, yl, **kw)[0]
    torch.cuda.synchronize()
    assert torch.equal(again, ref) and net.last_status == 0
