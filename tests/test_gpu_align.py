"""GPU tier of forced alignment: SynthesizerTrn.align, the scores / path-to-durations / counts-to-lengths entries and
infer(durations=) against the reference's fixtures (tests/golden/align_*.npz) and the float64 oracle
(tests/align_oracle.py, pinned to those fixtures by tests/test_cpu_align.py).

A MAS path is a discrete function of its scores, so equality with the reference is demanded only where the fixture
generator established that the path is stable (eighteen searches agree); elsewhere a path is judged by its float64
score against the float64 optimum, with a margin derived from the local-error gate, and by being a valid monotonic
path.  Stage tensors pass the project's gates: rel RMS <= 1e-5 and max |d| / rms(ref) <= 1e-4."""
import numpy as np
import pytest
import torch

from tests import align_oracle as ao, util
from tests.test_gpu_parity import ABS_RMS_GATE, ABS_RMS_OURS
from tests.test_gpu_vc_oracle import FLOW_MODELS, LOCAL, REL_RMS, SHAPES
from wetts_amd import SynthesizerTrn, _lib, config, synth

pytestmark = pytest.mark.gpu

SPEC = ao.SPEC
DEV = "cuda"


def vo():
    from oracle import vits_oracle
    return vits_oracle


# ---- helpers -----------------------------------------------------------------------------------------------------------
_NETS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """The models this module caches are destroyed when it is done (with their decoder fork streams), so the modules
    that run after it start from the device state they start from without it."""
    yield
    import gc
    _NETS.clear()
    _SWEEP.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _case_net(c, with_posterior=True):
    key = (str(c["model"]), int(c["n_vocab"]), int(c["n_speakers"]), int(c["weight_seed"]), with_posterior)
    if key not in _NETS:
        cfg, sd, psd = util.vc_case_model(c, SPEC)
        net = SynthesizerTrn(int(c["n_vocab"]), SPEC, 32, n_speakers=int(c["n_speakers"]),
                             **config.MODEL_CONFIGS[str(c["model"])])
        net.load_state_dict(dict(sd, **psd) if with_posterior else sd).to(DEV)
        _NETS[key] = (net, cfg, sd, psd)
    return _NETS[key]


def _synthetic(mname, n_vocab=40, n_spk=3, wseed=81, pseed=82):
    key = ("syn", mname, n_vocab, n_spk, wseed, pseed)
    if key not in _NETS:
        cfg = config.make_config(dict(config.MODEL_CONFIGS[mname]), n_vocab, n_spk)
        sd = synth.make_state_dict(cfg, wseed)
        psd = synth.make_posterior_state_dict(cfg, SPEC, pseed)
        net = SynthesizerTrn(n_vocab, SPEC, 32, n_speakers=n_spk, **config.MODEL_CONFIGS[mname])
        net.load_state_dict(dict(sd, **psd)).to(DEV)
        _NETS[key] = (net, util.cfg_dict(cfg), util.vc_weights(cfg, sd, psd, torch.float64))
    return _NETS[key]


def _align(net, x, xl, y, yl, sid, eps):
    """align() on CPU tensors -> dict of CPU tensors (the returned tuple and the kept stage tensors)."""
    sid_d = sid.to(DEV) if net.n_speakers > 0 else None
    attn, w, x_mask, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q) = net.align(
        x.to(DEV), xl.to(DEV), y.to(DEV), yl.to(DEV), sid=sid_d, eps_q=None if eps is None else eps.to(DEV))
    torch.cuda.synchronize()
    out = dict(attn=attn, w=w, x_mask=x_mask, y_mask=y_mask, z=z, z_p=z_p, m_p=m_p, logs_p=logs_p, m_q=m_q, logs_q=logs_q)
    la = net._last_align
    out.update(neg_cent=la["neg_cent"], path=la["path"], cum=la["cum"], frame2phone=la["frame2phone"], stats=la["stats"])
    return {k: v.detach().cpu() for k, v in out.items()}


def _gates(got, ref):
    a, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert a.shape == r.shape, (a.shape, r.shape)
    scale = max(util.rms(r), 1e-30)
    return util.rms(a - r) / scale, (float(np.abs(a - r).max()) / scale if a.size else 0.0)


def _check_search(tag, neg_cent, xl, yl, path, w, cum, f2p):
    """Search consistency: wetts_mas over the device's own scores is bit-for-bit the numpy search over the same array,
    and w / cum / frame2phone are numpy's column sum, cumsum and argmax of that path (-1 on rows without a cell)."""
    nc, xl, yl = np.asarray(neg_cent), np.asarray(xl), np.asarray(yl)
    want = vo().maximum_path_numpy(nc, yl, xl)
    assert np.array_equal(np.asarray(path), want), tag
    ws = want.sum(1).astype(np.float32)
    assert np.array_equal(np.asarray(w), ws), tag
    assert np.array_equal(np.asarray(cum), np.cumsum(ws, axis=-1, dtype=np.float32)), tag
    idx = np.where(want.sum(2) > 0, want.argmax(2), -1).astype(np.int32)
    assert np.array_equal(np.asarray(f2p), idx), tag


def _raw_search(nc_dev, xl, yl):
    """wetts_mas + wetts_path_to_durations on a device score tensor -> (path, w, cum, frame2phone, attn) on the CPU."""
    lib = _lib.load()
    B, Ty, Tx = nc_dev.shape
    t_xs = torch.as_tensor(np.asarray(xl), dtype=torch.int32).to(DEV)
    t_ys = torch.as_tensor(np.asarray(yl), dtype=torch.int32).to(DEV)
    path = torch.empty(B, Ty, Tx, dtype=torch.int32, device=DEV)
    values = torch.empty(B * Ty * Tx, dtype=torch.float32, device=DEV)
    w, cum = torch.empty(B, Tx, device=DEV), torch.empty(B, Tx, device=DEV)
    f2p = torch.empty(B, Ty, dtype=torch.int32, device=DEV)
    attn = torch.empty(B, Ty, Tx, device=DEV)
    s = _lib.current_stream_ptr()
    _lib.check(lib.wetts_mas(_lib.ptr(nc_dev), _lib.ptr(t_ys), _lib.ptr(t_xs), B, Ty, Tx, _lib.ptr(path), _lib.ptr(values),
                             values.numel() * 4, s), "mas")
    _lib.check(lib.wetts_path_to_durations(_lib.ptr(path), _lib.ptr(t_ys), _lib.ptr(t_xs), B, Tx, Ty, _lib.ptr(w),
                                           _lib.ptr(cum), _lib.ptr(f2p), _lib.ptr(attn), s), "path_to_durations")
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (path, w, cum, f2p, attn))


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ao.ALIGN_CASES)
def test_align_matches_reference_fixture(name):
    c = ao.load_align_case(name)
    net, cfg, sd, psd = _case_net(c)
    x, xl, y, yl, sid, eps = ao.case_tensors(c)
    got = _align(net, x, xl, y, yl, sid, eps)
    B, Ty, Tx = c["attn"].shape
    assert tuple(got["attn"].shape) == (B, 1, Ty, Tx) and tuple(got["w"].shape) == (B, 1, Tx)
    assert tuple(got["x_mask"].shape) == (B, 1, Tx) and tuple(got["y_mask"].shape) == (B, 1, Ty)
    stride = int(c["sub_stride"]) if "sub_stride" in c else None
    rows = {}
    for k in ao.STAGES:
        a = got[k].numpy()
        rows[k] = _gates(a[..., ::stride], c[k + "_sub"]) if stride else _gates(a, c[k])
    valid = ao.valid_mask(c["x_lengths"], c["y_lengths"], Tx, Ty)
    nc = got["neg_cent"].numpy()
    rows["neg_cent"] = (_gates(nc[:, ::stride][valid[:, ::stride]], c["neg_cent_sub"][valid[:, ::stride]]) if stride
                        else _gates(nc[valid], c["neg_cent"][valid]))
    rows["attn_equal"] = bool(np.array_equal(got["attn"][:, 0].numpy().astype(np.uint8), c["attn"]))
    print(name, "align vs reference (rel RMS, max|d|/rms):", rows)
    assert np.array_equal(got["x_mask"][:, 0].numpy(), c["x_mask"]) and np.array_equal(got["y_mask"][:, 0].numpy(), c["y_mask"])
    for k in ao.STAGES[:2] + ao.STAGES[4:]:  # z, z_p, m_q, logs_q first: a path difference would show in m_p / logs_p
        assert rows[k][0] <= REL_RMS and rows[k][1] <= LOCAL, (k, rows)
    assert rows["attn_equal"], rows
    assert np.array_equal(got["w"][:, 0].numpy(), c["w"])
    for k in ("m_p", "logs_p"):  # (neg_cent against the reference's f32 is printed; its gate is the float64 sweep's)
        assert rows[k][0] <= REL_RMS and rows[k][1] <= LOCAL, (k, rows)
    assert torch.equal(got["w"][:, 0].sum(-1), yl.float())
    assert torch.equal(got["attn"][:, 0].sum(-1), got["y_mask"][:, 0])
    _check_search(name, got["neg_cent"], xl, yl, got["path"], got["w"][:, 0], got["cum"], got["frame2phone"])


# ---- 2 / 3. the scores kernel alone, and the search over its output ----------------------------------------------------
_SWEEP = {}
SWEEP_TX = [1, 5, 31, 33, 128, 200]
SWEEP_TY = [1, 7, 63, 65, 600, 1000]


def _sweep_stages(mname):
    """z_p [3,I,1000] and m_p | logs_p [3,2I,200] of the float64 oracle on a ragged batch, once per model; the sweep
    slices them (valid lengths shrink with the slice) and rounds to float32 once."""
    if mname not in _SWEEP:
        n_vocab, n_spk = (256, 218) if mname == "v1" else (40, 3)
        net, cd, W = _synthetic(mname, n_vocab, n_spk)
        gen = torch.Generator().manual_seed(11)
        xl, yl = torch.tensor([200, 101, 1]), torch.tensor([1000, 577, 1])
        x = torch.randint(0, n_vocab, (3, 200), generator=gen)
        y = torch.rand(3, SPEC, 1000, generator=gen) ** 4 * 20.0
        y = y * (torch.arange(1000)[None, None, :] < yl[:, None, None])
        sid = torch.randint(0, n_spk, (3,), generator=gen)
        eps = torch.randn(3, cd["inter_channels"], 1000, generator=gen)
        st = ao.oracle_align(W, cd, x, xl, y, yl, sid, eps)
        _SWEEP[mname] = (net, st["z_p"].float(), torch.cat([st["m_p_x"], st["logs_p_x"]], 1).float(), xl, yl)
    return _SWEEP[mname]


@pytest.mark.parametrize("mname", ["tiny", "v1"])
def test_scores_kernel_sweep_against_float64(mname):
    """wetts_align_scores on float32 inputs against float64 scores of the same rounded inputs, valid cells only, from
    (1, 1, 1) through partial tiles in both dimensions.  Gate per shape: the larger of the project's stage gates and
    twice the error of the reference's f32 four-term expression (torch CPU, same inputs) against the same float64
    values.  Then the search over the kernel's own output (test 3 of the issue)."""
    net, z_all, stats_all, xl0, yl0 = _sweep_stages(mname)
    lib = _lib.load()
    I = z_all.shape[1]
    shapes = [(1, 1, 1)] + [(3, tx, ty) for tx in SWEEP_TX for ty in SWEEP_TY]
    worst = [0.0, 0.0, 0.0, 0.0]
    for B, Tx, Ty in shapes:
        z = z_all[:B, :, :Ty].contiguous()
        stats = stats_all[:B, :, :Tx].contiguous()
        xl, yl = np.minimum(xl0[:B].numpy(), Tx), np.minimum(yl0[:B].numpy(), Ty)
        nc_dev = torch.empty(B, Ty, Tx, device=DEV)
        z_dev, stats_dev = z.to(DEV), stats.to(DEV)  # (held: a temporary's memory could be handed out again)
        _lib.check(lib.wetts_align_scores(net._handle, _lib.ptr(z_dev), _lib.ptr(stats_dev), B, Tx, Ty,
                                          _lib.ptr(nc_dev), _lib.current_stream_ptr()), "align_scores")
        torch.cuda.synchronize()
        got = nc_dev.cpu().numpy()
        assert np.isfinite(got).all(), (Tx, Ty)
        want = ao.neg_cent_f64(z, stats[:, :I], stats[:, I:]).numpy()
        ref32 = ao.neg_cent_four_term(z, stats[:, :I], stats[:, I:]).numpy()
        v = ao.valid_mask(xl, yl, Tx, Ty)
        g_rel, g_loc = _gates(got[v], want[v])
        r_rel, r_loc = _gates(ref32[v], want[v])
        print(f"{mname} scores B={B} Tx={Tx} Ty={Ty}: kernel (rel RMS {g_rel:.3g}, max|d|/rms {g_loc:.3g})  "
              f"reference f32 expression (rel RMS {r_rel:.3g}, max|d|/rms {r_loc:.3g})")
        worst = [max(a, b) for a, b in zip(worst, (g_rel, g_loc, r_rel, r_loc))]
        assert g_rel <= max(REL_RMS, 2 * r_rel) and g_loc <= max(LOCAL, 2 * r_loc), (mname, B, Tx, Ty)
        xs = np.minimum(xl, yl)  # a monotonic path needs t_x <= t_y
        path, w, cum, f2p, attn = _raw_search(nc_dev, xs, yl)
        _check_search((mname, Tx, Ty), got, xs, yl, path, w, cum, f2p)
        assert np.array_equal(attn.numpy(), path.numpy().astype(np.float32))
    print(f"{mname} scores sweep worst: kernel (rel RMS {worst[0]:.3g}, max|d|/rms {worst[1]:.3g})  reference f32 "
          f"expression (rel RMS {worst[2]:.3g}, max|d|/rms {worst[3]:.3g})")


# ---- 4. oracle sweep where ties may occur ------------------------------------------------------------------------------
def _sweep_batch(B, Ty, lengths, tx_cap, n_vocab, seed, n_spk=3):
    gen = torch.Generator().manual_seed(seed)
    yl = torch.tensor(lengths, dtype=torch.long)
    xl = torch.clamp(torch.minimum(yl, torch.tensor(tx_cap)), min=1)
    Tx = int(xl.max())
    y = torch.rand(B, SPEC, Ty, generator=gen) ** 4 * 20.0
    y = y * (torch.arange(Ty)[None, None, :] < yl[:, None, None])
    x = torch.randint(0, n_vocab, (B, Tx), generator=gen)
    sid = torch.randint(0, n_spk, (B,), generator=gen)
    eps = torch.randn(B, 192, Ty, generator=gen)
    return x, xl, y, yl, sid, eps


@pytest.mark.parametrize("mname", FLOW_MODELS)
def test_align_oracle_sweep_path_judged_by_score(mname):
    """align() against the float64 oracle at the voice-conversion sweep's SHAPES crossed with Tx in {1, 2, Ty/2, Ty}.
    Stage tensors pass the gates (m_p / logs_p against the oracle's prior expanded along the DEVICE's path, so a
    legitimate path difference is not charged to them).  The path is judged by score:
        S(P_gpu) >= S(P_64) - 2 * t_y * 1e-4 * rms(neg_cent),
    S the float64 score along a path: each of the t_y cells of either path is within the local gate of its float64
    value, so the device's optimum cannot fall further than that behind the float64 optimum.  Derived, not measured."""
    net, cd, W = _synthetic(mname)
    differ = total = 0
    worst = {}
    for i, (B, Ty, lengths) in enumerate(SHAPES):
        for tx_cap in sorted({1, 2, max(1, Ty // 2), Ty}):
            x, xl, y, yl, sid, eps = _sweep_batch(B, Ty, lengths, tx_cap, 40, seed=300 + 10 * i + tx_cap)
            got = _align(net, x, xl, y, yl, sid, eps)
            ref = ao.oracle_align(W, cd, x, xl, y, yl, sid, eps)
            tag = (mname, B, Ty, tx_cap)
            assert torch.equal(got["y_mask"].double(), ref["y_mask"]) and torch.equal(got["x_mask"].double(), ref["x_mask"]), tag
            p_gpu = got["attn"][:, 0].numpy().astype(np.int32)
            ao.check_monotonic(p_gpu, xl, yl)
            ref = dict(ref, m_p=ao.expand(torch.from_numpy(p_gpu), ref["m_p_x"]),
                       logs_p=ao.expand(torch.from_numpy(p_gpu), ref["logs_p_x"]))
            for k in ao.STAGES:
                rel, loc = _gates(got[k].numpy(), ref[k].numpy())
                wk = worst.setdefault(k, [0.0, 0.0])
                wk[0], wk[1] = max(wk[0], rel), max(wk[1], loc)
                assert rel <= REL_RMS and loc <= LOCAL, (tag, k, rel, loc)
            nc64 = ref["neg_cent"].numpy()
            v = ao.valid_mask(xl, yl, nc64.shape[2], nc64.shape[1])
            rel, loc = _gates(got["neg_cent"].numpy()[v], nc64[v])
            wk = worst.setdefault("neg_cent", [0.0, 0.0])
            wk[0], wk[1] = max(wk[0], rel), max(wk[1], loc)
            margin = 2.0 * yl.numpy() * LOCAL * util.rms(nc64[v])
            s_gpu, s_64 = ao.path_score(nc64, p_gpu), ao.path_score(nc64, ref["path"])
            assert (s_gpu >= s_64 - margin).all(), (tag, s_gpu, s_64, margin)
            _check_search(tag, got["neg_cent"], xl, yl, got["path"], got["w"][:, 0], got["cum"], got["frame2phone"])
            total += 1
            differ += int(not np.array_equal(p_gpu, ref["path"]))
    print(f"{mname} align sweep: {differ} of {total} cases differ from the float64 path; worst (rel RMS, max|d|/rms):",
          {k: (float(f"{v[0]:.3g}"), float(f"{v[1]:.3g}")) for k, v in worst.items()})


# ---- 5. infer(durations=) ----------------------------------------------------------------------------------------------
DURATION_CASES = ["tiny_sdp_b3", "tiny_dp_b2", "tiny_sdp_nonoise", "tiny_sdp_single", "tiny_preconv2_spk_b3",
                  "tiny_mono_post_b2", "tiny_mono_inter_b3", "v1_b2", "v3_b2", "vits2_v1_b2", "tiny_vocos_b2"]


def _infer_net(case):
    cfg, sd, W, blob = util.case_model(case)
    net = SynthesizerTrn(int(case["n_vocab"]), 513, 32, n_speakers=int(case["n_speakers"]), **util.model_dict(case))
    net.load_state_dict(sd)
    return net.to(DEV)


@pytest.mark.parametrize("name", DURATION_CASES)
def test_infer_with_given_durations_reproduces_the_golden(name):
    """durations = the golden's attn summed over frames, with its eps_z: attn and y_mask equal, z_p / z and the audio
    within the gates of tests/test_gpu_parity.py; the duration predictor's arguments are ignored."""
    case = util.load_case(name)
    assert "attn" in case and "eps_z" in case
    net = _infer_net(case)
    ns = float(case["scales"][0])
    attn_ref = case["attn"].reshape(case["attn"].shape[0], -1, case["attn"].shape[-1])  # [B,Ty,Tx]
    dur = torch.from_numpy(attn_ref.sum(1).astype(np.int64))
    x, xl, sid = util.t(case["x"]).to(DEV), util.t(case["x_lengths"]).to(DEV), util.t(case["sid"]).to(DEV)
    o, attn, y_mask, (z, z_p, m_p, logs_p) = net.infer(x, xl, sid=sid, noise_scale=ns, length_scale=7.0, noise_scale_w=3.0,
                                                       eps_z=util.t(case["eps_z"]).to(DEV), durations=dur.to(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(attn.cpu().numpy().reshape(attn_ref.shape).astype(np.uint8), attn_ref.astype(np.uint8))
    assert np.array_equal(y_mask.cpu().numpy(), case["y_mask"])
    rows = {"z": util.rel_rms(z.cpu().numpy(), case["z"]), "audio_abs_rms": util.rms(o.cpu().numpy() - case["audio"])}
    if "z_p" in case:
        rows["z_p"] = util.rel_rms(z_p.cpu().numpy(), case["z_p"])
    print(name, "infer(durations=):", rows)
    assert rows.get("z_p", 0.0) < 1e-4 and rows["z"] < 2e-4
    assert rows["audio_abs_rms"] < ABS_RMS_OURS < ABS_RMS_GATE
    o2, attn2, *_ = net.infer(x, xl, sid=sid, noise_scale=ns, eps_z=util.t(case["eps_z"]).to(DEV),
                              durations=dur.unsqueeze(1).to(device=DEV, dtype=torch.int32))  # [B,1,Tx], another int type
    assert torch.equal(o2, o) and torch.equal(attn2, attn)


def test_infer_without_durations_is_unchanged_by_a_durations_call():
    case = util.load_case("tiny_sdp_b3")
    net = _infer_net(case)
    x, xl, sid = util.t(case["x"]).to(DEV), util.t(case["x_lengths"]).to(DEV), util.t(case["sid"]).to(DEV)

    def seeded():
        torch.manual_seed(1234)
        o, attn, y_mask, (z, z_p, m_p, logs_p) = net.infer(x, xl, sid=sid, noise_scale=0.667, noise_scale_w=0.8)
        torch.cuda.synchronize()
        return [t.clone() for t in (o, attn, y_mask, z, z_p, m_p, logs_p)]

    before = seeded()
    net.infer(x, xl, sid=sid, durations=torch.full(tuple(x.shape), 3, dtype=torch.long, device=DEV))
    after = seeded()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_infer_durations_errors():
    case = util.load_case("tiny_sdp_b3")
    net = _infer_net(case)
    x, xl, sid = util.t(case["x"]).to(DEV), util.t(case["x_lengths"]).to(DEV), util.t(case["sid"]).to(DEV)
    B, Tx = x.shape
    good = torch.full((B, Tx), 2, dtype=torch.long, device=DEV)
    bad = good.clone()
    bad[0, 1] = -1
    with pytest.raises(ValueError, match="negative"):
        net.infer(x, xl, sid=sid, durations=bad)
    assert net.last_status & _lib.STATUS_DURATION_NEGATIVE
    with pytest.raises(ValueError, match="durations must be"):
        net.infer(x, xl, sid=sid, durations=good[:, :-1])
    # a negative count BEHIND x_lengths is masked like any other padding, and all-zero counts give one silent frame
    pad = good.clone()
    pad[1, int(case["x_lengths"][1]):] = -5
    o, attn, y_mask, _ = net.infer(x, xl, sid=sid, durations=pad)
    o_ref, attn_ref, *_ = net.infer(x, xl, sid=sid, durations=good, eps_z=torch.zeros(B, 192, int(y_mask.shape[-1])),
                                    noise_scale=0.0)
    assert torch.equal(attn, attn_ref)
    assert torch.equal(y_mask[:, 0].sum(-1).cpu(), 2.0 * util.t(case["x_lengths"]).float())
    _, _, ym0, _ = net.infer(x, xl, sid=sid, durations=torch.zeros_like(good))
    assert tuple(ym0.shape) == (B, 1, 1)  # clamp_min(sum, 1), as durations_to_lengths


# ---- 6. round trip -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["align_tiny_b3", "align_tiny_dp_b2", "align_tiny_nospk_b2"])
def test_align_then_infer_round_trip(name):
    """align() -> w -> infer(durations=w, noise_scale=0): the recording's own frame counts and, bitwise, align()'s
    expanded prior mean."""
    c = ao.load_align_case(name)
    net, *_ = _case_net(c)
    x, xl, y, yl, sid, eps = ao.case_tensors(c)
    got = _align(net, x, xl, y, yl, sid, eps)
    sid_d = sid.to(DEV) if net.n_speakers > 0 else None
    B, Ty = y.shape[0], y.shape[2]
    o, attn, y_mask, (z, z_p, m_p, logs_p) = net.infer(x.to(DEV), xl.to(DEV), sid=sid_d, noise_scale=0,
                                                       eps_z=torch.zeros(B, 192, Ty, device=DEV),
                                                       durations=got["w"].to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(net._last["y_lengths"].cpu(), yl)
    assert torch.equal(m_p.cpu(), got["m_p"]) and torch.equal(logs_p.cpu(), got["logs_p"])
    assert torch.equal(attn.cpu(), got["attn"]) and torch.equal(y_mask.cpu(), got["y_mask"])
    assert tuple(o.shape) == (B, 1, Ty * net.hop_length)


# ---- 7. errors, padding, raggedness ------------------------------------------------------------------------------------
def test_align_errors_and_model_stays_usable():
    c = ao.load_align_case("align_tiny_b3")
    net, cfg, sd, psd = _case_net(c)
    x, xl, y, yl, sid, eps = ao.case_tensors(c)
    ref = _align(net, x, xl, y, yl, sid, eps)
    with pytest.raises(ValueError, match="more phonemes than frames"):
        _align(net, x, torch.tensor([12, 7, 9]), y, torch.tensor([37, 6, 29]), sid, eps)
    assert net.last_status & _lib.STATUS_ALIGN_TEXT_LONGER
    with pytest.raises(IndexError):
        _align(net, x, xl, y, yl, torch.tensor([0, 3, 1]), eps)
    with pytest.raises(IndexError):
        _align(net, torch.full_like(x, 40), xl, y, yl, sid, eps)
    bare, *_ = _case_net(c, with_posterior=False)
    with pytest.raises(_lib.WettsError, match="enc_q"):
        _align(bare, x, xl, y, yl, sid, eps)
    with pytest.raises(_lib.WettsError, match="enc_q"):  # the error voice_conversion gives
        bare.voice_conversion(y.to(DEV), yl.to(DEV), sid.to(DEV), sid.to(DEV))
    again = _align(net, x, xl, y, yl, sid, eps)
    for k in ("attn", "w", "z_p", "m_p", "neg_cent"):
        assert torch.equal(again[k], ref[k]), k
    assert net.last_status == 0


@pytest.mark.parametrize("name", ["align_tiny_b3", "align_aishell3_b4x600"])
def test_align_ignores_garbage_beyond_the_lengths(name):
    """Large values in y beyond y_lengths and arbitrary valid ids in x beyond x_lengths change no valid output."""
    c = ao.load_align_case(name)
    net, *_ = _case_net(c)
    x, xl, y, yl, sid, eps = ao.case_tensors(c)
    clean = _align(net, x, xl, y, yl, sid, eps)
    gen = torch.Generator().manual_seed(5)
    fv = torch.arange(y.shape[2])[None, :] < yl[:, None]
    pv = torch.arange(x.shape[1])[None, :] < xl[:, None]
    y2 = torch.where(fv.unsqueeze(1), y, 1e3 * torch.randn(y.shape, generator=gen).abs())
    x2 = torch.where(pv, x, torch.randint(0, int(c["n_vocab"]), x.shape, generator=gen))
    assert not torch.equal(y2, y) and not torch.equal(x2, x)
    dirty = _align(net, x2, xl, y2, yl, sid, eps)
    for k in ("attn", "w", "x_mask", "y_mask"):
        assert torch.equal(clean[k], dirty[k]), k
    for k in ao.STAGES:
        v = fv.unsqueeze(1).expand_as(clean[k])
        assert torch.equal(clean[k][v], dirty[k][v]), k
    v = torch.from_numpy(ao.valid_mask(xl, yl, x.shape[1], y.shape[2]))
    assert torch.equal(clean["neg_cent"][v], dirty["neg_cent"][v])


@pytest.mark.parametrize("name", ["align_tiny_b3", "align_aishell3_b4x600"])
def test_align_row_alone_equals_row_in_padded_batch(name):
    """Every row run alone at its own (Tx, Ty): attn bitwise the batch's, stage tensors within the gates."""
    c = ao.load_align_case(name)
    net, *_ = _case_net(c)
    x, xl, y, yl, sid, eps = ao.case_tensors(c)
    full = _align(net, x, xl, y, yl, sid, eps)
    for b in range(x.shape[0]):
        tx, ty = int(xl[b]), int(yl[b])
        one = _align(net, x[b:b + 1, :tx], xl[b:b + 1], y[b:b + 1, :, :ty].contiguous(), yl[b:b + 1], sid[b:b + 1],
                     eps[b:b + 1, :, :ty].contiguous())
        assert torch.equal(one["attn"][0, 0], full["attn"][b, 0, :ty, :tx]), b
        assert torch.equal(one["w"][0, 0], full["w"][b, 0, :tx]), b
        for k in ao.STAGES:
            rel, loc = _gates(one[k][0].numpy(), full[k][b, :, :ty].numpy())
            assert rel <= REL_RMS and loc <= LOCAL, (b, k, rel, loc)


# ---- 8. stream discipline ----------------------------------------------------------------------------------------------
def test_align_on_a_side_stream_with_one_read_back(monkeypatch):
    """align() on a non-default stream while the default stream is busy: the same attn, one read-back.  The stream is a
    HIP stream of the test's own, destroyed at the end, and the default stream is kept busy with element-wise work:
    the process is left with the streams it had, so the hardware queues later tests' side streams land on do not
    depend on whether this module ran before them."""
    import ctypes as C
    c = ao.load_align_case("align_tiny_b3")
    net, *_ = _case_net(c)
    x, xl, y, yl, sid, eps = (t.to(DEV) for t in ao.case_tensors(c))
    ref = net.align(x, xl, y, yl, sid=sid, eps_q=eps)[0].clone()
    torch.cuda.synchronize()
    calls = {"cpu": 0}
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        calls["cpu"] += 1
        return real_cpu(self, *a, **k)

    hip = _lib.load()  # the HIP runtime is a dependency of the library: its symbols resolve through the same handle
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    raw = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0 and raw.value  # hipStreamNonBlocking
    try:
        side = torch.cuda.ExternalStream(raw.value)
        busy = torch.zeros(16 << 20, device=DEV)
        torch.cuda.synchronize()
        for _ in range(50):  # keep the default stream busy while align() runs beside it
            busy.add_(1.0)
        monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
        with torch.cuda.stream(side):
            attn = net.align(x, xl, y, yl, sid=sid, eps_q=eps)[0]
        monkeypatch.undo()
        side.synchronize()
        assert calls["cpu"] == 1
        torch.cuda.synchronize()
        assert torch.equal(attn, ref)
    finally:
        monkeypatch.undo()
        torch.cuda.synchronize()
        net._last_align = None
        attn = None
        torch.cuda.empty_cache()  # blocks cached for the stream go before the stream does
        assert hip.hipStreamDestroy(raw) == 0
