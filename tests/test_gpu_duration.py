"""GPU tier of SynthesizerTrn.duration_loss (csrc/duration_loss.hip, wetts_duration_sdp_forward): the reference's fixtures
(tests/golden/dur_*.npz), and every stage of the stochastic duration predictor's forward pass against the float64 oracle
of tests/duration_oracle.py under the gates defined there (4 x the float32 oracle's own distance from float64) over
models x variants x kernel forms x shapes.  Every form is compared with the oracle, never with another form.

Forms (WETTS_TUNE is read at create, so a form is a model): default (dds_fused mode 1: small launches), dds_layerwise
(dds_fused=0), dds_fused64 (dds_fused=2: every DDSConv in one launch, 64-column tiles).  Variants: dp.flows.0 as synth
pins it (x10: the main flows run in the spline's linear tails) and unpinned (inside [-5, 5])."""
import os

import numpy as np
import pytest
import torch

from tests import align_oracle as ao, duration_oracle as do, encoder_input as ei, util
from tests.test_cpu_duration import fixture_inputs, fixture_model, FIXTURES
from wetts_amd import SynthesizerTrn, _lib, checkpoint, config, losses, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPEC = ao.SPEC
FORMS = {"default": None, "dds_layerwise": "dds_fused=0", "dds_fused64": "dds_fused=2"}
SWEEP = [(m, v, f) for m in do.SDP for v in do.VARIANTS for f in FORMS]
STAGES = ("z_q", "z", "nll_terms", "logq_terms", "nll", "logq", "per_utt", "rows", "l_length", "logw", "logw_", "total")
_REFS = {}
_MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_and_report():
    yield
    import gc
    _REFS.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = os.environ.get("WETTS_DURATION_MARGINS")  # the GPU run that records profiles/duration_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst multiple of the floor per stage (rel, local | scalar), gate = 4 x floor\n")
            for k in sorted(_MARGINS):
                f.write(f"{k}: {_MARGINS[k]}\n")


def _net(mname, variant="pinned", form="default", sd=None, n_spk=ei.N_SPK, n_vocab=ei.N_VOCAB):
    if sd is None:
        sd = do.weights(mname, variant)[1]
    net = SynthesizerTrn(n_vocab, SPEC, 32, n_speakers=n_spk, **config.MODEL_CONFIGS[mname])
    if FORMS[form] is not None:
        os.environ["WETTS_TUNE"] = FORMS[form]
    try:
        net.load_state_dict(sd).to(DEV)
    finally:
        os.environ.pop("WETTS_TUNE", None)
    return net


def _refs(mname, variant):
    """[(B, Tx, scale, inputs, float64 oracle stages)] over SHAPES[mname]: computed once, shared by every form."""
    if (mname, variant) not in _REFS:
        cfg, sd, cd, W32, W64 = do.weights(mname, variant)
        out = []
        for i, (B, Tx, sc) in enumerate(do.SHAPES[mname]):
            ins = do.inputs(B, Tx, 3000 + i, sc)
            out.append((B, Tx, sc, ins, do.stages(W64, cd, *ins)))
        _REFS[(mname, variant)] = out
    return _REFS[(mname, variant)]


def _gpu(net, x, xl, sid, w, e_q, eps_w):
    l_length, (x_enc, logw, logw_) = net.duration_loss(x.to(DEV), xl.to(DEV), w.to(DEV), sid=sid.to(DEV),
                                                       e_q=None if e_q is None else e_q.to(DEV),
                                                       eps_w=None if eps_w is None else eps_w.to(DEV))
    torch.cuda.synchronize()
    st = net._last_duration
    assert l_length is st["l_length"] and tuple(logw.shape) == tuple(logw_.shape) == (x.shape[0], 1, x.shape[1])
    out = {k: st[k].detach().cpu() for k in STAGES if st.get(k) is not None}
    out.update(x_enc=x_enc.detach().cpu(), x_mask=st["x_mask"].detach().cpu())
    return out


def _check_sdp(tag, mname, variant, got, ref, worst):
    pad = (ref["x_mask"] == 0)[:, 0]
    assert torch.equal(got["x_mask"].double(), ref["x_mask"][:, 0].double()), (tag, "x_mask")
    valid = ~pad
    assert float((ref["w_minus_u"][valid] - 1e-5).abs().min()) > 1e-6, (tag, "a position sits on the clamp")
    for s in do.TENSORS:
        g, r = got[s], ref[s]
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), (tag, s)
        p = pad.unsqueeze(1).expand_as(g) if g.dim() == 3 else pad
        assert bool((g[p] == 0).all()), (tag, s, "not zero behind x_lengths")
        rel, loc = do.gates(g, r)
        fl, (grel, gloc) = do.FLOOR[mname][variant][s], do.gate(mname, variant, s)
        w = worst.setdefault(s, [0.0, 0.0])
        w[0], w[1] = max(w[0], rel / fl[0]), max(w[1], loc / fl[1])
        d = (g.double() - r).abs()
        at = np.unravel_index(int(d.argmax()), d.shape)
        print(tag, s, f"rel {rel:.3g} (gate {grel:.3g}) local {loc:.3g} (gate {gloc:.3g}) max |d| at {at}")
        assert rel <= grel and loc <= gloc, (tag, s, rel, grel, loc, gloc, at)
    m = dict(nll=do.scalar_err(got["nll"], ref["nll"], ref["abs_total"]),
             logq=do.scalar_err(got["logq"], ref["logq"], ref["abs_total"]),
             per_utt=do.scalar_err(got["per_utt"], ref["per_utt"], ref["abs_total"] / ref["lens"].double()))
    for s, v in m.items():
        worst[s] = max(worst.get(s, 0.0), v / do.FLOOR[mname][variant][s])
        print(tag, s, f"|d| / abs_total {v:.3g} (gate {do.gate(mname, variant, s):.3g})")
        assert v <= do.gate(mname, variant, s), (tag, s, v)
    n = float(ref["x_mask"].sum())
    err = do.scalar_err(got["l_length"], ref["l_length"], ref["abs_total"] / n)
    assert err <= do.gate(mname, variant, "nll") + do.gate(mname, variant, "logq"), (tag, "l_length", err)
    assert torch.equal(got["rows"], got["nll"] + got["logq"])


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_duration_loss_matches_reference_fixture(name):
    c = util.load_case(name)
    cfg, sd, cd = fixture_model(c)
    mname, n_spk = str(c["model"]), int(c["n_speakers"])
    net = _net(mname, sd=sd, n_spk=n_spk, n_vocab=int(c["n_vocab"]))
    x, xl, sid, w, e_q, eps_w = fixture_inputs(c)
    l_length, (x_enc, logw, logw_) = net.duration_loss(x.to(DEV), xl.to(DEV), w.to(DEV),
                                                       sid=sid.to(DEV) if n_spk > 0 else None, e_q=e_q.to(DEV),
                                                       eps_w=eps_w.to(DEV))
    n = float((torch.arange(x.shape[1])[None] < xl[:, None]).sum())
    err = do.scalar_err(l_length.cpu(), torch.from_numpy(c["l_length"]), torch.from_numpy(c["abs_total"]) / n)
    rel, loc = do.gates(logw.cpu(), torch.from_numpy(c["logw"]))
    m = do.logw_gate_model(mname)
    # logw_: exact except for the f32 log -- 4 x the float32 oracle's own distance from float64
    r64 = torch.log(torch.from_numpy(c["w"]).double().unsqueeze(1) + 1e-6) * torch.from_numpy(c["logw_"] != 0)
    own = float((torch.log(torch.from_numpy(c["w"]).unsqueeze(1) + 1e-6).double() - r64).abs().max())
    dl = float((logw_.cpu().double() - r64).abs().max())
    print(f"{name}: l_length {l_length.cpu().tolist()} reference {c['l_length'].tolist()} |d|/scale {err:.3g} (gate "
          f"{do.FIXTURE_GATE:.3g}); logw rel {rel:.3g} local {loc:.3g}; logw_ max|d| {dl:.3g} (float32 log {own:.3g})")
    assert err <= do.FIXTURE_GATE
    assert rel <= ei.REL_GATE[m]["logw"] and loc <= ei.LOCAL_GATE[m]["logw"]
    assert dl <= 4 * max(own, 2.0 ** -24)
    assert tuple(x_enc.shape) == (x.shape[0], net.hidden_channels, x.shape[1])


# ---- 2. the oracle sweep -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,variant,form", SWEEP)
def test_sdp_forward_sweep_matches_float64_oracle(mname, variant, form):
    net = _net(mname, variant, form)
    worst = {}
    for B, Tx, sc, ins, ref in _refs(mname, variant):
        got = _gpu(net, *ins)
        _check_sdp((mname, variant, form, B, Tx, sc), mname, variant, got, ref, worst)
        # logw_: exact except for the float32 log -- 4 x the float32 oracle's own distance from float64
        own = do.gates(torch.log(ins[3] + 1e-6) * ref["x_mask"].float(), ref["logw_"])[1]
        loc = do.gates(got["logw_"].unsqueeze(1), ref["logw_"])[1]
        assert loc <= 4 * own, (B, Tx, "logw_", loc, own)
    fig = {s: ([round(v, 2) for v in w] if isinstance(w, list) else round(w, 2)) for s, w in worst.items()}
    _MARGINS[f"{mname} {variant} {form}"] = fig
    print(f"{mname} {variant} {form}: worst multiple of the floor per stage {fig}")


# ---- 3. repeatability ----------------------------------------------------------------------------------------------------
def test_calls_repeat_bit_for_bit_and_kernels_on_a_row_alone_give_the_rows_bits():
    net = _net("tiny", "unpinned")
    ins = do.inputs(5, 300, 77)
    a, b = _gpu(net, *ins), _gpu(net, *ins)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in net._last_duration.items()}
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=DEV)
    for r in range(5):
        row = {k: st[k][r:r + 1].contiguous() for k in ("nll_terms", "logq_terms", "z", "e_q", "x_mask", "logw", "w")}
        nll, logq, both, per = (torch.empty(1, **f32) for _ in range(4))
        _lib.check(lib.wetts_duration_reduce(net._handle, *(_lib.ptr(row[k]) for k in
                                                              ("nll_terms", "logq_terms", "z", "e_q", "x_mask")), 1, 300,
                                             _lib.ptr(nll), _lib.ptr(logq), _lib.ptr(both), _lib.ptr(per),
                                             _lib.current_stream_ptr()), "duration_reduce")
        tgt, rows, pu = torch.empty(1, 300, **f32), torch.empty(1, **f32), torch.empty(1, **f32)
        _lib.check(lib.wetts_duration_dp_loss(net._handle, _lib.ptr(row["logw"]), _lib.ptr(row["w"]),
                                              _lib.ptr(row["x_mask"]), 1, 300, _lib.ptr(tgt), _lib.ptr(rows), _lib.ptr(pu),
                                              _lib.current_stream_ptr()), "duration_dp_loss")
        torch.cuda.synchronize()
        for name, alone, inside in (("nll", nll, st["nll"]), ("logq", logq, st["logq"]), ("both", both, st["rows"]),
                                    ("per_utt", per, st["per_utt"])):
            assert torch.equal(alone[0], inside[r]), (r, name, float(alone[0]), float(inside[r]))
        assert torch.equal(tgt[0], st["logw_"][r]), r
    # the elementwise kernels on the batch's own stage tensors, whole and cut to one row: the same bits
    sd = {k: v.to(DEV).contiguous() for k, v in net.state_dict().items() if k.startswith("dp.")}
    B, T, H, s_ = 5, 300, net.hidden_channels, _lib.current_stream_ptr
    h = (3.0 * torch.randn(B, 29, T, generator=torch.Generator().manual_seed(83))).to(DEV)  # a ConvFlow's projection
    status = torch.zeros(1, dtype=torch.int64, device=DEV)

    def affine(x, mask, n):
        out = torch.empty(n, 2, T, **f32)
        _lib.check(lib.wetts_duration_affine_forward(_lib.ptr(x), _lib.ptr(sd["dp.post_flows.0.m"]),
                                                     _lib.ptr(sd["dp.post_flows.0.logs"]), _lib.ptr(mask), n, T,
                                                     _lib.ptr(out), s_()), "affine_forward")
        return (out,)

    def spline(z, hh, mask, n, ch0):
        z, acc = z.clone(), torch.zeros(n, T, **f32)
        _lib.check(lib.wetts_duration_spline_forward(_lib.ptr(z), ch0, _lib.ptr(hh), _lib.ptr(mask), float(H) ** 0.5, n, T,
                                                     -1.0, _lib.ptr(acc), s_()), "spline_forward")
        return z, acc

    def dequant(zq, w, mask, n, chu):
        z, nt, qt = torch.empty(n, 2, T, **f32), torch.zeros(n, T, **f32), torch.zeros(n, T, **f32)
        _lib.check(lib.wetts_duration_dequant_log(_lib.ptr(zq), chu, _lib.ptr(w), _lib.ptr(mask), n, T, _lib.ptr(z),
                                                  _lib.ptr(nt), _lib.ptr(qt), _lib.ptr(status), s_()), "dequant_log")
        return z, nt, qt

    def pre(w, mask, n):
        out = torch.empty(n, H, T, **f32)
        _lib.check(lib.wetts_duration_pre(_lib.ptr(w), _lib.ptr(mask), _lib.ptr(sd["dp.post_pre.weight"]),
                                          _lib.ptr(sd["dp.post_pre.bias"]), n, H, T, _lib.ptr(out), s_()), "duration_pre")
        return (out,)

    cut = lambda t, r: t[r:r + 1].contiguous()
    mask = st["x_mask"]
    steps = {
        "affine_forward": (affine, (st["e_q"], mask), ()),
        "spline_forward ch0=0": (spline, (st["z_q"], h, mask), (0,)),
        "spline_forward ch0=1": (spline, (st["z"], h, mask), (1,)),
        "dequant_log chu=0": (dequant, (st["z_q"], st["w"], mask), (0,)),
        "dequant_log chu=1": (dequant, (st["z_q"], st["w"], mask), (1,)),
        "duration_pre": (pre, (st["w"], mask), ()),
    }
    for name, (fn, tensors, extra) in steps.items():
        whole = fn(*tensors, B, *extra)
        for r in range(B):
            alone = fn(*(cut(t, r) for t in tensors), 1, *extra)
            torch.cuda.synchronize()
            for i, (a_, w_) in enumerate(zip(alone, whole)):
                assert bool(torch.isfinite(w_).all()) and torch.equal(a_[0], w_[r]), (name, r, i)
    assert bool((dequant(st["z_q"], st["w"], mask, B, 0)[0][:, 1] == st["z_q"][:, 1]).all())  # z1 passes through
    assert int(status.item()) == 0
    # a row alone through the whole call: another dispatch (dds_fused_supported depends on B and T), so the gates
    cfg, sd, cd, W32, W64 = do.weights("tiny", "unpinned")
    one = tuple(t[1:2] for t in ins)
    _check_sdp(("row alone",), "tiny", "unpinned", _gpu(net, *one), do.stages(W64, cd, *one), {})


# ---- 4. padding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", ["tiny", "tiny_dp"])
def test_garbage_behind_x_lengths_changes_no_output_bit(mname):
    net = _net(mname)
    x, xl, sid, w, e_q, eps_w = do.inputs(3, 65, 78)
    valid = torch.arange(65)[None] < xl[:, None]
    gen = torch.Generator().manual_seed(79)
    x2 = torch.where(valid, x, torch.randint(0, ei.N_VOCAB, x.shape, generator=gen))
    w2 = torch.where(valid[:, None], w, -1e30 * torch.rand(w.shape, generator=gen) + 5)
    w2[0, 0, -1] = float("nan") if not valid[0, -1] else w2[0, 0, -1]
    e2 = torch.where(valid[:, None], e_q, 1e30 * torch.randn(e_q.shape, generator=gen))
    assert int((~valid).sum()) > 0 and not torch.equal(w2, w) and not torch.equal(x2, x)
    a, b = _gpu(net, x, xl, sid, w, e_q, eps_w), _gpu(net, x2, xl, sid, w2, e2, eps_w)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k  # x_enc, the returned encoder output, included
    pad = (~valid)[:, None].expand_as(a["x_enc"])
    assert bool((a["x_enc"][pad] == 0).all()) and bool((b["x_enc"][pad] == 0).all())


# ---- 5. the DurationPredictor model ---------------------------------------------------------------------------------------
def test_dp_model_matches_the_oracle_and_logw_is_encodes():
    mname = "tiny_dp"
    net = _net(mname)
    cfg, sd, cd, W32, W64 = do.weights(mname)
    assert net._dur_blob is None
    worst = 0.0
    for i, (B, Tx, sc) in enumerate(do.SHAPES[mname]):
        ins = do.inputs(B, Tx, 3000 + i, sc)
        got, ref = _gpu(net, *ins), do.stages(W64, cd, *ins)
        err = do.scalar_err(got["rows"], ref["rows"], ref["abs_total"])
        worst = max(worst, err)
        assert err <= do.GATE_FACTOR * do.DP_FLOOR[0], (B, Tx, err)
        n = float(ref["x_mask"].sum())
        assert do.scalar_err(got["l_length"], ref["l_length"], ref["abs_total"] / n) <= do.GATE_FACTOR * do.DP_FLOOR[0]
        assert do.gates(got["logw_"].unsqueeze(1), ref["logw_"])[1] <= do.GATE_FACTOR * do.DP_FLOOR[1][1]
        x, xl, sid = (t.to(DEV) for t in ins[:3])
        enc = net._encode(x, xl, sid, 0.667, 1.0, 0.8, None, None)
        assert torch.equal(enc["logw"].cpu(), got["logw"]), (B, Tx)
        assert "nll" not in got and float(got["total"][0]) == float(got["total"][1])
    print(f"tiny_dp: worst |d| / abs_total of the row sums {worst:.3g} (gate {do.GATE_FACTOR * do.DP_FLOOR[0]:.3g})")


# ---- 6. seeding -------------------------------------------------------------------------------------------------------------
def test_draws_follow_torch_manual_seed_and_injected_noise_overrides_it():
    net = _net("tiny")
    x, xl, sid, w, e_q, eps_w = do.inputs(2, 33, 80)
    torch.manual_seed(5)
    a = _gpu(net, x, xl, sid, w, None, None)
    b = _gpu(net, x, xl, sid, w, None, None)
    torch.manual_seed(5)
    c = _gpu(net, x, xl, sid, w, None, None)
    assert all(torch.equal(a[k], c[k]) for k in a)
    assert not torch.equal(a["nll"], b["nll"]) and not torch.equal(a["logw"], b["logw"])
    torch.manual_seed(5)
    d = _gpu(net, x, xl, sid, w, e_q, eps_w)
    torch.manual_seed(6)
    e = _gpu(net, x, xl, sid, w, e_q, eps_w)
    assert all(torch.equal(d[k], e[k]) for k in d) and not torch.equal(d["nll"], a["nll"])


# ---- 7. read-back and isolation -------------------------------------------------------------------------------------------
def test_one_read_back_and_other_entry_points_unchanged(monkeypatch):
    c = ao.load_align_case("align_tiny_b3")
    cfg, sd, psd = util.vc_case_model(c, SPEC)
    dsd = synth.make_duration_state_dict(cfg, 9)
    net = SynthesizerTrn(int(c["n_vocab"]), SPEC, 32, n_speakers=int(c["n_speakers"]), **config.MODEL_CONFIGS["tiny"])
    net.load_state_dict(dict(sd, **psd, **dsd)).to(DEV)
    x, xl, y, yl, sid, eps = (t.to(DEV) for t in ao.case_tensors(c))

    def others():
        torch.manual_seed(9)
        o, attn, _, (z, *_) = net.infer(x, xl, sid=sid, noise_scale=0.667, noise_scale_w=0.8)
        a_attn, w, _, _, (az, az_p, *_) = net.align(x, xl, y, yl, sid=sid, eps_q=eps)
        torch.cuda.synchronize()
        return [t.clone() for t in (o, attn, z, a_attn, w, az, az_p)]

    before = others()  # before the lazy upload of the duration tensors
    assert not net._dur_on_device
    w = before[4]
    calls = {"cpu": 0}
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        calls["cpu"] += 1
        return real_cpu(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    try:
        net.duration_loss(x, xl, w, sid=sid)
        net.duration_loss(x, xl, w[:, 0], sid=sid, e_q=torch.zeros(3, 2, x.shape[1], device=DEV))
    finally:
        monkeypatch.undo()
    assert calls["cpu"] == 2 and net._dur_on_device
    for a, b in zip(before, others()):
        assert torch.equal(a, b)
    plain = SynthesizerTrn(int(c["n_vocab"]), SPEC, 32, n_speakers=int(c["n_speakers"]), **config.MODEL_CONFIGS["tiny"])
    plain.load_state_dict(dict(sd, **psd)).to(DEV)
    o2 = plain.infer(x, xl, sid=sid, noise_scale=0.0, noise_scale_w=0.0)[0]
    assert torch.equal(o2, net.infer(x, xl, sid=sid, noise_scale=0.0, noise_scale_w=0.0)[0])
    out = {k: v.to(DEV) for k, v in net.state_dict().items() if k in dsd}
    assert set(out) == set(dsd) and all(torch.equal(out[k].cpu(), dsd[k]) for k in dsd)


# ---- 8. teacher_forced_losses(with_duration=True) -------------------------------------------------------------------------
def test_teacher_forced_losses_with_duration_is_duration_loss_on_the_alignment():
    from tests import recon_oracle as ro
    c = ro.load_recon_case("recon_vits2_v1_b2")  # a hop-256 model: the recipes' mel settings apply
    cfg, sd, psd = util.vc_case_model(c, SPEC)
    net = SynthesizerTrn(int(c["n_vocab"]), SPEC, 32, n_speakers=int(c["n_speakers"]),
                         **config.MODEL_CONFIGS[str(c["model"])])
    net.load_state_dict(dict(sd, **psd, **synth.make_duration_state_dict(cfg, 9))).to(DEV)
    x, xl, y, yl, sid, eps = (t.to(DEV) for t in ao.case_tensors(c))
    B, Tx = x.shape
    gen = torch.Generator().manual_seed(81)
    e_q, eps_w = torch.randn(B, 2, Tx, generator=gen).to(DEV), torch.randn(B, 2, Tx, generator=gen).to(DEV)
    ids = torch.from_numpy(c["ids_slice"]).to(DEV)
    kw = dict(sid=sid, segment_size=int(c["segment"]), ids_slice=ids, eps_q=eps)
    spec_hps = lambda **train: config.HParams(data=dict(ro.MEL, sampling_rate=int(c["sampling_rate_mel"])), model={},
                                              train=dict(c_mel=45, c_kl=1.0, **train))
    plain = losses.teacher_forced_losses(net, spec_hps(), x, xl, y, yl, **kw)
    assert set(plain) == {"loss_mel", "loss_kl", "mel", "kl", "mel_per_utt", "kl_per_utt", "y_hat", "ids_slice", "y_mel",
                          "y_hat_mel"}
    full = losses.teacher_forced_losses(net, spec_hps(c_dur=2.0), x, xl, y, yl, with_duration=True, e_q=e_q, eps_w=eps_w,
                                        **kw)
    assert set(full) == set(plain) | {"loss_dur", "dur", "dur_per_utt"}
    for k in plain:
        assert torch.equal(plain[k], full[k]), k
    w = net.align(x, xl, y, yl, sid=sid, eps_q=eps)[1]
    l_length, _ = net.duration_loss(x, xl, w, sid=sid, e_q=e_q, eps_w=eps_w)
    st = net._last_duration
    assert torch.equal(full["dur_per_utt"], st["per_utt"]) and torch.equal(full["dur"], st["total"][0])
    assert float(full["loss_dur"].cpu()) == float(np.float32(full["dur"].cpu()) * np.float32(2.0))
    assert abs(float(l_length.double().sum()) - float(full["dur"])) <= 1e-6 * abs(float(full["dur"]))
    one = losses.teacher_forced_losses(net, spec_hps(), x, xl, y, yl, with_duration=True, e_q=e_q, eps_w=eps_w, **kw)
    assert torch.equal(one["loss_dur"], one["dur"]) and torch.equal(one["dur"], full["dur"])


# ---- 9. errors -------------------------------------------------------------------------------------------------------------
def test_bad_durations_and_missing_tensors_raise_and_leave_the_model_usable():
    net = _net("tiny")
    x, xl, sid, w, e_q, eps_w = do.inputs(2, 33, 82)
    good = _gpu(net, x, xl, sid, w, e_q, eps_w)
    full = int(torch.argmax(xl))  # the row of 33 phonemes: position 3 is under the mask
    for bad_value, what in ((-1.0, "negative"), (float("nan"), "NaN"), (float("inf"), "NaN")):
        wb = w.clone()
        wb[full, 0, 3] = bad_value
        with pytest.raises(ValueError, match=what):
            _gpu(net, x, xl, sid, wb, e_q, eps_w)
        again = _gpu(net, x, xl, sid, w, e_q, eps_w)
        assert all(torch.equal(good[k], again[k]) for k in good)
    xb = x.clone()
    xb[0, 0] = ei.N_VOCAB
    with pytest.raises(IndexError):
        _gpu(net, xb, xl, sid, w, e_q, eps_w)
    with pytest.raises(IndexError):
        _gpu(net, x, xl, torch.full_like(sid, ei.N_SPK), w, e_q, eps_w)
    with pytest.raises(ValueError, match="w must be"):
        net.duration_loss(x.to(DEV), xl.to(DEV), w[:, :, :5].to(DEV), sid=sid.to(DEV))
    bare = _net("tiny", sd=ei.weights("tiny")[1])
    with pytest.raises(RuntimeError, match=r"dp\.flows\.1"):
        bare.duration_loss(x.to(DEV), xl.to(DEV), w.to(DEV), sid=sid.to(DEV))
    o = bare.infer(x.to(DEV), xl.to(DEV), sid=sid.to(DEV), noise_scale=0.0, noise_scale_w=0.0)[0]
    assert bool(torch.isfinite(o).all())
    again = _gpu(net, x, xl, sid, w, e_q, eps_w)
    assert all(torch.equal(good[k], again[k]) for k in good)
    dp = _net("tiny_dp")
    wb = w.clone()
    wb[full, 0, 0] = -2.0
    with pytest.raises(ValueError, match="negative"):
        _gpu(dp, x, xl, sid, wb, None, None)
    assert bool(torch.isfinite(_gpu(dp, x, xl, sid, w, None, None)["l_length"]).all())
