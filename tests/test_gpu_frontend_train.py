"""GPU tier of frontend training (csrc/frontend_train.hip, wetts_amd.frontend_train): grad() on the 16 fixture cases
against float64 autograd at the same weights (fo.gate, 4 x the stored float32 floor) and against the reference's stored
samples (fo.fixture_gate), losses and counts equal to score(); every stage entry alone against float64 within 4 x torch's
float32 floor of the same stage, computed here on the CPU; the bit conditions; the conventions; AdamW alone; three step()s
on the trajectory case, link by link; the round trip through state_dict() and set_dtype(); the command line.
Shapes: N = 3, 15, 99, 195 tokens; d = 312 / 768, ff = 1200 / 2048, classes 34 / 470 / 5, dk = 26 / 96."""
import ctypes as C
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import frontend_oracle as fo
from tests import frontend_score_oracle as so
from tests import frontend_train_oracle as to
from wetts_amd import FrontendModel, _lib, checkpoint
from wetts_amd import frontend_train
from wetts_amd.frontend_train import FrontendTrainer

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = fo.NUM_PROSODY
_RUN, _MARGINS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_and_report():
    yield
    import gc
    _RUN.clear()
    _KEEP.clear()
    to._REF.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = os.environ.get("WETTS_FRONTEND_TRAIN_MARGINS")  # the GPU run that records profiles/frontend_train_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst multiple of a gate per case (1 = at the gate; gate = 4 x floor against float64, 5 x floor against "
                    "the reference's float32), then the tensor that gave it\n")
            for k in sorted(_MARGINS):
                f.write(f"{k}: {_MARGINS[k]}\n")


def _model(cname, P, sd=None):
    return FrontendModel(P, R, fo.BERT_CONFIGS[cname]).load_state_dict(sd or so.weights(cname, P)[0]).to(DEV)


def _run(cname, P, lens):
    """(model, trainer, ids, mask, labels, FrontendScores, {name: gradient}, flat gradient) of a case, computed once."""
    k = (cname, P, tuple(lens))
    if k not in _RUN:
        ids, mask, pl, rl, _, _ = to.reference(cname, P, lens)
        net = _model(cname, P)
        tr = FrontendTrainer(net, num_training_steps=4)
        s, g = tr.grad({"input_ids": ids, "attention_mask": mask}, pl, rl)
        _RUN[k] = (net, tr, ids, mask, pl, rl, s, {n: t.cpu() for n, t in g.items()}, tr.last_grad.cpu())
    return _RUN[k]


def _hold(tag, figs, floors, gate):
    """figs {name: (rel, local)} against gate(floors[name]); records the worst multiple."""
    top, who = 0.0, None
    for n, v in figs.items():
        g = gate(floors[n])
        mult = max(v[0] / g[0], v[1] / g[1])
        if mult > top:
            top, who = mult, n
    print(tag, "worst multiple of a gate", round(top, 3), who)
    _MARGINS[tag] = (round(top, 3), who)
    for n, v in figs.items():
        g = gate(floors[n])
        assert fo.within(v, g), f"{tag} {n}: rel {v[0]:.3e} (gate {g[0]:.3e}) local {v[1]:.3e} (gate {g[1]:.3e})"


# ---- 1. grad() on the fixture cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,P,lens", to.CASES)
def test_grad_against_float64_autograd_and_the_reference(cname, P, lens):
    net, tr, ids, mask, pl, rl, s, grads, flat = _run(cname, P, lens)
    c = to.load_fixture(cname, P, lens)
    want = to.reference(cname, P, lens)[5]
    floors = {n: c["floor_grad_" + n] for n in to.TRAINABLE}
    live = [n for n in to.TRAINABLE if float(want[n].norm()) > 0]
    assert len(live) >= 14 and all(grads[n].dtype == torch.float32 and grads[n].shape == want[n].shape for n in to.TRAINABLE)
    for n in set(to.TRAINABLE) - set(live):
        assert not bool(grads[n].view(torch.int32).any()), n  # an empty head: exact zeros
    name = to.case_name(cname, P, lens)
    _hold("oracle " + name, {n: fo.gates(grads[n].double(), want[n]) for n in live}, floors, fo.gate)
    _hold("fixture " + name, {n: to.sample_figure(to.sample(grads[n])[0], torch.from_numpy(c["grad_" + n]), c["norm_" + n],
                                                  grads[n].numel()) for n in live}, floors, fo.fixture_gate)
    # losses and counts: score()'s own, to the bit
    ref = net.score({"input_ids": ids, "attention_mask": mask}, pl, rl)
    assert torch.equal(s.packed().cpu(), ref.packed().cpu())
    assert torch.equal(s.nll_phone.cpu().view(torch.int32), ref.nll_phone.cpu().view(torch.int32))
    assert torch.equal(s.pred_prosody.cpu(), ref.pred_prosody.cpu())
    # exact zeros in the padding of the blob's layout
    pad = torch.ones(flat.numel(), dtype=torch.bool)
    for _, o, k, _ in tr.layout:
        pad[o:o + k] = False
    assert not bool(flat[pad].view(torch.int32).any())


# ---- 2. the stages alone ---------------------------------------------------------------------------------------------------------
_KEEP = []


def _dev(t):
    """A device copy that lives until the test module is released (its address goes into a launch)."""
    _KEEP.append(t.to(DEV).contiguous())
    return _KEEP[-1]


def _stage_hold(tag, got, f64, f32):
    floor = fo.gates(f32.double(), f64)
    fig = fo.gates(got.cpu().double(), f64)
    g = fo.gate(floor)
    print(tag, "figure", fig, "floor", floor)
    _MARGINS["stage " + tag] = (round(max(fig[0] / g[0], fig[1] / g[1]), 3), None)
    assert fo.within(fig, g), f"{tag}: rel {fig[0]:.3e} (gate {g[0]:.3e}) local {fig[1]:.3e} (gate {g[1]:.3e})"


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


GEMM_SHAPES = ((3, 34, 312), (15, 470, 312), (99, 5, 768), (99, 312, 1200), (195, 1200, 312), (195, 768, 96), (99, 936, 312))


@pytest.mark.parametrize("N,M,K", GEMM_SHAPES)
@pytest.mark.parametrize("epi", (0, 1, 2))
def test_linear_dgrad_alone(N, M, K, epi):
    lib = _lib.load()
    ldy = M + 5  # a slice of a wider buffer, as the classifier's dlogits are
    dy = _rand((N, ldy), 1 + N + M).float()
    w = _rand((M, K), 2 + M + K, 1 / math.sqrt(M)).float()
    aux = _rand((N, K), 3 + N).float()
    out = torch.full((N, K), float("nan"), device=DEV)
    _lib.check(lib.wetts_frontend_linear_dgrad(_lib.ptr(_dev(dy)), ldy, _lib.ptr(_dev(w)), N, M, K, epi, _lib.ptr(_dev(aux)),
                                               _lib.ptr(out), _lib.current_stream_ptr()), "dgrad")

    def ref(t):
        v = dy[:, :M].to(t) @ w.to(t)
        return v * (aux > 0).to(t) if epi == 1 else (v + aux.to(t) if epi == 2 else v)
    _stage_hold(f"dgrad {N}x{M}x{K} epi {epi}", out, ref(torch.float64), ref(torch.float32))


@pytest.mark.parametrize("N,M,K", GEMM_SHAPES)
def test_linear_wgrad_and_bias_sums_alone(N, M, K):
    lib = _lib.load()
    ldy = M + 5
    dy = _rand((N, ldy), 11 + N + M).float()
    x = _rand((N, K), 12 + N + K).float()
    nbytes = int(lib.wetts_frontend_linear_wgrad_workspace_bytes(N, M, K))
    ws = torch.full((nbytes // 4 + 1,), float("nan"), device=DEV)
    dw, db = torch.full((M, K), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)
    _lib.check(lib.wetts_frontend_linear_wgrad(_lib.ptr(_dev(dy)), ldy, _lib.ptr(_dev(x)), N, M, K, _lib.ptr(dw), _lib.ptr(db),
                                               _lib.ptr(ws), nbytes, _lib.current_stream_ptr()), "wgrad")
    _stage_hold(f"wgrad {N}x{M}x{K}", dw, dy[:, :M].double().t() @ x.double(), dy[:, :M].t() @ x)
    _stage_hold(f"bias sums {N}x{M}", db, dy[:, :M].double().sum(0), dy[:, :M].sum(0))


@pytest.mark.parametrize("N,Cn", ((3, 312), (15, 768), (99, 312), (195, 768), (99, 1024)))
def test_layer_norm_backward_alone(N, Cn):
    lib = _lib.load()
    x = (_rand((N, Cn), 21 + N) * 1.5 + 0.3).float()
    dy = _rand((N, Cn), 22 + N).float()
    gamma = (1 + 0.2 * _rand((Cn,), 23)).float()
    nfl = (2 * N + 63) // 64 * 64 + (N + 63) // 64 * Cn
    ws = torch.full((nfl,), float("nan"), device=DEV)
    dx = torch.full((N, Cn), float("nan"), device=DEV)
    dg, dbt = torch.full((Cn,), float("nan"), device=DEV), torch.full((Cn,), float("nan"), device=DEV)
    _lib.check(lib.wetts_frontend_layer_norm_backward(_lib.ptr(_dev(dy)), _lib.ptr(_dev(x)), _lib.ptr(_dev(gamma)), 1e-5, N, Cn,
                                                      _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(dbt), _lib.ptr(ws), nfl * 4,
                                                      _lib.current_stream_ptr()), "layer_norm_backward")

    def ref(t):
        xx, gg = x.to(t).requires_grad_(True), gamma.to(t).requires_grad_(True)
        bb = torch.zeros(Cn, dtype=t, requires_grad=True)
        return torch.autograd.grad(F.layer_norm(xx, (Cn,), gg, bb, 1e-5), (xx, gg, bb), dy.to(t))
    for tag, got, a, b in zip(("dx", "dgamma", "dbeta"), (dx, dg, dbt), ref(torch.float64), ref(torch.float32)):
        _stage_hold(f"layer norm backward {N}x{Cn} {tag}", got, a, b)


@pytest.mark.parametrize("cname,lens", (("tiny", (3,)), ("tiny", (9, 6)), ("tiny", (33, 32, 31)), ("base", (65, 64, 63)),
                                        ("base", (9, 6)), ("tiny", (20, 2))))
def test_attention_backward_alone(cname, lens):
    """dk = 26 (tiny, 12 heads) and 96 (base, 8 heads); (20, 2): a row that is padding right after [CLS] [SEP]."""
    lib = _lib.load()
    c = fo.config(cname)
    H, d = c["transform_heads"], c["hidden_size"]
    ids, mask = fo.inputs(lens, 4242 + sum(lens))
    B, T = mask.shape
    qkv = _rand((B, T, 3 * d), 31 + T, 0.7).float()
    dctx = (_rand((B, T, d), 32 + T) * (mask != 0).unsqueeze(-1)).float()  # a padded query carries no gradient

    def ref(t):
        q = qkv.to(t).requires_grad_(True)
        o = fo.attention(q, mask, H)
        return o.detach(), torch.autograd.grad(o, q, dctx.to(t))[0]
    o64, g64 = ref(torch.float64)
    _, g32 = ref(torch.float32)
    maskf = _dev((mask != 0).float())
    ctx = torch.empty(B, T, d, device=DEV)
    _lib.check(lib.wetts_frontend_attention(_lib.ptr(_dev(qkv)), _lib.ptr(maskf), B, T, H, d // H, _lib.ptr(ctx),
                                            _lib.current_stream_ptr()), "attention")
    nfl = 2 * ((B * H * T * T + 63) // 64 * 64)
    ws = torch.full((nfl,), float("nan"), device=DEV)
    out = torch.full((B, T, 3 * d), float("nan"), device=DEV)
    _lib.check(lib.wetts_frontend_attention_backward(_lib.ptr(_dev(qkv)), _lib.ptr(maskf), _lib.ptr(ctx), _lib.ptr(_dev(dctx)), B, T,
                                                     H, d // H, _lib.ptr(out), _lib.ptr(ws), nfl * 4, _lib.current_stream_ptr()),
               "attention_backward")
    _stage_hold(f"attention backward {cname} {lens}", out, g64, g32)
    if bool((mask == 0).any()):  # a masked key receives exactly zero (dK and dV), a padded query's dQ is zero too
        assert float(out.cpu()[mask == 0].abs().max()) == 0.0


@pytest.mark.parametrize("N,P", ((3, 34), (15, 470), (99, 34), (195, 470)))
def test_ce_backward_alone(N, P):
    lib = _lib.load()
    g = torch.Generator().manual_seed(41 + N)
    zp, zr = (_rand((N, P), 42 + N) * 3).float(), (_rand((N, R), 43 + N) * 3).float()
    mask = (torch.rand(N, generator=g) < 0.8).long()
    mask[0] = 1
    pl = torch.where(torch.rand(N, generator=g) < 0.4, torch.randint(0, P, (N,), generator=g), torch.full((N,), -100))
    rl = torch.where(torch.rand(N, generator=g) < 0.8, torch.randint(0, R, (N,), generator=g), torch.full((N,), -100))
    pl[0], rl[0] = 1, 2
    pl, rl = torch.where(mask != 0, pl, torch.full_like(pl, -100)), torch.where(mask != 0, rl, torch.full_like(rl, -100))
    counts = torch.zeros(22, dtype=torch.int64)
    counts[0], counts[2] = int((pl >= 0).sum()), int((rl >= 0).sum())
    w = 0.3
    out = torch.full((N, P + R), float("nan"), device=DEV)
    _lib.check(lib.wetts_frontend_ce_backward(_lib.ptr(_dev(zp)), _lib.ptr(_dev(zr)), _lib.ptr(_dev(mask.float())), _lib.ptr(_dev(pl)),
                                              _lib.ptr(_dev(rl)), _lib.ptr(_dev(counts)), N, P, R, w, _lib.ptr(out),
                                              _lib.current_stream_ptr()), "ce_backward")

    def ref(t):
        a, b = zp.to(t).requires_grad_(True), zr.to(t).requires_grad_(True)
        loss = w * F.cross_entropy(a, pl, ignore_index=-100) + (1 - w) * F.cross_entropy(b, rl, ignore_index=-100)
        return torch.cat(torch.autograd.grad(loss, (a, b)), 1)
    _stage_hold(f"ce backward {N}x{P}", out, ref(torch.float64), ref(torch.float32))
    dead = ((pl < 0).unsqueeze(1).expand(N, P), (rl < 0).unsqueeze(1).expand(N, R))
    assert not bool(out.cpu()[torch.cat(dead, 1)].view(torch.int32).any())  # exact zeros where nothing is scored


# ---- 3. bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,P,lens", (("tiny", 34, (9, 6)), ("base", 470, (33, 32, 31)), ("tiny", 470, (65, 64, 63))))
def test_same_bits_again_with_other_pad_ids_and_a_nan_workspace(cname, P, lens):
    net, tr, ids, mask, pl, rl, s, grads, flat = _run(cname, P, lens)
    x = {"input_ids": ids, "attention_mask": mask}
    tr.grad(x, pl, rl)
    assert torch.equal(tr.last_grad.cpu().view(torch.int32), flat.view(torch.int32))
    ids2 = torch.where(mask != 0, ids, torch.full_like(ids, 9))
    assert not torch.equal(ids2, ids)
    tr.grad({"input_ids": ids2, "attention_mask": mask}, pl, rl)
    assert torch.equal(tr.last_grad.cpu().view(torch.int32), flat.view(torch.int32))
    tr._ws.fill_(float("nan"))
    s3, _ = tr.grad(x, pl, rl)
    assert torch.equal(tr.last_grad.cpu().view(torch.int32), flat.view(torch.int32))
    assert torch.equal(s3.packed().cpu(), s.packed().cpu())


# ---- 4. conventions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", fo.CONFIGS)
def test_empty_head_reports_nan_and_contributes_no_gradient(cname):
    P, lens = 34, (9, 6)
    ids, mask, pl, rl, _, _ = to.reference(cname, P, lens)
    c = to.load_fixture(cname, P, lens)
    tr = FrontendTrainer(_model(cname, P), num_training_steps=4, polyphone_weight=0.3)
    s, g = tr.grad({"input_ids": ids, "attention_mask": mask}, None, rl)
    h = s.host()
    assert math.isnan(h.phone_loss) and math.isnan(h.loss) and math.isfinite(h.prosody_loss)
    _, want = to.autograd(so.weights(cname, P)[1], cname, ids, mask, None, rl, 0.3)
    assert all(bool(torch.isfinite(t).all()) for t in g.values())
    assert not bool(g["phone_classifier.weight"].cpu().view(torch.int32).any())
    live = [n for n in to.TRAINABLE if not n.startswith("phone")]
    _hold(f"empty head {cname}", {n: fo.gates(g[n].cpu().double(), want[n]) for n in live},
          {n: c["floor_grad_" + n] for n in live}, fo.gate)


def test_flagged_labels_are_raised_by_host_and_absent_from_the_gradient():
    cname, P, lens = "tiny", 34, (9, 6)
    net, tr, ids, mask, pl, rl, s, grads, flat = _run(cname, P, lens)
    x = {"input_ids": ids, "attention_mask": mask}
    bad = pl.clone()
    assert mask[1, 8] == 0 and pl[0, 0] == so.IGNORE_ID
    bad[0, 0] = P + 3  # outside the classes
    s2, _ = tr.grad(x, bad, rl)
    with pytest.raises(IndexError):
        s2.host()
    assert torch.equal(tr.last_grad.cpu().view(torch.int32), flat.view(torch.int32))
    bad = pl.clone()
    bad[1, 8] = 1  # at a padded token
    s3, _ = tr.grad(x, bad, rl)
    with pytest.raises(ValueError):
        s3.host()
    assert torch.equal(tr.last_grad.cpu().view(torch.int32), flat.view(torch.int32))


# ---- 5. AdamW alone ----------------------------------------------------------------------------------------------------------------------
def _adamw_case(n=8192, seed=7):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.05
    grad = torch.randn(n, generator=g) * 10 ** torch.randint(-6, 1, (n,), generator=g).float()
    grad[:128] = 0.0
    grad[128:256] = 1e-12 * torch.sign(torch.randn(128, generator=g))
    p[:16] = 0.0
    m = torch.randn(n, generator=g) * 0.1 * grad.abs()
    v = (torch.rand(n, generator=g) + 0.5) * grad * grad
    return p, grad, m, v


@pytest.mark.parametrize("t", (1, 2, 1000))
@pytest.mark.parametrize("lr", (1e-3, 0.0))
def test_adamw_alone(t, lr):
    lib = _lib.load()
    p0, g, m0, v0 = _adamw_case()
    if t == 1:
        m0, v0 = torch.zeros_like(m0), torch.zeros_like(v0)
    b1, b2 = 0.9, 0.999
    p, m, v = _dev(p0).clone(), _dev(m0).clone(), _dev(v0).clone()
    _lib.check(lib.wetts_frontend_adamw(_lib.ptr(p), _lib.ptr(_dev(g)), _lib.ptr(m), _lib.ptr(v), p.numel(), lr, b1, b2, 1e-8, 0.01,
                                        1 - b1 ** t, 1 - b2 ** t, _lib.current_stream_ptr()), "adamw")
    p64, m64, v64 = to.adamw_step(p0.double(), g.double(), m0.double(), v0.double(), t, lr)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=lr, foreach=False)
    opt.state[ref] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    ref.grad = g.clone()
    opt.step()
    st = opt.state[ref]
    if lr == 0.0:
        assert torch.equal(p.cpu().view(torch.int32), p0.view(torch.int32))
    for tag, got, fig, floor in (("p", p, to.adamw_figure(p, p64, p0), to.adamw_figure(ref.detach(), p64, p0)),
                                 ("m", m, to.state_figure(m, m64), to.state_figure(st["exp_avg"], m64)),
                                 ("v", v, to.state_figure(v, v64), to.state_figure(st["exp_avg_sq"], v64))):
        floor = max(floor, 1.0)  # never below half an ulp
        print(f"adamw t={t} lr={lr} {tag}: figure {fig:.3f} floor {floor:.3f}")
        _MARGINS[f"adamw t={t} lr={lr} {tag}"] = (round(fig / (4 * floor), 3), None)
        assert fig <= 4 * floor, (tag, fig, floor)


# ---- 6. three steps on the trajectory case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", fo.CONFIGS)
def test_three_steps_link_by_link(cname):
    c = to.load_traj(cname)
    P, lens = int(c["num_polyphones"]), tuple(int(v) for v in c["lens"])
    fx = to.load_fixture(cname, P, lens)
    floors = {n: fx["floor_grad_" + n] for n in to.TRAINABLE}
    ids, mask, pl, rl, _, _ = to.reference(cname, P, lens)
    x = {"input_ids": ids, "attention_mask": mask}
    sd = so.weights(cname, P)[0]
    net = _model(cname, P)
    tr = FrontendTrainer(net, lr=float(c["base_lr"]), num_training_steps=int(c["total_steps"]))
    frozen = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    for t in range(1, int(c["steps"]) + 1):
        assert tr.lr == float(c["lr"][t - 1])
        lr = tr.lr
        p_old = tr.weights().cpu()
        st = tr.state_dict()
        s = tr.step(x, pl, rl)
        g, p_new = tr.last_grad.cpu(), tr.weights().cpu()
        # the gradient against float64 autograd AT THE DEVICE'S WEIGHTS
        W = dict(frozen)
        W.update({n: v.double() for n, v in tr.named(p_old).items()})
        losses64, want = to.autograd(W, cname, ids, mask, pl, rl)
        _hold(f"trajectory {cname} step {t}", {n: fo.gates(tr.named(g)[n].double(), want[n]) for n in to.TRAINABLE}, floors, fo.gate)
        # the update against float64 AdamW on the device's own (p, g, m, v)
        for n in to.TRAINABLE:
            po, gg = tr.named(p_old)[n], tr.named(g)[n]
            p64, _, _ = to.adamw_step(po.double(), gg.double(), st["exp_avg"][n].double(), st["exp_avg_sq"][n].double(), t, lr)
            ref = torch.nn.Parameter(po.clone())
            opt = torch.optim.AdamW([ref], lr=lr, foreach=False)
            opt.state[ref] = {"step": torch.tensor(float(t - 1)), "exp_avg": st["exp_avg"][n].clone(),
                              "exp_avg_sq": st["exp_avg_sq"][n].clone()}
            ref.grad = gg.clone()
            opt.step()
            floor = max(to.adamw_figure(ref.detach(), p64, po), 1.0)
            assert to.adamw_figure(tr.named(p_new)[n], p64, po) <= 4 * floor, (t, n)
        h = s.host()
        fig = fo.gates(torch.tensor([h.phone_loss, h.prosody_loss], dtype=torch.float64), torch.from_numpy(c["losses"][t - 1][:2]).double())
        assert fo.within(fig, fo.fixture_gate(c["floor_loss"])), (t, fig, c["floor_loss"])
    assert tr.step_count == 3 and tr.lr == float(c["base_lr"]) * 0.25


# ---- 7. round trip ---------------------------------------------------------------------------------------------------------------------------
def test_trained_weights_round_trip_through_state_dict_and_the_16_bit_packing():
    cname, P, lens = "tiny", 34, (33, 32, 31)
    ids, mask, pl, rl, _, _ = to.reference(cname, P, lens)
    x = {"input_ids": ids, "attention_mask": mask}
    before = so.weights(cname, P)[0]
    net = _model(cname, P)
    tr = FrontendTrainer(net, num_training_steps=4)
    for _ in range(2):
        tr.step(x, pl, rl)
    sd = net.state_dict()
    assert set(sd) == {n for n, _, _, _ in checkpoint.frontend_layout(net.config)}
    assert all(not torch.equal(sd[n], before[n]) for n in to.TRAINABLE)
    assert all(torch.equal(sd[n], before[n]) for n in sd if n.startswith("bert."))  # BERT is never written
    fresh = _model(cname, P, sd)
    a, b = net.forward(x), fresh.forward(x)
    assert all(torch.equal(u.cpu().view(torch.int32), v.cpu().view(torch.int32)) for u, v in zip(a, b))
    net.set_dtype(torch.bfloat16)
    fresh16 = FrontendModel(P, R, fo.BERT_CONFIGS[cname]).set_dtype(torch.bfloat16).load_state_dict(sd).to(DEV)
    a, b = net.forward(x), fresh16.forward(x)
    assert all(torch.equal(u.cpu().view(torch.int32), v.cpu().view(torch.int32)) for u, v in zip(a, b))
    with pytest.raises(ValueError):
        tr.step(x, pl, rl)  # a 16-bit model is refused


# ---- 8. the command line -----------------------------------------------------------------------------------------------------------------------
def test_command_line_trains_two_epochs_on_the_toy_data(tmp_path, capsys):
    d = tmp_path / fo.BERT_CONFIGS["tiny"]["_name_or_path"]
    d.mkdir()
    shutil.copy(os.path.join(fo.TOY, "vocab.txt"), d)
    (d / "config.json").write_text(json.dumps(fo.BERT_CONFIGS["tiny"]))
    ckpt = str(tmp_path / "init.pt")
    torch.save(fo.weights("tiny")[0], ckpt)
    data = os.path.join(fo.TOY, "data")
    poly, pros = os.path.join(data, "polyphone_cv.txt"), os.path.join(data, "prosody_cv.txt")
    out = tmp_path / "exp"
    frontend_train.main(["--polyphone_dict", os.path.join(fo.TOY, "lexicon", "polyphone.txt"), "--prosody_dict",
                         os.path.join(fo.TOY, "lexicon", "prosody.txt"), "--train_polyphone_data", poly, "--cv_polyphone_data", poly,
                         "--train_prosody_data", pros, "--cv_prosody_data", pros, "--batch_size", "8", "--num_epochs", "2",
                         "--model_dir", str(out), "--bert_name_or_path", str(d), "--checkpoint", ckpt, "--seed", "3"])
    lines = capsys.readouterr().out.splitlines()
    assert os.path.exists(out / "0.pt") and os.path.exists(out / "1.pt")
    # a batch of one kind of line has no label for the other head (NaN): the two heads' losses are averaged on their own
    rows = {e: np.asarray([[float(l.split()[8]), float(l.split()[12])] for l in lines if l.startswith(f"Epoch {e} [CV] progress")])
            for e in (0, 1)}
    assert len(rows[0]) and rows[0].shape == rows[1].shape and any(l.startswith("Epoch 0 [TRAIN] progress 0/") for l in lines)
    cv = {e: float(0.5 * np.nanmean(rows[e][:, 0]) + 0.5 * np.nanmean(rows[e][:, 1])) for e in (0, 1)}
    assert cv[1] < cv[0], cv
    sd = torch.load(out / "1.pt", map_location="cpu", weights_only=True)
    # what train.py:215 saves: every key of the initial checkpoint with its shape (the pooler the device never reads
    # included), so that the reference's strict load_state_dict takes the file; BERT unchanged, the trained tensors moved
    init = fo.weights("tiny")[0]
    assert any(k.startswith("bert.pooler.") for k in init)
    for e in (0, 1):
        got = torch.load(out / f"{e}.pt", map_location="cpu", weights_only=True)
        assert list(got) == list(init) and all(got[k].shape == init[k].shape and got[k].dtype == init[k].dtype for k in init)
    assert all(torch.equal(sd[k], init[k]) for k in init if k.startswith("bert."))
    assert all(not torch.equal(sd[k], init[k]) for k in to.TRAINABLE)
