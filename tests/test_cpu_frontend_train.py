"""CPU tier of frontend training: the float64 oracle of tests/frontend_train_oracle.py against the reference's fixtures
(tests/golden/frontend_train_*.npz), its hand-written backward pass against autograd, its AdamW against torch.optim.AdamW,
the schedule, the injected defects (each has to move a figure to at least 10 x its gate on the fixtures' shapes, or the
fixtures could not tell a broken kernel from a good one) and the host-side checks of wetts_amd.frontend_train."""
import numpy as np
import pytest
import torch

from tests import frontend_oracle as fo
from tests import frontend_score_oracle as so
from tests import frontend_train_oracle as to
from wetts_amd import FrontendModel
from wetts_amd.frontend_train import FrontendTrainer, linear_schedule

DEFECT_CASES = (("tiny", 34, (9, 6)), ("tiny", 34, (33, 32, 31)), ("tiny", 470, (65, 64, 63)), ("base", 34, (9, 6)))


@pytest.mark.parametrize("cname,P,lens", to.CASES)
def test_oracle_reproduces_the_reference_fixture(cname, P, lens):
    c = to.load_fixture(cname, P, lens)
    sc = so.load_fixture(cname, P, lens)
    ids, mask, pl, rl, losses, grads = to.reference(cname, P, lens)
    assert str(c["inputs_sha256"]) == str(sc["inputs_sha256"]) and str(c["labels_sha256"]) == str(sc["labels_sha256"])
    for k, hd in enumerate(("phone", "prosody")):
        if np.isnan(c["losses"][k]):
            assert bool(torch.isnan(losses[k]))
            continue
        fig = fo.gates(torch.tensor([float(c["losses"][k])], dtype=torch.float64), losses[k:k + 1])
        assert fo.within(fig, fo.fixture_gate(sc["floor_loss_" + hd])), (hd, fig)
    for n in to.TRAINABLE:
        got, total, norm = to.sample(grads[n])
        want = torch.from_numpy(c["grad_" + n])
        assert got.shape == want.shape and want.numel() <= to.SAMPLE and want.dtype == torch.float32
        g = fo.fixture_gate(c["floor_grad_" + n])
        if float(c["norm_" + n]) == 0.0:
            assert norm == 0.0
            continue
        fig = to.sample_figure(want, got, norm, grads[n].numel())
        assert fo.within(fig, g), (n, fig, g)
        assert abs(norm - float(c["norm_" + n])) <= g[0] * norm, n


@pytest.mark.parametrize("cname", fo.CONFIGS)
def test_oracle_reproduces_the_reference_trajectory(cname):
    c = to.load_traj(cname)
    P, lens = int(c["num_polyphones"]), tuple(int(v) for v in c["lens"])
    ids, mask, pl, rl, _, _ = to.reference(cname, P, lens)
    W = dict(so.weights(cname, P)[1])
    m = {n: torch.zeros_like(W[n]) for n in to.TRAINABLE}
    v = {n: torch.zeros_like(W[n]) for n in to.TRAINABLE}
    lrs = to.lr_list(float(c["base_lr"]), int(c["total_steps"]), int(c["steps"]))
    assert c["lr"].dtype == np.float64 and c["lr"].tolist() == lrs
    for t in range(1, int(c["steps"]) + 1):
        losses, G = to.autograd(W, cname, ids, mask, pl, rl)
        fig = fo.gates(torch.from_numpy(c["losses"][t - 1][:2]).double(), losses)
        assert fo.within(fig, fo.fixture_gate(c["floor_loss"])), (t, fig)
        for n in to.TRAINABLE:
            W[n], m[n], v[n] = to.adamw_step(W[n], G[n], m[n], v[n], t, lrs[t - 1])


@pytest.mark.parametrize("cname,P,lens", DEFECT_CASES)
def test_backward_by_hand_equals_autograd(cname, P, lens):
    ids, mask, pl, rl, losses, grads = to.reference(cname, P, lens)
    l2, g2 = to.manual(so.weights(cname, P)[1], cname, ids, mask, pl, rl)
    assert torch.equal(torch.isnan(l2), torch.isnan(losses)) and torch.allclose(l2, losses, rtol=1e-13, atol=0, equal_nan=True)
    for n in to.TRAINABLE:
        fig = fo.gates(g2[n], grads[n])
        assert fig[0] <= 1e-13 and fig[1] <= 1e-12, (n, fig)


def test_key_bias_gradient_is_zero_and_the_tensor_is_gated_whole():
    _, _, _, _, _, grads = to.reference("tiny", 34, (9, 6))
    g = grads["transform.self_attn.in_proj_bias"]
    d = g.numel() // 3
    assert float(g[d:2 * d].norm()) <= 1e-14 * float(g.norm()) and float(g.norm()) > 0


@pytest.mark.parametrize("fault", to.GRAD_FAULTS)
def test_injected_gradient_defect_is_seen(fault):
    w = 0.3  # (at 0.5 the weight on both heads is no defect)
    top = 0.0
    for cname, P, lens in DEFECT_CASES:
        c = to.load_fixture(cname, P, lens)
        ids, mask, pl, rl, _, _ = to.reference(cname, P, lens)
        W = so.weights(cname, P)[1]
        _, want = to.autograd(W, cname, ids, mask, pl, rl, w)
        _, got = to.manual(W, cname, ids, mask, pl, rl, w, fault)
        for n in to.TRAINABLE:
            fig, g = fo.gates(got[n], want[n]), fo.gate(c["floor_grad_" + n])
            top = max(top, fig[0] / g[0], fig[1] / g[1])
    assert top >= 10.0, (fault, top)


def _adamw_inputs(n=4096, seed=5):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.05
    grad = torch.randn(n, generator=g) * 10 ** torch.randint(-6, 1, (n,), generator=g).float()
    grad[:64] = 0.0
    grad[64:128] = 1e-12 * torch.sign(torch.randn(64, generator=g))
    return p, grad


def test_adamw_restatement_equals_torch_in_float64():
    p0, g = _adamw_inputs()
    lrs = to.lr_list(1e-3, 4, 3)
    ref = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, foreach=False)
    p, m, v = p0.double(), torch.zeros(p0.numel(), dtype=torch.float64), torch.zeros(p0.numel(), dtype=torch.float64)
    for t in range(1, 4):
        for group in opt.param_groups:
            group["lr"] = lrs[t - 1]
        ref.grad = (g.double() * t).clone()
        opt.step()
        old = p
        p, m, v = to.adamw_step(p, g.double() * t, m, v, t, lrs[t - 1])
        st = opt.state[ref]
        # relative to what the element is made of: |p| + |p - p_old| for a parameter (where the update cancels the
        # parameter the difference of two roundings is not small against the remainder), the value itself for m and v
        for got, want, scale in ((p, ref.detach(), ref.detach().abs() + (ref.detach() - old).abs()), (m, st["exp_avg"], None),
                                 (v, st["exp_avg_sq"], None)):
            scale = want.abs() if scale is None else scale
            assert float(((got - want).abs() / scale.clamp_min(1e-300)).max()) <= 1e-15, t


@pytest.mark.parametrize("fault", to.ADAMW_FAULTS)
def test_injected_adamw_defect_is_seen(fault):
    p0, g = _adamw_inputs()
    z = torch.zeros_like(p0)
    top = 0.0
    for t in (1, 2):
        p64, _, _ = to.adamw_step(p0.double(), g.double(), z.double(), z.double(), t, 1e-3)
        ref = torch.nn.Parameter(p0.clone())
        opt = torch.optim.AdamW([ref], lr=1e-3, foreach=False)
        opt.state[ref] = {"step": torch.tensor(float(t - 1)), "exp_avg": z.clone(), "exp_avg_sq": z.clone()}
        ref.grad = g.clone()
        opt.step()
        floor = max(to.adamw_figure(ref.detach(), p64, p0), 1.0)
        bad, _, _ = to.adamw_step(p0, g, z, z, t, 1e-3, fault=fault)
        top = max(top, to.adamw_figure(bad, p64, p0) / (4 * floor))
    assert top >= 10.0, (fault, top)


def test_schedule_is_the_linear_one_in_double():
    for lr, S in ((1e-3, 4), (3e-4, 7), (1.0, 1)):
        want = [lr * max(0.0, (S - t) / S) for t in range(S + 3)]
        assert [linear_schedule(lr, S, t) for t in range(S + 3)] == want
        assert to.lr_list(lr, S, S + 3) == want


def _model(cname="tiny"):
    return FrontendModel(fo.NUM_POLYPHONES, fo.NUM_PROSODY, fo.BERT_CONFIGS[cname])


def test_host_side_refusals():
    with pytest.raises(NotImplementedError, match="dropout"):
        FrontendTrainer(_model(), num_training_steps=4, dropout=0.1)
    with pytest.raises(ValueError, match="float32"):
        FrontendTrainer(_model().set_dtype(torch.bfloat16), num_training_steps=4)
    with pytest.raises(ValueError, match="num_training_steps"):
        FrontendTrainer(_model(), num_training_steps=0)
    with pytest.raises(NotImplementedError):
        _model().train()
    with pytest.raises(TypeError):
        FrontendTrainer(object(), num_training_steps=4)


def test_trainer_knows_the_trainable_span_and_the_reference_keys():
    import wetts_amd
    assert wetts_amd.FrontendTrainer is FrontendTrainer
    tr = FrontendTrainer(_model(), lr=1e-3, num_training_steps=4)
    assert tuple(n for n, _, _, _ in tr.layout) == to.TRAINABLE and tr.layout[0][1] == 0
    assert tr.span[1] % 4 == 0 and tr.span[1] >= sum(k for _, _, k, _ in tr.layout)
    assert tr.lr == 1e-3 and tr.step_count == 0
    sd = so.weights("tiny", fo.NUM_POLYPHONES)[0]
    assert {n: tuple(s) for n, _, _, s in tr.layout} == {n: tuple(sd[n].shape) for n in to.TRAINABLE}
