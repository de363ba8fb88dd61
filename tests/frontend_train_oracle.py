"""Float64 restatement of the frontend's training step on top of frontend_oracle / frontend_score_oracle: the loss of
frontend/train.py:71-84, its gradient with respect to the 16 tensors the reference trains (model.py:30-31 freezes BERT) --
once by autograd through the oracles' own forward pass, once written out by hand stage by stage (what
csrc/frontend_train.hip computes), so that a defect can be injected into any stage -- torch.optim.AdamW's single-tensor
algorithm and the linear schedule.  Plain torch; no `transformers`.

Conventions (include/wetts_hip.h): a head without a scored label reports NaN and contributes ZERO gradient; a label
outside its classes or at a padded token is not scored."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import frontend_oracle as fo
from tests import frontend_score_oracle as so

TRAINABLE = ("transform.self_attn.in_proj_weight", "transform.self_attn.in_proj_bias", "transform.self_attn.out_proj.weight",
             "transform.self_attn.out_proj.bias", "transform.linear1.weight", "transform.linear1.bias",
             "transform.linear2.weight", "transform.linear2.bias", "transform.norm1.weight", "transform.norm1.bias",
             "transform.norm2.weight", "transform.norm2.bias", "phone_classifier.weight", "phone_classifier.bias",
             "prosody_classifier.weight", "prosody_classifier.bias")
CASES = so.CASES
TRAJ_LENS = (33, 32, 31)
TRAJ_STEPS, TRAJ_TOTAL, TRAJ_LR = 3, 4, 1e-3
SAMPLE = 1024  # values kept per gradient tensor in a fixture (a fixed stride over the flattened tensor)
TILE = 32

# mean over all tokens instead of the scored ones; the polyphone weight on both heads; the softmax backward without its
# delta term; a masked key receiving gradient; unbiased variance in the LayerNorm backward; no ReLU mask; the residual's
# gradient dropped at the second add (the first add's only reaches the frozen BERT: no trained tensor can see it); dK
# without the 1 / sqrt(dk) of the scores; the last token tile left out of every wgrad; the ragged class tile left out of
# the polyphone classifier's dgrad
GRAD_FAULTS = ("mean_over_all_tokens", "weight_on_both_heads", "no_delta", "masked_key_gradient", "unbiased_variance",
               "no_relu_mask", "no_residual_gradient", "no_q_scale_in_dk", "dropped_token_tile", "dropped_class_tile")
ADAMW_FAULTS = ("no_bias_correction", "l2_instead_of_decoupled")


def case_name(cname, P, lens):
    return f"frontend_train_{cname}_p{P}_b{len(lens)}x{max(lens)}"


def traj_name(cname):
    return f"frontend_train_traj_{cname}"


def stride(numel):
    return max(1, -(-int(numel) // SAMPLE))


def sample(t):
    """The fixed-stride sample of a tensor, its float64 sum and L2 norm."""
    f = t.detach().reshape(-1)
    return f[::stride(f.numel())].clone(), float(f.double().sum()), float(f.double().norm())


def sample_figure(got, want, norm, numel):
    """fo.gates' (rel RMS, max |d| / rms) of a tensor's fixed-stride sample against the stored one, with the rms of the
    WHOLE tensor (norm / sqrt(numel), stored beside the sample) as the scale: the floors are figures of whole tensors, and
    a sample that misses a tensor's few large rows has a much smaller rms of its own."""
    d = got.detach().double().reshape(-1) - want.detach().double().reshape(-1)
    rms = float(norm) / math.sqrt(float(numel))
    return float(d.pow(2).mean().sqrt()) / rms, float(d.abs().max()) / rms


def scored(mask, labels, M):
    if labels is None:
        return torch.zeros_like(mask, dtype=torch.bool)
    return (mask != 0) & (labels >= 0) & (labels < M)


# ---- autograd through the oracles' own forward pass -----------------------------------------------------------------------
def autograd(W, cname, ids, mask, pl, rl, w=0.5):
    """-> (losses [2] (NaN for an empty head), {name: gradient}) at W's dtype.  W is left unchanged."""
    Wg = dict(W)
    for n in TRAINABLE:
        Wg[n] = W[n].detach().clone().requires_grad_(True)
    x = fo.forward(Wg, cname, ids, mask)["transform"]
    zp, zr = so.logits(Wg, x)
    losses, total = [], None
    for z, lab, wh in ((zp, pl, w), (zr, rl, 1 - w)):
        _, _, loss, n, _ = so.head(z, mask, lab)
        losses.append(loss.detach())
        if n > 0:
            total = wh * loss if total is None else total + wh * loss
    grads = {n: torch.zeros_like(W[n]) for n in TRAINABLE}
    if total is not None:
        for n, g in zip(TRAINABLE, torch.autograd.grad(total, [Wg[n] for n in TRAINABLE], allow_unused=True)):
            if g is not None:
                grads[n] = g
    return torch.stack(losses), grads


# ---- the backward pass by hand ---------------------------------------------------------------------------------------------
def _ln_backward(dy, x, gamma, eps, fault=None):
    C = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / (C - 1 if fault == "unbiased_variance" else C)
    rstd = 1 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).reshape(-1, C), dy.reshape(-1, C)


def _wgrad(dy, x, fault=None):
    """dy [B, T, M], x [B, T, K] -> (dW [M, K], db [M]) over the tokens."""
    dy2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
    if fault == "dropped_token_tile":
        N = dy2.shape[0]
        keep = 64 * ((N - 1) // 64) if N > 64 else 16 * ((N - 1) // 16)
        dy2, x2 = dy2[:keep], x2[:keep]
    return dy2.t() @ x2, dy2.sum(0)


def manual(W, cname, ids, mask, pl, rl, w=0.5, fault=None):
    """-> (losses [2], {name: gradient}): the stages of csrc/frontend_train.hip in torch at W's dtype."""
    c = fo.config(cname)
    d, H, eps = c["hidden_size"], c["transform_heads"], 1e-5
    dk = d // H
    B, T = ids.shape
    G = {}
    h0 = fo.forward(W, cname, ids, mask)["bert"]
    # forward of `transform`, every intermediate kept
    qkv = F.linear(h0, W[TRAINABLE[0]], W[TRAINABLE[1]])
    q, k, v = (t.reshape(B, T, H, dk).transpose(1, 2) for t in qkv.split(d, dim=2))
    scale = 1 / math.sqrt(dk)
    s = (q @ k.transpose(2, 3)) * scale
    sm = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    p = torch.nan_to_num(torch.softmax(sm, dim=-1), nan=0.0)
    o = p @ v
    ctx = o.transpose(1, 2).reshape(B, T, d)
    s1 = F.linear(ctx, W["transform.self_attn.out_proj.weight"], W["transform.self_attn.out_proj.bias"]) + h0
    h1 = fo.layer_norm(s1, W["transform.norm1.weight"], W["transform.norm1.bias"], eps)
    ffa = F.relu(F.linear(h1, W["transform.linear1.weight"], W["transform.linear1.bias"]))
    s2 = F.linear(ffa, W["transform.linear2.weight"], W["transform.linear2.bias"]) + h1
    xo = fo.layer_norm(s2, W["transform.norm2.weight"], W["transform.norm2.bias"], eps)
    zp, zr = so.logits(W, xo)
    # cross-entropy backward
    losses, dls = [], []
    for hd, (z, lab, wh) in enumerate(((zp, pl, w), (zr, rl, 1 - w))):
        M = z.shape[-1]
        sc = scored(mask, lab, M)
        n = int(sc.sum())
        losses.append(so.head(z, mask, lab)[2])
        if n == 0:
            dls.append(torch.zeros_like(z))
            continue
        den = mask.numel() if fault == "mean_over_all_tokens" else n
        if fault == "weight_on_both_heads":
            wh = w
        onehot = F.one_hot(lab.clamp(0, M - 1), M).to(z.dtype)
        dls.append((wh / den) * (torch.softmax(z, -1) - onehot) * sc.unsqueeze(-1).to(z.dtype))
    dlp, dlr = dls
    G["phone_classifier.weight"], G["phone_classifier.bias"] = _wgrad(dlp, xo, fault)
    G["prosody_classifier.weight"], G["prosody_classifier.bias"] = _wgrad(dlr, xo, fault)
    Wp = W["phone_classifier.weight"]
    if fault == "dropped_class_tile":
        keep = TILE * ((Wp.shape[0] - 1) // TILE)
        dxo = dlp[..., :keep] @ Wp[:keep] + dlr @ W["prosody_classifier.weight"]
    else:
        dxo = dlp @ Wp + dlr @ W["prosody_classifier.weight"]
    ds2, gg, gb = _ln_backward(dxo, s2, W["transform.norm2.weight"], eps, fault)
    G["transform.norm2.weight"], G["transform.norm2.bias"] = gg.sum(0), gb.sum(0)
    G["transform.linear2.weight"], G["transform.linear2.bias"] = _wgrad(ds2, ffa, fault)
    dff = ds2 @ W["transform.linear2.weight"]
    if fault != "no_relu_mask":
        dff = dff * (ffa > 0).to(dff.dtype)
    G["transform.linear1.weight"], G["transform.linear1.bias"] = _wgrad(dff, h1, fault)
    dh1 = dff @ W["transform.linear1.weight"]
    if fault != "no_residual_gradient":
        dh1 = dh1 + ds2
    ds1, gg, gb = _ln_backward(dh1, s1, W["transform.norm1.weight"], eps, fault)
    G["transform.norm1.weight"], G["transform.norm1.bias"] = gg.sum(0), gb.sum(0)
    G["transform.self_attn.out_proj.weight"], G["transform.self_attn.out_proj.bias"] = _wgrad(ds1, ctx, fault)
    dctx = ds1 @ W["transform.self_attn.out_proj.weight"]
    # attention backward
    do = dctx.reshape(B, T, H, dk).transpose(1, 2)
    pb = torch.softmax(s, dim=-1) if fault == "masked_key_gradient" else p
    dp = do @ v.transpose(2, 3)
    delta = torch.zeros_like(dp[..., :1]) if fault == "no_delta" else (do * o).sum(-1, keepdim=True)
    dS = pb * (dp - delta)
    dq = (dS @ k) * scale
    dkk = dS.transpose(2, 3) @ q
    if fault != "no_q_scale_in_dk":
        dkk = dkk * scale
    dv = pb.transpose(2, 3) @ do
    dqkv = torch.cat([t.transpose(1, 2).reshape(B, T, d) for t in (dq, dkk, dv)], 2)
    G[TRAINABLE[0]], G[TRAINABLE[1]] = _wgrad(dqkv, h0, fault)
    return torch.stack(losses), {n: G[n] for n in TRAINABLE}


# ---- AdamW and the schedule ---------------------------------------------------------------------------------------------------
def adamw_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, fault=None):
    """torch.optim.AdamW's documented single-tensor algorithm, step t (1-based) -> (p, m, v) new tensors at p's dtype."""
    b1, b2 = betas
    if fault == "l2_instead_of_decoupled":
        g = g + weight_decay * p
    else:
        p = p * (1 - lr * weight_decay)
    m = m + (g - m) * (1 - b1)  # (the groupings are torch's: lerp_, mul_().addcmul_(), addcdiv_())
    v = v * b2 + ((1 - b2) * g) * g
    bc1, bc2 = (1.0, 1.0) if fault == "no_bias_correction" else (1 - b1 ** t, 1 - b2 ** t)
    p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
    return p, m, v


def lr_list(lr, total, steps):
    """get_scheduler("linear", num_warmup_steps=0, num_training_steps=total): the lr of the steps 0 .. steps - 1."""
    return [lr * max(0.0, (total - t) / total) for t in range(steps)]


def adamw_figure(p, p64, p_old):
    """max over the elements of |p - p64| / (2^-24 (|p64| + |p64 - p_old|)); 0 / 0 (nothing to move, nothing moved) is 0."""
    p, p64, p_old = (t.detach().double().cpu().reshape(-1) for t in (p, p64, p_old))
    den = fo.HALF_ULP * (p64.abs() + (p64 - p_old).abs())
    err = (p - p64).abs()
    fig = torch.where(den > 0, err / den, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(fig.max()) if fig.numel() else 0.0


def state_figure(x, x64):
    """The same measure for m and v: |x - x64| / (2^-24 |x64|)."""
    return adamw_figure(x, x64, x64)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def load_fixture(cname, P, lens):
    return np.load(os.path.join(fo.GOLDEN, case_name(cname, P, lens) + ".npz"))


def load_traj(cname):
    return np.load(os.path.join(fo.GOLDEN, traj_name(cname) + ".npz"))


_REF = {}


def reference(cname, P, lens):
    """(ids, mask, phone labels, prosody labels, float64 losses, {name: float64 gradient}) of a case, computed once per
    process and left unchanged."""
    key = (cname, P, tuple(lens))
    if key not in _REF:
        ids, mask, pl, rl, _, _ = so.reference(cname, P, lens)
        losses, grads = autograd(so.weights(cname, P)[1], cname, ids, mask, pl, rl)
        _REF[key] = (ids, mask, pl, rl, losses, grads)
    return _REF[key]
