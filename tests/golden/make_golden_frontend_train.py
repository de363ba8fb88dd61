#!/usr/bin/env python3
"""Generates the frontend training fixtures by running the REAL reference: its FrontendModel (frontend/model.py), imported
unmodified by path, the loss statements of frontend/train.py:71-84 lifted out of its AST
(make_golden_frontend_score.lifted), loss.backward(), torch.optim.AdamW and transformers' get_scheduler("linear")
themselves.  Run in the build container only:

    python tests/golden/make_golden_frontend_train.py

The model runs in eval mode with gradients enabled: with every dropout p = 0 its train mode gives bit-identical losses
and gradients (the eval fast path is not taken when a parameter requires grad), and dropout is the one thing the device
trainer does not do.  A head without a scored label (the reference's 0 / 0) is left out of the loss that is
differentiated: the fixtures record the convention of include/wetts_hip.h, zero gradient from an empty head.

Written:
  tests/golden/frontend_train_{tiny,base}_p{34,470}_b{B}x{T}.npz  one per case of frontend_train_oracle.CASES (the scoring
      fixtures' seeds, inputs and labels): the reference's two float32 losses; per trained tensor a fixed-stride sample of
      its float32 gradient (grad_<name>, at most 1024 values), the float64 sum and L2 norm of the whole gradient
      (sum_<name>, norm_<name>); floor_grad_<name>: the reference's float32 gradient against the float64 oracle's
      autograd in fo.gates' measure (rel RMS, max |d| / rms), the worst over the config's cases; the digests.
  tests/golden/frontend_train_traj_{tiny,base}.npz  three AdamW steps (S = 4, lr 1e-3) at P = 34, lens (33, 32, 31): the
      scheduler's lr list as doubles, the three (phone, prosody, weighted) losses, and floor_loss: the reference's float32
      losses against the float64 trajectory (oracle gradients, oracle AdamW), worst over the steps."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import frontend_oracle as fo  # noqa: E402
from tests import frontend_score_oracle as so  # noqa: E402
from tests import frontend_train_oracle as to  # noqa: E402
from tests.golden.make_golden_disc import state_dict_digest  # noqa: E402
from tests.golden.make_golden_frontend import inputs_digest  # noqa: E402
from tests.golden.make_golden_frontend_score import build_reference, labels_digest, lifted  # noqa: E402


def reference_step(net, cv, ids, mask, pl, rl, w=0.5):
    """train.py:71-84 on one batch and loss.backward() -> (losses [2], weighted loss, {name: gradient}) float32."""
    import torch.nn.functional as F
    inputs = {"input_ids": ids, "token_type_ids": torch.zeros_like(ids), "attention_mask": mask}
    a = {"torch": torch, "F": F, "IGNORE_ID": so.IGNORE_ID, "compute_accuracy": lambda *x: 0.0, "model": net,
         "inputs": inputs, "phone_labels": pl, "prosody_labels": rl, "polyphone_weight": w}
    net.zero_grad(set_to_none=True)
    exec(cv, a)
    parts = [(w, a["phone_loss"], pl), (1 - w, a["prosody_loss"], rl)]
    live = [wh * l for wh, l, lab in parts if int((lab != so.IGNORE_ID).sum())]
    if len(live) == 2:
        a["loss"].backward()  # the reference's own sum
    elif live:
        live[0].backward()
    params = dict(net.named_parameters())
    trained = sorted(n for n, p in params.items() if p.requires_grad)
    assert trained == sorted(to.TRAINABLE), trained
    grads = {n: (params[n].grad.detach().clone() if params[n].grad is not None else torch.zeros_like(params[n]))
             for n in to.TRAINABLE}
    return torch.stack([a["phone_loss"].detach(), a["prosody_loss"].detach()]), a["loss"].detach(), grads


def case_fixtures(tmp, cv):
    for cname in fo.CONFIGS:
        nets = {P: build_reference(cname, P, tmp) for P, _ in so.CLASS_COUNTS}
        cases, floors = {}, {}
        for c, P, lens in to.CASES:
            if c != cname:
                continue
            ids, mask, pl, rl, L64, G64 = to.reference(cname, P, lens)
            L32, loss32, G32 = reference_step(nets[P], cv, ids, mask, pl, rl)
            # pad content: other ids at the padded positions leave every gradient bit-identical
            ids2 = torch.where(mask != 0, ids, torch.full_like(ids, 7))
            G32b = reference_step(nets[P], cv, ids2, mask, pl, rl)[2]
            assert all(torch.equal(G32[n], G32b[n]) for n in to.TRAINABLE), (cname, P, lens)
            for n in to.TRAINABLE:
                floors[n] = fo.worst(floors.get(n), fo.gates(G32[n], G64[n]))
            cases[(P, lens)] = (ids, mask, pl, rl, L32, loss32, G32)
        print(cname, "floors:", {k.replace("transform.", "t."): tuple(float(f"{x:.2g}") for x in v) for k, v in floors.items()})
        for (P, lens), (ids, mask, pl, rl, L32, loss32, G32) in cases.items():
            sc = so.load_fixture(cname, P, lens)
            out = dict(weight_seed=fo.WSEED, state_dict_sha256=state_dict_digest(so.weights(cname, P)[0]),
                       input_seed=int(sc["input_seed"]), inputs_sha256=inputs_digest(ids, mask), labels_sha256=labels_digest(pl, rl),
                       lens=np.asarray(lens, np.int64), num_polyphones=P, losses=L32.numpy(), loss=loss32.numpy())
            for n in to.TRAINABLE:
                s, total, norm = to.sample(G32[n])
                out["grad_" + n], out["sum_" + n], out["norm_" + n] = s.numpy(), np.float64(total), np.float64(norm)
                out["floor_grad_" + n] = np.asarray(floors[n], np.float64)
            path = os.path.join(HERE, to.case_name(cname, P, lens) + ".npz")
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path), "bytes")


def trajectories(tmp, cv):
    from transformers import get_scheduler
    P, lens = fo.NUM_POLYPHONES, to.TRAJ_LENS
    for cname in fo.CONFIGS:
        net = build_reference(cname, P, tmp)
        ids, mask, pl, rl, _, _ = to.reference(cname, P, lens)
        opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=to.TRAJ_LR)
        sched = get_scheduler("linear", optimizer=opt, num_warmup_steps=0, num_training_steps=to.TRAJ_TOTAL)
        W64 = dict(so.weights(cname, P)[1])
        m = {n: torch.zeros_like(W64[n]) for n in to.TRAINABLE}
        v = {n: torch.zeros_like(W64[n]) for n in to.TRAINABLE}
        lrs, rows, floor = [], [], None
        want = to.lr_list(to.TRAJ_LR, to.TRAJ_TOTAL, to.TRAJ_STEPS)
        for t in range(1, to.TRAJ_STEPS + 1):
            lrs.append(float(sched.get_last_lr()[0]))
            L32, loss32, _ = reference_step(net, cv, ids, mask, pl, rl)  # leaves .grad for the optimiser
            opt.step()
            sched.step()
            L64, G64 = to.autograd(W64, cname, ids, mask, pl, rl)
            for n in to.TRAINABLE:
                W64[n], m[n], v[n] = to.adamw_step(W64[n], G64[n], m[n], v[n], t, want[t - 1])
            rows.append([float(L32[0]), float(L32[1]), float(loss32)])
            floor = fo.worst(floor, fo.gates(L32.double(), L64))
        assert lrs == want, (lrs, want)
        out = dict(weight_seed=fo.WSEED, num_polyphones=P, lens=np.asarray(lens, np.int64), lr=np.asarray(lrs, np.float64),
                   losses=np.asarray(rows, np.float32), floor_loss=np.asarray(floor, np.float64), steps=to.TRAJ_STEPS,
                   total_steps=to.TRAJ_TOTAL, base_lr=np.float64(to.TRAJ_LR))
        path = os.path.join(HERE, to.traj_name(cname) + ".npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes", rows, "floor_loss", floor)


def main():
    cv = lifted()[1]
    with tempfile.TemporaryDirectory() as tmp:
        case_fixtures(tmp, cv)
        trajectories(tmp, cv)


if __name__ == "__main__":
    main()
