"""Training the text frontend on the device: the other half of frontend/train.py.

    trainer = FrontendTrainer(model, lr=1e-3, num_training_steps=epochs * len(loader))
    scores = trainer.step(inputs, phone_labels, prosody_labels)      # train.py:71-101 on one batch

    python -m wetts_amd.frontend_train --polyphone_dict D --prosody_dict D --train_polyphone_data F ... --model_dir OUT

What is trained is what the reference trains (frontend/model.py:30-31 freezes BERT): the 12 `transform.*` tensors and the
4 classifier tensors.  The optimiser is torch.optim.AdamW's algorithm at its defaults with the linear schedule of
train.py:184-190.  The forward pass, the loss, its gradient and the update run in csrc/frontend_train.hip; no torch op
touches an activation or a gradient, and step() reads nothing back.

ONE known difference from train.py: dropout.  The reference's model.train() turns on p = 0.1 dropout in `transform` and
inside the frozen BERT; its masks come from torch's generator.  Here the step differentiates the dropout-free forward
pass (`dropout=0.0`; any other value raises NotImplementedError).

Empty head: a batch without a scored label for a head reports that head's loss (and `loss`) as NaN, exactly as
FrontendModel.score() does, and the head contributes ZERO gradient (the reference's 0 / 0 would write NaN into every
weight).  Labels the status word flags (outside their classes, at a padded token) are not scored and contribute none."""
import argparse
import ctypes as C
import os
import sys
from functools import partial

import torch

from . import _lib, checkpoint
from .frontend import FrontendModel, FrontendScores, HostScores
from .frontend_data import FrontendDataset, VocabTokenizer, collate_fn, read_table


def linear_schedule(lr, num_training_steps, step):
    """transformers' get_scheduler("linear", num_warmup_steps=0, num_training_steps=S) after `step` scheduler steps:
    lr * max(0, (S - step) / S), in double."""
    return float(lr) * max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps)))


class FrontendTrainer:
    """train.py:96-101 and :184-190 for a FrontendModel on a device.  grad() computes the loss and its gradient, step()
    also applies AdamW and the scheduler.  The model itself stays as it is (its train() still raises): after step(),
    its forward(), score() and state_dict() see the new weights."""

    def __init__(self, model, lr=1e-3, num_training_steps=1, polyphone_weight=0.5, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.01, dropout=0.0):
        if not isinstance(model, FrontendModel):
            raise TypeError("model must be a wetts_amd.FrontendModel")
        if float(dropout) != 0.0:
            raise NotImplementedError("dropout is not implemented: the step differentiates the dropout-free forward pass "
                                      "(train-mode dropout in `transform` and BERT is a follow-up); pass dropout=0.0")
        if model._precision != 0:
            raise ValueError("training is float32 only: call model.set_dtype(torch.float32) first")
        if int(num_training_steps) < 1:
            raise ValueError(f"num_training_steps must be at least 1, got {num_training_steps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or lr < 0 or eps < 0 or weight_decay < 0:
            raise ValueError("lr, eps and weight_decay must not be negative, the betas in [0, 1)")
        self.model = model
        self.base_lr, self.num_training_steps = float(lr), int(num_training_steps)
        self.polyphone_weight = float(polyphone_weight)
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.step_count = 0
        cfg = checkpoint.frontend_c_config(model.config)
        off, num = C.c_int64(), C.c_int64()
        _lib.check(_lib.load().wetts_frontend_trainable_span(C.byref(cfg), C.byref(off), C.byref(num)),
                   "frontend_trainable_span")
        self.span = (int(off.value), int(num.value))
        self.layout = [(n, o - self.span[0], k, shape) for n, o, k, shape in checkpoint.frontend_layout(model.config)
                       if o >= self.span[0]]
        self._m = self._v = None

    @property
    def lr(self):
        """The learning rate the next step uses."""
        return linear_schedule(self.base_lr, self.num_training_steps, self.step_count)

    def _state(self):
        self.model._require()
        if self._m is None or self._m.device != self.model.device:
            self._m = torch.zeros(self.span[1], dtype=torch.float32, device=self.model.device)
            self._v = torch.zeros(self.span[1], dtype=torch.float32, device=self.model.device)
        return self._m, self._v

    def _grad(self, inputs, phone_labels, prosody_labels):
        m = self.model
        if m._precision != 0:
            raise ValueError("training is float32 only: the model was switched to a 16-bit mode")
        ids, tt, mask = m._inputs(inputs["input_ids"], inputs.get("token_type_ids"), inputs.get("attention_mask"))
        B, T = ids.shape
        pl, rl = m._labels(phone_labels, "phone_labels", B, T), m._labels(prosody_labels, "prosody_labels", B, T)
        lib = _lib.load()
        nbytes = int(lib.wetts_frontend_train_workspace_bytes(m._handle, B, T))
        if nbytes < 0:
            raise _lib.WettsError(f"frontend_train_workspace_bytes: {_lib.last_error()}")
        dev = m.device
        with torch.cuda.device(dev):
            ws = self._workspace((nbytes + 3) // 4, dev)
            grad = torch.empty(self.span[1], dtype=torch.float32, device=dev)
            nll = torch.empty(2, B, T, dtype=torch.float32, device=dev)
            pred = torch.empty(2, B, T, dtype=torch.int32, device=dev)
            losses = torch.empty(2, dtype=torch.float32, device=dev)
            counts = torch.empty(22, dtype=torch.int64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(lib.wetts_frontend_grad(m._handle, _lib.ptr(ids), _lib.ptr(tt), _lib.ptr(mask), _lib.ptr(pl),
                                               _lib.ptr(rl), B, T, self.polyphone_weight, _lib.ptr(grad), _lib.ptr(losses),
                                               _lib.ptr(counts), _lib.ptr(nll[0]), _lib.ptr(nll[1]), _lib.ptr(pred[0]),
                                               _lib.ptr(pred[1]), _lib.ptr(ws), nbytes, _lib.ptr(status),
                                               _lib.current_stream_ptr()), "frontend_grad")
        return FrontendScores(losses, counts, nll, pred, status, self.polyphone_weight), grad

    _ws = None

    def _workspace(self, floats, dev):
        """The scratch of a step (hook for tests that fill it beforehand)."""
        if self._ws is None or self._ws.numel() < floats or self._ws.device != dev:
            self._ws = torch.empty(floats, dtype=torch.float32, device=dev)
        return self._ws

    def named(self, flat):
        """{reference key: view} of a buffer in the trainable span's layout."""
        return {n: flat[o:o + k].view(shape) for n, o, k, shape in self.layout}

    def grad(self, inputs, phone_labels=None, prosody_labels=None):
        """-> (FrontendScores, {reference key: device tensor}): the loss of train.py:71-84 and its gradient.  No update."""
        scores, grad = self._grad(inputs, phone_labels, prosody_labels)
        self.last_grad = grad
        return scores, self.named(grad)

    def step(self, inputs, phone_labels=None, prosody_labels=None):
        """train.py:71-101 on one batch -> the FrontendScores of the batch BEFORE the update (what train.py logs)."""
        scores, grad = self._grad(inputs, phone_labels, prosody_labels)
        self.last_grad = grad
        m, v = self._state()
        t = self.step_count + 1
        b1, b2 = self.betas
        with torch.cuda.device(self.model.device):
            _lib.check(_lib.load().wetts_frontend_adamw_step(self.model._handle, _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v),
                                                             self.lr, b1, b2, self.eps, self.weight_decay, 1.0 - b1 ** t,
                                                             1.0 - b2 ** t, _lib.current_stream_ptr()), "frontend_adamw_step")
        self.step_count = t
        self.model._stale = True
        return scores

    def weights(self):
        """The trainable span as it is on the device now (a copy), in the span's layout; named() keys it."""
        self.model._require()
        with torch.cuda.device(self.model.device):
            out = torch.empty(self.span[1], dtype=torch.float32, device=self.model.device)
            _lib.check(_lib.load().wetts_frontend_read_weights(self.model._handle, self.span[0], self.span[1], _lib.ptr(out),
                                                               _lib.current_stream_ptr()), "frontend_read_weights")
        return out

    def state_dict(self):
        """The optimiser's state: step, exp_avg and exp_avg_sq per reference key (CPU tensors), and the schedule."""
        m, v = self._state()
        return {"step": self.step_count, "lr": self.base_lr, "num_training_steps": self.num_training_steps,
                "exp_avg": {k: t.cpu().clone() for k, t in self.named(m).items()},
                "exp_avg_sq": {k: t.cpu().clone() for k, t in self.named(v).items()}}

    def load_optimizer_state(self, state):
        m, v = self._state()
        for buf, key in ((m, "exp_avg"), (v, "exp_avg_sq")):
            views = self.named(buf)
            for k, t in state[key].items():
                if k not in views or tuple(views[k].shape) != tuple(t.shape):
                    raise ValueError(f"optimizer state {key}[{k!r}] does not match the model")
                views[k].copy_(t.to(torch.float32))
        self.step_count = int(state["step"])
        return self


# ---- python -m wetts_amd.frontend_train ---------------------------------------------------------------------------------
def get_args(argv=None):
    """train.py:104-151's arguments, plus --checkpoint and --seed."""
    parser = argparse.ArgumentParser(prog="python -m wetts_amd.frontend_train", description="training your network")
    parser.add_argument("--polyphone_dict", required=True, help="polyphone dict")
    parser.add_argument("--prosody_dict", required=True, help="prosody dict")
    parser.add_argument("--train_polyphone_data", required=True, help="train data file")
    parser.add_argument("--cv_polyphone_data", required=True, help="cv data file")
    parser.add_argument("--train_prosody_data", required=True, help="train data file")
    parser.add_argument("--cv_prosody_data", required=True, help="cv data file")
    parser.add_argument("--gpu", type=int, default=0, help="device index")
    parser.add_argument("--batch_size", type=int, default=32, help="batch size")
    parser.add_argument("--num_epochs", type=int, default=4, help="num training epochs")
    parser.add_argument("--log_interval", type=int, default=1, help="log interval")
    parser.add_argument("--lr", type=float, default=0.001, help="learning rate")
    parser.add_argument("--polyphone_weight", type=float, default=0.5, help="polyphone task weight")
    parser.add_argument("--model_dir", required=True, help="save model dir")
    parser.add_argument("--bert_name_or_path", default="bert-chinese-base",
                        help="local directory holding the BERT's config.json and vocab.txt")
    parser.add_argument("--checkpoint", required=True, help="the initial state_dict (BERT included), as torch.save wrote it")
    parser.add_argument("--seed", type=int, default=0, help="seed of the training set's shuffle")
    return parser.parse_args(argv)


def _log(epoch, tag, batch, total, h):
    """train.py:87-92."""
    logstr = "Epoch {} [{}] progress {}/{} loss {:.6f}".format(epoch, tag, batch, total, h.loss)
    logstr += " polyphone_loss {:.6f} polyphone_acc {:.6f}".format(h.phone_loss, h.phone_acc)
    logstr += " prosody_loss {:.6f} prosody_acc {:.6f}".format(h.prosody_loss, h.prosody_acc)
    return logstr


def run(args):
    """train.py:154-216 -> the printed log lines.  An epoch's rows are read back in ONE copy after its last batch.
    `{epoch}.pt` holds the keys of --checkpoint (the trained tensors replaced), as train.py:215 saves the whole module."""
    polyphone_dict, prosody_dict = read_table(args.polyphone_dict), read_table(args.prosody_dict)
    tokenizer = VocabTokenizer(os.path.join(args.bert_name_or_path, "vocab.txt"))
    train = FrontendDataset(tokenizer, args.train_polyphone_data, polyphone_dict, args.train_prosody_data, prosody_dict)
    cv = FrontendDataset(tokenizer, args.cv_polyphone_data, polyphone_dict, args.cv_prosody_data, prosody_dict)
    gen = torch.Generator().manual_seed(args.seed)
    col = partial(collate_fn, tokenizer=tokenizer)
    train_loader = torch.utils.data.DataLoader(train, batch_size=args.batch_size, shuffle=True, collate_fn=col, generator=gen)
    cv_loader = torch.utils.data.DataLoader(cv, batch_size=args.batch_size, shuffle=False, collate_fn=col)
    model = FrontendModel(len(polyphone_dict), len(prosody_dict), os.path.join(args.bert_name_or_path, "config.json"),
                          bert_name_or_path=args.bert_name_or_path)
    init = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    model.load_state_dict(init).to(f"cuda:{args.gpu}")
    trainer = FrontendTrainer(model, lr=args.lr, num_training_steps=max(1, args.num_epochs * len(train_loader)),
                              polyphone_weight=args.polyphone_weight)
    os.makedirs(args.model_dir, exist_ok=True)
    lines = []
    w = args.polyphone_weight
    for epoch in range(args.num_epochs):
        print("Epoch {}/{}...".format(epoch, args.num_epochs))
        for tag, loader in (("TRAIN", train_loader), ("CV", cv_loader)):
            rows = []
            for inputs, pl, rl in loader:
                s = trainer.step(inputs, pl, rl) if tag == "TRAIN" else model.score(inputs, pl, rl, polyphone_weight=w)
                rows.append(s.packed())
            if not rows:
                continue
            back = torch.stack(rows).cpu()
            for batch, row in enumerate(back):
                if batch % args.log_interval == 0:
                    lines.append(_log(epoch, tag, batch, len(rows), HostScores.from_packed(row, w)))
                    print(lines[-1])
            sys.stdout.flush()
        # train.py:215 saves the whole module: what the device model does not read (bert.pooler.*, position_ids) is carried
        # over from --checkpoint, so that the reference's strict load_state_dict (test_polyphone.py:69) finds every key
        trained = model.state_dict()
        out = {k: trained.get(k, v) for k, v in init.items()}
        out.update({k: v for k, v in trained.items() if k not in out})
        torch.save(out, os.path.join(args.model_dir, "{}.pt".format(epoch)))
    return lines


def main(argv=None):
    run(get_args(argv))


if __name__ == "__main__":
    main()
