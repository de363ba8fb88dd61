"""The text frontend on the device: the reference's BERT polyphone / prosody model (frontend/model.py:21-73), its exported
graph's session (frontend/export_onnx.py:72-91), cli/frontend.py's `Frontend` and cli/model.py's `Model`.

    front = Frontend(front_dir)                       # final.pt + config.json + vocab.txt + lexicon/
    model = Model(InferenceSession(net_g), phone_table, speaker_table, front)
    phonemes, audio = model.synthesis("今天天气怎么样", "default")

Everything between the string and the samples runs in csrc/frontend.hip and the existing synthesis path; there is no
CPU inference, no onnxruntime and no `transformers` import.  Evaluation only; training is frontend_train.FrontendTrainer.

Padded positions: the reference leaves whatever its torch build computes at a token whose attention_mask is 0; here both
outputs are ZEROS there."""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib, checkpoint
from .frontend_data import IGNORE_ID  # noqa: F401  (-100, frontend/dataset.py:19)

# frontend/model.py:33-42: substring of bert_name_or_path -> (d_model, nhead, dim_feedforward) of `transform`
TRANSFORM_SHAPES = (("bert-chinese-base", (768, 8, 2048)), ("TinyBERT_4L_zh_backup", (312, 12, 1200)))
# what set_dtype accepts (SynthesizerTrn.set_decoder_dtype's names) -> wetts_frontend_set_precision's number
PRECISIONS = {torch.float32: 0, "f32": 0, "fp32": 0, torch.bfloat16: 1, "bf16": 1, torch.float16: 2, "f16": 2, "fp16": 2}


def frontend_precision(dtype):
    """0 (f32) / 1 (bf16) / 2 (f16) of a dtype or name; None means f32.  ValueError for anything else."""
    if dtype is None:
        return 0
    try:
        return PRECISIONS[dtype]
    except (KeyError, TypeError):
        raise ValueError(f"dtype must be torch.float32 / bfloat16 / float16 or 'f32' / 'bf16' / 'f16', got {dtype!r}") from None


def transform_shape(bert_name_or_path):
    """The reference's rule; raises ValueError for a name it would `assert False` on."""
    for key, shape in TRANSFORM_SHAPES:
        if key in str(bert_name_or_path):
            return shape
    raise ValueError(f"unsupport model {bert_name_or_path!r}: the reference knows "
                     f"{[k for k, _ in TRANSFORM_SHAPES]} (pass transform_heads= and transform_ff= for another BERT)")


def frontend_config(num_polyphones, num_prosody, bert_config, transform_heads=None, transform_ff=None,
                    bert_name_or_path=None):
    """The config dict of wetts_frontend_config_t from an HF BERT `config.json` (dict or path)."""
    if isinstance(bert_config, (str, os.PathLike)):
        with open(bert_config, encoding="utf-8") as f:
            bert_config = json.load(f)
    bc = dict(bert_config)
    if bc.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"hidden_act = {bc['hidden_act']!r} is not supported (only \"gelu\", the exact erf form)")
    if bc.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"position_embedding_type = {bc['position_embedding_type']!r} is not supported (only \"absolute\")")
    for k in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size",
              "max_position_embeddings"):
        if k not in bc:
            raise ValueError(f"bert_config has no {k!r}")
    d = int(bc["hidden_size"])
    if transform_heads is None or transform_ff is None:
        name = bert_name_or_path if bert_name_or_path is not None else bc.get("_name_or_path", "")
        dm, nh, ff = transform_shape(name)
        if dm != d:
            raise ValueError(f"{name!r} selects a transform of d_model {dm}, but hidden_size is {d}")
        transform_heads = nh if transform_heads is None else transform_heads
        transform_ff = ff if transform_ff is None else transform_ff
    return dict(vocab_size=int(bc["vocab_size"]), hidden_size=d, num_layers=int(bc["num_hidden_layers"]),
                num_heads=int(bc["num_attention_heads"]), intermediate_size=int(bc["intermediate_size"]),
                max_position_embeddings=int(bc["max_position_embeddings"]), type_vocab_size=int(bc.get("type_vocab_size", 2)),
                layer_norm_eps=float(bc.get("layer_norm_eps", 1e-12)), transform_heads=int(transform_heads),
                transform_ff=int(transform_ff), num_polyphones=int(num_polyphones), num_prosody=int(num_prosody))


class FrontendModel:
    """frontend/model.py's FrontendModel as an evaluation module on the device.  `bert_config`: an HF config.json (dict
    or path); `transform`'s heads and feed-forward width follow the reference's rule on bert_config["_name_or_path"] (or
    `bert_name_or_path=`) unless given."""

    def __init__(self, num_polyphones, num_prosody, bert_config, transform_heads=None, transform_ff=None,
                 bert_name_or_path=None):
        self.config = frontend_config(num_polyphones, num_prosody, bert_config, transform_heads, transform_ff,
                                      bert_name_or_path)
        checkpoint.frontend_layout(self.config)  # raises ValueError for a shape the kernels do not cover: no slow path
        self.num_polyphones, self.num_prosody = self.config["num_polyphones"], self.config["num_prosody"]
        self.training = False
        self._blob = None
        self._handle = None
        self._device = None
        self._status = None
        self._precision = 0
        self._stale = False  # the device weights are newer than _blob (FrontendTrainer.step sets it)

    # ---- nn.Module-like surface ----
    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("the frontend is evaluation only (no gradients)")
        return self

    def load_state_dict(self, state_dict, strict=True):
        """What frontend/train.py:215 saves.  Every tensor the model reads must be present with its shape; the pooler
        and position_ids are ignored."""
        self._blob = checkpoint.pack_frontend_blob(self.config, state_dict)
        self._stale = False
        if self._device is not None:
            self._create()
        return self

    def state_dict(self):
        """The tensors the model uses, reference-keyed (after FrontendTrainer.step: the trained ones, read back here)."""
        self._require_blob()
        self._sync_blob()
        return {name: self._blob[off:off + numel].reshape(shape).clone()
                for name, off, numel, shape in checkpoint.frontend_layout(self.config)}

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("FrontendModel runs on a HIP device only (there is no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._device = device
        if self._blob is not None:
            self._create()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))

    def set_dtype(self, dtype):
        """The operands of the Linears of the BERT layers and of `transform`: torch.float32 (the default), torch.bfloat16
        or torch.float16 (or "f32" / "bf16" / "f16"): both operands rounded to the type, exact products, f32
        accumulation and f32 epilogues; embeddings, LayerNorms, attention, classifiers, softmaxes, decisions and scoring
        stay f32.  May be called before or after .to(device); on a device it packs the 16-bit weight copies (a set-up
        call: it allocates and drains), float32 frees them.  bfloat16 is the recommended type."""
        prec = frontend_precision(dtype)
        if self._handle is not None:
            with torch.cuda.device(self._device):
                _lib.check(_lib.load().wetts_frontend_set_precision(self._handle, prec), "frontend_set_precision")
        self._precision = prec
        return self

    @property
    def dtype(self):
        return (torch.float32, torch.bfloat16, torch.float16)[self._precision]

    @property
    def device(self):
        return self._device

    def _require_blob(self):
        if self._blob is None:
            raise RuntimeError("no weights: call load_state_dict() first")

    def _sync_blob(self):
        """Brings the trainable tail of _blob up to date with the device after training (one copy)."""
        if not self._stale or self._handle is None:
            return
        lib = _lib.load()
        off, num = C.c_int64(), C.c_int64()
        cfg = checkpoint.frontend_c_config(self.config)
        _lib.check(lib.wetts_frontend_trainable_span(C.byref(cfg), C.byref(off), C.byref(num)), "frontend_trainable_span")
        with torch.cuda.device(self._device):
            dev = torch.empty(num.value, dtype=torch.float32, device=self._device)
            _lib.check(lib.wetts_frontend_read_weights(self._handle, off.value, num.value, _lib.ptr(dev),
                                                       _lib.current_stream_ptr()), "frontend_read_weights")
            self._blob[off.value:off.value + num.value] = dev.cpu()
        self._stale = False

    def _create(self):
        self._sync_blob()
        self._destroy()
        lib = _lib.load()
        with torch.cuda.device(self._device):
            dev = self._blob.to(self._device)
            h = C.c_void_p()
            cfg = checkpoint.frontend_c_config(self.config)
            _lib.check(lib.wetts_frontend_create(C.byref(cfg), _lib.ptr(dev), dev.numel(), _lib.current_stream_ptr(),
                                                 C.byref(h)), "frontend_create")
            self._status = torch.zeros(1, dtype=torch.int32, device=self._device)
            self._handle = h
            if self._precision:
                _lib.check(lib.wetts_frontend_set_precision(h, self._precision), "frontend_set_precision")

    def _destroy(self):
        if self._handle is not None:
            _lib.load().wetts_frontend_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _require(self):
        self._require_blob()
        if self._handle is None:
            raise RuntimeError("the frontend is not on a device: call .to('cuda') / .cuda() first")

    # ---- forward ----
    def _inputs(self, ids, token_type_ids, attention_mask):
        """-> (ids, token types or None, mask or None) as contiguous int64 tensors on the model's device; host checks."""
        self._require()
        ids = torch.as_tensor(ids)
        if ids.dim() != 2 or ids.dtype in (torch.float16, torch.float32, torch.float64, torch.bfloat16):
            raise ValueError(f"input_ids must be an integer [B, T] tensor, got {ids.dtype} {tuple(ids.shape)}")
        B, T = ids.shape
        if B < 1 or T < 1:
            raise ValueError(f"input_ids {tuple(ids.shape)}: B and T must be at least 1")
        if T > self.config["max_position_embeddings"]:
            raise ValueError(f"T = {T} exceeds the {self.config['max_position_embeddings']} positions of the table")
        out = []
        for t, n in ((ids, "input_ids"), (token_type_ids, "token_type_ids"), (attention_mask, "attention_mask")):
            if t is None:
                out.append(None)
                continue
            t = torch.as_tensor(t)
            if tuple(t.shape) != (B, T):
                raise ValueError(f"{n} must be [{B}, {T}], got {tuple(t.shape)}")
            out.append(t.to(device=self._device, dtype=torch.int64).contiguous())
        return out

    def _raise_status(self, bits):
        if bits & _lib.STATUS_TOKEN_ID_RANGE:
            raise IndexError("index out of range in self: a token id is outside [0, vocab_size)")
        if bits & _lib.STATUS_TYPE_ID_RANGE:
            raise IndexError("index out of range in self: a token type id is outside [0, type_vocab_size)")

    def _launch(self, ids, tt, mask, softmax):
        """One forward pass; no read-back.  -> (phone [B, T, P], prosody [B, T, R]) device tensors; the status word is
        left for the caller (forward() reads it; Frontend reads it with the decisions)."""
        B, T = ids.shape
        lib = _lib.load()
        nbytes = int(lib.wetts_frontend_workspace_bytes(self._handle, B, T))
        if nbytes < 0:
            raise _lib.WettsError(f"frontend_workspace_bytes: {_lib.last_error()}")
        with torch.cuda.device(self._device):
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self._device)
            phone = torch.empty(B, T, self.num_polyphones, dtype=torch.float32, device=self._device)
            pros = torch.empty(B, T, self.num_prosody, dtype=torch.float32, device=self._device)
            self._status.zero_()
            _lib.check(lib.wetts_frontend_forward(self._handle, _lib.ptr(ids), _lib.ptr(tt), _lib.ptr(mask), B, T,
                                                  1 if softmax else 0, _lib.ptr(phone), _lib.ptr(pros), _lib.ptr(ws),
                                                  _lib.ptr(self._status), _lib.current_stream_ptr()), "frontend_forward")
        return phone, pros

    def _run(self, ids, token_type_ids, attention_mask, softmax):
        ids, tt, mask = self._inputs(ids, token_type_ids, attention_mask)
        phone, pros = self._launch(ids, tt, mask, softmax)
        self._raise_status(int(self._status.item()))  # the one read-back of the call
        return phone, pros

    def forward(self, x):
        """frontend/model.py:52-63 -> (phone_logits [B, T, P], prosody_logits [B, T, R]); x["token_type_ids"] (zeros)
        and x["attention_mask"] (ones) are optional."""
        return self._run(x["input_ids"], x.get("token_type_ids"), x.get("attention_mask"), False)

    __call__ = forward

    def export_forward(self, x):
        """frontend/model.py:65-73: [1, T] ids -> the two softmaxes."""
        assert x.shape[0] == 1
        return self._run(x, None, None, True)

    def probs(self, ids, attention_mask=None):
        """export_forward for a padded batch: [B, T] ids and mask -> the two softmaxes (zeros at padded tokens)."""
        return self._run(ids, None, attention_mask, True)

    def decide(self, ids, attention_mask, cand, cand_len):
        """One forward pass and cli/frontend.py:70-81's decisions on the device, ONE read-back: cand [B, T, max_cand]
        int32 class ids and cand_len [B, T] -> (choice [B, T], prosody [B, T]) as numpy int32: the index of the first
        candidate of the largest probability, and the lowest prosody class of the largest probability."""
        ids, _, mask = self._inputs(ids, None, attention_mask)
        B, T = ids.shape
        cand = torch.as_tensor(cand, dtype=torch.int32)
        if cand.dim() != 3 or tuple(cand.shape[:2]) != (B, T) or cand.shape[2] < 1:
            raise ValueError(f"cand must be [{B}, {T}, max_cand], got {tuple(cand.shape)}")
        cand_len = torch.as_tensor(cand_len, dtype=torch.int32)
        if tuple(cand_len.shape) != (B, T):
            raise ValueError(f"cand_len must be [{B}, {T}], got {tuple(cand_len.shape)}")
        cand, cand_len = cand.to(self._device).contiguous(), cand_len.to(self._device).contiguous()
        phone, pros = self._launch(ids, None, mask, True)
        out = torch.empty(2 * B * T + 1, dtype=torch.int32, device=self._device)
        with torch.cuda.device(self._device):
            _lib.check(_lib.load().wetts_frontend_decide(_lib.ptr(phone), _lib.ptr(pros), _lib.ptr(cand), _lib.ptr(cand_len),
                                                         B * T, self.num_polyphones, self.num_prosody, cand.shape[2],
                                                         _lib.ptr(out[:B * T]), _lib.ptr(out[B * T:2 * B * T]),
                                                         _lib.current_stream_ptr()), "frontend_decide")
            out[2 * B * T:] = self._status
        host = out.cpu().numpy()
        self._raise_status(int(host[-1]))
        return host[:B * T].reshape(B, T), host[B * T:2 * B * T].reshape(B, T)

    def _labels(self, labels, name, B, T):
        if labels is None:
            return None
        labels = torch.as_tensor(labels)
        if tuple(labels.shape) != (B, T) or labels.is_floating_point() or labels.dtype == torch.bool:
            raise ValueError(f"{name} must be an integer [{B}, {T}] tensor, got {labels.dtype} {tuple(labels.shape)}")
        return labels.to(device=self._device, dtype=torch.int64).contiguous()

    def score(self, inputs, phone_labels=None, prosody_labels=None, *, polyphone_weight=0.5):
        """The validation pass of frontend/train.py:63-84 and the counts of test_polyphone.py:76-82 and
        test_prosody.py:81-100 in one call on the device, without logits: `inputs` as forward() takes it, labels int
        [B, T] with IGNORE_ID = -100 (None: all ignored) -> FrontendScores of device tensors.  No read-back here; the
        status word (a label outside its classes, a label at a padded token) is raised by FrontendScores.host()."""
        ids, tt, mask = self._inputs(inputs["input_ids"], inputs.get("token_type_ids"), inputs.get("attention_mask"))
        B, T = ids.shape
        pl, rl = self._labels(phone_labels, "phone_labels", B, T), self._labels(prosody_labels, "prosody_labels", B, T)
        w = float(polyphone_weight)
        lib = _lib.load()
        nbytes = int(lib.wetts_frontend_score_workspace_bytes(self._handle, B, T))
        if nbytes < 0:
            raise _lib.WettsError(f"frontend_score_workspace_bytes: {_lib.last_error()}")
        with torch.cuda.device(self._device):
            ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self._device)
            nll = torch.empty(2, B, T, dtype=torch.float32, device=self._device)
            pred = torch.empty(2, B, T, dtype=torch.int32, device=self._device)
            losses = torch.empty(2, dtype=torch.float32, device=self._device)
            counts = torch.empty(22, dtype=torch.int64, device=self._device)
            status = torch.zeros(1, dtype=torch.int32, device=self._device)
            _lib.check(lib.wetts_frontend_score(self._handle, _lib.ptr(ids), _lib.ptr(tt), _lib.ptr(mask), _lib.ptr(pl),
                                                _lib.ptr(rl), B, T, _lib.ptr(nll[0]), _lib.ptr(nll[1]), _lib.ptr(pred[0]),
                                                _lib.ptr(pred[1]), _lib.ptr(losses), _lib.ptr(counts), _lib.ptr(ws), nbytes,
                                                _lib.ptr(status), _lib.current_stream_ptr()), "frontend_score")
        return FrontendScores(losses, counts, nll, pred, status, w)


def compute_accuracy(counts, head):
    """train.py:31-40 on accumulated counts (a sequence of 22 numbers, or FrontendScores.counts read back):
    correct / total of `head` ("phone" / "polyphone" or "prosody"); NaN for a head without labels."""
    if head not in ("phone", "polyphone", "prosody"):
        raise ValueError(f"head must be 'phone', 'polyphone' or 'prosody', got {head!r}")
    o = 2 if head == "prosody" else 0
    total, correct = int(counts[o]), int(counts[o + 1])
    return float(correct) / float(total) if total > 0 else float("nan")


def prosody_f1(counts, exclude_end=False):
    """test_prosody.py:95-100 on accumulated counts -> (pw, pph, iph) f1 scores, 2 TP / (2 TP + FP + FN); an empty
    denominator gives 0.0, which is what sklearn.metrics.f1_score returns there."""
    if len(counts) != 22:
        raise ValueError(f"counts must hold 22 numbers, got {len(counts)}")
    o = 13 if exclude_end else 4
    out = []
    for th in range(3):
        tp, fp, fn = (int(counts[o + 3 * th + i]) for i in range(3))
        den = 2 * tp + fp + fn
        out.append(2 * tp / den if den else 0.0)
    return tuple(out)


class FrontendScores:
    """What FrontendModel.score() returns, all on the device: phone_loss, prosody_loss, loss (0-dim f32; NaN for a head
    without labels, and then for `loss`, as in the reference), counts int64 [22] (include/wetts_hip.h), and per token
    nll_phone, nll_prosody f32 [B, T] (0 where the label is ignored), pred_phone, pred_prosody int32 [B, T] (-1 at a
    padded token).  host() reads everything it reports back in ONE copy."""

    def __init__(self, losses, counts, nll, pred, status, polyphone_weight):
        self.phone_loss, self.prosody_loss = losses[0], losses[1]
        self.polyphone_weight = polyphone_weight
        self.counts = counts
        self.nll_phone, self.nll_prosody = nll[0], nll[1]
        self.pred_phone, self.pred_prosody = pred[0], pred[1]
        self._losses, self._status = losses, status

    @property
    def loss(self):
        """train.py:83-84 on the two device scalars, in f32 as the reference forms it.  Formed when asked for: like
        packed(), bookkeeping on a handful of numbers AFTER the kernels (as decide() appends its status word), not
        arithmetic on activations."""
        w = self.polyphone_weight
        return w * self.phone_loss + (1 - w) * self.prosody_loss

    def packed(self):
        """The int64 device vector host() reads back: the 22 counts, the bits of the two f32 losses, the status word
        (a 25-element copy after the kernels, as decide() packs its status word: no arithmetic)."""
        return torch.cat([self.counts, self._losses.view(torch.int32).to(torch.int64), self._status.to(torch.int64)])

    def host(self):
        """-> HostScores of Python numbers; raises IndexError for a label outside its classes (torch: `Target .. is out
        of bounds`) and ValueError for a label at a padded token."""
        return HostScores.from_packed(self.packed().cpu(), self.polyphone_weight)


def raise_score_status(bits):
    """The WETTS_STATUS_* bits of a scoring call as the exceptions torch / this project raise."""
    if bits & (_lib.STATUS_TOKEN_ID_RANGE | _lib.STATUS_TYPE_ID_RANGE):
        raise IndexError("index out of range in self: a token or token type id is outside its table")
    if bits & _lib.STATUS_LABEL_RANGE:
        raise IndexError("Target is out of bounds: a label is neither IGNORE_ID (-100) nor a class of its head")
    if bits & _lib.STATUS_LABEL_AT_PAD:
        raise ValueError("a label other than IGNORE_ID (-100) sits at a token whose attention_mask is 0")


class HostScores:
    """FrontendScores on the host: phone_loss, prosody_loss, loss, phone_acc, prosody_acc (NaN for an empty head, as
    compute_accuracy returns), num_total / num_correct (the polyphone head's, test_polyphone.py:72-73), counts (a list of
    22 ints) and f1(exclude_end=False) -> (pw, pph, iph)."""

    @classmethod
    def from_packed(cls, row, polyphone_weight=0.5):
        """From one read-back row of FrontendScores.packed(); raises what the status word asks for."""
        row = torch.as_tensor(row, dtype=torch.int64).cpu()
        raise_score_status(int(row[24]))
        pl, rl = row[22:24].to(torch.int32).view(torch.float32).numpy()
        # train.py:83-84: `1 - w` is formed in double and rounded once, each product and the sum in f32
        w = float(polyphone_weight)
        return cls((pl, rl, np.float32(w) * pl + np.float32(1 - w) * rl), row[:22].tolist())

    def __init__(self, losses, counts):
        self.phone_loss, self.prosody_loss, self.loss = (float(v) for v in losses)
        self.counts = [int(v) for v in counts]
        self.phone_acc, self.prosody_acc = compute_accuracy(self.counts, "phone"), compute_accuracy(self.counts, "prosody")
        self.num_total, self.num_correct = self.counts[0], self.counts[1]

    def f1(self, exclude_end=False):
        return prosody_f1(self.counts, exclude_end)


def load_frontend_model(model_dir, device="cuda", dtype=None):
    """FrontendModel from `final.pt` (frontend/train.py:215's state_dict) and `config.json` (the BERT's HF config) in
    model_dir.  The classifier widths are read from the checkpoint.  `dtype`: FrontendModel.set_dtype's argument
    (None: float32)."""
    sd = torch.load(os.path.join(model_dir, "final.pt"), map_location="cpu", weights_only=True)
    for k in ("phone_classifier.weight", "prosody_classifier.weight"):
        if k not in sd:
            raise KeyError(f"{k} missing from {os.path.join(model_dir, 'final.pt')}")
    model = FrontendModel(sd["phone_classifier.weight"].shape[0], sd["prosody_classifier.weight"].shape[0],
                          os.path.join(model_dir, "config.json"))
    return model.set_dtype(dtype if dtype is not None else torch.float32).load_state_dict(sd).to(device)


class _Arg:
    def __init__(self, name, shape, type_):
        self.name, self.shape, self.type = name, shape, type_


class FrontendSession:
    """onnxruntime-shaped session of the frontend's exported graph (export_onnx.py:72-91): input `input` [1, T] int64,
    outputs `polyphone_output` [1, T, P] and `prosody_output` [1, T, R], the two softmaxes of export_forward."""

    def __init__(self, model_or_dir, device="cuda", dtype=None):
        """`dtype`: FrontendModel.set_dtype's argument; None leaves a given model as it is (float32 for a directory)."""
        if isinstance(model_or_dir, FrontendModel):
            self.model = model_or_dir if dtype is None else model_or_dir.set_dtype(dtype)
        else:
            self.model = load_frontend_model(model_or_dir, device, dtype)
        self.model._require()

    def get_inputs(self):
        return [_Arg("input", [1, "T"], "tensor(int64)")]

    def get_outputs(self):
        return [_Arg("polyphone_output", [1, "T", self.model.num_polyphones], "tensor(float)"),
                _Arg("prosody_output", [1, "T", self.model.num_prosody], "tensor(float)")]

    def run(self, output_names, feeds, run_options=None):
        names = [o.name for o in self.get_outputs()]
        if output_names is not None and any(n not in names for n in output_names):
            raise ValueError(f"unknown output among {output_names}: the graph has {names}")
        ids = torch.as_tensor(np.asarray(feeds["input"]), dtype=torch.int64)
        outs = dict(zip(names, (t.cpu().numpy() for t in self.model.export_forward(ids))))
        return [outs[n] for n in (names if output_names is None else output_names)]


def host_decisions(pinyin_prob, prosody_prob, cands):
    """cli/frontend.py:70-81 on host arrays, literally: pinyin_prob [T, P], prosody_prob [T, R], cands[i] the class ids of
    token i's candidates -> ([index of the chosen candidate per token], [prosody class per token])."""
    choice = []
    for i, arr in enumerate(cands):
        if len(arr) > 1:
            poly_probs = [pinyin_prob[i][c] for c in arr]
            choice.append(poly_probs.index(max(poly_probs)))
        else:
            choice.append(0)
    return choice, np.asarray(prosody_prob).argmax(axis=1).tolist()


class Frontend:
    """cli/frontend.py's Frontend: the same table readers, the same compute(text).  model_dir holds `final.pt` and
    `config.json` (nothing here reads `final.onnx`), `vocab.txt` and `lexicon/{polyphone.txt, pinyin_dict.txt,
    lexicon.txt}`.  `session=`: any object with the exported graph's run() (then the decisions are the reference's host
    code on its outputs); by default the model runs on the device and the decisions are made there too.  `dtype`:
    FrontendModel.set_dtype's argument for that model (None: float32); a given session keeps its own."""

    def __init__(self, model_dir, session=None, device="cuda", dtype=None):
        frontend_precision(dtype)  # (a bad dtype is refused before anything is read)
        self.token2id = self.read_list(os.path.join(model_dir, "vocab.txt"))
        self.polyphone2id = self.read_list(os.path.join(model_dir, "lexicon", "polyphone.txt"))
        self.id2polyphone = {v: k for k, v in self.polyphone2id.items()}
        self.char2pinyins = self.read_char2pinyins(os.path.join(model_dir, "lexicon", "pinyin_dict.txt"))
        self.pinyin2phones = self.read_pinyin2phones(os.path.join(model_dir, "lexicon", "lexicon.txt"))
        self.model = None
        if session is None:
            self.model = load_frontend_model(model_dir, device, dtype)
            if self.model.num_polyphones != len(self.polyphone2id):
                raise ValueError(f"final.pt classifies {self.model.num_polyphones} polyphones, polyphone.txt lists "
                                 f"{len(self.polyphone2id)}")
            session = FrontendSession(self.model)
        self.session = session

    def read_list(self, fname):
        table = {}
        with open(fname, encoding="utf-8") as fin:
            for i, line in enumerate(fin):
                table[line.strip()] = i
        return table

    def read_char2pinyins(self, fname):
        table = {}
        with open(fname, encoding="utf-8") as fin:
            for line in fin:
                arr = line.split()
                assert len(arr) == 2
                table[arr[0]] = arr[1].split(",")
        return table

    def read_pinyin2phones(self, fname):
        table = {}
        with open(fname, encoding="utf-8") as fin:
            for line in fin:
                arr = line.split()
                assert len(arr) >= 2
                table[arr[0]] = arr[1:]
        return table

    def _tokens(self, text):
        """-> (token ids, per token the candidate pinyins ([] for [CLS] / [SEP])); KeyError like the reference."""
        tokens = ["[CLS]"] + [str(x) for x in text] + ["[SEP]"]
        ids = [self.token2id[x] for x in tokens]
        return ids, [[]] + [self.char2pinyins[x] for x in tokens[1:-1]] + [[]]

    def _phonemes(self, arrs, choice, prosodys):
        """cli/frontend.py:82-86 from the decisions of one text (all tokens, [CLS] and [SEP] included)."""
        outputs = ["sil"]
        for i in range(1, len(arrs) - 1):
            outputs.extend(self.pinyin2phones[arrs[i][choice[i]]])
            outputs.append("#{}".format(prosodys[i - 1]))  # the reference indexes the prosody from [CLS]'s row
        outputs[-1] = "#4"
        return outputs

    def compute(self, text):
        if self.model is not None:
            return self.compute_batch([text])[0]
        ids, arrs = self._tokens(text)
        outputs = self.session.run(None, {"input": np.expand_dims(np.array(ids), axis=0)})
        cands = [[self.polyphone2id[p] for p in a] if len(a) > 1 else [] for a in arrs]
        choice, prosodys = host_decisions(outputs[0][0], outputs[1][0], cands)
        return self._phonemes(arrs, choice, prosodys)

    def compute_batch(self, texts):
        """compute() of every text; with the device model: one padded forward pass, the decisions on the device and one
        read-back for the whole list."""
        texts = list(texts)
        if self.model is None or not texts:
            return [self.compute(t) for t in texts]
        toks = [self._tokens(t) for t in texts]
        B, T = len(toks), max(len(ids) for ids, _ in toks)
        K = max([len(a) for _, arrs in toks for a in arrs] + [1])
        ids = np.zeros((B, T), np.int64)
        mask = np.zeros((B, T), np.int64)
        cand = np.full((B, T, K), -1, np.int32)
        clen = np.zeros((B, T), np.int32)
        for b, (tid, arrs) in enumerate(toks):
            ids[b, :len(tid)] = tid
            mask[b, :len(tid)] = 1
            for i, a in enumerate(arrs):
                if len(a) > 1:
                    cand[b, i, :len(a)] = [self.polyphone2id[p] for p in a]
                    clen[b, i] = len(a)
        choice, pros = self.model.decide(ids, mask, cand, clen)
        return [self._phonemes(arrs, choice[b].tolist(), pros[b].tolist()) for b, (_, arrs) in enumerate(toks)]


class Model:
    """cli/model.py's Model on existing parts: `backend_session` an InferenceSession (session.py) of the acoustic model,
    `phone_table` / `speaker_table` dicts or `symbol id` files, `frontend` a Frontend.  No hub download."""

    def __init__(self, backend_session, phone_table, speaker_table, frontend):
        self.frontend = frontend
        self.session = backend_session
        self.phone2id = self.read_table(phone_table) if isinstance(phone_table, (str, os.PathLike)) else dict(phone_table)
        self.speaker2id = self.read_table(speaker_table) if isinstance(speaker_table, (str, os.PathLike)) \
            else dict(speaker_table)

    def read_table(self, fname):
        table = {}
        with open(fname, encoding="utf-8") as fin:
            for line in fin:
                arr = line.split()
                assert len(arr) == 2
                table[arr[0]] = int(arr[1])
        return table

    def synthesis(self, text, speaker="default"):
        """cli/model.py:43-61 -> (phonemes, int16 audio)."""
        phonemes = self.frontend.compute(text)
        phonemes_id = [self.phone2id[x] for x in phonemes]
        scales = [0.667, 1.0, 0.8]
        sid = self.speaker2id.get(speaker, 0)
        outputs = self.session.run(None, {
            "input": np.expand_dims(np.array(phonemes_id), axis=0),
            "input_lengths": np.array([len(phonemes)]),
            "scales": np.expand_dims(np.array(scales, dtype=np.float32), axis=0),
            "sid": np.array([sid]),
        })
        audio = outputs[0][0][0]
        audio = (audio * 32767).astype(np.int16)
        return phonemes, audio
