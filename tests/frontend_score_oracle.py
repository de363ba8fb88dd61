"""Float64 restatement of the frontend's scoring on top of frontend_oracle.forward: the validation pass of
frontend/train.py:43-94 (F.cross_entropy with ignore_index, compute_accuracy, the weighted sum), the masked accuracy counts
of frontend/test_polyphone.py:72-86 and the slicing and binarisation of frontend/test_prosody.py:77-102, with the cases,
the seeded labels and the injected defects.  Plain torch; no `transformers`, no sklearn.

`score` works on the transform layer's output x (what wetts_frontend_score_heads receives), so that a defect in the
classifier itself (a dropped bias, a lost class tile) can be injected.  Counts follow include/wetts_hip.h:
[0..1] phone total / correct, [2..3] prosody total / correct, [4..12] TP, FP, FN at > 0, > 1, > 2 over the positions
1 .. len_b, [13..21] the same with exclude_end."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import frontend_oracle as fo

IGNORE_ID = -100
CLASS_COUNTS = ((34, 5), (470, 5))  # fo.weights' own sizes; the reference lexicon's (14 full class tiles and one of 22)
# N = 3 (one token tile almost empty); padded tokens; N = 99 and N = 195 leave the 64-token tiles ragged
SHAPES = ((3,), (9, 6), (33, 32, 31), (65, 64, 63))
CASES = tuple((c, P, lens) for c in fo.CONFIGS for P, _ in CLASS_COUNTS for lens in SHAPES)
TILE = 32  # classes per tile of fe_score_tile_kernel

FAULTS = ("mean_over_all_tokens", "label_off_by_one", "no_bias", "lost_ragged_tile", "pad_class_in_sum", "f1_end_off_by_one",
          "exclude_end_swapped", "argmax_highest_on_tie")


def config(cname, P):
    return dict(fo.config(cname), num_polyphones=int(P))


_W = {}


def weights(cname, P):
    """(float32 state_dict, float64 state_dict); P = 34 is fo.weights itself."""
    if P == fo.NUM_POLYPHONES:
        return fo.weights(cname)
    if (cname, P) not in _W:
        from wetts_amd import synth
        sd = synth.make_frontend_state_dict(config(cname, P), fo.WSEED)
        _W[(cname, P)] = (sd, {k: v.to(torch.float64) for k, v in sd.items() if v.is_floating_point()})
    return _W[(cname, P)]


def case_name(cname, P, lens):
    return f"frontend_score_{cname}_p{P}_b{len(lens)}x{max(lens)}"


def case_seed(P, lens):
    return 9000 + 100 * len(lens) + max(lens) + (0 if P == fo.NUM_POLYPHONES else 50000)


def make_labels(lens, seed, pred_phone, pred_prosody, P, R):
    """Seeded labels [B, T] int64: even rows are prosody rows (every character labelled in [0, R)), odd rows polyphone
    rows (each character labelled with probability 0.3); a single-row batch carries both kinds.  A label is the given
    prediction (the float64 oracle's argmax) with probability 1/2 and uniform otherwise.  [CLS], [SEP], padding: -100."""
    g = torch.Generator().manual_seed(int(seed) + 77)
    B, T = len(lens), max(lens)
    pl = torch.full((B, T), IGNORE_ID, dtype=torch.int64)
    rl = torch.full((B, T), IGNORE_ID, dtype=torch.int64)
    for b, n in enumerate(lens):
        chars = n - 2
        for lab, pred, M, prob, mine in ((rl, pred_prosody, R, 1.0, b % 2 == 0 or B == 1),
                                         (pl, pred_phone, P, 0.3, b % 2 == 1 or B == 1)):
            take = torch.rand(chars, generator=g) < prob
            own = torch.rand(chars, generator=g) < 0.5
            rnd = torch.randint(0, M, (chars,), generator=g)
            if mine:
                v = torch.where(own, pred[b, 1:n - 1].to(torch.int64), rnd)
                lab[b, 1:n - 1] = torch.where(take, v, torch.full_like(v, IGNORE_ID))
    return pl, rl


def logits(W, x, fault=None):
    nb = fault == "no_bias"
    return (F.linear(x, W["phone_classifier.weight"], None if nb else W["phone_classifier.bias"]),
            F.linear(x, W["prosody_classifier.weight"], None if nb else W["prosody_classifier.bias"]))


def head(z, mask, labels, fault=None):
    """One head.  z [B, T, M], labels [B, T] or None -> (nll [B, T], pred [B, T] int64, loss, total, correct)."""
    M = z.shape[-1]
    on = mask != 0
    labels = torch.full(mask.shape, IGNORE_ID, dtype=torch.int64) if labels is None else labels
    idx = torch.arange(M).expand(z.shape)
    mx = z.max(-1, keepdim=True).values
    if fault == "argmax_highest_on_tie":
        pred = torch.where(z == mx, idx, torch.full_like(idx, -1)).max(-1).values
    else:
        pred = torch.where(z == mx, idx, torch.full_like(idx, M)).min(-1).values  # the lowest index of the maximum
    e = torch.exp(z - mx)
    if fault == "lost_ragged_tile" and M > TILE:
        e = e[..., :TILE * ((M - 1) // TILE)]
    s = e.sum(-1)
    if fault == "pad_class_in_sum":
        s = s + (TILE * math.ceil(M / TILE) - M) * torch.exp(z[..., M - 1] - mx[..., 0])
    lse = mx[..., 0] + torch.log(s)
    scored = on & (labels >= 0) & (labels < M)
    lab = labels.clamp(0, M - 1)
    if fault == "label_off_by_one":
        lab = (lab + 1) % M
    nll = torch.where(scored, lse - z.gather(-1, lab.unsqueeze(-1))[..., 0], torch.zeros_like(lse))
    pred = torch.where(on, pred, torch.full_like(pred, -1))
    total = int(scored.sum())
    correct = int((scored & (pred == lab)).sum())
    den = mask.numel() if fault == "mean_over_all_tokens" else total
    loss = nll.sum() / torch.tensor(float(den), dtype=nll.dtype)  # 0 / 0 = NaN, as F.cross_entropy without a target
    return nll, pred, loss, total, correct


def f1_counts(pred, labels, exclude_end, fault=None):
    """test_prosody.py:83-100 literally, up to sklearn: the lists `pred` and `label` grown row by row, then TP, FP, FN of
    the three binarisations."""
    if fault == "exclude_end_swapped":
        exclude_end = not exclude_end
    plist, llist = [], []
    lengths = torch.sum(labels != IGNORE_ID, dim=1)
    for i in range(pred.shape[0]):
        n = int(lengths[i]) - (1 if fault == "f1_end_off_by_one" else 0)
        if exclude_end:
            plist.extend(pred[i][1:max(n, 0)].tolist())
            llist.extend(labels[i][1:max(n, 0)].tolist())
        else:
            plist.extend(pred[i][1:max(n + 1, 0)].tolist())
            llist.extend(labels[i][1:max(n + 1, 0)].tolist())
    out = []
    for th in (0, 1, 2):
        y = [1 if x > th else 0 for x in llist]
        p = [1 if x > th else 0 for x in plist]
        out += [sum(a and b for a, b in zip(y, p)), sum((not a) and b for a, b in zip(y, p)),
                sum(a and (not b) for a, b in zip(y, p))]
    return out


def score(W, x, mask, phone_labels, prosody_labels, fault=None):
    """-> dict(nll_phone, nll_prosody [B, T] at W's dtype, pred_phone, pred_prosody [B, T] int64 (-1 at padded tokens),
    losses [2], counts int64 [22])."""
    zp, zr = logits(W, x, fault)
    np_, pp, lp, tp, cp = head(zp, mask, phone_labels, fault)
    nr, pr, lr, tr, cr = head(zr, mask, prosody_labels, fault)
    rl = torch.full(mask.shape, IGNORE_ID, dtype=torch.int64) if prosody_labels is None else prosody_labels
    counts = [tp, cp, tr, cr] + f1_counts(pr, rl, False, fault) + f1_counts(pr, rl, True, fault)
    return dict(nll_phone=np_, nll_prosody=nr, pred_phone=pp, pred_prosody=pr, losses=torch.stack([lp, lr]),
                counts=torch.tensor(counts, dtype=torch.int64))


def f1(counts, exclude_end=False):
    """(pw, pph, iph) = 2 TP / (2 TP + FP + FN); 0.0 for an empty denominator (sklearn's value)."""
    c = [int(v) for v in counts]
    o = 13 if exclude_end else 4
    out = []
    for th in range(3):
        tp, fp, fn = c[o + 3 * th:o + 3 * th + 3]
        out.append(2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
    return tuple(out)


def labelled(t, labels):
    """The values at the labelled tokens, [n_labelled]."""
    return t[labels != IGNORE_ID]


def load_fixture(cname, P, lens):
    return np.load(os.path.join(fo.GOLDEN, case_name(cname, P, lens) + ".npz"))


_REF = {}


def reference(cname, P, lens):
    """(ids, mask, phone labels, prosody labels, float64 x, float64 score dict) of a fixture case, computed once per
    process and left unchanged."""
    key = (cname, P, tuple(lens))
    if key not in _REF:
        c = load_fixture(cname, P, lens)
        ids, mask = fo.inputs(lens, int(c["input_seed"]))
        pl, rl = torch.from_numpy(c["phone_labels"].astype(np.int64)), torch.from_numpy(c["prosody_labels"].astype(np.int64))
        W64 = weights(cname, P)[1]
        x = fo.forward(W64, cname, ids, mask)["transform"]
        _REF[key] = (ids, mask, pl, rl, x, score(W64, x, mask, pl, rl))
    return _REF[key]


TIES = {"phone": (3, (7, 40)), "prosody": (1, (4,))}  # the class and its copies (40: another class tile, where P > 40)


def tie_weights(cname, P):
    """The float32 state_dict with classifier rows made EQUAL, so that logits tie exactly, and the tied class's bias raised
    so that it often is the maximum: phone classes 7 and (where P > 40) 40 copy class 3 (+4), prosody class 4 copies
    class 1 (+1).  The lowest index has to win every such tie."""
    sd = dict(weights(cname, P)[0])
    for name, (lo, his), boost in (("phone_classifier", TIES["phone"], 4.0), ("prosody_classifier", TIES["prosody"], 1.0)):
        w, b = sd[name + ".weight"].clone(), sd[name + ".bias"].clone()
        b[lo] += boost
        for hi in his:
            if hi < w.shape[0]:
                w[hi], b[hi] = w[lo], b[lo]
        sd[name + ".weight"], sd[name + ".bias"] = w, b
    return sd
