#!/usr/bin/env python3
"""Generates the frontend scoring fixtures by running the REAL reference: its FrontendModel (frontend/model.py) and its
FrontendDataset / collate_fn (frontend/dataset.py), both imported unmodified by path, and the scoring statements of its
three scripts, lifted out of their ASTs and executed as they are spelled (the scripts themselves parse arguments and load
tokenizers at import): the CV branch of frontend/train.py:71-84 with its compute_accuracy, the counting of
frontend/test_polyphone.py:77-82, and the slicing of frontend/test_prosody.py:82-93 with its three sklearn f1_score calls.
Run in the build container only:

    python tests/golden/make_golden_frontend_score.py

Written:
  tests/golden/frontend_score_{tiny,base}_p{34,470}_b{B}x{T}.npz  one per case of frontend_score_oracle.CASES: seeds and
      digests, the seeded labels, the reference's float32 per-token nll at the labelled tokens (F.cross_entropy with
      reduction="none" on the same permuted logits), its two losses and their weighted sum, the 22 counts (from the
      lifted statements; TP / FP / FN from the very lists the reference hands to sklearn), sklearn's six f1 scores, and
      the floors floor_nll_* / floor_loss_* / floor_logits_*: the reference's float32 against the float64 oracle, the
      worst over the config's cases, (rel RMS, max |d| / rms).
  tests/golden/frontend_data_kat.npz  what the reference's FrontendDataset + collate_fn give on
      tests/golden/frontend_toy/data/{polyphone,prosody}_cv.txt with a BertTokenizer on the toy vocab.txt (one batch per
      file), and the numbers and printed lines its three scripts' statements give there on the tiny (34, 5) checkpoint in
      batches of 8.

DECISION STABILITY is a condition of a fixture, as in make_golden_frontend.py: a case is written only if the argmax of
every valid token of both heads is the same under the float64 oracle, the reference's float32 and sixteen copies of the
oracle's logits with uniform noise of amplitude fixture_gate(floor_logits)[1] x rms(logits).  A case that fails moves to
another input seed (+1000); the seed used is recorded.  The labels follow the oracle's argmax with probability 1/2, so
`correct` is neither 0 nor `total`: asserted wherever a head has at least 8 labels."""
import ast
import contextlib
import hashlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests import frontend_oracle as fo  # noqa: E402
from tests import frontend_score_oracle as so  # noqa: E402
from tests.golden.make_golden_disc import state_dict_digest  # noqa: E402
from tests.golden.make_golden_frontend import _load, inputs_digest  # noqa: E402

REF_FRONT = os.path.join(ref_import.REF_ROOT, "wetts", "frontend")
EVAL_BATCH = 8  # the cv set is the polyphone lines, then the prosody lines: its second batch holds both kinds


def labels_digest(pl, rl):
    h = hashlib.sha256()
    for t in (pl, rl):
        h.update(t.to(torch.int64).contiguous().numpy().tobytes())
    return h.hexdigest()


def _tree(name):
    return ast.parse(open(os.path.join(REF_FRONT, name)).read())


def _fn(tree, name):
    return next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)


def _first(node, kind):
    return next(n for n in ast.walk(node) if isinstance(n, kind))


def _code(stmts, name):
    return compile(ast.Module(body=stmts, type_ignores=[]), name, "exec")


def _not_pbar(s):
    return "pbar" not in ast.unparse(s)


def lifted():
    """-> (compute_accuracy, cv_step, polyphone_step, prosody_step, prosody_scores): the reference's own statements."""
    tr = _tree("train.py")
    ns = {"torch": torch, "IGNORE_ID": so.IGNORE_ID}
    exec(_code([_fn(tr, "compute_accuracy")], "train.py"), ns)
    # train.py:70-84: the statements of the batch loop from the forward pass to the weighted sum
    body = _first(_fn(tr, "train_or_cv"), ast.For).body
    keep = [s for s in body if isinstance(s, ast.Assign) and "inputs[" not in ast.unparse(s.targets[0])
            and ".to(device)" not in ast.unparse(s)]
    assert [ast.unparse(s.targets[0]) for s in keep] == ["(phone_logits, prosody_logits)", "phone_loss", "phone_acc",
                                                         "prosody_loss", "prosody_acc", "loss"], [ast.unparse(s) for s in keep]
    cv = _code(keep, "train.py")
    # test_polyphone.py:77-82
    body = [s for s in _first(_fn(_tree("test_polyphone.py"), "main"), ast.For).body if _not_pbar(s)]
    assert len(body) == 6, [ast.unparse(s) for s in body]
    poly = _code(body, "test_polyphone.py")
    # test_prosody.py:82-93 (the batch loop) and :95-100 (the three f1_score calls)
    w = _first(_fn(_tree("test_prosody.py"), "main"), ast.With)
    loop = _first(w, ast.For)
    pbody = [s for s in loop.body if _not_pbar(s)]
    assert len(pbody) == 4, [ast.unparse(s) for s in pbody]
    f1s = [s for s in w.body if isinstance(s, ast.Assign) and "f1_score" in ast.unparse(s.value)]
    assert len(f1s) == 3
    return ns["compute_accuracy"], cv, poly, _code(pbody, "test_prosody.py"), _code(f1s, "test_prosody.py")


def reference_scores(net, L, inputs, pl, rl, w=0.5):
    """Everything the three scripts compute on one batch -> dict (tensors, lists)."""
    from sklearn.metrics import f1_score
    compute_accuracy, cv, poly, pros, pros_f1 = L
    base = {"torch": torch, "F": F, "IGNORE_ID": so.IGNORE_ID, "compute_accuracy": compute_accuracy, "model": net}
    with torch.no_grad():
        a = dict(base, inputs=inputs, phone_labels=pl, prosody_labels=rl, polyphone_weight=w)
        exec(cv, a)
        # the per-token terms of the same calls
        nll_p = F.cross_entropy(a["phone_logits"].permute(0, 2, 1), pl, ignore_index=so.IGNORE_ID, reduction="none")
        nll_r = F.cross_entropy(a["prosody_logits"].permute(0, 2, 1), rl, ignore_index=so.IGNORE_ID, reduction="none")
        b = dict(base, inputs=inputs, labels=pl, num_total=0, num_correct=0)
        exec(poly, b)
        # compute_accuracy's own counts for the prosody head (train.py:32-36)
        mask = rl != so.IGNORE_ID
        r_total = int(torch.sum(mask))
        r_correct = int(torch.sum(a["prosody_logits"].argmax(-1).masked_select(mask) == rl.masked_select(mask)))
        counts = [int(b["num_total"]), int(b["num_correct"]), r_total, r_correct]
        f1 = []
        lists = []
        for ex in (False, True):
            c = dict(base, inputs=inputs, labels=rl, pred=[], label=[], args=types.SimpleNamespace(exclude_end=ex),
                     f1_score=lambda y, p: float(f1_score(y, p)) if len(y) else 0.0)  # sklearn refuses empty lists
            exec(pros, c)
            exec(pros_f1, c)
            f1.append([c["pw_f1_score"], c["pph_f1_score"], c["iph_f1_score"]])
            lists.append((list(c["pred"]), list(c["label"])))
            for th in (0, 1, 2):
                y = np.asarray([1 if x > th else 0 for x in c["label"]], bool)
                p = np.asarray([1 if x > th else 0 for x in c["pred"]], bool)
                counts += [int((y & p).sum()), int((~y & p).sum()), int((y & ~p).sum())]
    for n, t in (("phone", a["phone_acc"]), ("prosody", a["prosody_acc"])):
        o = 0 if n == "phone" else 2
        assert (np.isnan(t) and counts[o] == 0) or t == counts[o + 1] / counts[o], (n, t, counts)
    return dict(phone_logits=a["phone_logits"], prosody_logits=a["prosody_logits"], nll_phone=nll_p, nll_prosody=nll_r,
                losses=torch.stack([a["phone_loss"], a["prosody_loss"]]), loss=a["loss"], counts=counts, f1=f1, lists=lists,
                num=(b["num_total"], b["num_correct"]), accs=(a["phone_acc"], a["prosody_acc"]))


def build_reference(cname, P, tmp):
    from transformers import BertConfig, BertModel
    FrontendModel = _load(os.path.join(REF_FRONT, "model.py"), "ref_frontend_model").FrontendModel
    bc = {k: v for k, v in fo.BERT_CONFIGS[cname].items() if k not in ("_name_or_path", "model_type")}
    torch.manual_seed(0)
    path = os.path.join(tmp, fo.BERT_CONFIGS[cname]["_name_or_path"])
    if not os.path.exists(path):
        BertModel(BertConfig(**bc)).save_pretrained(path)
    net = FrontendModel(P, fo.NUM_PROSODY, path)
    res = net.load_state_dict(so.weights(cname, P)[0], strict=False)
    assert not res.missing_keys and set(res.unexpected_keys) <= {"bert.embeddings.position_ids"}, res
    return net.eval()


def run_case(cname, P, net, L, lens, seed):
    ids, mask = fo.inputs(lens, seed)
    W64 = so.weights(cname, P)[1]
    x64 = fo.forward(W64, cname, ids, mask)["transform"]
    z64 = so.logits(W64, x64)
    o0 = so.score(W64, x64, mask, None, None)
    pl, rl = so.make_labels(lens, seed, o0["pred_phone"], o0["pred_prosody"], P, fo.NUM_PROSODY)
    o64 = so.score(W64, x64, mask, pl, rl)
    inputs = {"input_ids": ids, "token_type_ids": torch.zeros_like(ids), "attention_mask": mask}
    ref = reference_scores(net, L, inputs, pl, rl)
    floor = {}
    for hd, lab, k in (("phone", pl, 0), ("prosody", rl, 1)):
        floor["logits_" + hd] = fo.gates(fo.valid(ref[hd + "_logits"], mask), fo.valid(z64[k], mask))
        if int((lab != so.IGNORE_ID).sum()):
            floor["nll_" + hd] = fo.gates(so.labelled(ref["nll_" + hd], lab), so.labelled(o64["nll_" + hd], lab))
            floor["loss_" + hd] = fo.gates(ref["losses"][k:k + 1], o64["losses"][k:k + 1])
        else:
            assert bool(torch.isnan(ref["losses"][k])) and bool(torch.isnan(o64["losses"][k]))
    assert ref["counts"] == o64["counts"].tolist(), (cname, P, lens, ref["counts"], o64["counts"].tolist())
    for ex in (False, True):
        assert np.allclose(so.f1(ref["counts"], ex), ref["f1"][int(ex)], rtol=0, atol=1e-15), (ref["counts"], ref["f1"])
    for o in (0, 2):
        if ref["counts"][o] >= 8:
            assert 0 < ref["counts"][o + 1] < ref["counts"][o], (cname, P, lens, ref["counts"])
    return dict(ids=ids, mask=mask, pl=pl, rl=rl, z64=z64, ref=ref, o64=o64, floor=floor)


def stable(case, floors):
    m = case["mask"]
    rng = np.random.default_rng(12345)
    for k, hd in enumerate(("phone", "prosody")):
        z = fo.valid(case["z64"][k], m).numpy()
        want = z.argmax(1)
        if not np.array_equal(fo.valid(case["ref"][hd + "_logits"], m).numpy().argmax(1), want):
            return False
        amp = fo.fixture_gate(floors["logits_" + hd])[1] * np.sqrt(np.mean(z ** 2))
        for _ in range(16):
            if not np.array_equal((z + rng.uniform(-1, 1, z.shape) * amp).argmax(1), want):
                return False
    return True


def score_fixtures(tmp, L):
    for cname in fo.CONFIGS:
        nets = {P: build_reference(cname, P, tmp) for P, _ in so.CLASS_COUNTS}
        keys = [(P, lens) for P, _ in so.CLASS_COUNTS for lens in so.SHAPES]
        seeds = {k: so.case_seed(*k) for k in keys}
        cases = {}
        for _ in range(50):
            for k in keys:
                if k not in cases:
                    cases[k] = run_case(cname, k[0], nets[k[0]], L, k[1], seeds[k])
            floors = {}
            for c in cases.values():
                for n, v in c["floor"].items():
                    floors[n] = fo.worst(floors.get(n), v)
            bad = [k for k in keys if not stable(cases[k], floors)]
            for k in bad:
                print(f"{cname} {k}: seed {seeds[k]} has an unstable argmax")
                seeds[k] += 1000
                del cases[k]
            if not bad:
                break
        else:
            raise SystemExit(f"{cname}: no stable seeds found")
        print(cname, "floors:", {k: tuple(float(f"{x:.3g}") for x in v) for k, v in floors.items()})
        for (P, lens), c in cases.items():
            ref = c["ref"]
            out = dict(weight_seed=fo.WSEED, state_dict_sha256=state_dict_digest(so.weights(cname, P)[0]), input_seed=seeds[(P, lens)],
                       inputs_sha256=inputs_digest(c["ids"], c["mask"]), lens=np.asarray(lens, np.int64), num_polyphones=P,
                       decisions_stable=1, phone_labels=c["pl"].numpy().astype(np.int16),
                       prosody_labels=c["rl"].numpy().astype(np.int16), labels_sha256=labels_digest(c["pl"], c["rl"]),
                       nll_phone=so.labelled(ref["nll_phone"], c["pl"]).numpy(),
                       nll_prosody=so.labelled(ref["nll_prosody"], c["rl"]).numpy(), losses=ref["losses"].numpy(),
                       loss=ref["loss"].numpy(), counts=np.asarray(ref["counts"], np.int64), f1=np.asarray(ref["f1"], np.float64),
                       **{"floor_" + k: np.asarray(v, np.float64) for k, v in floors.items()})
            path = os.path.join(HERE, so.case_name(cname, P, lens) + ".npz")
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path), "bytes", "counts", ref["counts"])


def data_kat(tmp, L):
    from transformers import BertTokenizer
    ds = _load(os.path.join(REF_FRONT, "dataset.py"), "ref_frontend_dataset")
    tk = BertTokenizer(vocab=os.path.join(fo.TOY, "vocab.txt"))
    tables = {}
    for n in ("polyphone", "prosody"):
        tables[n] = {l.strip(): i for i, l in enumerate(open(os.path.join(fo.TOY, "lexicon", n + ".txt"), encoding="utf8"))}
    out = {}
    log = io.StringIO()
    sets = {}
    with contextlib.redirect_stdout(log):
        sets["polyphone"] = ds.FrontendDataset(tk, polyphone_file=os.path.join(fo.TOY, "data", "polyphone_cv.txt"),
                                               polyphone_dict=tables["polyphone"])
        sets["prosody"] = ds.FrontendDataset(tk, prosody_file=os.path.join(fo.TOY, "data", "prosody_cv.txt"),
                                             prosody_dict=tables["prosody"])
        sets["cv"] = ds.FrontendDataset(tk, os.path.join(fo.TOY, "data", "polyphone_cv.txt"), tables["polyphone"],
                                        os.path.join(fo.TOY, "data", "prosody_cv.txt"), tables["prosody"])
    out["log"] = np.asarray(log.getvalue())
    for n, d in sets.items():
        inputs, pl, rl = ds.collate_fn([d[i] for i in range(len(d))], tk)
        out.update({f"{n}_input_ids": inputs["input_ids"].numpy().astype(np.int16),
                    f"{n}_token_type_ids": inputs["token_type_ids"].numpy().astype(np.int16),
                    f"{n}_attention_mask": inputs["attention_mask"].numpy().astype(np.int16),
                    f"{n}_phone_labels": pl.numpy().astype(np.int16), f"{n}_prosody_labels": rl.numpy().astype(np.int16)})
    # the three scripts on the tiny (34, 5) checkpoint, in batches of EVAL_BATCH
    net = build_reference("tiny", fo.NUM_POLYPHONES, tmp)
    batches = {n: [ds.collate_fn([d[i] for i in range(s, min(s + EVAL_BATCH, len(d)))], tk) for s in range(0, len(d), EVAL_BATCH)]
               for n, d in sets.items()}
    tot = np.zeros(22, np.int64)
    num_total, num_correct = 0, 0
    for inputs, pl, rl in batches["polyphone"]:
        r = reference_scores(net, L, dict(inputs), pl, rl)
        tot += np.asarray(r["counts"], np.int64)
        num_total, num_correct = num_total + r["num"][0], num_correct + r["num"][1]  # test_polyphone.py:79, 82
    out["polyphone_counts"] = tot
    out["polyphone_line"] = np.asarray("Accuracy: {}".format(num_correct / num_total))  # test_polyphone.py:86
    # test_prosody.py grows its two lists over ALL batches before the f1 calls
    from sklearn.metrics import f1_score
    tot = np.zeros(22, np.int64)
    f1 = []
    for ex in (False, True):
        pred, label = [], []
        for inputs, pl, rl in batches["prosody"]:
            r = reference_scores(net, L, dict(inputs), pl, rl)
            pred += r["lists"][int(ex)][0]
            label += r["lists"][int(ex)][1]
            if not ex:
                tot += np.asarray(r["counts"], np.int64)
        f1.append([float(f1_score([1 if x > th else 0 for x in label], [1 if x > th else 0 for x in pred])) for th in (0, 1, 2)])
    out["prosody_counts"], out["prosody_f1"] = tot, np.asarray(f1, np.float64)
    out["prosody_lines"] = np.asarray(["pw f1_score {} pph f1_score {} iph f1_score {}".format(*v) for v in f1])  # :101
    for ex in (False, True):
        assert np.allclose(so.f1(tot, ex), f1[int(ex)], rtol=0, atol=1e-15), (tot, f1)
    rows = []
    for inputs, pl, rl in batches["cv"]:
        r = reference_scores(net, L, dict(inputs), pl, rl, w=0.5)
        rows.append([float(r["loss"]), float(r["losses"][0]), r["accs"][0], float(r["losses"][1]), r["accs"][1]])
    out["cv_rows"] = np.asarray(rows, np.float64)  # loss, polyphone_loss, polyphone_acc, prosody_loss, prosody_acc per batch
    path = os.path.join(HERE, "frontend_data_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print(out["log"], out["polyphone_line"], out["prosody_lines"], out["cv_rows"], sep="\n")


def main():
    L = lifted()
    with tempfile.TemporaryDirectory() as tmp:
        if "--data-only" not in sys.argv:
            score_fixtures(tmp, L)
        data_kat(tmp, L)


if __name__ == "__main__":
    main()
