"""CPU tier of the frontend's scoring: the float64 oracle (tests/frontend_score_oracle.py) against the reference's fixtures
(tests/golden/frontend_score_*.npz), the injected defects (each has to break a gate or a count the GPU tier holds the device
to), the data readers of wetts_amd.frontend_data against what the reference's FrontendDataset + collate_fn gave on the toy
files (tests/golden/frontend_data_kat.npz; no `transformers` here), the host helpers and the header / binding agreement."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

from tests import frontend_oracle as fo
from tests import frontend_score_oracle as so
from tests.golden.make_golden_disc import state_dict_digest
from tests.golden.make_golden_frontend import inputs_digest
from tests.golden.make_golden_frontend_score import labels_digest
from wetts_amd import _lib, frontend, frontend_data, frontend_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="needs a built wetts_amd/lib/libwetts_hip.so")
FLOORS = ("nll_phone", "nll_prosody", "loss_phone", "loss_prosody", "logits_phone", "logits_prosody")
ENTRIES = ("wetts_frontend_score", "wetts_frontend_score_heads")


def _figures(o, c, pl, rl):
    """{key: (rel, local)} of the reference's float32 (fixture c) against the float64 results o."""
    figs = {}
    for hd, lab, k in (("phone", pl, 0), ("prosody", rl, 1)):
        if int((lab != so.IGNORE_ID).sum()) == 0:
            assert np.isnan(c["losses"][k]) and bool(torch.isnan(o["losses"][k])), hd
            continue
        figs["nll_" + hd] = fo.gates(torch.from_numpy(c["nll_" + hd]), so.labelled(o["nll_" + hd], lab))
        figs["loss_" + hd] = fo.gates(torch.from_numpy(c["losses"][k:k + 1]), o["losses"][k:k + 1])
    return figs


# ---- 1. the oracle and the fixtures ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,P,lens", so.CASES)
def test_oracle_reproduces_the_reference_fixture(cname, P, lens):
    c = so.load_fixture(cname, P, lens)
    assert state_dict_digest(so.weights(cname, P)[0]) == str(c["state_dict_sha256"]) and int(c["num_polyphones"]) == P
    ids, mask, pl, rl, x, o = so.reference(cname, P, lens)
    assert inputs_digest(ids, mask) == str(c["inputs_sha256"]) and tuple(c["lens"]) == tuple(lens)
    assert labels_digest(pl, rl) == str(c["labels_sha256"]) and int(c["decisions_stable"]) == 1
    # the labels are the seeded function of the oracle's own predictions
    bare = so.score(so.weights(cname, P)[1], x, mask, None, None)
    again = so.make_labels(lens, int(c["input_seed"]), bare["pred_phone"], bare["pred_prosody"], P, fo.NUM_PROSODY)
    assert torch.equal(again[0], pl) and torch.equal(again[1], rl)
    assert not bool((pl[mask == 0] != so.IGNORE_ID).any()) and not bool((rl[mask == 0] != so.IGNORE_ID).any())
    for k, v in _figures(o, c, pl, rl).items():  # one floor from the reference's float32 by the floor's definition
        assert fo.within(v, fo.gate(c["floor_" + k], 1.0001)), (k, v, c["floor_" + k])
    assert o["counts"].tolist() == c["counts"].tolist()
    for ex in (False, True):
        assert np.allclose(so.f1(c["counts"], ex), c["f1"][int(ex)], rtol=0, atol=1e-15)
        assert frontend.prosody_f1(c["counts"].tolist(), ex) == so.f1(c["counts"], ex)
    for o_ in (0, 2):  # neither all right nor all wrong wherever a head has labels to speak of
        if c["counts"][o_] >= 8:
            assert 0 < c["counts"][o_ + 1] < c["counts"][o_]
    w = np.float32(0.5)
    want = w * c["losses"][0] + (np.float32(1) - w) * c["losses"][1]
    assert (np.isnan(want) and np.isnan(c["loss"])) or want == c["loss"]  # train.py:83-84 in float32


def test_fixture_floors_are_shared_by_a_config():
    for cname in fo.CONFIGS:
        cs = [so.load_fixture(cname, P, lens) for c, P, lens in so.CASES if c == cname]
        assert len(cs) == len(so.CLASS_COUNTS) * len(so.SHAPES)
        for k in FLOORS:
            assert all(np.array_equal(c["floor_" + k], cs[0]["floor_" + k]) for c in cs), k
            assert cs[0]["floor_" + k].shape == (2,) and 0 < cs[0]["floor_" + k][0] < 1e-5, k


# ---- 2. injected defects -------------------------------------------------------------------------------------------------
DEFECT_CASES = [(c, P, lens) for c, P, lens in so.CASES if len(lens) > 1]


def _tie_case(cname, P):
    """x, mask and the clean float64 scores under so.tie_weights: exact ties at the maximum."""
    W = {k: v.double() for k, v in so.tie_weights(cname, P).items() if v.is_floating_point()}
    ids, mask = fo.inputs((33, 32, 31), 515)
    x = fo.forward(W, cname, ids, mask)["transform"]
    return W, x, mask


@pytest.mark.parametrize("fault", so.FAULTS)
def test_injected_defect_breaks_a_gate_or_a_count(fault):
    hits = []
    if fault == "argmax_highest_on_tie":  # shows only where logits tie exactly
        for cname in fo.CONFIGS:
            W, x, mask = _tie_case(cname, 470)
            good, bad = so.score(W, x, mask, None, None), so.score(W, x, mask, None, None, fault=fault)
            on = mask != 0
            for hd, (lo, his) in so.TIES.items():
                g, b = good["pred_" + hd][on], bad["pred_" + hd][on]
                assert int((g == lo).sum()) >= 8 and not any(bool((g == hi).any()) for hi in his), (cname, hd)
                if not torch.equal(g, b):
                    hits.append((cname, hd))
        assert hits
        return
    for cname, P, lens in DEFECT_CASES:
        c = so.load_fixture(cname, P, lens)
        ids, mask, pl, rl, x, good = so.reference(cname, P, lens)
        bad = so.score(so.weights(cname, P)[1], x, mask, pl, rl, fault=fault)
        over = 0.0
        for hd, lab, k in (("phone", pl, 0), ("prosody", rl, 1)):
            if int((lab != so.IGNORE_ID).sum()):
                for key, fig in (("nll_" + hd, fo.gates(so.labelled(bad["nll_" + hd], lab), so.labelled(good["nll_" + hd], lab))),
                                 ("loss_" + hd, fo.gates(bad["losses"][k:k + 1], good["losses"][k:k + 1]))):
                    g = fo.gate(c["floor_" + key])
                    over = max(over, fig[0] / g[0], fig[1] / g[1])
        if over > 1.0 or bad["counts"].tolist() != good["counts"].tolist():
            hits.append((cname, P, lens, round(over, 1)))
    print(fault, hits)
    assert hits, fault


# ---- 3. the data readers ---------------------------------------------------------------------------------------------------
def _toy_sets():
    tk = frontend_data.VocabTokenizer(os.path.join(fo.TOY, "vocab.txt"))
    poly = frontend_data.read_table(os.path.join(fo.TOY, "lexicon", "polyphone.txt"))
    pros = frontend_data.read_table(os.path.join(fo.TOY, "lexicon", "prosody.txt"))
    pf, rf = os.path.join(fo.TOY, "data", "polyphone_cv.txt"), os.path.join(fo.TOY, "data", "prosody_cv.txt")
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        sets = {"polyphone": frontend_data.FrontendDataset(tk, polyphone_file=pf, polyphone_dict=poly),
                "prosody": frontend_data.FrontendDataset(tk, prosody_file=rf, prosody_dict=pros),
                "cv": frontend_data.FrontendDataset(tk, pf, poly, rf, pros)}
    return tk, sets, log.getvalue()


def test_data_readers_reproduce_the_reference_on_the_toy_files():
    kat = np.load(os.path.join(fo.GOLDEN, "frontend_data_kat.npz"))
    tk, sets, log = _toy_sets()
    assert log == str(kat["log"])  # "Reading N .. data" and the "Ignore line .." of the malformed prosody line
    assert "Ignore line" in log and (len(sets["polyphone"]), len(sets["prosody"]), len(sets["cv"])) == (12, 11, 23)
    for n, d in sets.items():
        inputs, pl, rl = frontend_data.collate_fn([d[i] for i in range(len(d))], tk)
        for k, got in (("input_ids", inputs["input_ids"]), ("token_type_ids", inputs["token_type_ids"]),
                       ("attention_mask", inputs["attention_mask"]), ("phone_labels", pl), ("prosody_labels", rl)):
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), kat[f"{n}_{k}"].astype(np.int64)), (n, k)
    ids = kat["polyphone_input_ids"]
    assert (ids == tk.unk_token_id).sum() == 1  # the one character outside the toy vocabulary
    # the unknown polyphone (ma5) leaves its character ignored: that line carries no label
    assert (kat["polyphone_phone_labels"] != so.IGNORE_ID).sum(1).min() == 0
    assert frontend_data.IGNORE_ID == so.IGNORE_ID == frontend.IGNORE_ID == -100


def test_line_parsers_follow_the_format_rules():
    M = frontend_data.MARK
    assert M == "▁"
    pp = frontend_data.parse_polyphone_line
    assert pp(f"今天{M}di2{M}气\n") == [("今天", "di2"), ("气", None)]
    assert pp(f"{M}今{M}ba1{M}") == [("今", "ba1")] and pp("今天\n") == [("今天", None)]  # marks at the ends carry nothing
    assert pp(f"今{M}a{M}天{M}b{M}气{M}c") == [("今", "a"), ("天", "b"), ("气", "c")]
    pr = frontend_data.parse_prosody_line
    assert pr("今天 #1 天气 #0 怎么样 #4\n", 5) == [("今天", 1), ("天气", 0), ("怎么样", 4)] and pr("\n", 5) == []
    for bad in ("今天 #1 天气", "今天 1", "今天 #", "今天 #x", "今天 #5", "今天 #-1", "今天 #1.0", "今天 #２"):
        assert pr(bad, 5) is None, bad  # odd fields; no '#'; no digits; not digits; rank >= 5; signs, points, non-ASCII digits
    assert pr("今天 #05", 6) == [("今天", 5)]


def test_vocab_tokenizer_contract():
    tk = frontend_data.VocabTokenizer(os.path.join(fo.TOY, "vocab.txt"))
    assert tk.encode("今天 x") == [5, 6, tk.unk_token_id] and tk.encode("今", add_special_tokens=True) == [2, 5, 3]
    out = tk([["今天", "气"], ["我"]], padding=True, truncation=True, is_split_into_words=True, return_tensors="pt")
    assert out["input_ids"].tolist() == [[2, 5, 6, 7, 3], [2, 11, 3, 0, 0]]
    assert out["attention_mask"].tolist() == [[1, 1, 1, 1, 1], [1, 1, 1, 0, 0]] and not bool(out["token_type_ids"].any())
    with pytest.raises(ValueError):
        tk([["今"]], padding=False)
    short = frontend_data.VocabTokenizer(os.path.join(fo.TOY, "vocab.txt"), model_max_length=4)
    assert short([["今天气怎么样"]])["input_ids"].tolist() == [[2, 5, 6, 3]]


# ---- 4. host helpers ---------------------------------------------------------------------------------------------------------
def test_compute_accuracy_and_prosody_f1_on_accumulated_counts():
    a = [10, 4, 20, 5] + [3, 1, 2, 0, 0, 0, 5, 0, 0] + [2, 1, 1, 0, 0, 0, 4, 0, 0]
    b = [6, 6, 0, 0] + [1, 0, 0, 0, 2, 0, 0, 0, 1] + [0] * 9
    tot = [x + y for x, y in zip(a, b)]
    assert frontend.compute_accuracy(tot, "phone") == 10 / 16 == frontend.compute_accuracy(tot, "polyphone")
    assert frontend.compute_accuracy(tot, "prosody") == 5 / 20
    assert np.isnan(frontend.compute_accuracy(b, "prosody"))  # compute_accuracy's value without a label
    assert frontend.prosody_f1(tot) == (8 / 11, 0.0, 10 / 11) and frontend.prosody_f1(tot, True) == (4 / 6, 0.0, 1.0)
    assert frontend.prosody_f1([0] * 22) == (0.0, 0.0, 0.0)  # sklearn's value for an empty denominator
    with pytest.raises(ValueError):
        frontend.compute_accuracy(tot, "tone")
    with pytest.raises(ValueError):
        frontend.prosody_f1(tot[:21])


def test_host_scores_from_a_packed_row():
    def row(pl, rl, bits, counts):
        f = torch.tensor([pl, rl], dtype=torch.float32).view(torch.int32).to(torch.int64)
        return torch.cat([torch.tensor(counts, dtype=torch.int64), f, torch.tensor([bits], dtype=torch.int64)])
    counts = [4, 1, 8, 6] + [1] * 18
    h = frontend.HostScores.from_packed(row(2.5, 1.25, 0, counts), 0.25)
    assert (h.phone_loss, h.prosody_loss, h.loss) == (2.5, 1.25, 0.25 * 2.5 + 0.75 * 1.25)
    assert (h.phone_acc, h.prosody_acc, h.num_total, h.num_correct) == (0.25, 0.75, 4, 1) and h.f1() == (0.5, 0.5, 0.5)
    # train.py:83-84: `1 - w` in double, rounded once (0.6: float32(1) - float32(0.6) is one ulp away from float32(0.4))
    h = frontend.HostScores.from_packed(row(2.5, 1.3, 0, counts), 0.6)
    assert np.float32(1) - np.float32(0.6) != np.float32(1 - 0.6)
    assert h.loss == float(np.float32(0.6) * np.float32(2.5) + np.float32(1 - 0.6) * np.float32(1.3))
    assert h.loss == float(0.6 * torch.tensor(2.5) + (1 - 0.6) * torch.tensor(1.3))  # the reference's expression
    h = frontend.HostScores.from_packed(row(float("nan"), -1.5, 0, [0, 0] + counts[2:]))
    assert np.isnan(h.phone_loss) and np.isnan(h.loss) and np.isnan(h.phone_acc) and h.prosody_loss == -1.5
    with pytest.raises(IndexError, match="out of bounds"):
        frontend.HostScores.from_packed(row(1.0, 1.0, _lib.STATUS_LABEL_RANGE, counts))
    with pytest.raises(ValueError, match="attention_mask"):
        frontend.HostScores.from_packed(row(1.0, 1.0, _lib.STATUS_LABEL_AT_PAD, counts))
    with pytest.raises(IndexError):
        frontend.HostScores.from_packed(row(1.0, 1.0, _lib.STATUS_TOKEN_ID_RANGE, counts))


def test_score_refuses_bad_arguments_before_any_launch():
    m = frontend.FrontendModel(fo.NUM_POLYPHONES, fo.NUM_PROSODY, fo.BERT_CONFIGS["tiny"])
    with pytest.raises(RuntimeError, match="no weights"):
        m.score({"input_ids": torch.zeros(1, 3, dtype=torch.int64)})


def test_eval_cli_takes_the_reference_flags():
    base = ["--polyphone_dict", "a", "--prosody_dict", "b", "--checkpoint", "c"]
    a = frontend_eval.get_args(["polyphone"] + base + ["--test_data", "t"])
    assert (a.batch_size, a.bert_name_or_path, a.test_data) == (32, "bert-chinese-base", "t")
    a = frontend_eval.get_args(["prosody", "--exclude_end"] + base + ["--test_data", "t", "--batch_size", "4"])
    assert a.exclude_end and a.batch_size == 4
    a = frontend_eval.get_args(["cv"] + base + ["--cv_polyphone_data", "p", "--cv_prosody_data", "r", "--polyphone_weight", "0.3"])
    assert (a.cv_polyphone_data, a.cv_prosody_data, a.polyphone_weight) == ("p", "r", 0.3)
    for bad in (["polyphone"] + base, ["cv"] + base + ["--test_data", "t"], ["polyphone", "--exclude_end"] + base + ["--test_data", "t"],
                ["polyphone", "--epoch", "1"] + base + ["--test_data", "t"]):
        with pytest.raises(SystemExit):
            frontend_eval.get_args(bad)


# ---- 5. header / binding agreement ---------------------------------------------------------------------------------------------
@needs_lib
def test_header_and_binding_agree_on_the_new_entries():
    src = open(os.path.join(ROOT, "include", "wetts_hip.h")).read()
    assert int(re.search(r"#define WETTS_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 12  # additive only
    lib = _lib.load()
    kinds = {"int32_t": _lib._I32, "int64_t": _lib._I64}
    for name in ENTRIES:
        m = re.search(r"int32_t " + name + r"\(([^;]*)\);", src)
        assert m and hasattr(lib, name), name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib._I32 and len(argtypes) == len(args), (name, args)
        for a, t in zip(args, argtypes):  # pointers bind as void*, scalars by their C type
            assert t is (_lib._P if "*" in a else kinds[a.split()[0]]), (name, a, t)
    assert re.search(r"int64_t wetts_frontend_score_workspace_bytes\(const wetts_frontend_t\* f, int32_t B, int32_t T\);", src)
    assert _lib.SIGNATURES["wetts_frontend_score_workspace_bytes"] == (_lib._I64, [_lib._P, _lib._I32, _lib._I32])
    bits = dict(re.findall(r"#define WETTS_STATUS_(LABEL_[A-Z_]+) (\d+)", src))
    assert {k: int(v) for k, v in bits.items()} == dict(LABEL_RANGE=_lib.STATUS_LABEL_RANGE, LABEL_AT_PAD=_lib.STATUS_LABEL_AT_PAD)
    assert (_lib.STATUS_LABEL_RANGE, _lib.STATUS_LABEL_AT_PAD) == (512, 1024)
