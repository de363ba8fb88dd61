"""CPU tier of the text frontend: the float64 oracle (tests/frontend_oracle.py) against the reference's fixtures
(tests/golden/frontend_*.npz), the blob packer, the loader's errors, cli/frontend.py's decision logic on stubbed
probabilities (tie rules, the '#4' overwrite, compute_batch) and the injected defects, each of which has to land above
the gate the GPU tier holds the device to."""
import json
import os

import numpy as np
import pytest
import torch

from tests import frontend_oracle as fo
from tests.golden.make_golden_disc import state_dict_digest
from tests.golden.make_golden_frontend import inputs_digest
from wetts_amd import _lib, checkpoint, frontend, synth

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="needs a built wetts_amd/lib/libwetts_hip.so")
CASES = [(c, lens) for c in fo.CONFIGS for lens in fo.FIXTURE_SHAPES]


def floor_of(c, key):
    return tuple(float(v) for v in c["floor_" + key])


# ---- 1. the oracle and the fixtures ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,lens", CASES)
def test_oracle_reproduces_the_reference_fixture(cname, lens):
    c = fo.load_fixture(cname, lens)
    assert state_dict_digest(fo.weights(cname)[0]) == str(c["state_dict_sha256"])
    ids, mask, st64 = fo.reference(cname, lens)
    assert inputs_digest(ids, mask) == str(c["inputs_sha256"]) and tuple(c["lens"]) == tuple(lens)
    assert int(c["decisions_stable"]) == 1
    st32 = fo.forward(fo.weights(cname)[0], cname, ids, mask)
    rows = np.cumsum([0] + list(lens))
    for k in fo.OUTPUTS:
        want = torch.from_numpy(c[k])
        assert want.shape[0] == sum(lens)
        # the float64 oracle is one floor from the reference's float32 by the floor's definition
        assert fo.within(fo.gates(want, fo.valid(st64[k], mask)), fo.gate(floor_of(c, k), 1.0001)), k
        assert fo.within(fo.gates(fo.valid(st32[k], mask), want), fo.fixture_gate(floor_of(c, k))), k
        assert not bool(st64[k][mask == 0].any()), k  # zeros at padded tokens
    pp, rr = fo.valid(st64["phone_prob"], mask).numpy(), fo.valid(st64["prosody_prob"], mask).numpy()
    for b, t in enumerate(fo.texts(ids, mask)):
        got = fo.decisions(t, pp[rows[b]:rows[b + 1]], rr[rows[b]:rows[b + 1]])
        assert " ".join(got) == str(c["phonemes"][b]), (b, t)
        assert got[0] == "sil" and got[-1] == "#4"


def test_fixture_floors_are_shared_by_a_config():
    for cname in fo.CONFIGS:
        cs = [fo.load_fixture(cname, lens) for lens in fo.FIXTURE_SHAPES]
        for k in fo.OUTPUTS + fo.STAGES:
            assert all(np.array_equal(c["floor_" + k], cs[0]["floor_" + k]) for c in cs), k
            assert cs[0]["floor_" + k].shape == (2,) and 0 < cs[0]["floor_" + k][0] < 1e-5, k


# ---- 2. config, packer, loader -----------------------------------------------------------------------------------------
def test_config_follows_the_reference_rule():
    for cname in fo.CONFIGS:
        assert frontend.frontend_config(fo.NUM_POLYPHONES, fo.NUM_PROSODY, fo.BERT_CONFIGS[cname]) == fo.config(cname)
    bc = dict(fo.BERT_CONFIGS["base"], _name_or_path="somewhere/else")
    with pytest.raises(ValueError, match="unsupport model"):
        frontend.frontend_config(3, 5, bc)
    assert frontend.frontend_config(3, 5, bc, bert_name_or_path="x/bert-chinese-base/y")["transform_heads"] == 8
    assert frontend.frontend_config(3, 5, bc, transform_heads=4, transform_ff=64)["transform_ff"] == 64
    with pytest.raises(ValueError, match="hidden_act"):
        frontend.frontend_config(3, 5, dict(bc, hidden_act="relu"), 8, 2048)
    with pytest.raises(ValueError, match="position_embedding_type"):
        frontend.frontend_config(3, 5, dict(bc, position_embedding_type="relative_key"), 8, 2048)
    with pytest.raises(ValueError, match="d_model"):
        frontend.frontend_config(3, 5, dict(fo.BERT_CONFIGS["tiny"], _name_or_path="bert-chinese-base"))


def test_config_is_read_from_a_json_path(tmp_path):
    p = tmp_path / "config.json"
    p.write_text(json.dumps(fo.BERT_CONFIGS["tiny"]))
    assert frontend.frontend_config(fo.NUM_POLYPHONES, fo.NUM_PROSODY, str(p)) == fo.config("tiny")


@needs_lib
@pytest.mark.parametrize("cname", fo.CONFIGS)
def test_packer_round_trips_every_tensor(cname):
    cfg, sd = fo.config(cname), fo.weights(cname)[0]
    layout = checkpoint.frontend_layout(cfg)
    blob = checkpoint.pack_frontend_blob(cfg, sd)
    assert blob.numel() == checkpoint.frontend_numel(cfg) and blob.dtype == torch.float32
    names = [n for n, *_ in layout]
    assert len(set(names)) == len(names)
    assert set(names) == {k for k in sd if not k.startswith("bert.pooler.") and k != "bert.embeddings.position_ids"}
    end = 0
    for name, off, numel, shape in layout:
        assert off % 4 == 0 and off >= end and tuple(sd[name].shape) == shape, name
        assert torch.equal(blob[off:off + numel].reshape(shape), sd[name]), name
        end = off + numel
    at = {n: (o, k) for n, o, k, _ in layout}
    for i in range(cfg["num_layers"]):  # q | k | v form ONE packed projection: no gap between them
        p = f"bert.encoder.layer.{i}.attention.self."
        for kind in ("weight", "bias"):
            q, k, v = (at[p + f"{n}.{kind}"] for n in ("query", "key", "value"))
            assert q[0] + q[1] == k[0] and k[0] + k[1] == v[0], (i, kind)
    m = frontend.FrontendModel(fo.NUM_POLYPHONES, fo.NUM_PROSODY, fo.BERT_CONFIGS[cname]).load_state_dict(sd)
    back = m.state_dict()
    assert set(back) == set(names) and all(torch.equal(back[n], sd[n]) for n in names)


@needs_lib
def test_loader_raises_on_each_kind_of_bad_checkpoint():
    cfg, sd = fo.config("tiny"), fo.weights("tiny")[0]
    lean = {k: v for k, v in sd.items() if not k.startswith("bert.pooler.") and k != "bert.embeddings.position_ids"}
    assert torch.equal(checkpoint.pack_frontend_blob(cfg, lean), checkpoint.pack_frontend_blob(cfg, sd))
    for gone in ("bert.embeddings.position_embeddings.weight", "bert.encoder.layer.1.attention.self.key.bias",
                 "transform.self_attn.in_proj_weight", "prosody_classifier.bias"):
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            checkpoint.pack_frontend_blob(cfg, {k: v for k, v in sd.items() if k != gone})
    for name, shape in (("phone_classifier.weight", (fo.NUM_POLYPHONES + 1, 312)), ("transform.linear1.weight", (2048, 312)),
                        ("bert.embeddings.word_embeddings.weight", (fo.VOCAB, 768))):
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            checkpoint.pack_frontend_blob(cfg, dict(sd, **{name: torch.zeros(shape)}))
    for bad in (dict(hidden_size=316), dict(num_heads=7), dict(transform_ff=1204), dict(hidden_size=2048), dict(num_prosody=0)):
        with pytest.raises(ValueError):
            checkpoint.frontend_layout(dict(cfg, **bad))
    with pytest.raises(ValueError, match="layer_norm_eps"):
        checkpoint.frontend_layout({k: v for k, v in cfg.items() if k != "layer_norm_eps"})
    m = frontend.FrontendModel(fo.NUM_POLYPHONES, fo.NUM_PROSODY, fo.BERT_CONFIGS["tiny"])
    with pytest.raises(RuntimeError, match="no weights"):
        m.state_dict()
    with pytest.raises(ValueError, match="HIP device"):
        m.to("cpu")
    with pytest.raises(NotImplementedError):
        m.train()


def test_synthetic_state_dict_is_seeded_and_unit_scaled():
    cfg = fo.config("tiny")
    a, b, c = (synth.make_frontend_state_dict(cfg, s) for s in (3, 3, 4))
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["phone_classifier.weight"], c["phone_classifier.weight"])
    ids, mask = fo.inputs((9, 6), 1)
    st = fo.forward({k: v.double() for k, v in a.items() if v.is_floating_point()}, "tiny", ids, mask)
    for k in ("phone_logits", "prosody_logits"):  # O(1) logits: probabilities away from 0 and 1
        r = float(fo.valid(st[k], mask).pow(2).mean().sqrt())
        assert 0.3 < r < 3.0, (k, r)


# ---- 3. cli/frontend.py's logic on stubbed probabilities --------------------------------------------------------------------
class StubSession:
    """The exported graph's run() returning prepared probabilities: fn(ids [T]) -> ([T, P], [T, R])."""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def run(self, names, feeds):
        self.calls += 1
        ids = np.asarray(feeds["input"])
        assert names is None and ids.ndim == 2 and ids.shape[0] == 1
        a, b = self.fn(ids[0])
        return [np.asarray(a, np.float32)[None], np.asarray(b, np.float32)[None]]


def _seeded(ids):
    rng = np.random.default_rng(int(np.sum(ids * np.arange(1, len(ids) + 1))))
    return rng.random((len(ids), fo.NUM_POLYPHONES)), rng.random((len(ids), fo.NUM_PROSODY))


def test_compute_on_stubbed_probabilities_is_the_reference_logic():
    f = frontend.Frontend(fo.TOY, session=StubSession(_seeded))
    token2id, poly2id, c2p, p2p = fo.toy_tables()
    assert f.token2id == token2id and f.polyphone2id == poly2id and f.char2pinyins == c2p and f.pinyin2phones == p2p
    for text in ("今", "今天天气怎么样", "我们你好的是不了在人有这个上中大为和国"):
        ids = np.asarray([token2id[t] for t in ["[CLS]"] + list(text) + ["[SEP]"]])
        assert f.compute(text) == fo.decisions(text, *_seeded(ids))
    out = f.compute("今天")
    assert out[0] == "sil" and out[-1] == "#4" and len(out) == 1 + 2 * 3


def test_tie_rules_and_the_last_break():
    """Equal probabilities everywhere: list.index(max(..)) takes the FIRST candidate, numpy's argmax the LOWEST class; the
    last break is overwritten by '#4'.  The prosody of character i is read from row i (the reference indexes its
    per-character list into rows that start at [CLS])."""
    token2id, poly2id, c2p, p2p = fo.toy_tables()
    f = frontend.Frontend(fo.TOY, session=StubSession(lambda ids: (np.full((len(ids), fo.NUM_POLYPHONES), 0.5),
                                                                    np.full((len(ids), fo.NUM_PROSODY), 0.2))))
    text = "天么的"  # 2, 3 and 4 candidates
    want = ["sil"]
    for ch in text:
        want += p2p[c2p[ch][0]] + ["#0"]
    want[-1] = "#4"
    assert f.compute(text) == want

    def peaked(ids):
        a = np.full((len(ids), fo.NUM_POLYPHONES), 0.1)
        b = np.full((len(ids), fo.NUM_PROSODY), 0.1)
        for i in range(len(ids)):
            b[i, [1, 3][i % 2]] = 0.9  # row 0 ([CLS]) -> class 1, row 1 -> class 3, ..
            b[i, 4] = 0.9 if i % 2 else 0.1  # a tie between classes 3 and 4 on odd rows: the lower one
        a[2, poly2id[c2p["么"][1]]] = a[2, poly2id[c2p["么"][2]]] = 0.7  # a tie between candidates 1 and 2: the first
        return a, b
    f2 = frontend.Frontend(fo.TOY, session=StubSession(peaked))
    got = f2.compute(text)
    want = ["sil"] + p2p[c2p["天"][0]] + ["#1"] + p2p[c2p["么"][1]] + ["#3"] + p2p[c2p["的"][0]] + ["#4"]
    assert got == want


def test_unknown_characters_raise_key_error_and_compute_batch_equals_compute():
    s = StubSession(_seeded)
    f = frontend.Frontend(fo.TOY, session=s)
    with pytest.raises(KeyError):
        f.compute("今x")  # not in vocab.txt
    with pytest.raises(KeyError):
        f.compute("今，")  # in vocab.txt, not in pinyin_dict.txt
    texts = ["今天天气怎么样", "我", "你好的是不了在人有这个"]
    assert f.compute_batch(texts) == [f.compute(t) for t in texts] and f.compute_batch([]) == []


def test_host_decisions_helper_matches_the_oracle():
    rng = np.random.default_rng(5)
    pp, rr = rng.random((6, fo.NUM_POLYPHONES)), rng.random((6, fo.NUM_PROSODY))
    cands = [[], [3, 1], [], [7, 7, 2], [0, 33, 5, 9], []]
    choice, pros = frontend.host_decisions(pp, rr, cands)
    assert choice == [0 if len(c) < 2 else int(np.argmax([pp[i][k] for k in c])) for i, c in enumerate(cands)]
    assert pros == rr.argmax(1).tolist()


def test_model_synthesis_feeds_the_backend_as_the_reference_does():
    class Backend:
        def run(self, names, feeds):
            self.feeds = feeds
            return [np.full((1, 1, 7), 0.5, np.float32)]
    f = frontend.Frontend(fo.TOY, session=StubSession(_seeded))
    b = Backend()
    m = frontend.Model(b, os.path.join(fo.TOY, "phones.txt"), os.path.join(fo.TOY, "speaker.txt"), f)
    phonemes, audio = m.synthesis("今天", "nobody")
    assert phonemes == f.compute("今天") and audio.dtype == np.int16 and audio.tolist() == [16383] * 7
    assert b.feeds["input"].shape == (1, len(phonemes)) and b.feeds["input_lengths"].tolist() == [len(phonemes)]
    assert b.feeds["scales"].dtype == np.float32 and np.allclose(b.feeds["scales"], [[0.667, 1.0, 0.8]])
    assert b.feeds["sid"].tolist() == [0]


# ---- 4. injected defects ----------------------------------------------------------------------------------------------------
DEFECT_SHAPES = ((9, 6), (33, 32, 31))


@pytest.mark.parametrize("fault", fo.FAULTS)
def test_injected_defect_lands_above_its_gate(fault):
    """Each defect, evaluated in float64, is measured like the device: the worst figure over the shapes at the stage
    where it shows (the embeddings or one of the four outputs) against GATE_FACTOR x that stage's floor."""
    hit = 0
    for cname in fo.CONFIGS:
        if fault == "transform_12_heads" and fo.config(cname)["transform_heads"] == 12:
            continue  # the defect IS the tiny branch's head count
        c = fo.load_fixture(cname, DEFECT_SHAPES[0])
        worst = {}
        for lens in DEFECT_SHAPES:
            ids, mask, st64 = fo.reference(cname, lens)
            bad = fo.forward(fo.weights(cname)[1], cname, ids, mask, fault=fault)
            for k in ("embed",) + fo.OUTPUTS:
                worst[k] = fo.worst(worst.get(k), fo.gates(fo.valid(bad[k], mask), fo.valid(st64[k], mask)))
        over = {k: (v[0] / fo.gate(floor_of(c, k))[0], v[1] / fo.gate(floor_of(c, k))[1]) for k, v in worst.items()}
        print(fault, cname, {k: tuple(float(f"{x:.3g}") for x in v) for k, v in over.items()})
        assert max(max(v) for v in over.values()) > 1.0, (fault, cname, over)
        hit += 1
    assert hit >= 1


def test_cli_takes_text_only_with_a_frontend_directory():
    from wetts_amd import inference
    base = ["--checkpoint", "G.pth", "--cfg", "c.json", "--outdir", "o", "--phone_table", "p.txt"]
    a = inference.get_args(base + ["--test_file", "t.txt"])
    assert a.test_file == "t.txt" and a.front_dir is None and a.text_file is None  # the reference's flags: unchanged
    a = inference.get_args(base + ["--front_dir", "f", "--text_file", "x.txt"])
    assert a.front_dir == "f" and a.text_file == "x.txt" and a.speaker == "default"
    for bad in ([], ["--text_file", "x.txt"], ["--front_dir", "f"], ["--test_file", "t", "--front_dir", "f", "--text_file", "x"]):
        with pytest.raises(SystemExit):
            inference.get_args(base + bad)
