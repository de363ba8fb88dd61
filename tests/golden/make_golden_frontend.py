#!/usr/bin/env python3
"""Generates the frontend golden vectors (tests/golden/frontend_{tiny,base}_b{B}x{T}.npz) by running the REAL reference's
FrontendModel (frontend/model.py, imported unmodified by path) and its cli `Frontend.compute` (cli/frontend.py; the
`onnxruntime` import at its top is stubbed where the package is absent, and its session is the reference model's own
export_forward) on the seeded synthetic checkpoint of synth.make_frontend_state_dict.  Run in the build container only:

    python tests/golden/make_golden_frontend.py

A seeded transformers.BertModel is written with save_pretrained into a temporary directory whose name contains the
reference's model name, so the reference's own constructor (AutoModel.from_pretrained) and its branch run; the synthetic
state_dict is then loaded into that model.  No pretrained weights are involved and no weights are stored.

Stored per config and shape of frontend_oracle.FIXTURE_SHAPES: the seeds, the sha256 of the weights and of the inputs,
the reference's float32 logits and probabilities at the valid tokens, the phoneme list compute() gives for every row on
the toy lexicon (tests/golden/frontend_toy), and the float32 floors: floor_<output> = the reference's forward pass against
the float64 oracle, floor_<stage> = torch's float32 evaluation of a stand-alone stage against its float64 evaluation on
the same inputs; each the worst over the config's shapes, (rel RMS, max |d| / rms).

DECISION STABILITY is a condition of a fixture.  A decision is a discrete function of its probabilities, so a case is
only written when every polyphone and prosody decision is the same under (a) the float64 oracle, (b) the reference's
float32 (the padded batch AND the row alone, which is what compute() runs) and (c) sixteen copies of (a) with
independent uniform noise of amplitude (GATE_FACTOR + 1) x floor_local x rms(probabilities) -- the fixture gate.  A case that
fails moves to another input seed (+1000); the seed used is recorded, with decisions_stable = 1."""
import hashlib
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests import frontend_oracle as fo  # noqa: E402
from tests.golden.make_golden_disc import state_dict_digest  # noqa: E402

REF_WETTS = os.path.join(ref_import.REF_ROOT, "wetts")


def inputs_digest(ids, mask):
    h = hashlib.sha256()
    for t in (ids, mask):
        h.update(t.to(torch.int64).contiguous().numpy().tobytes())
    return h.hexdigest()


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    """(the reference's FrontendModel class, its cli Frontend class), both unmodified."""
    model = _load(os.path.join(REF_WETTS, "frontend", "model.py"), "ref_frontend_model")
    try:
        import onnxruntime  # noqa: F401
    except ImportError:  # cli/frontend.py only constructs an InferenceSession in __init__, which is not run here
        sys.modules["onnxruntime"] = types.ModuleType("onnxruntime")
    cli = _load(os.path.join(REF_WETTS, "cli", "frontend.py"), "ref_cli_frontend")
    return model.FrontendModel, cli.Frontend


def build_reference(cname, tmp):
    from transformers import BertConfig, BertModel
    FrontendModel, Frontend = import_reference()
    bc = {k: v for k, v in fo.BERT_CONFIGS[cname].items() if k not in ("_name_or_path", "model_type")}
    torch.manual_seed(0)
    path = os.path.join(tmp, fo.BERT_CONFIGS[cname]["_name_or_path"])
    BertModel(BertConfig(**bc)).save_pretrained(path)
    net = FrontendModel(fo.NUM_POLYPHONES, fo.NUM_PROSODY, path)
    sd = fo.weights(cname)[0]
    res = net.load_state_dict(sd, strict=False)
    assert not res.missing_keys and set(res.unexpected_keys) <= {"bert.embeddings.position_ids"}, res
    net.eval()
    assert net.transform.self_attn.num_heads == fo.TRANSFORM[cname][0] and net.transform.linear1.out_features == fo.TRANSFORM[cname][1]

    class Session:  # the exported graph IS export_forward (export_onnx.py:68)
        def run(self, _, feeds):
            with torch.no_grad():
                a, b = net.export_forward(torch.from_numpy(np.asarray(feeds["input"])).to(torch.int64))
            return [a.numpy(), b.numpy()]

    front = Frontend.__new__(Frontend)
    front.session = Session()
    front.token2id = front.read_list(os.path.join(fo.TOY, "vocab.txt"))
    front.polyphone2id = front.read_list(os.path.join(fo.TOY, "lexicon", "polyphone.txt"))
    front.id2polyphone = {v: k for k, v in front.polyphone2id.items()}
    front.char2pinyins = front.read_char2pinyins(os.path.join(fo.TOY, "lexicon", "pinyin_dict.txt"))
    front.pinyin2phones = front.read_pinyin2phones(os.path.join(fo.TOY, "lexicon", "lexicon.txt"))
    return net, front


def run_case(cname, net, front, lens, seed):
    ids, mask = fo.inputs(lens, seed)
    with torch.no_grad():
        lp, lr = net({"input_ids": ids, "token_type_ids": torch.zeros_like(ids), "attention_mask": mask})
    ref = dict(phone_logits=lp, prosody_logits=lr, phone_prob=torch.softmax(lp, -1), prosody_prob=torch.softmax(lr, -1))
    sd, W64 = fo.weights(cname)
    st64 = fo.forward(W64, cname, ids, mask)
    txt = fo.texts(ids, mask)
    return dict(ids=ids, mask=mask, ref={k: fo.valid(v, mask) for k, v in ref.items()}, st64=st64, texts=txt,
                phonemes=[front.compute(t) for t in txt],
                out_floor={k: fo.gates(fo.valid(ref[k], mask), fo.valid(st64[k], mask)) for k in fo.OUTPUTS},
                stage_floor={s: fo.gates(fn(sd, i), fn(W64, i)) for s, (i, fn) in fo.stage_cases(cname, ids, mask).items()})


def stable(case, lens, floors):
    """The eighteen-fold agreement of the module docstring."""
    tables = fo.toy_tables()
    rows = np.cumsum([0] + list(lens))
    want = case["phonemes"]
    m = case["mask"]
    p64, r64 = fo.valid(case["st64"]["phone_prob"], m).numpy(), fo.valid(case["st64"]["prosody_prob"], m).numpy()
    cands = [(p64, r64), (case["ref"]["phone_prob"].numpy(), case["ref"]["prosody_prob"].numpy())]
    rng = np.random.default_rng(12345)
    for _ in range(16):
        cands.append(tuple(a + rng.uniform(-1, 1, a.shape) * fo.fixture_gate(floors[k])[1] * np.sqrt(np.mean(a ** 2))
                           for a, k in ((p64, "phone_prob"), (r64, "prosody_prob"))))
    for pp, rr in cands:
        for b, t in enumerate(case["texts"]):
            if fo.decisions(t, pp[rows[b]:rows[b + 1]], rr[rows[b]:rows[b + 1]], tables) != want[b]:
                return False
    return True


def main():
    with tempfile.TemporaryDirectory() as tmp:
        for cname in fo.CONFIGS:
            net, front = build_reference(cname, tmp)
            digest = state_dict_digest(fo.weights(cname)[0])
            seeds = {lens: fo.case_seed(lens) for lens in fo.FIXTURE_SHAPES}
            cases = {}
            for _ in range(50):
                for lens in fo.FIXTURE_SHAPES:
                    if lens not in cases:
                        cases[lens] = run_case(cname, net, front, lens, seeds[lens])
                floors = {}
                for c in cases.values():
                    for k, v in list(c["out_floor"].items()) + list(c["stage_floor"].items()):
                        floors[k] = fo.worst(floors.get(k), v)
                bad = [lens for lens in fo.FIXTURE_SHAPES if not stable(cases[lens], lens, floors)]
                for lens in bad:
                    print(f"{cname} {lens}: seed {seeds[lens]} has an unstable decision")
                    seeds[lens] += 1000
                    del cases[lens]
                if not bad:
                    break
            else:
                raise SystemExit(f"{cname}: no stable seeds found")
            print(cname, "floors:", {k: tuple(float(f"{x:.3g}") for x in v) for k, v in floors.items()})
            for lens, c in cases.items():
                out = dict(weight_seed=fo.WSEED, state_dict_sha256=digest, input_seed=seeds[lens],
                           inputs_sha256=inputs_digest(c["ids"], c["mask"]), lens=np.asarray(lens, np.int64),
                           decisions_stable=1, phonemes=np.asarray([" ".join(p) for p in c["phonemes"]]),
                           **{k: v.numpy() for k, v in c["ref"].items()},
                           **{"floor_" + k: np.asarray(v, np.float64) for k, v in floors.items()})
                path = os.path.join(HERE, fo.case_name(cname, lens) + ".npz")
                np.savez_compressed(path, **out)
                print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
