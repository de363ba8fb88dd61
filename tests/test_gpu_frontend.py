"""GPU tier of the text frontend (csrc/frontend.hip, wetts_amd/frontend.py): the reference's fixtures
(tests/golden/frontend_*.npz), every stand-alone stage and the whole forward pass against the float64 oracle of
tests/frontend_oracle.py under the gates defined there (4 x the float32 floor stored in the fixtures), the zeros at padded
tokens, the bit-exact conditions (a row alone, repeats, softmax 0 / 1), the error paths, the ORT-shaped session, the
decisions on the device and Model.synthesis.  Tiles: 64 GEMM columns in two halves of 32, 16 queries and 64 keys per
attention block, 4 tokens per LayerNorm / classifier block; frontend_oracle.FIXTURE_SHAPES put their edges inside."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import frontend_oracle as fo
from tests.golden.make_golden_disc import state_dict_digest
from tests.golden.make_golden_frontend import inputs_digest
from wetts_amd import Frontend, FrontendModel, FrontendSession, Model, SynthesizerTrn, _lib, checkpoint, config, synth
from wetts_amd.session import InferenceSession

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(c, lens) for c in fo.CONFIGS for lens in fo.FIXTURE_SHAPES]
_NET, _DEVW, _FRONT, _MARGINS = {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_and_report():
    yield
    import gc
    _NET.clear()
    _DEVW.clear()
    _FRONT.clear()
    fo._REF.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = os.environ.get("WETTS_FRONTEND_MARGINS")  # the GPU run that records profiles/frontend_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst multiple of a gate per case (1 = at the gate; gate = 4 x floor), then the (rel, local) figures\n")
            for k in sorted(_MARGINS):
                f.write(f"{k}: {_MARGINS[k]}\n")


def _net(cname):
    if cname not in _NET:
        _NET[cname] = FrontendModel(fo.NUM_POLYPHONES, fo.NUM_PROSODY, fo.BERT_CONFIGS[cname]) \
            .load_state_dict(fo.weights(cname)[0]).to(DEV)
    return _NET[cname]


def _w(cname, name):
    """A float32 weight on the device; "qkv0.weight" / "qkv0.bias": layer 0's packed projection."""
    key = (cname, name)
    if key not in _DEVW:
        sd = fo.weights(cname)[0]
        if name.startswith("qkv0."):
            t = torch.cat([sd[f"bert.encoder.layer.0.attention.self.{n}.{name[5:]}"] for n in ("query", "key", "value")], 0)
        else:
            t = sd[name]
        _DEVW[key] = t.to(DEV).contiguous()
    return _DEVW[key]


def _front_dir(cname, tmp_path_factory):
    """A model directory as wetts_amd.frontend.Frontend reads it: final.pt, config.json, vocab.txt, lexicon/."""
    if cname not in _FRONT:
        d = str(tmp_path_factory.mktemp("front_" + cname))
        shutil.copy(os.path.join(fo.TOY, "vocab.txt"), d)
        shutil.copytree(os.path.join(fo.TOY, "lexicon"), os.path.join(d, "lexicon"))
        torch.save(fo.weights(cname)[0], os.path.join(d, "final.pt"))
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump(fo.BERT_CONFIGS[cname], f)
        _FRONT[cname] = Frontend(d)
    return _FRONT[cname]


def _figs(d):
    return {k: tuple(float(f"{x:.3g}") for x in v) for k, v in d.items()}


def _check(figs, c, tag, fixture=False):
    """Asserts {key: (rel, local)} against the gates of fixture `c`; records the worst multiple of a gate."""
    top = 0.0
    for k, v in figs.items():
        g = (fo.fixture_gate if fixture else fo.gate)(c["floor_" + k])
        top = max(top, v[0] / g[0], v[1] / g[1])
    print(tag, _figs(figs), "worst multiple of a gate", round(top, 3))
    for k, v in figs.items():
        g = (fo.fixture_gate if fixture else fo.gate)(c["floor_" + k])
        assert fo.within(v, g), f"{tag} {k}: rel {v[0]:.3e} (gate {g[0]:.3e}) local {v[1]:.3e} (gate {g[1]:.3e})"
    _MARGINS[tag] = (round(top, 3), _figs(figs))


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,lens", CASES)
def test_matches_reference_fixture(cname, lens, tmp_path_factory):
    """First the regenerated weights' and inputs' digests; then logits and probabilities at the valid tokens against the
    reference's float32 (4 + 1 floors), and the phoneme lists of compute_batch() and compute(), exactly."""
    c = fo.load_fixture(cname, lens)
    assert state_dict_digest(fo.weights(cname)[0]) == str(c["state_dict_sha256"])
    ids, mask = fo.inputs(lens, int(c["input_seed"]))
    assert inputs_digest(ids, mask) == str(c["inputs_sha256"])
    net = _net(cname)
    lp, lr = net({"input_ids": ids, "attention_mask": mask})
    pp, pr = net.probs(ids, mask)
    got = dict(phone_logits=lp, prosody_logits=lr, phone_prob=pp, prosody_prob=pr)
    figs = {k: fo.gates(fo.valid(got[k].cpu(), mask), torch.from_numpy(c[k])) for k in fo.OUTPUTS}
    _check(figs, c, f"fixture {fo.case_name(cname, lens)}", fixture=True)
    front = _front_dir(cname, tmp_path_factory)
    texts = fo.texts(ids, mask)
    want = [str(p).split(" ") for p in c["phonemes"]]
    assert front.compute_batch(texts) == want
    assert front.compute(texts[-1]) == want[-1]


# ---- 2. every stand-alone stage against the float64 oracle -----------------------------------------------------------------
def _run_stage(cname, stage, i):
    """The device entry of a stage on the oracle's float32 inputs -> the output tensor (device)."""
    lib, s = _lib.load(), _lib.current_stream_ptr()
    net, cfg = _net(cname), fo.config(cname)
    d = cfg["hidden_size"]
    if stage == "embed":
        ids, mask = i["ids"].to(DEV), i["mask"].to(DEV)
        B, T = ids.shape
        out, mf = torch.empty(B, T, d, device=DEV), torch.empty(B, T, device=DEV)
        _lib.check(lib.wetts_frontend_embed(net._handle, _lib.ptr(ids), None, _lib.ptr(mask), B, T, _lib.ptr(out), _lib.ptr(mf),
                                            None, s), stage)
        assert torch.equal(mf.cpu(), i["mask"].to(torch.float32))
        return out
    if stage.startswith("linear_"):
        x = i["x"].to(DEV).contiguous()
        B, T, K = x.shape
        name = "qkv0" if stage == "linear_bias" else i["name"]
        w, b = _w(cname, name + ".weight"), _w(cname, name + ".bias")
        res = i["res"].to(DEV).contiguous() if "res" in i else None
        out = torch.empty(B, T, w.shape[0], device=DEV)
        epi = ("linear_bias", "linear_gelu", "linear_relu", "linear_residual").index(stage)
        _lib.check(lib.wetts_frontend_linear(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(res), B * T, K, w.shape[0], epi,
                                             _lib.ptr(out), s), stage)
        return out
    if stage == "add_layer_norm":
        x, res = i["x"].to(DEV).contiguous(), i["res"].to(DEV).contiguous()
        out = torch.empty_like(x)
        _lib.check(lib.wetts_frontend_add_layer_norm(_lib.ptr(x), _lib.ptr(res), _lib.ptr(_w(cname, i["name"] + ".weight")),
                                                     _lib.ptr(_w(cname, i["name"] + ".bias")), cfg["layer_norm_eps"],
                                                     x.shape[0] * x.shape[1], d, _lib.ptr(out), s), stage)
        return out
    if stage.startswith("attention_"):
        qkv, mf = i["qkv"].to(DEV).contiguous(), i["mask"].to(DEV, torch.float32).contiguous()
        B, T, _ = qkv.shape
        out = torch.empty(B, T, d, device=DEV)
        _lib.check(lib.wetts_frontend_attention(_lib.ptr(qkv), _lib.ptr(mf), B, T, i["heads"], d // i["heads"], _lib.ptr(out),
                                                s), stage)
        return out
    x, mf = i["x"].to(DEV).contiguous(), i["mask"].to(DEV, torch.float32).contiguous()
    B, T, _ = x.shape
    ph, pr = torch.empty(B, T, fo.NUM_POLYPHONES, device=DEV), torch.empty(B, T, fo.NUM_PROSODY, device=DEV)
    _lib.check(lib.wetts_frontend_heads(net._handle, _lib.ptr(x), _lib.ptr(mf), B * T, 1 if stage == "heads_probs" else 0,
                                        _lib.ptr(ph), _lib.ptr(pr), s), stage)
    return torch.cat([ph, pr], 2)


@pytest.mark.parametrize("cname,lens", CASES)
def test_every_stage_against_float64_oracle(cname, lens):
    c = fo.load_fixture(cname, lens)
    ids, mask, _ = fo.reference(cname, lens)
    W64 = fo.weights(cname)[1]
    figs = {}
    with torch.cuda.device(0):
        for stage, (i, fn) in fo.stage_cases(cname, ids, mask).items():
            got = _run_stage(cname, stage, i)
            torch.cuda.synchronize()
            figs[stage] = fo.gates(got.cpu(), fn(W64, i))
    assert set(figs) == set(fo.STAGES)
    _check(figs, c, f"stages {fo.case_name(cname, lens)}")


# ---- 3. the forward pass -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,lens", CASES)
def test_forward_against_float64_oracle_and_padded_zeros(cname, lens):
    c = fo.load_fixture(cname, lens)
    ids, mask, st64 = fo.reference(cname, lens)
    net = _net(cname)
    lp, lr = net({"input_ids": ids, "token_type_ids": torch.zeros_like(ids), "attention_mask": mask})
    pp, pr = net.probs(ids, mask)
    got = {k: v.cpu() for k, v in dict(phone_logits=lp, prosody_logits=lr, phone_prob=pp, prosody_prob=pr).items()}
    figs = {k: fo.gates(fo.valid(got[k], mask), fo.valid(st64[k], mask)) for k in fo.OUTPUTS}
    _check(figs, c, f"forward {fo.case_name(cname, lens)}")
    for k in fo.OUTPUTS:  # padded tokens: zeros, bit for bit
        assert not bool(got[k][mask == 0].view(torch.int32).any()), k
    # softmax = 1 is the softmax of what softmax = 0 returns: within the stand-alone heads' gate of the float64 softmax
    for lg, pb in (("phone_logits", "phone_prob"), ("prosody_logits", "prosody_prob")):
        want = torch.softmax(fo.valid(got[lg], mask).double(), -1)
        assert fo.within(fo.gates(fo.valid(got[pb], mask), want), fo.gate(c["floor_heads_probs"])), pb
        assert bool(((fo.valid(got[pb], mask).double().sum(1) - 1).abs() < 1e-5).all())


@pytest.mark.parametrize("cname", fo.CONFIGS)
@pytest.mark.parametrize("lens", [s for s in fo.FIXTURE_SHAPES if len(s) > 1])
def test_row_alone_equals_the_row_in_the_padded_batch_bit_for_bit(cname, lens):
    ids, mask = fo.inputs(lens, 4242)
    net = _net(cname)
    batch = [t.clone() for t in net({"input_ids": ids, "attention_mask": mask})] + list(net.probs(ids, mask))
    again = list(net({"input_ids": ids, "attention_mask": mask})) + list(net.probs(ids, mask))
    for a, b in zip(batch, again):
        assert torch.equal(a, b)
    for b, n in enumerate(lens):
        alone = list(net({"input_ids": ids[b:b + 1, :n]})) + list(net.export_forward(ids[b:b + 1, :n]))
        for k, (a, full) in enumerate(zip(alone, batch)):
            assert torch.equal(a[0], full[b, :n]), (b, k)


@pytest.mark.parametrize("cname", fo.CONFIGS)
def test_a_fully_masked_row_gives_zeros_and_disturbs_no_other_row(cname):
    ids, mask = fo.inputs((9, 6), 4243)
    mask[1] = 0
    net = _net(cname)
    lp, lr = net({"input_ids": ids, "attention_mask": mask})
    pp, pr = net.probs(ids, mask)
    alone = list(net({"input_ids": ids[:1]})) + list(net.export_forward(ids[:1]))
    for got, a in zip((lp, lr, pp, pr), alone):
        assert bool(torch.isfinite(got).all()) and not bool(got[1].any()) and torch.equal(got[0], a[0])


# ---- 4. errors -------------------------------------------------------------------------------------------------------------
def test_out_of_range_ids_raise_index_error_and_a_clean_call_follows():
    net = _net("tiny")
    ids, mask = fo.inputs((9, 6), 11)
    clean = [t.clone() for t in net.probs(ids, mask)]
    for bad in (fo.VOCAB, -1):
        x = ids.clone()
        x[1, 2] = bad
        with pytest.raises(IndexError):
            net({"input_ids": x, "attention_mask": mask})
    with pytest.raises(IndexError):
        net({"input_ids": ids, "token_type_ids": torch.full_like(ids, 2), "attention_mask": mask})
    for a, b in zip(net.probs(ids, mask), clean):
        assert torch.equal(a, b)


def test_too_many_positions_and_empty_shapes_are_refused_before_any_launch():
    net = _net("tiny")
    with pytest.raises(ValueError, match="81"):
        net({"input_ids": torch.full((1, fo.POSITIONS + 1), 5)})
    with pytest.raises(ValueError):
        net({"input_ids": torch.zeros(0, 4, dtype=torch.int64)})
    with pytest.raises(ValueError):
        net({"input_ids": torch.zeros(2, 0, dtype=torch.int64)})
    with pytest.raises(AssertionError):
        net.export_forward(torch.full((2, 4), 5))
    # the library's own host check: the outputs keep their contents
    lib = _lib.load()
    T = fo.POSITIONS + 1
    ids = torch.full((1, T), 5, device=DEV)
    ph = torch.full((1, T, fo.NUM_POLYPHONES), 7.0, device=DEV)
    pr = torch.full((1, T, fo.NUM_PROSODY), 7.0, device=DEV)
    ws = torch.empty(int(lib.wetts_frontend_workspace_bytes(net._handle, 1, T)) // 4, device=DEV)
    for B, t in ((1, T), (0, 4), (1, 0)):
        rc = lib.wetts_frontend_forward(net._handle, _lib.ptr(ids), None, None, B, t, 0, _lib.ptr(ph), _lib.ptr(pr), _lib.ptr(ws),
                                        None, _lib.current_stream_ptr())
        assert rc == -1, (B, t, rc)
    torch.cuda.synchronize()
    assert bool((ph == 7.0).all()) and bool((pr == 7.0).all())
    assert lib.wetts_frontend_workspace_bytes(net._handle, 0, 4) < 0


# ---- 5. session, decisions, synthesis ----------------------------------------------------------------------------------------
def test_session_run_equals_export_forward():
    net = _net("base")
    sess = FrontendSession(net)
    ids, _ = fo.inputs((33,), 12)
    out = sess.run(None, {"input": ids.numpy()})
    want = net.export_forward(ids)
    assert len(out) == 2 and all(isinstance(o, np.ndarray) and o.dtype == np.float32 for o in out)
    assert np.array_equal(out[0], want[0].cpu().numpy()) and np.array_equal(out[1], want[1].cpu().numpy())
    assert out[0].shape == (1, 33, fo.NUM_POLYPHONES) and out[1].shape == (1, 33, fo.NUM_PROSODY)
    assert [i.name for i in sess.get_inputs()] == ["input"]
    assert [o.name for o in sess.get_outputs()] == ["polyphone_output", "prosody_output"]
    assert np.array_equal(sess.run(["prosody_output"], {"input": ids.numpy()})[0], out[1])
    with pytest.raises(ValueError):
        sess.run(["nope"], {"input": ids.numpy()})


def test_decisions_on_the_device_follow_the_tie_rules():
    """wetts_frontend_decide on prepared probabilities: the first of equal candidates, the lowest of equal prosody
    classes, candidates in the given order (not by class id)."""
    lib = _lib.load()
    N, P, R, K = 5, 6, 5, 4
    pp = torch.tensor([[.1, .2, .3, .4, .5, .6], [.5, .5, .5, .5, .5, .5], [.1, .9, .1, .9, .1, .1], [.3, .2, .1, .0, .0, .0],
                       [.0, .0, .0, .0, .0, 1.]], device=DEV)
    pr = torch.tensor([[.2, .2, .2, .2, .2], [.1, .4, .4, .1, .0], [.0, .0, .0, .0, 1.], [.3, .1, .3, .3, .0],
                       [.1, .2, .3, .4, .0]], device=DEV)
    cand = torch.tensor([[5, 0, -1, -1], [4, 2, 0, -1], [3, 1, 0, 2], [2, 1, 0, -1], [-1, -1, -1, -1]], dtype=torch.int32,
                        device=DEV)
    clen = torch.tensor([2, 3, 4, 3, 0], dtype=torch.int32, device=DEV)
    ch, ps = torch.full((N,), -7, dtype=torch.int32, device=DEV), torch.full((N,), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.wetts_frontend_decide(_lib.ptr(pp), _lib.ptr(pr), _lib.ptr(cand), _lib.ptr(clen), N, P, R, K, _lib.ptr(ch),
                                         _lib.ptr(ps), _lib.current_stream_ptr()), "decide")
    assert ch.tolist() == [0, 0, 0, 2, 0] and ps.tolist() == [0, 1, 4, 0, 3]


def test_model_synthesis_on_the_toy_lexicon(tmp_path_factory):
    """The README example: text -> phonemes -> int16 audio, with the length infer() gives for the same phonemes and seed."""
    front = _front_dir("tiny", tmp_path_factory)
    phone_table = os.path.join(fo.TOY, "phones.txt")
    n_vocab = sum(1 for _ in open(phone_table))
    cfg = config.make_config(config.MODEL_CONFIGS["tiny"], n_vocab, 2)
    net = SynthesizerTrn(n_vocab, 513, 32, n_speakers=2, **config.MODEL_CONFIGS["tiny"])
    net.load_state_dict(synth.make_state_dict(cfg, 3)).to(DEV)
    model = Model(InferenceSession(net), phone_table, os.path.join(fo.TOY, "speaker.txt"), front)
    text = "今天天气怎么样"
    torch.manual_seed(1234)
    phonemes, audio = model.synthesis(text, "default")
    assert phonemes == front.compute(text) and phonemes[0] == "sil" and phonemes[-1] == "#4"
    assert isinstance(audio, np.ndarray) and audio.dtype == np.int16 and audio.ndim == 1
    x = torch.tensor([[model.phone2id[p] for p in phonemes]], device=DEV)
    torch.manual_seed(1234)
    o, *_ = net.infer(x, torch.tensor([x.shape[1]], device=DEV), sid=torch.tensor([0], device=DEV), noise_scale=0.667,
                      length_scale=1.0, noise_scale_w=0.8)
    assert audio.shape[0] == o.shape[2] > 0
    assert np.array_equal(audio, (o[0, 0].cpu().numpy() * 32767).astype(np.int16))
