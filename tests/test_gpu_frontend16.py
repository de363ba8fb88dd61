"""GPU tier of the text frontend's 16-bit mode (csrc/frontend16.hip, FrontendModel.set_dtype), against the spec of
tests/frontend16_oracle.py: every Linear launch alone in every kernel form against float64 on the rounded operands (gate
1 per element, gate 2 against torch's float32 floor), forward() and score() end to end within 3 x D of the full float64
model, the decisions, determinism, and switching the mode.  Kernel forms: 1 = K split (64 tokens per block), 2 / 3 =
tiled GEMM (64 / 128 tokens per block); the launcher takes 1 up to 64 tokens, beyond them 3 where its grid
ceil(M / 128) * ceil(N / 128) has 512 blocks and 2 otherwise."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import frontend16_oracle as f16o
from tests import frontend_oracle as fo
from tests import frontend_score_oracle as so
from wetts_amd import Frontend, FrontendModel, FrontendSession, Model, SynthesizerTrn, _lib, config, synth
from wetts_amd.session import InferenceSession

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(c, lens) for c in fo.CONFIGS for lens in fo.FIXTURE_SHAPES]
TYPES = list(f16o.DTYPES)
_NET, _MARGINS, _LEFT_OUT = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_and_report():
    yield
    import gc
    _NET.clear()
    fo._REF.clear()
    f16o._D.clear()
    f16o._STAGE.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = os.environ.get("WETTS_FRONTEND16_MARGINS")  # the GPU run that records profiles/frontend16_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst multiple of each gate per case (1 = at the gate).  launches: (gate 1 = (K + 4) 2^-24 S per element, "
                    "gate 2 = 4 x torch's float32 floor on the same rounded operands); forward: multiples of D, the mode's own "
                    "precision loss (gate 3); score: (phone, prosody) relative error of the loss against the float64 model's in "
                    "multiples of D_rel of the head's logits (gate 3); decisions: share of tokens left out (gate 0.15), wrong "
                    "among the kept\n")
            for k in sorted(_MARGINS):
                f.write(f"{k}: {_MARGINS[k]}\n")


def _net(cname, tname="f32"):
    if (cname, tname) not in _NET:
        _NET[(cname, tname)] = FrontendModel(fo.NUM_POLYPHONES, fo.NUM_PROSODY, fo.BERT_CONFIGS[cname]) \
            .load_state_dict(fo.weights(cname)[0]).to(DEV).set_dtype(tname)
    return _NET[(cname, tname)]


def _linear16(x, w, b, res, epi, tname, form):
    """wetts_frontend_linear16 on float32 host tensors -> the output on the host."""
    lib = _lib.load()
    N, K = x.shape
    M = w.shape[0]
    xd, wd, bd = x.to(DEV).contiguous(), w.to(DEV).contiguous(), b.to(DEV).contiguous()
    rd = res.to(DEV).contiguous() if res is not None else None
    nbytes = int(lib.wetts_frontend_linear16_workspace_bytes(K, M))
    assert nbytes == 2 * K * M
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=DEV)
    out = torch.full((N, M), float("nan"), device=DEV)
    _lib.check(lib.wetts_frontend_linear16(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(rd), N, K, M, epi,
                                           f16o.PRECISION[tname], form, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                           _lib.current_stream_ptr()), "frontend_linear16")
    torch.cuda.synchronize()
    return out.cpu()


def _record(tag, m1, m2):
    old = _MARGINS.get(tag, (0.0, 0.0))
    _MARGINS[tag] = (round(max(old[0], m1 or 0.0), 3), round(max(old[1], m2), 3))


# ---- 1. every Linear launch alone -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("cname,lens", CASES)
def test_stage_launches_in_every_form_against_float64_on_the_rounded_operands(cname, lens, tname):
    """The four Linear stages of frontend_oracle.stage_cases (N = 3, 18, 99, 195, 80; K = 312 / 768 / 256; M = 936 / 1200 /
    312 / 2304 / 2048), the launcher's choice and each forced form."""
    dtype = f16o.DTYPES[tname]
    launches = f16o.stage_launches(cname, lens)
    assert set(launches) == set(f16o.EPILOGUES)
    bad = []
    for stage, (x, w, b, res) in launches.items():
        epi = f16o.EPILOGUES.index(stage)
        ref = f16o.launch_reference(x, w, b, res, dtype, epi)
        for form in (0, 1, 2, 3):
            m = f16o.launch_multiples(_linear16(x, w, b, res, epi, tname, form), x, w, b, res, dtype, epi, ref)
            print(fo.case_name(cname, lens), tname, stage, "form", form, "gate 1 x", m[0], "gate 2 x", round(m[1], 3))
            _record(f"launch {tname} form{form} {stage}", *m)
            if not f16o.launch_ok(m):
                bad.append((stage, form, m))
    assert not bad, bad


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("form", sorted(f16o.FORM_TILE), ids=lambda f: f"form{f}")
def test_seeded_launches_at_the_tile_edges_of_a_form(form, tname):
    """N in {1, tile - 1, tile, tile + 1, 2 tile + 3} x (K, M) in {(8, 4), (24, 36), (312, 312), (1200, 312), (768, 100)}:
    the smallest shape, K % 16 == 8 and K % 32 != 0 tails, M % 32 != 0 and M < one row tile, more than one block."""
    dtype, tile = f16o.DTYPES[tname], f16o.FORM_TILE[form]
    bad = []
    for N in f16o.edge_tokens(tile):
        for K, M in f16o.EDGE_KM:
            x, w, b, res = f16o.random_launch(N, K, M, 1000 * form + N + K + M)
            for epi in range(4):
                r = res if epi == 3 else None
                m = f16o.launch_multiples(_linear16(x, w, b, r, epi, tname, form), x, w, b, r, dtype, epi)
                _record(f"edges {tname} form{form} {f16o.EPILOGUES[epi]}", *m)
                if not f16o.launch_ok(m):
                    bad.append((N, K, M, epi, m))
    print("form", form, tname, {k: v for k, v in _MARGINS.items() if k.startswith(f"edges {tname} form{form}")})
    assert not bad, bad


@pytest.mark.parametrize("tname", TYPES)
def test_the_launcher_takes_each_form_on_its_side_of_the_thresholds(tname):
    """Form 1 up to 64 tokens; beyond them form 3 where ceil(M / 128) ceil(N / 128) >= 512 (M = 1024: from 63 x 128 + 1
    tokens) and form 2 below.  The library names its choice (wetts_frontend_linear16_form, the function form 0 goes
    through), and form 0 gives that form's bits.  K = 312 = 20 MFMA steps: the K split adds them in another order than
    the tiles, so its bits differ from theirs (asserted: the comparison can fail).  The two tiles add an element's steps
    in the same order and give the same bits (asserted too), so between them the named choice is what is checked here;
    test_a_batch_on_the_128_token_tile_gives_the_bits_of_its_halves_on_the_64_token_tile runs form 3 end to end."""
    lib = _lib.load()
    for N, M, form in ((64, 36, 1), (65, 36, 2), (63 * 128, 1024, 2), (63 * 128 + 1, 1024, 3)):
        assert lib.wetts_frontend_linear16_form(N, M) == form, (N, M)
        x, w, b, res = f16o.random_launch(N, 312, M, 50 + N)
        bits = {f: _linear16(x, w, b, res, 3, tname, f).view(torch.int32) for f in (0, 1, 2, 3)}
        assert torch.equal(bits[0], bits[form]), (N, M, form)
        assert not torch.equal(bits[1], bits[2]) and torch.equal(bits[2], bits[3]), (N, M)


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("form", sorted(f16o.FORM_TILE), ids=lambda f: f"form{f}")
def test_a_launch_repeats_its_bits_and_permuted_rows_permute_them(form, tname):
    """Every form on its own, across its block edges: an output row is a function of its own token alone."""
    N = 2 * f16o.FORM_TILE[form] + 3
    x, w, b, res = f16o.random_launch(N, 312, 100, 77 + form)
    first = _linear16(x, w, b, res, 3, tname, form).view(torch.int32)
    assert torch.equal(_linear16(x, w, b, res, 3, tname, form).view(torch.int32), first)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    assert torch.equal(_linear16(x[perm], w, b, res[perm], 3, tname, form).view(torch.int32), first[perm])


def test_an_f16_operand_out_of_range_is_infinite_as_ieee_says():
    x, w, b, _ = f16o.random_launch(5, 16, 8, 3)
    x[2, 3] = 1e5  # beyond 65504: +inf at f16, finite at bf16
    y16 = _linear16(x, w, b, None, 0, "f16", 1)
    assert not bool(torch.isfinite(y16[2]).any()) and bool(torch.isfinite(y16[[0, 1, 3, 4]]).all())
    assert bool(torch.isfinite(_linear16(x, w, b, None, 0, "bf16", 1)).all())


# ---- 2. forward and score end to end ----------------------------------------------------------------------------------------
def _forward(net, ids, mask):
    lp, lr = net({"input_ids": ids, "attention_mask": mask})
    pp, pr = net.probs(ids, mask)
    return {k: v.cpu() for k, v in dict(phone_logits=lp, prosody_logits=lr, phone_prob=pp, prosody_prob=pr).items()}


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("cname,lens", CASES)
def test_forward_and_score_within_three_d_of_the_float64_model(cname, lens, tname):
    D, ids, mask, st64 = f16o.precision_loss(cname, lens, tname)
    net = _net(cname, tname)
    got = _forward(net, ids, mask)
    mult = f16o.e2e_multiples(got, st64, mask, D)
    worst = f16o.e2e_worst(mult)
    print(fo.case_name(cname, lens), tname, {k: tuple(round(x, 3) for x in v) for k, v in mult.items()})
    _MARGINS[f"forward {tname} {fo.case_name(cname, lens)}"] = (round(worst, 3), {k: tuple(round(x, 3) for x in v) for k, v in mult.items()})
    assert worst <= f16o.E2E_FACTOR, mult
    for k in fo.OUTPUTS:  # padded tokens: zeros, bit for bit
        assert not bool(got[k][mask == 0].view(torch.int32).any()), k
    # score(): labels around the float64 model's own predictions
    P, R = fo.NUM_POLYPHONES, fo.NUM_PROSODY
    z64 = (st64["phone_logits"], st64["prosody_logits"])
    pl, rl = so.make_labels(lens, fo.case_seed(lens), so.head(z64[0], mask, None)[1], so.head(z64[1], mask, None)[1], P, R)
    s = net.score({"input_ids": ids, "attention_mask": mask}, pl, rl)
    h = s.host()
    # the same relative gate as the logits': |loss - loss64| / |loss64| <= 3 x D_rel of the head's logits
    mults = []
    for name, z, lab, loss in (("phone_logits", z64[0], pl, h.phone_loss), ("prosody_logits", z64[1], rl, h.prosody_loss)):
        want = float(so.head(z, mask, lab)[2])
        mults.append(abs(loss - want) / abs(want) / max(D[name][0], fo.HALF_ULP))
        print(name, "loss", loss, "float64", want, "relative error in multiples of D_rel", round(mults[-1], 3))
    _MARGINS[f"score {tname} {fo.case_name(cname, lens)}"] = tuple(round(m, 3) for m in mults)
    assert max(mults) <= f16o.E2E_FACTOR, mults
    # the integer counts are the counts of the device's own predictions
    pp, pr = s.pred_phone.cpu().to(torch.int64), s.pred_prosody.cpu().to(torch.int64)
    assert bool((pp[mask == 0] == -1).all()) and bool((pr[mask == 0] == -1).all())
    want = [int((pl != so.IGNORE_ID).sum()), int(((pp == pl) & (pl != so.IGNORE_ID)).sum()),
            int((rl != so.IGNORE_ID).sum()), int(((pr == rl) & (rl != so.IGNORE_ID)).sum())] + \
        so.f1_counts(pr, rl, False) + so.f1_counts(pr, rl, True)
    assert h.counts == [int(v) for v in want]


# ---- 3. decisions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("cname", fo.CONFIGS)
def test_decisions_equal_the_float64_models_where_its_margin_exceeds_the_gate(cname, tname):
    """Device argmax of phone_prob / prosody_prob = the float64 model's at every token whose float64 top-two margin
    exceeds 2 x (3 D_local rms(ref)); closer tokens are left out, at most 15 % of them per config over the five shapes."""
    kept = left = wrong = 0
    for lens in fo.FIXTURE_SHAPES:
        D, ids, mask, st64 = f16o.precision_loss(cname, lens, tname)
        pp, pr = _net(cname, tname).probs(ids, mask)
        for k, got in (("phone_prob", pp), ("prosody_prob", pr)):
            ref = fo.valid(st64[k], mask)
            top = ref.topk(2, dim=-1).values
            rms = float(ref.pow(2).mean().sqrt())
            sure = (top[:, 0] - top[:, 1]) > 2 * f16o.E2E_FACTOR * D[k][1] * rms
            same = fo.valid(got.cpu(), mask).argmax(-1) == ref.argmax(-1)
            kept, left, wrong = kept + int(sure.sum()), left + int((~sure).sum()), wrong + int((sure & ~same).sum())
    share = left / (kept + left)
    print(cname, tname, "kept", kept, "left out", left, "share", round(share, 4), "wrong among the kept", wrong)
    _MARGINS[f"decisions {tname} {cname}"] = (round(share, 4), wrong)
    assert wrong == 0 and share <= 0.15


def _front_dir(cname, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("front16_" + cname))
    shutil.copy(os.path.join(fo.TOY, "vocab.txt"), d)
    shutil.copytree(os.path.join(fo.TOY, "lexicon"), os.path.join(d, "lexicon"))
    torch.save(fo.weights(cname)[0], os.path.join(d, "final.pt"))
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(fo.BERT_CONFIGS[cname], f)
    return d


def test_model_synthesis_runs_in_bf16_on_the_toy_lexicon(tmp_path_factory):
    d = _front_dir("tiny", tmp_path_factory)
    f32, bf16 = Frontend(d), Frontend(d, dtype=torch.bfloat16)
    assert f32.model.dtype == torch.float32 and bf16.model.dtype == torch.bfloat16
    assert FrontendSession(d, dtype="f16").model.dtype == torch.float16
    phone_table = os.path.join(fo.TOY, "phones.txt")
    n_vocab = sum(1 for _ in open(phone_table))
    cfg = config.make_config(config.MODEL_CONFIGS["tiny"], n_vocab, 2)
    net = SynthesizerTrn(n_vocab, 513, 32, n_speakers=2, **config.MODEL_CONFIGS["tiny"])
    net.load_state_dict(synth.make_state_dict(cfg, 3)).to(DEV)
    text = "今天天气怎么样"
    out = []
    for front in (f32, bf16):
        torch.manual_seed(1234)
        phonemes, audio = Model(InferenceSession(net), phone_table, os.path.join(fo.TOY, "speaker.txt"), front).synthesis(text)
        assert phonemes[0] == "sil" and phonemes[-1] == "#4" and audio.dtype == np.int16 and audio.ndim == 1 and audio.size > 0
        out.append(phonemes)
    assert len(out[0]) == len(out[1])
    assert bf16.compute_batch([text, text[:3]])[0] == out[1]


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("cname,lens", [("tiny", (9, 6)), ("base", (33, 32, 31)), ("tiny", (65, 64, 63)),
                                        ("tiny", (80,) * 25 + (41,))], ids=["form1", "form2-base", "form2-tiny", "form2-wide"])
def test_repeats_row_permutations_and_padding_contents_leave_the_bits(cname, lens, tname):
    """18, 99 and 195 tokens (the K-split and the 64-token tile) and 26 x 80 = 2080 tokens (17 column blocks of 64)."""
    ids, mask = fo.inputs(lens, 4242)
    net = _net(cname, tname)
    first = _forward(net, ids, mask)
    again = _forward(net, ids, mask)
    for k in fo.OUTPUTS:
        assert torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)), k
    perm = torch.tensor(list(range(1, len(lens))) + [0])
    moved = _forward(net, ids[perm], mask[perm])
    for k in fo.OUTPUTS:
        assert torch.equal(moved[k].view(torch.int32), first[k][perm].view(torch.int32)), k
    other = torch.where(mask == 0, torch.randint(5, 45, ids.shape, generator=torch.Generator().manual_seed(7)), ids)
    assert not torch.equal(other, ids)
    padded = _forward(net, other, mask)
    for k in fo.OUTPUTS:
        assert torch.equal(padded[k].view(torch.int32), first[k].view(torch.int32)), k


@pytest.mark.parametrize("tname", TYPES)
def test_a_batch_on_the_128_token_tile_gives_the_bits_of_its_halves_on_the_64_token_tile(tname):
    """Form 3 through the forward pass.  The fixture shapes stay below its threshold, so 82 x 80 = 6560 tokens of the tiny
    config: 52 column blocks of 128, times the 10 row blocks of the three M = 1200 Linears (feed-forward in of both
    layers and of `transform`) = 520 blocks >= 512.  Either half, 41 x 80 = 3280 tokens, runs every Linear on the
    64-token tile.  Both tiles add an element's k steps in the same order and every other kernel treats a row by
    itself, so the whole batch gives the bits of its halves -- which the fixture cases hold to the float64 model."""
    lib, c = _lib.load(), fo.config("tiny")
    d, wide = c["hidden_size"], c["intermediate_size"]
    assert wide == c["transform_ff"] == 1200
    lens = tuple(80 - i % 7 for i in range(82))
    ids, mask = fo.inputs(lens, 808)
    B, T = ids.shape
    assert lens[41:].count(80) and [lib.wetts_frontend_linear16_form(B * T, M) for M in (3 * d, d, wide)] == [2, 2, 3]
    assert {lib.wetts_frontend_linear16_form(41 * T, M) for M in (3 * d, d, wide)} == {2}
    net = _net("tiny", tname)
    whole = _forward(net, ids, mask)
    halves = [_forward(net, ids[r], mask[r]) for r in (slice(0, 41), slice(41, 82))]
    for k in fo.OUTPUTS:
        assert bool(whole[k][mask != 0].abs().sum() > 0), k
        assert torch.equal(whole[k].view(torch.int32), torch.cat([h[k] for h in halves]).view(torch.int32)), k


# ---- 5. switching the mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", fo.CONFIGS)
def test_f32_after_bf16_is_the_f32_of_a_handle_that_never_left_it(cname):
    lib = _lib.load()
    ids, mask = fo.inputs((33, 32, 31), 99)
    never = _forward(_net(cname), ids, mask)
    net = FrontendModel(fo.NUM_POLYPHONES, fo.NUM_PROSODY, fo.BERT_CONFIGS[cname]).load_state_dict(fo.weights(cname)[0]).to(DEV)
    B, T = ids.shape
    sizes = [(int(lib.wetts_frontend_workspace_bytes(net._handle, B, T)), int(lib.wetts_frontend_score_workspace_bytes(net._handle, B, T)))]
    assert lib.wetts_frontend_get_precision(net._handle) == 0
    net.set_dtype(torch.bfloat16)
    assert lib.wetts_frontend_get_precision(net._handle) == 1
    sizes.append((int(lib.wetts_frontend_workspace_bytes(net._handle, B, T)), int(lib.wetts_frontend_score_workspace_bytes(net._handle, B, T))))
    there = _forward(net, ids, mask)
    assert not torch.equal(there["phone_logits"], never["phone_logits"])  # the mode is really on
    # a refused request leaves the mode as it is
    assert lib.wetts_frontend_set_precision(net._handle, 3) == -1 and lib.wetts_frontend_get_precision(net._handle) == 1
    with pytest.raises(ValueError):
        net.set_dtype("int8")
    still = _forward(net, ids, mask)
    assert net.dtype == torch.bfloat16 and torch.equal(still["phone_logits"].view(torch.int32), there["phone_logits"].view(torch.int32))
    net.set_dtype("f16")
    assert lib.wetts_frontend_get_precision(net._handle) == 2
    net.set_dtype(torch.float32)
    assert lib.wetts_frontend_get_precision(net._handle) == 0
    sizes.append((int(lib.wetts_frontend_workspace_bytes(net._handle, B, T)), int(lib.wetts_frontend_score_workspace_bytes(net._handle, B, T))))
    assert sizes[2] == sizes[0] and all(min(s) > 0 for s in sizes)
    back = _forward(net, ids, mask)
    for k in fo.OUTPUTS:
        assert torch.equal(back[k].view(torch.int32), never[k].view(torch.int32)), k


def test_layer_entry_follows_the_mode():
    """wetts_frontend_layer in bf16 = the layer of the forward pass: layer 0 on the embeddings, against the float64 spec."""
    cname, lens = "tiny", (33, 32, 31)
    lib, s = _lib.load(), _lib.current_stream_ptr()
    ids, mask, _ = fo.reference(cname, lens)
    W64 = fo.weights(cname)[1]
    c = fo.config(cname)
    B, T = ids.shape
    h0 = fo.embed(W64, ids, torch.zeros_like(ids), c["layer_norm_eps"])
    lin = lambda x, w, b: f16o.linear16(x, w, b, torch.bfloat16)  # noqa: E731
    want = f16o._block16(W64, fo.bert_block_names(W64, 0), h0, mask, c["num_heads"], fo.gelu, c["layer_norm_eps"], lin)
    full = fo.block(W64, fo.bert_block_names(W64, 0), h0, mask, c["num_heads"], fo.gelu, c["layer_norm_eps"])
    outs = {}
    for tname in ("f32", "bf16"):
        net = _net(cname, tname)
        x = h0.to(torch.float32).to(DEV).contiguous()
        mf = mask.to(DEV, torch.float32).contiguous()
        ws = torch.empty(int(lib.wetts_frontend_workspace_bytes(net._handle, B, T)) // 4, device=DEV)
        _lib.check(lib.wetts_frontend_layer(net._handle, 0, _lib.ptr(x), _lib.ptr(mf), B, T, _lib.ptr(ws), s), "frontend_layer")
        torch.cuda.synchronize()
        outs[tname] = fo.valid(x.cpu(), mask)
    D = fo.gates(fo.valid(want, mask), fo.valid(full, mask))
    fig = fo.gates(outs["bf16"], fo.valid(full, mask))
    print("layer 0 bf16", fig, "D", D)
    assert fig[0] <= f16o.E2E_FACTOR * D[0] and fig[1] <= f16o.E2E_FACTOR * D[1]
    assert fo.gates(outs["f32"], fo.valid(full, mask))[0] < 0.01 * D[0]  # the f32 handle next to it is untouched
