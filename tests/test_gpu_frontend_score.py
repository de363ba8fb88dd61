"""GPU tier of the frontend's scoring (csrc/frontend_score.hip, FrontendModel.score, wetts_amd.frontend_eval): the
reference's fixtures (tests/golden/frontend_score_*.npz) and the float64 oracle of tests/frontend_score_oracle.py under the
gates of frontend_oracle (4 x the stored float32 floor against the oracle, 4 + 1 floors against the reference's float32),
predictions and all 22 counts for equality; the stage entry on the oracle's x; the bit-exact conditions (repeats, a row
alone, a permutation of rows, forward()'s argmax, exact ties); the conventions (an empty head, None labels, the two label
errors) and the three subcommands of frontend_eval on the toy directory.  Tiles: 32 classes x 64 tokens per block;
(34, 5) gives a ragged class tile of 2 and a prosody tile with 27 clamped rows, (470, 5) fourteen full tiles and one of
22; N = 3, 15, 99, 195 tokens leave the token tiles ragged."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import frontend_oracle as fo
from tests import frontend_score_oracle as so
from tests.golden.make_golden_disc import state_dict_digest
from tests.golden.make_golden_frontend import inputs_digest
from wetts_amd import FrontendModel, _lib, frontend_eval

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = fo.NUM_PROSODY
_NET, _RUN, _MARGINS = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_and_report():
    yield
    import gc
    _NET.clear()
    _RUN.clear()
    so._REF.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = os.environ.get("WETTS_FRONTEND_SCORE_MARGINS")  # the GPU run that records profiles/frontend_score_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst multiple of a gate per case (1 = at the gate; gate = 4 x floor against the float64 oracle, 5 x floor "
                    "against the reference's float32), then the (rel, local) figures\n")
            for k in sorted(_MARGINS):
                f.write(f"{k}: {_MARGINS[k]}\n")


def _net(cname, P, sd=None, key=None):
    k = (cname, P, key)
    if k not in _NET:
        _NET[k] = FrontendModel(P, R, fo.BERT_CONFIGS[cname]).load_state_dict(sd or so.weights(cname, P)[0]).to(DEV)
    return _NET[k]


def _run(cname, P, lens):
    """(fixture, ids, mask, phone labels, prosody labels, FrontendScores, HostScores) of a case, scored once."""
    k = (cname, P, tuple(lens))
    if k not in _RUN:
        c = so.load_fixture(cname, P, lens)
        ids, mask, pl, rl, _, _ = so.reference(cname, P, lens)
        s = _net(cname, P).score({"input_ids": ids, "attention_mask": mask}, pl, rl)
        _RUN[k] = (c, ids, mask, pl, rl, s, s.host())
    return _RUN[k]


def _figs(d):
    return {k: tuple(float(f"{x:.3g}") for x in v) for k, v in d.items()}


def _check(figs, c, tag, fixture=False):
    top = 0.0
    gate = fo.fixture_gate if fixture else fo.gate
    for k, v in figs.items():
        g = gate(c["floor_" + k])
        top = max(top, v[0] / g[0], v[1] / g[1])
    print(tag, _figs(figs), "worst multiple of a gate", round(top, 3))
    _MARGINS[tag] = (round(top, 3), _figs(figs))
    for k, v in figs.items():
        g = gate(c["floor_" + k])
        assert fo.within(v, g), f"{tag} {k}: rel {v[0]:.3e} (gate {g[0]:.3e}) local {v[1]:.3e} (gate {g[1]:.3e})"


def _figures(nll_p, nll_r, losses, pl, rl, want_p, want_r, want_losses):
    """{key: (rel, local)} of the per-token nll at the labelled tokens and of the two losses; a head without labels has
    to give NaN where the reference gives NaN and carries no figure."""
    figs = {}
    for hd, lab, got, want, k in (("phone", pl, nll_p, want_p, 0), ("prosody", rl, nll_r, want_r, 1)):
        if int((lab != so.IGNORE_ID).sum()) == 0:
            assert np.isnan(float(losses[k])) and np.isnan(float(want_losses[k])), hd
            continue
        figs["nll_" + hd] = fo.gates(so.labelled(got, lab), want)
        figs["loss_" + hd] = fo.gates(torch.tensor([float(losses[k])], dtype=torch.float64),
                                      torch.tensor([float(want_losses[k])], dtype=torch.float64))
    return figs


# ---- 1. the reference's fixtures and the float64 oracle ----------------------------------------------------------------
@pytest.mark.parametrize("cname,P,lens", so.CASES)
def test_score_matches_reference_fixture(cname, P, lens):
    c, ids, mask, pl, rl, s, h = _run(cname, P, lens)
    assert state_dict_digest(so.weights(cname, P)[0]) == str(c["state_dict_sha256"])
    assert inputs_digest(ids, mask) == str(c["inputs_sha256"]) and int(c["decisions_stable"]) == 1
    figs = _figures(s.nll_phone.cpu(), s.nll_prosody.cpu(), (h.phone_loss, h.prosody_loss), pl, rl,
                    torch.from_numpy(c["nll_phone"]), torch.from_numpy(c["nll_prosody"]), c["losses"])
    _check(figs, c, f"fixture {so.case_name(cname, P, lens)}", fixture=True)
    assert h.counts == c["counts"].tolist()
    assert s.counts.cpu().tolist() == h.counts and (h.num_total, h.num_correct) == (h.counts[0], h.counts[1])
    for ex in (False, True):
        assert np.allclose(h.f1(ex), c["f1"][int(ex)], rtol=0, atol=1e-15), (ex, h.f1(ex), c["f1"])
    w = np.float32(0.5)
    want = float(w * np.float32(h.phone_loss) + (np.float32(1) - w) * np.float32(h.prosody_loss))
    assert (np.isnan(want) and np.isnan(h.loss) and np.isnan(float(s.loss))) or h.loss == want == float(s.loss)
    for acc, o in ((h.phone_acc, 0), (h.prosody_acc, 2)):
        assert (np.isnan(acc) and h.counts[o] == 0) or acc == h.counts[o + 1] / h.counts[o]


@pytest.mark.parametrize("cname,P,lens", so.CASES)
def test_score_against_float64_oracle(cname, P, lens):
    c, ids, mask, pl, rl, s, h = _run(cname, P, lens)
    o64 = so.reference(cname, P, lens)[5]
    figs = _figures(s.nll_phone.cpu(), s.nll_prosody.cpu(), (h.phone_loss, h.prosody_loss), pl, rl,
                    so.labelled(o64["nll_phone"], pl), so.labelled(o64["nll_prosody"], rl), o64["losses"])
    _check(figs, c, f"oracle {so.case_name(cname, P, lens)}")
    assert h.counts == o64["counts"].tolist()
    for hd, lab in (("phone", pl), ("prosody", rl)):
        pred, nll = getattr(s, "pred_" + hd).cpu(), getattr(s, "nll_" + hd).cpu()
        assert pred.dtype == torch.int32 and nll.dtype == torch.float32 and pred.shape == nll.shape == mask.shape
        assert torch.equal(pred.to(torch.int64), o64["pred_" + hd]), hd  # -1 at the padded tokens on both sides
        assert not bool(nll[lab == so.IGNORE_ID].view(torch.int32).any()), hd  # zeros where nothing is scored


# ---- 2. the stage entry on the oracle's x ------------------------------------------------------------------------------
def _score_heads(net, x, maskf, pl, rl, B, T, per_token=True):
    lib = _lib.load()
    nbytes = int(lib.wetts_frontend_score_workspace_bytes(net._handle, B, T))
    ws = torch.empty(nbytes // 4 + 1, device=DEV)
    nll = torch.full((2, B, T), 7.0, device=DEV)
    pred = torch.full((2, B, T), -7, dtype=torch.int32, device=DEV)
    losses, counts = torch.empty(2, device=DEV), torch.empty(22, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    outs = (p(nll[0]), p(nll[1]), p(pred[0]), p(pred[1])) if per_token else (None, None, None, None)
    _lib.check(lib.wetts_frontend_score_heads(net._handle, p(x), p(maskf), p(pl), p(rl), B, T, *outs, p(losses), p(counts),
                                              p(ws), nbytes, p(status), _lib.current_stream_ptr()), "score_heads")
    torch.cuda.synchronize()
    return nll.cpu(), pred.cpu(), losses.cpu(), counts.cpu(), int(status.item())


@pytest.mark.parametrize("cname", fo.CONFIGS)
@pytest.mark.parametrize("P", [p for p, _ in so.CLASS_COUNTS])
@pytest.mark.parametrize("lens", [(9, 6), (65, 64, 63)])
def test_score_heads_stage_against_float64_oracle(cname, P, lens):
    c = so.load_fixture(cname, P, lens)
    ids, mask, pl, rl, x64, _ = so.reference(cname, P, lens)
    x32 = x64.to(torch.float32)
    want = so.score(so.weights(cname, P)[1], x32.double(), mask, pl, rl)
    B, T = mask.shape
    args = (_net(cname, P), x32.to(DEV).contiguous(), mask.to(DEV, torch.float32).contiguous(), pl.to(DEV), rl.to(DEV), B, T)
    nll, pred, losses, counts, status = _score_heads(*args)
    assert status == 0
    figs = _figures(nll[0], nll[1], losses, pl, rl, so.labelled(want["nll_phone"], pl), so.labelled(want["nll_prosody"], rl),
                    want["losses"])
    _check(figs, c, f"stage {so.case_name(cname, P, lens)}")
    assert counts.tolist() == want["counts"].tolist()
    assert torch.equal(pred[0].to(torch.int64), want["pred_phone"]) and torch.equal(pred[1].to(torch.int64), want["pred_prosody"])
    # the four per-token outputs may be NULL: the same losses and counts, bit for bit
    _, _, losses2, counts2, _ = _score_heads(*args, per_token=False)
    assert torch.equal(losses.view(torch.int32), losses2.view(torch.int32)) and torch.equal(counts, counts2)


# ---- 3. bit-exact conditions ---------------------------------------------------------------------------------------------
def _bits(s):
    return [t.cpu().view(torch.int32) if t.dtype == torch.float32 else t.cpu()
            for t in (s.nll_phone, s.nll_prosody, s.pred_phone, s.pred_prosody)]


@pytest.mark.parametrize("cname,P", [(c, p) for c in fo.CONFIGS for p, _ in so.CLASS_COUNTS])
@pytest.mark.parametrize("lens", [s for s in so.SHAPES if len(s) > 1])
def test_repeats_rows_alone_and_permutations_are_bit_identical(cname, P, lens):
    c, ids, mask, pl, rl, s, h = _run(cname, P, lens)
    net = _net(cname, P)
    full = _bits(s)
    again = net.score({"input_ids": ids, "attention_mask": mask}, pl, rl)
    assert all(torch.equal(a, b) for a, b in zip(_bits(again), full))
    assert torch.equal(again.packed().cpu(), s.packed().cpu())
    for b, n in enumerate(lens):  # a row alone, without its padding
        alone = net.score({"input_ids": ids[b:b + 1, :n]}, pl[b:b + 1, :n], rl[b:b + 1, :n])
        for k, (a, f) in enumerate(zip(_bits(alone), full)):
            assert torch.equal(a[0], f[b, :n]), (b, k)
    perm = list(range(len(lens)))[::-1]
    q = net.score({"input_ids": ids[perm], "attention_mask": mask[perm]}, pl[perm], rl[perm])
    for k, (a, f) in enumerate(zip(_bits(q), full)):
        assert torch.equal(a, f[perm]), k
    assert q.host().counts == h.counts  # counts are sums over rows


@pytest.mark.parametrize("cname,P,lens", so.CASES)
def test_predictions_are_the_argmax_of_forward_logits(cname, P, lens):
    c, ids, mask, pl, rl, s, h = _run(cname, P, lens)
    lp, lr = _net(cname, P)({"input_ids": ids, "attention_mask": mask})
    on = mask != 0
    for got, z in ((s.pred_phone, lp), (s.pred_prosody, lr)):
        assert torch.equal(got.cpu()[on].to(torch.int64), z.cpu().argmax(-1)[on])
        assert bool((got.cpu()[~on] == -1).all())


@pytest.mark.parametrize("cname", fo.CONFIGS)
def test_exact_ties_go_to_the_lowest_class_within_a_tile_and_across_tiles(cname):
    P, lens = 470, (33, 32, 31)
    net = _net(cname, P, so.tie_weights(cname, P), "ties")
    ids, mask = fo.inputs(lens, 515)
    s = net.score({"input_ids": ids, "attention_mask": mask})
    on = mask != 0
    for pred, (lo, his) in ((s.pred_phone.cpu()[on], so.TIES["phone"]), (s.pred_prosody.cpu()[on], so.TIES["prosody"])):
        assert int((pred == lo).sum()) >= 8, (lo, pred.tolist())  # the tie is at the maximum often enough
        assert not any(bool((pred == hi).any()) for hi in his), (his, pred.tolist())


# ---- 4. conventions --------------------------------------------------------------------------------------------------------
def test_a_head_without_labels_gives_nan_and_leaves_the_other_head_alone():
    cname, P, lens = "tiny", 34, (33, 32, 31)
    c, ids, mask, pl, rl, s, h = _run(cname, P, lens)
    net = _net(cname, P)
    x = {"input_ids": ids, "attention_mask": mask}
    only_r, only_p = net.score(x, None, rl), net.score(x, pl, None)
    ignored = net.score(x, torch.full_like(pl, so.IGNORE_ID), rl)
    assert torch.equal(only_r.packed().cpu(), ignored.packed().cpu())  # None = all -100
    assert all(torch.equal(a, b) for a, b in zip(_bits(only_r), _bits(ignored)))
    hr, hp = only_r.host(), only_p.host()
    assert np.isnan(hr.phone_loss) and np.isnan(hr.phone_acc) and np.isnan(hr.loss) and hr.counts[:2] == [0, 0]
    assert hr.prosody_loss == h.prosody_loss and hr.prosody_acc == h.prosody_acc and hr.counts[2:] == h.counts[2:]
    assert np.isnan(hp.prosody_loss) and np.isnan(hp.prosody_acc) and hp.counts[2:] == [0] * 20 and hp.f1() == (0.0, 0.0, 0.0)
    assert hp.phone_loss == h.phone_loss and hp.phone_acc == h.phone_acc and hp.counts[:2] == h.counts[:2]
    assert torch.equal(only_p.nll_phone, s.nll_phone) and torch.equal(only_r.nll_prosody, s.nll_prosody)
    assert torch.equal(only_p.pred_prosody, s.pred_prosody)  # predictions do not depend on labels
    hw = net.score(x, pl, rl, polyphone_weight=0.25).host()
    assert hw.loss == float(np.float32(0.25) * np.float32(h.phone_loss) + np.float32(0.75) * np.float32(h.prosody_loss))


def test_label_errors_raise_and_a_clean_call_follows():
    cname, P, lens = "tiny", 34, (9, 6)
    c, ids, mask, pl, rl, s, h = _run(cname, P, lens)
    net = _net(cname, P)
    x = {"input_ids": ids, "attention_mask": mask}
    for head, bad in (("phone", P), ("phone", -1), ("prosody", R), ("prosody", -101)):
        a, b = pl.clone(), rl.clone()
        (a if head == "phone" else b)[0, 2] = bad
        with pytest.raises(IndexError, match="out of bounds"):
            net.score(x, a, b).host()
    a = pl.clone()
    a[1, 7] = 3  # row 1 has 6 tokens: a padded position
    with pytest.raises(ValueError, match="attention_mask"):
        net.score(x, a, rl).host()
    with pytest.raises(ValueError):
        net.score(x, pl[:, :-1], rl)
    with pytest.raises(ValueError):
        net.score(x, pl.to(torch.float32), rl)
    bad_ids = ids.clone()
    bad_ids[0, 1] = fo.VOCAB
    with pytest.raises(IndexError):
        net.score({"input_ids": bad_ids, "attention_mask": mask}, pl, rl).host()
    assert torch.equal(net.score(x, pl, rl).packed().cpu(), s.packed().cpu())


@pytest.mark.parametrize("cname", fo.CONFIGS)
def test_f1_slices_with_ignored_labels_padded_tokens_and_the_clip_at_T(cname):
    """Hand-made prosody labels on the stable inputs of the (33, 32, 31) fixture, against the oracle's literal
    test_prosody.py:83-93: row 0 labels every position, [CLS] and [SEP] included, so len_b = T and Python's slice clips;
    row 1 labels its 32 valid tokens, so position 32 of `1 .. 32` is a padded token (label -100, prediction -1); row 2
    has two ignored labels inside `1 .. len_b`.  The polyphone head carries no label."""
    P, lens = 34, (33, 32, 31)
    ids, mask, _, _, x64, _ = so.reference(cname, P, lens)
    B, T = mask.shape
    g = torch.Generator().manual_seed(99)
    rl = torch.full((B, T), so.IGNORE_ID, dtype=torch.int64)
    rl[0] = torch.randint(0, R, (T,), generator=g)
    rl[1, :32] = torch.randint(0, R, (32,), generator=g)
    rl[2, 1:30] = torch.randint(0, R, (29,), generator=g)
    rl[2, 10:12] = so.IGNORE_ID
    len_b = (rl != so.IGNORE_ID).sum(1).tolist()
    assert len_b == [T, 32, 27] and mask[1, 32] == 0 and bool((rl[2, 1:28] == so.IGNORE_ID).any())
    want = so.score(so.weights(cname, P)[1], x64, mask, None, rl)
    s = _net(cname, P).score({"input_ids": ids, "attention_mask": mask}, None, rl)
    h = s.host()
    assert torch.equal(s.pred_prosody.cpu().to(torch.int64), want["pred_prosody"]) and int(s.pred_prosody[1, 32]) == -1
    assert h.counts == want["counts"].tolist()
    assert h.counts[4:13] != h.counts[13:22] and sum(h.counts[4:13]) > 0  # both ranges are populated and differ
    # a weight whose complement is not exact in float32: host and device form train.py:83-84 alike
    s3 = _net(cname, P).score({"input_ids": ids, "attention_mask": mask}, so.reference(cname, P, lens)[2], rl,
                              polyphone_weight=0.6)
    assert s3.host().loss == float(s3.loss)


# ---- 5. frontend_eval on the toy directory -----------------------------------------------------------------------------------
def test_frontend_eval_prints_the_reference_lines_on_the_toy_data(tmp_path, capsys):
    kat = np.load(os.path.join(fo.GOLDEN, "frontend_data_kat.npz"))
    d = tmp_path / fo.BERT_CONFIGS["tiny"]["_name_or_path"]
    d.mkdir()
    shutil.copy(os.path.join(fo.TOY, "vocab.txt"), d)
    (d / "config.json").write_text(json.dumps(fo.BERT_CONFIGS["tiny"]))
    ckpt = str(tmp_path / "final.pt")
    torch.save(fo.weights("tiny")[0], ckpt)
    data = os.path.join(fo.TOY, "data")
    common = ["--polyphone_dict", os.path.join(fo.TOY, "lexicon", "polyphone.txt"), "--prosody_dict",
              os.path.join(fo.TOY, "lexicon", "prosody.txt"), "--batch_size", "8", "--checkpoint", ckpt, "--bert_name_or_path",
              str(d)]
    poly = ["--test_data", os.path.join(data, "polyphone_cv.txt")]
    pros = ["--test_data", os.path.join(data, "prosody_cv.txt")]
    assert frontend_eval.run(frontend_eval.get_args(["polyphone"] + common + poly)) == [str(kat["polyphone_line"])]
    assert frontend_eval.run(frontend_eval.get_args(["prosody"] + common + pros)) == [str(kat["prosody_lines"][0])]
    assert frontend_eval.run(frontend_eval.get_args(["prosody", "--exclude_end"] + common + pros)) == [str(kat["prosody_lines"][1])]
    capsys.readouterr()
    frontend_eval.main(["cv"] + common + ["--cv_polyphone_data", poly[1], "--cv_prosody_data", pros[1]])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch 0 [CV] progress")]
    rows = kat["cv_rows"]
    assert len(lines) == len(rows)
    for i, (line, row) in enumerate(zip(lines, rows)):
        f = line.split()
        assert f[:5] == ["Epoch", "0", "[CV]", "progress", f"{i}/{len(rows)}"]
        assert f[5:15:2] == ["loss", "polyphone_loss", "polyphone_acc", "prosody_loss", "prosody_acc"]
        got = np.asarray([float(v) for v in f[6:16:2]])
        # values below 4.1 within the fixture gate of a loss (5 floors of at most 4e-7: 2e-6 relative, 8.2e-6 absolute),
        # plus the rounding of the six printed decimals (5e-7) and of the stored reference (float32 in float64: none)
        assert np.array_equal(np.isnan(got), np.isnan(row)) and np.allclose(got, row, rtol=0, atol=1e-5, equal_nan=True), (line, row)
