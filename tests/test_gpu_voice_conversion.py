"""GPU tier: SynthesizerTrn.voice_conversion (posterior encoder -> flow -> flow^-1 -> decoder) against the live
reference's voice_conversion (tests/golden/vc_*.npz, made by tests/golden/make_golden_vc.py), plus the properties the
goldens do not pin: exact invertibility of the forward flow, seeding, the lazily uploaded posterior leaving infer()
untouched, the 16-bit flow / decoder modes, and the error surface."""
import numpy as np
import pytest
import torch

from tests import util
from wetts_amd import SynthesizerTrn, _lib, config, synth

pytestmark = pytest.mark.gpu

SPEC = 513
VC_CASES = ["vc_tiny_b3", "vc_vits2_v1_b2", "vc_tiny_preconv2_spk_b3", "vc_tiny_mono_post_b2", "vc_tiny_mono_inter_b3",
            "vc_tiny_vocos_b2", "vc_aishell3_b4x600"]
# one model per flow type: plain, pre_conv, pre_conv2, mono_layer_post_residual, mono_layer_inter_residual
FLOW_TYPE_CASES = ["vc_tiny_b3", "vc_vits2_v1_b2", "vc_tiny_preconv2_spk_b3", "vc_tiny_mono_post_b2",
                   "vc_tiny_mono_inter_b3"]


_load = util.load_vc_case


def _net(case, with_posterior=True):
    mname = str(case["model"])
    cfg, sd, psd = util.vc_case_model(case, SPEC)
    net = SynthesizerTrn(int(case["n_vocab"]), SPEC, 32, n_speakers=int(case["n_speakers"]),
                         **config.MODEL_CONFIGS[mname])
    net.load_state_dict(dict(sd, **psd) if with_posterior else sd)
    return net.to("cuda"), cfg


def _inputs(case):
    dev = "cuda"
    return (torch.from_numpy(case["y"].astype(np.float32)).to(dev), torch.from_numpy(case["y_lengths"]).to(dev),
            torch.from_numpy(case["sid_src"]).to(dev), torch.from_numpy(case["sid_tgt"]).to(dev),
            torch.from_numpy(case["eps"]).to(dev))


def _vc(net, case, **kw):
    y, yl, ss, st, eps = _inputs(case)
    return net.voice_conversion(y, yl, ss, st, eps_q=kw.pop("eps_q", eps), **kw)


def _rel(a, ref):
    return util.rel_rms(a, ref)


@pytest.mark.parametrize("name", VC_CASES)
def test_voice_conversion_matches_reference_golden(name):
    case = _load(name)
    net, cfg = _net(case)
    o_hat, y_mask, (z, z_p, z_hat) = _vc(net, case)
    torch.cuda.synchronize()
    st = net._last_vc
    got = dict(z=z, m_q=st["m_q"], logs_q=st["logs_q"], z_p=z_p, z_hat=z_hat)
    rows = {"y_mask_equal": bool(np.array_equal(y_mask.cpu().numpy(), case["y_mask"]))}
    if "sub_strides" in case:
        sa, sz = (int(v) for v in case["sub_strides"])
        assert tuple(o_hat.shape) == tuple(int(v) for v in case["audio_shape"])
        for k, v in got.items():
            rows[k] = _rel(v.cpu().numpy()[..., ::sz], case[k + "_sub"])
        audio = o_hat.cpu().numpy()
        rows["audio_abs_rms"] = util.rms(audio[..., ::sa] - case["audio_sub"])
        rows["audio_sum_rel"] = abs(float(audio.astype(np.float64).sum()) - float(case["audio_sum"])) / \
            max(1.0, abs(float(case["audio_sum"])))
        rows["audio_sqsum_rel"] = abs(float((audio.astype(np.float64) ** 2).sum()) - float(case["audio_sqsum"])) / \
            float(case["audio_sqsum"])
    else:
        for k, v in got.items():
            rows[k] = _rel(v.cpu().numpy(), case[k])
        assert o_hat.shape == case["audio"].shape
        rows["audio_abs_rms"] = util.rms(o_hat.cpu().numpy() - case["audio"])
    print(name, rows)  # the stage-wise figures (pytest -s), also part of every failure message below
    assert rows["y_mask_equal"], rows
    for k in ("z", "m_q", "logs_q"):
        assert rows[k] < 1e-4, (k, rows)
    for k in ("z_p", "z_hat"):
        assert rows[k] < 2e-4, (k, rows)
    assert rows["audio_abs_rms"] < 1e-4, rows
    if "audio_sqsum_rel" in rows:
        assert rows["audio_sqsum_rel"] < 1e-3, rows


@pytest.mark.parametrize("name", FLOW_TYPE_CASES)
def test_flow_forward_then_reverse_is_identity(name):
    """flow^-1(flow(z, g), g) == z on valid frames (every coupling here is exactly invertible on mask-1 frames)."""
    case = _load(name)
    net, cfg = _net(case)
    net._require_posterior()
    B, I, Ty = len(case["y_lengths"]), cfg.inter_channels, int(case["y"].shape[2])
    gen = torch.Generator().manual_seed(5)
    z = torch.randn(B, I, Ty, generator=gen).cuda()
    y_mask = (torch.arange(Ty)[None, :] < torch.from_numpy(case["y_lengths"])[:, None]).float().cuda()
    z = z * y_mask[:, None, :]
    g = net._speaker(torch.from_numpy(case["sid_src"]).cuda(), B)
    nws = max(int(_lib.load().wetts_posterior_workspace_bytes(net._handle, B, Ty)),
              int(_lib.load().wetts_workspace_bytes(net._handle, B, 0, Ty)))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    z_p = net._flow_pass(z, y_mask, g, False, ws, nws)
    back = net._flow_pass(z_p, y_mask, g, True, ws, nws)
    torch.cuda.synchronize()
    valid = y_mask[:, None, :].expand_as(z).bool()
    err = float((back - z)[valid].pow(2).mean().sqrt() / z[valid].pow(2).mean().sqrt())
    moved = float((z_p - z)[valid].pow(2).mean().sqrt() / z[valid].pow(2).mean().sqrt())
    assert moved > 1e-2, moved  # the forward flow is not an identity
    assert err < 1e-5, err


def test_seed_reproducible_and_noise_drawn():
    case = _load("vc_tiny_b3")
    net, _ = _net(case)
    y, yl, ss, st, _ = _inputs(case)
    torch.manual_seed(1234)
    a, _, (za, _, _) = net.voice_conversion(y, yl, ss, st)
    torch.manual_seed(1234)
    b, _, (zb, _, _) = net.voice_conversion(y, yl, ss, st)
    torch.manual_seed(4321)
    _, _, (zc, _, _) = net.voice_conversion(y, yl, ss, st)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(za, zb)
    assert not torch.equal(za, zc)


@pytest.mark.parametrize("name", ["vc_tiny_b3", "vc_tiny_mono_post_b2"])
def test_infer_unchanged_by_voice_conversion(name):
    """The lazily uploaded posterior and the forward flow's extra `pre` copies disturb nothing infer() computes."""
    case = _load(name)
    net, cfg = _net(case)
    B, Tx = 2, 9
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(0, int(case["n_vocab"]), (B, Tx), generator=gen).cuda()
    xl = torch.tensor([9, 6]).cuda()
    sid = torch.tensor([0, 1]).cuda()
    eps_w = torch.randn(B, 2, Tx, generator=gen).cuda()

    def run():
        torch.manual_seed(7)
        o, _, _, (z, *_) = net.infer(x, xl, sid=sid, noise_scale=0.667, noise_scale_w=0.8, eps_w=eps_w)
        torch.cuda.synchronize()
        return o.clone(), z.clone()

    o0, z0 = run()
    assert not net._post_on_device  # infer() alone uploads no posterior
    _vc(net, case)
    o1, z1 = run()
    assert torch.equal(o0, o1) and torch.equal(z0, z1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_flow_and_decoder(dtype):
    case = _load("vc_vits2_v1_b2")
    net, _ = _net(case)
    o32, _, (_, _, zh32) = _vc(net, case)
    o32, zh32 = o32.clone(), zh32.clone()
    net.set_flow_dtype(dtype).set_decoder_dtype(dtype)
    o16, _, (_, _, zh16) = _vc(net, case)
    torch.cuda.synchronize()
    assert _rel(zh16.cpu().numpy(), zh32.cpu().numpy()) < 3e-2
    assert util.rms(o16.cpu().numpy() - o32.cpu().numpy()) < 2e-3
    net.set_flow_dtype(torch.float32).set_decoder_dtype(torch.float32)
    ob, _, (_, _, zhb) = _vc(net, case)
    torch.cuda.synchronize()
    assert torch.equal(ob, o32) and torch.equal(zhb, zh32)


def test_errors_and_model_stays_usable():
    case = _load("vc_tiny_b3")
    net, _ = _net(case)
    ref, _, _ = _vc(net, case)
    ref = ref.clone()
    y, yl, ss, st, eps = _inputs(case)
    with pytest.raises(IndexError):
        net.voice_conversion(y, yl, ss, torch.tensor([0, 3, 1]).cuda(), eps_q=eps)
    again, _, _ = _vc(net, case)
    torch.cuda.synchronize()
    assert torch.equal(again, ref)
    # a checkpoint without enc_q: infer() works, voice_conversion says why it cannot
    bare, _ = _net(case, with_posterior=False)
    with pytest.raises(_lib.WettsError, match="enc_q"):
        bare.voice_conversion(y, yl, ss, st, eps_q=eps)
    o, *_ = bare.infer(torch.tensor([[1, 2, 3]]).cuda(), torch.tensor([3]).cuda(), sid=torch.tensor([0]).cuda())
    assert torch.isfinite(o).all()
    # n_speakers == 0: no emb_g, as in the reference
    cfg0 = config.make_config(dict(config.MODEL_CONFIGS["tiny"]), 40, 0)
    net0 = SynthesizerTrn(40, SPEC, 32, n_speakers=0, **config.MODEL_CONFIGS["tiny"])
    net0.load_state_dict(dict(synth.make_state_dict(cfg0, 1), **synth.make_posterior_state_dict(cfg0, SPEC, 2)))
    net0.to("cuda")
    with pytest.raises(AttributeError):
        net0.voice_conversion(y, yl, ss, st, eps_q=eps)
    o0, *_ = net0.infer(torch.tensor([[1, 2, 3]]).cuda(), torch.tensor([3]).cuda())
    assert torch.isfinite(o0).all()
