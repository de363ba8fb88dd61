"""GPU tier: SynthesizerTrn.voice_conversion against the float64 oracle (oracle/vits_oracle.py: posterior_encoder,
flow_forward, flow_reverse, decoder; pinned to the reference's goldens by tests/test_cpu_voice_conversion.py) at the
shapes the fixed goldens never reach: every flow type at tiny and ragged batches, spec_channels whose K tail is 1, 4, 0
and 1 mod 16, full-size batches on the big conv tiles, inputs with garbage beyond y_lengths, the 16-bit forward flow
against its numerics spec, and the device noise draw against Philox.

The transformer-flow models run a second list at tile-edge frame counts (TILE_SHAPES): the oracle otherwise sees their
attention at no Ty above 23.

Every comparison is over whole tensors of the same padded batch, padded frames included, with two gates per stage:
rel RMS <= 1e-5 and max |d| / rms(ref) <= 1e-4 (a local-error gate: one wrong tile or last frame does not hide in a
whole-tensor RMS).  Audio: abs RMS <= 1e-4, as in the infer() sweep.  Each test prints its worst figures per stage."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util
from wetts_amd import SynthesizerTrn, config, synth

pytestmark = pytest.mark.gpu

SPEC = 513
STAGES = ("z", "m_q", "logs_q", "z_p", "z_hat")
REL_RMS, LOCAL, AUDIO_ABS = 1e-5, 1e-4, 1e-4
FLOW_MODELS = ["tiny", "vits2_v1", "tiny_preconv2_spk", "tiny_mono_post", "tiny_mono_inter", "tiny_vocos"]
# (B, Ty_in, y_lengths): ragged, a length-1 row in every multi-row batch; (1, 3), (5, 9) and (2, 17) pad every row
SHAPES = [(1, 1, [1]), (1, 2, [2]), (1, 3, [2]), (1, 4, [4]), (1, 5, [5]), (2, 7, [7, 1]), (3, 23, [1, 23, 12]),
          (5, 9, [3, 8, 1, 5, 6]), (4, 16, [16, 1, 9, 14]), (2, 17, [1, 11])]

# The transformer flows at tile-edge frame counts.  Ty_in: the 32-query strips and 32-key tiles of attn_flash_kernel
# (window-less, dk = 48: its four waves walk the keys in strides of 128, so 129 .. 256 frames give a wave a second
# tile, 545 frames five to wave 0 with one key in the last) and of the windowed kernels of the pre_conv2 flows
# (dk = 96: attn_small_kernel up to 128 frames, the matrix-core path with three 32-row d-blocks beyond).  Ragged: one
# full row, one of length 1, one 1 past a multiple of 32; B cycles over 1, 2, 3.
# tests/test_cpu_encoder_gate.py asserts what the list reaches of each kernel form.
TF_MODELS = ["vits2_v1", "tiny_preconv2_spk", "tiny_mono_post", "tiny_mono_inter", "tiny_vits2_vocos"]
TILE_LENGTHS = (31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 161, 257, 545)


def _tile_rows(B, Ty):
    rows = [Ty, 1, 32 * ((Ty - 2) // 32) + 1 if Ty >= 34 else max(1, Ty - 2)][:B]
    return rows[Ty % B:] + rows[:Ty % B]


TILE_SHAPES = [((1, 2, 3)[i % 3], Ty, _tile_rows((1, 2, 3)[i % 3], Ty)) for i, Ty in enumerate(TILE_LENGTHS)]
# (model, WETTS_TUNE at create): pre_conv2 a second time on the kernels behind the one-launch attention -- the scalar
# ones below 64 frames, the matrix-core path from 64
TILE_SWEEP = [(m, None) for m in TF_MODELS] + [("tiny_preconv2_spk", "attn_small_max_t=0")]


def _model(mname, n_vocab=40, n_spk=3, spec=SPEC, wseed=81, pseed=82, tune=None):
    """(device net, cfg dict, float64 folded weights incl. enc_q) of a synthetic checkpoint; `tune`: WETTS_TUNE at
    create (a per-model setting)."""
    cfg = config.make_config(dict(config.MODEL_CONFIGS[mname]), n_vocab, n_spk)
    sd = synth.make_state_dict(cfg, wseed)
    psd = synth.make_posterior_state_dict(cfg, spec, pseed)
    net = SynthesizerTrn(n_vocab, spec, 32, n_speakers=n_spk, **config.MODEL_CONFIGS[mname])
    if tune is not None:
        os.environ["WETTS_TUNE"] = tune
    try:
        net.load_state_dict(dict(sd, **psd)).to("cuda")
    finally:
        os.environ.pop("WETTS_TUNE", None)
    return net, util.cfg_dict(cfg), util.vc_weights(cfg, sd, psd, torch.float64)


def _batch(B, spec, Ty, lengths, seed, n_spk=3, pad=None):
    """Heavy-tailed positive magnitudes (like a spectrogram, tools/bench_vc.py), zero beyond y_lengths unless `pad`
    gives the value to put there; speaker ids; a standard-normal posterior draw."""
    gen = torch.Generator().manual_seed(seed)
    yl = torch.tensor(lengths, dtype=torch.long)
    y = torch.rand(B, spec, Ty, generator=gen) ** 4 * 20.0
    ss = torch.randint(0, n_spk, (B,), generator=gen)
    st = torch.randint(0, n_spk, (B,), generator=gen)
    eps = torch.randn(B, 192, Ty, generator=gen)
    valid = (torch.arange(Ty)[None, :] < yl[:, None]).unsqueeze(1)
    # (the padding has a stream of its own: everything else is the same with and without it)
    y = torch.where(valid, y, torch.zeros(()) if pad is None else pad(y.shape, torch.Generator().manual_seed(seed + 1)))
    return y, yl, ss, st, eps


def _gpu(net, y, yl, ss, st, eps):
    o, y_mask, (z, z_p, z_hat) = net.voice_conversion(y.cuda(), yl.cuda(), ss.cuda(), st.cuda(), eps_q=eps.cuda())
    torch.cuda.synchronize()
    lv = net._last_vc
    out = dict(z=z, m_q=lv["m_q"], logs_q=lv["logs_q"], z_p=z_p, z_hat=z_hat, o_hat=o, y_mask=y_mask)
    return {k: v.detach().cpu() for k, v in out.items()}


def _oracle(W, cd, y, yl, ss, st, eps, stages=STAGES, decode=True):
    """float64 oracle stages of the same padded batch; the flows and the decoder only as far as `stages` needs."""
    d = torch.float64
    with torch.no_grad():
        g_src = F.embedding(ss, W["emb_g.weight"]).unsqueeze(-1)
        g_tgt = F.embedding(st, W["emb_g.weight"]).unsqueeze(-1)
        z, m_q, logs_q, y_mask = vo().posterior_encoder(W, cd, y.to(d), yl, g_src, eps.to(d))
        out = dict(z=z, m_q=m_q, logs_q=logs_q, y_mask=y_mask)
        if "z_p" in stages or "z_hat" in stages:
            out["z_p"] = vo().flow_forward(W, cd, z, y_mask, g_src)
        if "z_hat" in stages:
            out["z_hat"] = vo().flow_reverse(W, cd, out["z_p"], y_mask, g_tgt)
            if decode:
                out["o_hat"] = vo().decoder(W, cd, out["z_hat"] * y_mask, g_tgt)
    return out


def vo():
    from oracle import vits_oracle
    return vits_oracle


def _gates(got, ref):
    """(rel RMS, max |d| / rms(ref)) over the whole tensor."""
    a, r = got.double().numpy(), ref.double().numpy()
    assert a.shape == r.shape, (a.shape, r.shape)
    scale = max(util.rms(r), 1e-30)
    return util.rms(a - r) / scale, float(np.abs(a - r).max()) / scale


def _check(tag, got, ref, stages, worst):
    """Asserts both gates on every stage (and the audio, when the oracle decoded) and keeps the worst figures."""
    assert torch.equal(got["y_mask"].reshape(ref["y_mask"].shape).double(), ref["y_mask"]), tag
    for k in stages:
        rel, loc = _gates(got[k], ref[k])
        w = worst.setdefault(k, [0.0, 0.0])
        w[0], w[1] = max(w[0], rel), max(w[1], loc)
        assert rel <= REL_RMS and loc <= LOCAL, (tag, k, rel, loc)
    if "o_hat" in ref:
        assert got["o_hat"].shape == ref["o_hat"].shape, tag
        err = util.rms((got["o_hat"].double() - ref["o_hat"]).numpy())
        worst["audio_abs_rms"] = max(worst.get("audio_abs_rms", 0.0), err)
        assert err <= AUDIO_ABS, (tag, "audio", err)


def _report(tag, worst):
    print(tag, "worst (rel RMS, max|d|/rms):", {k: v if isinstance(v, float) else (float(f"{v[0]:.3g}"),
                                                                                   float(f"{v[1]:.3g}"))
                                                for k, v in worst.items()})


# ---- a. every flow type at tiny and ragged shapes ----------------------------------------------------------------
@pytest.mark.parametrize("mname", FLOW_MODELS)
def test_vc_shape_sweep_matches_float64_oracle(mname):
    """B = 1..5, Ty_in = 1..23 (rows of 1 to 3 frames past a multiple of 4, length-1 rows, batches where every row is
    padded): the small-launch conv schedule, partial time tiles and the row re-padding of both flow directions."""
    net, cd, W = _model(mname)
    worst = {}
    for i, (B, Ty, lengths) in enumerate(SHAPES):
        if mname == "tiny_vocos" and Ty < 2:
            continue  # nn.ReflectionPad1d([1, 0]) needs two frames (decoders.py:265), as in the infer() sweep
        y, yl, ss, st, eps = _batch(B, SPEC, Ty, lengths, seed=100 + i)
        _check((mname, B, Ty), _gpu(net, y, yl, ss, st, eps), _oracle(W, cd, y, yl, ss, st, eps), STAGES, worst)
    _report(f"{mname} shape sweep", worst)


# ---- a2. the transformer flows at tile-edge frame counts ---------------------------------------------------------------
_TILE_REFS = {}


def _tile_refs(mname):
    """[(B, Ty, batch, float64 oracle stages)] over TILE_SHAPES: computed once per model, shared by its forms."""
    if mname not in _TILE_REFS:
        cfg = config.make_config(dict(config.MODEL_CONFIGS[mname]), 40, 3)
        W = util.vc_weights(cfg, synth.make_state_dict(cfg, 81), synth.make_posterior_state_dict(cfg, SPEC, 82),
                            torch.float64)
        cd, out = util.cfg_dict(cfg), []
        for i, (B, Ty, lengths) in enumerate(TILE_SHAPES):
            batch = _batch(B, SPEC, Ty, lengths, seed=300 + i)
            out.append((B, Ty, batch, _oracle(W, cd, *batch, decode=False)))
        _TILE_REFS[mname] = out
    return _TILE_REFS[mname]


@pytest.mark.parametrize("mname,tune", TILE_SWEEP)
def test_vc_transformer_flows_at_tile_edges_match_float64_oracle(mname, tune):
    """Posterior encoder, forward flow and flow^-1 (no decode) of every transformer-flow model over TILE_SHAPES, at this
    file's gates."""
    net, cd, W = _model(mname, tune=tune)
    worst = {}
    for B, Ty, batch, ref in _tile_refs(mname):
        _check((mname, tune, B, Ty), _gpu(net, *batch), ref, STAGES, worst)
    _report(f"{mname} {tune or 'default'} tile-edge sweep", worst)


# ---- b. spec_channels: the posterior pre conv's K tail ------------------------------------------------------------
@pytest.mark.parametrize("spec", [1, 17, 80, 100, 513, 1025])
def test_vc_spec_channels_sweep(spec):
    """pre conv with K = spec_channels read in place from the caller's [B, spec, Ty_in] rows: K below one 16-channel
    chunk (1), K tails of 1 (17, 513, 1025), 0 (80) and 4 (100) mod 16, at odd Ty_in and ragged lengths, on the
    small-launch schedule (3 x 37) and on the tiled one (4 x 301)."""
    net, cd, W = _model("tiny", spec=spec, pseed=90 + spec)
    worst = {}
    for B, Ty, lengths in [(3, 37, [29, 37, 1]), (4, 301, [301, 257, 99, 1])]:
        y, yl, ss, st, eps = _batch(B, spec, Ty, lengths, seed=spec * 10 + B)
        stages = ("z", "m_q", "logs_q", "z_p")
        _check((spec, B, Ty), _gpu(net, y, yl, ss, st, eps), _oracle(W, cd, y, yl, ss, st, eps, stages), stages,
               worst)
    _report(f"spec_channels {spec}", worst)


# ---- c / d. full size: the big conv tiles, and garbage beyond y_lengths -------------------------------------------
_V1 = {}


def _v1():
    """HiFi-GAN v1 with the 218-row AISHELL-3 speaker table (BASELINE.json configs[3]), shared by the full-size tests."""
    if not _V1:
        _V1["m"] = _model("v1", n_vocab=256, n_spk=218, wseed=35, pseed=36)
    return _V1["m"]


FULL = {
    # tools/bench_vc.py's shape, every row full
    "b16x768": (16, 768, [768] * 16),
    # ragged, odd Ty_in, no length a multiple of 4, one under 100
    "b8x1001": (8, 1001, [1001, 998, 731, 517, 263, 97, 999, 850]),
    # 24 x 767 (rows of 768): the cost model's 64 x 128 tile for the pre conv and 128 x 128 for the WN in_layers
    "b24x767": (24, 767, [767, 1, 500, 766, 765, 3, 767, 401, 250, 767, 123, 600, 767, 11, 767, 333, 767, 700,
                          767, 2, 767, 505, 767, 9]),
}


@pytest.mark.parametrize("shape", list(FULL))
def test_vc_full_size_matches_float64_oracle(shape):
    """Posterior encoder, forward flow and flow^-1 of v1 at full size (the decoder is pinned at full size by the infer()
    tests).  The conv instances these launch, read from a rocprofv3 --kernel-trace of this test
    (conv_mfma_kernel<MB, NB, WM, WN, epilogue, MRF, FAST>: a tile of 32*MB*WM rows x 32*NB*WN columns):
      16 x 768 and 8 x 1001: the posterior pre conv (K = 513) on 64 x 64, conv_mfma_kernel<1, 1, 2, 2, 4, false, false>,
        and every WN in_layer (k = 5, gate epilogue) on 64 x 64, conv_mfma_kernel<1, 1, 2, 2, 5, false, true>: at these
        shapes launch_conv's cost model prefers 64 x 64 to 64 x 128 and 128 x 128 (fewer than 1.5 big tiles per CU).
      24 x 767: the pre conv on 64 x 128, conv_mfma_kernel<1, 2, 2, 2, 4, false, false>, and the WN in_layers on
        128 x 128, conv_mfma_kernel<1, 4, 4, 1, 5, false, true>."""
    net, cd, W = _v1()
    B, Ty, lengths = FULL[shape]
    y, yl, ss, st, eps = _batch(B, SPEC, Ty, lengths, seed=Ty + B, n_spk=218)
    worst = {}
    _check(shape, _gpu(net, y, yl, ss, st, eps), _oracle(W, cd, y, yl, ss, st, eps, decode=False), STAGES, worst)
    _report(f"v1 {shape}", worst)


def _big_padding(shape, gen):
    return 1e3 * torch.randn(shape, generator=gen).abs()


@pytest.mark.parametrize("which", ["tiny", "v1"])
def test_vc_padding_invariance(which):
    """Large finite values in y beyond y_lengths change nothing: every stage is bit-identical to the zero-padded run on
    valid frames, and z, m_q, logs_q are exactly 0 on padded frames (encoders.py:96-98: pre(x) * x_mask,
    proj(x) * x_mask, (m + eps * exp(logs)) * x_mask)."""
    if which == "tiny":
        net, _, _ = _model("tiny")
        B, Ty, lengths, n_spk = 3, 23, [1, 23, 12], 3
    else:
        net, _, _ = _v1()
        (B, Ty, lengths), n_spk = FULL["b8x1001"], 218
    clean = _gpu(net, *_batch(B, SPEC, Ty, lengths, seed=7, n_spk=n_spk))
    y, yl, ss, st, eps = _batch(B, SPEC, Ty, lengths, seed=7, n_spk=n_spk, pad=_big_padding)
    assert float(y.max()) > 1e3
    dirty = _gpu(net, y, yl, ss, st, eps)
    valid = (torch.arange(Ty)[None, :] < yl[:, None]).unsqueeze(1)
    assert torch.equal(clean["y_mask"], dirty["y_mask"])
    for k in STAGES:
        v = valid.expand_as(clean[k])
        assert torch.equal(clean[k][v], dirty[k][v]), k
        if k in ("z", "m_q", "logs_q"):
            assert bool((dirty[k][~v] == 0).all()) and bool((clean[k][~v] == 0).all()), k
    print(which, "padding invariance: bit-identical on", int(valid.sum()), "valid frames per channel")


# ---- e. 16-bit forward flow against its numerics spec ------------------------------------------------------------
@pytest.mark.parametrize("name", ["vc_vits2_v1_b2", "vc_aishell3_b4x600"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_forward_flow_matches_its_spec(name, dtype):
    """set_flow_dtype(16-bit): z_p against oracle.flow_forward(wn_dtype=) on the device's own z, at the reverse
    direction's gates (1e-2 bf16, 2e-3 f16 rel RMS on valid frames); the posterior encoder is f32 in every mode, so z,
    m_q and logs_q stay bit-identical to the f32 run under any flow and decoder precision."""
    from tests.test_gpu_voice_conversion import _inputs, _net
    case = util.load_vc_case(name)
    net, cfg = _net(case)
    cd = util.cfg_dict(cfg)
    y, yl, ss, st, eps = _inputs(case)

    def run():
        net.voice_conversion(y, yl, ss, st, eps_q=eps)
        torch.cuda.synchronize()
        return {k: v.detach().cpu() for k, v in net._last_vc.items()}

    f32 = run()
    net.set_flow_dtype(dtype)
    got = run()
    for dec in (torch.bfloat16, torch.float16, torch.float32):
        net.set_decoder_dtype(dec)
        again = run()
        for k in ("z", "m_q", "logs_q"):
            assert torch.equal(again[k], f32[k]), (k, dec)
    net.set_flow_dtype(torch.float32)
    for k in ("z", "m_q", "logs_q"):
        assert torch.equal(got[k], f32[k]), k
    W = util.vc_weights(cfg, *util.vc_case_model(case, SPEC)[1:])
    g = F.embedding(ss.cpu(), W["emb_g.weight"]).unsqueeze(-1)
    ym = got["y_mask"].unsqueeze(1)
    with torch.no_grad():
        spec = vo().flow_forward(W, cd, got["z"], ym, g, wn_dtype=dtype)
    valid = ym.bool().expand_as(spec)
    r_spec = util.rel_rms(got["z_p"][valid].numpy(), spec[valid].numpy())
    r_f32 = util.rel_rms(got["z_p"][valid].numpy(), f32["z_p"][valid].numpy())
    print(name, dtype, "forward flow z_p vs 16-bit spec", r_spec, "vs f32 mode", r_f32)
    assert np.isfinite(got["z_p"].numpy()).all()
    assert r_spec < (1e-2 if dtype == torch.bfloat16 else 2e-3)


# ---- f. the device noise draw is the Philox stream at the generator's offset -------------------------------------
def test_device_posterior_draw_is_philox_at_generator_offset():
    """eps_q=None: z == (m_q + philox_randn(n, seed, offset) * exp(logs_q)) * y_mask with (seed, offset) read from the
    default CUDA generator before the call, and the offset advanced as SynthesizerTrn._randn documents (a multiple of
    4 covering ceil(n / 4) Philox counters)."""
    net, _, _ = _model("tiny")
    B, Ty, lengths = 3, 23, [1, 23, 12]
    y, yl, ss, st, _ = _batch(B, SPEC, Ty, lengths, seed=3)
    torch.manual_seed(97)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    seed, offset = gen.initial_seed(), int(gen.get_offset())
    _, y_mask, (z, _, _) = net.voice_conversion(y.cuda(), yl.cuda(), ss.cuda(), st.cuda())
    torch.cuda.synchronize()
    n = B * 192 * Ty
    assert int(gen.get_offset()) == offset + ((n + 3) // 4 + 3) // 4 * 4
    eps = torch.from_numpy(vo().philox_randn(n, seed, offset).astype(np.float64)).view(B, 192, Ty)
    m_q, logs_q = net._last_vc["m_q"].cpu().double(), net._last_vc["logs_q"].cpu().double()
    want = (m_q + eps * torch.exp(logs_q)) * y_mask.cpu().double()
    rel = util.rel_rms(z.cpu().numpy(), want.numpy())
    print("device draw vs Philox: rel RMS", rel)
    assert rel < 1e-6
