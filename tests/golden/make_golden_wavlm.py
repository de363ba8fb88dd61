#!/usr/bin/env python3
"""Generates the WavLM golden vectors (tests/golden/wavlm_{tiny,wide}_r{rate}_b{B}x{L}.npz and the two known-answer files)
by running the REAL reference's WavLMLoss (losses.py:63-153) and WavLMDiscriminator (model/discriminators.py:452-498),
imported unmodified, around transformers' own WavLMModel, on the seeded synthetic weights of
synth.make_wavlm_state_dict / make_wavlm_discriminator_state_dict.  Run in the build container only:

    python tests/golden/make_golden_wavlm.py

`transformers` is imported first, for real; then oracle/ref_import.py's stubs go in, and the torchaudio stub's
transforms.Resample is set HERE to tests/wavlm_oracle.ResampleStandIn: torchaudio is not installed, so the resampler in
these fixtures is a restatement of torchaudio's published arithmetic, NOT torchaudio -- the one non-reference piece.
A WavLMModel(config) carrying the synthetic weights is written with save_pretrained into a temporary directory, and the
reference's WavLMLoss is constructed on that directory (its AutoModel.from_pretrained runs).  No pretrained weights are
involved and none are stored.

Stored per config and shape of wavlm_oracle.SHAPES: the seeds, the reference's float32 resampled audio (wide: of the
first row), ALL hidden states of every row as `hidden` where that keeps the file under 1 MiB -- every case but wide at 65
frames x 4 rows and at 130 frames, which keep `hidden_last`: the last hidden state of the first real and the first
generated row --, discriminator outputs [2B, T] and the three losses from the reference's
own methods (loss_lm at B = 1 from the reference's model and formula: its forward() squeezes the batch away there and
fails), and the float32 floors floor_<figure> = (rel RMS, max |d| / rms) of the reference's float32 pass against the
float64 oracle (floor_loss_*_per_utt: its hidden states and outputs reduced per row by the oracle's formula),
floor_<stage> = torch's float32 evaluation of a stand-alone stage against its float64 evaluation; each the worst over the
config's shapes.

SENSITIVITY is a condition of a fixture: at the shapes of at least 18 frames (where every bucket range is reached) each
injected defect of wavlm_oracle.FAULTS must move its figure to at least 10 x the gate; the figures are stored as
sens_<fault>."""
import os
import sys
import tempfile

import numpy as np
import torch

import transformers  # noqa: F401  (first, for real: the stubs below must not shadow anything it imports)
from transformers import WavLMConfig, WavLMModel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests import wavlm_oracle as wo  # noqa: E402

SENS_MIN_FRAMES = 18
HIDDEN_BYTES = 900_000  # all hidden states are stored where they leave the file under 1 MiB
SENS_FACTOR = 10.0


def import_reference():
    ref_import.install_stubs()
    sys.modules["torchaudio"].transforms.Resample = wo.ResampleStandIn
    if ref_import.REF_VITS not in sys.path:
        sys.path.insert(0, ref_import.REF_VITS)
    from losses import WavLMLoss  # noqa
    from model.discriminators import WavLMDiscriminator  # noqa
    return WavLMLoss, WavLMDiscriminator


def build_reference(cname, rate, tmp):
    WavLMLoss, WavLMDiscriminator = import_reference()
    (sd, _), (dd, _) = wo.weights(cname)
    path = os.path.join(tmp, f"wavlm-{cname}")
    if not os.path.isdir(path):
        model = WavLMModel(WavLMConfig(**wo.HF_CONFIGS[cname]))
        res = model.load_state_dict(sd, strict=False)  # masked_spec_embed exists only with mask_time_prob > 0
        assert not res.missing_keys and set(res.unexpected_keys) <= {"masked_spec_embed"}, res
        model.save_pretrained(path, safe_serialization=False)
    c = wo.HF_CONFIGS[cname]
    wd = WavLMDiscriminator(c["hidden_size"], wo.slm_layers(cname), wo.INITIAL_CHANNEL[cname])
    wd.load_state_dict(dd, strict=True)
    wl = WavLMLoss(path, wd, rate, wo.SLM_SR)
    wl.eval()
    return wl


def sensitivity_ok(fig, gate):
    return fig[0] >= SENS_FACTOR * gate[0] and fig[1] >= SENS_FACTOR * gate[1]


def make_case(cname, shape, wl):
    rate, L, B = shape
    seed = wo.case_seed(shape)
    wav, rec = wo.inputs(shape, seed)
    both = torch.cat([wav, rec], 0)
    with torch.no_grad():
        res32 = wl.resample(both)
        hid32 = wl.wavlm(input_values=res32, output_hidden_states=True).hidden_states
        d32 = wl.discriminator_forward(both)
        if B > 1:
            lm32 = wl(wav, rec)
        else:
            lm32 = sum(torch.mean(torch.abs(h[:B] - h[B:])) for h in hid32)
        gen32 = wl.generator(rec)
        slm32 = wl.discriminator(wav, rec)
        o = wo.forward(cname, shape, wav, rec)
        T = o["hidden"][0].shape[1]
        assert T == wo.frames(cname, res32.shape[1]) and len(hid32) == wo.slm_layers(cname)
        out = dict(input_seed=seed, wseed=wo.WSEED, dseed=wo.DSEED, frames=T, resampled_len=res32.shape[1],
                   d=d32.numpy(), loss_lm=float(lm32), loss_lm_gen=float(gen32), loss_slm=float(slm32))
        hid = torch.stack(hid32, 0)
        out["resampled"] = (res32 if cname == "tiny" else res32[:1]).numpy()
        if hid.numel() * 4 <= HIDDEN_BYTES:
            out["hidden"] = hid.numpy()
        else:
            out["hidden_last"] = hid32[-1][[0, B]].numpy()
        out["floor_resample"] = wo.gates(res32, o["resampled"])
        fl = None
        for a, r in zip(hid32, o["hidden"]):
            fl = wo.worst(fl, wo.gates(a, r))
        out["floor_hidden"] = fl
        out["floor_d"] = wo.gates(d32, o["d"])
        for k, v in (("loss_lm", lm32), ("loss_lm_gen", gen32), ("loss_slm", slm32)):
            out["floor_" + k] = wo.rel_err(v, o[k])
        # the per-utterance forms have no counterpart in the reference: its float32 hidden states and outputs reduced
        # per row (wavlm_oracle.losses) against the float64 oracle
        pu32 = wo.losses(list(hid32), d32, B)
        for k in ("loss_lm", "loss_lm_gen", "loss_slm"):
            out["floor_" + k + "_per_utt"] = wo.gates(pu32[k + "_per_utt"], o[k + "_per_utt"])
        (sd, W64), (dd, D64) = wo.weights(cname)
        for stage, (inp, fn) in wo.stage_cases(cname, shape, wav, rec).items():
            out["floor_" + stage] = wo.gates(fn(sd, dd, inp), fn(W64, D64, inp))
        if T >= SENS_MIN_FRAMES:
            for f in wo.faults(cname):
                bad = wo.forward(cname, shape, wav, rec, fault=f)
                if wo.FAULT_STAGE[f] == "disc":
                    out["sens_" + f] = wo.gates(bad["d"], o["d"])
                else:
                    out["sens_" + f] = wo.gates(bad["hidden"][-1], o["hidden"][-1])
    return {k: np.asarray(v) for k, v in out.items()}


def make_kats():
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    rel = torch.arange(-2047, 2048)
    out = dict(rel=rel.numpy())
    for nb, md in ((16, 12), (320, 800)):
        att = WavLMAttention(embed_dim=16, num_heads=4, num_buckets=nb, max_distance=md)
        out[f"bucket_{nb}_{md}"] = att._relative_positions_bucket(rel).numpy().astype(np.int32)
    np.savez_compressed(os.path.join(wo.GOLDEN, "wavlm_bucket_kat.npz"), **out)
    model = WavLMModel(WavLMConfig(**wo.HF_CONFIGS["tiny"]))
    L = torch.arange(400, 2001)
    np.savez_compressed(os.path.join(wo.GOLDEN, "wavlm_lengths_kat.npz"), samples=L.numpy(),
                        frames=model._get_feat_extract_output_lengths(L).numpy())


def main():
    torch.manual_seed(0)
    make_kats()
    with tempfile.TemporaryDirectory() as tmp:
        for cname in wo.CONFIGS:
            cases = {shape: make_case(cname, shape, build_reference(cname, shape[0], tmp)) for shape in wo.SHAPES}
            # A floor is the worst over the config's shapes (tests/frontend_oracle.py's convention): one case's figure is
            # ONE draw of a rounding error -- for a loss scalar it can land near zero by luck -- and says little about
            # the next input; the worst of the seven is the better estimate of what float32 does to this network.
            floors = {}
            for case in cases.values():
                for k, v in case.items():
                    if k.startswith("floor_"):
                        floors[k] = np.asarray(wo.worst(tuple(floors[k]) if k in floors else None, tuple(v)))
            for shape, case in cases.items():
                case.update(floors)
                for f in wo.faults(cname):
                    if "sens_" + f not in case:
                        continue
                    gate = wo.gate_of(case["floor_d" if wo.FAULT_STAGE[f] == "disc" else "floor_hidden"])
                    if not sensitivity_ok(case["sens_" + f], gate):
                        raise SystemExit(f"{wo.case_name(cname, shape)}: defect {f} moves its figure to {case['sens_' + f]}, "
                                         f"less than {SENS_FACTOR} x the gate {gate}: the fixture would not see it")
                path = os.path.join(wo.GOLDEN, wo.case_name(cname, shape) + ".npz")
                np.savez_compressed(path, **case)
                print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, T = {int(case['frames'])}, floor_hidden = "
                      f"{case['floor_hidden']}, floor_d = {case['floor_d']}, loss_lm = {float(case['loss_lm']):.6f}", flush=True)
                assert os.path.getsize(path) <= 1 << 20, path


if __name__ == "__main__":
    main()
