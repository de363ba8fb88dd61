#!/usr/bin/env python3
"""Generates the duration-loss golden vectors (tests/golden/dur_*.npz) by running the REAL reference's duration
predictor (imported unmodified through oracle/ref_import.py) as SynthesizerTrn.forward runs it (models.py:196-206),
under no_grad and eval, on seeded synthetic checkpoints.  Run in the build container only:

    python tests/golden/make_golden_dur.py

One fixture per case of make_golden_align.CASES: the case's token ids (its token seed), lengths and speaker ids, and
its stored alignment's durations w = attn.sum(2).  The checkpoint is make_state_dict + make_posterior_state_dict of the
alignment case, extended by synth.make_duration_state_dict(cfg, duration_seed).  The two torch.randn draws of the
stochastic duration predictor (duration_predictors.py:229 e_q, :257 the reverse pass's z) are injected by shape
(B, 2, Tx), first call e_q, second call eps_w, and the call count is asserted.

Stored (a few KB each): e_q, eps_w, w, l_length, logw, logw_, the float64 oracle's abs_total and lens, the module's own
state_dict() keys and shapes under `dp.` (key_names / key_shapes), the seeds and the checksum of the duration blob."""
import contextlib
import io
import os
import sys
import unittest.mock as mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OUT, ROOT, build_reference  # noqa: E402
from make_golden_align import CASES, SPEC, build_unconditioned_reference  # noqa: E402

sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests import align_oracle as ao, duration_oracle as do, util  # noqa: E402
from wetts_amd import checkpoint, config, synth  # noqa: E402

ONLY = os.environ.get("WETTS_GOLDEN_ONLY")
DSEED_BASE = 181  # duration seed of a case = DSEED_BASE + its index in CASES; draw seed = duration seed + 40


def run_case(idx, name, spec):
    mname, n_vocab, n_spk, frames, xls, sids, wseed, pseed = spec[:8]
    align = util.load_case(name)
    dseed = DSEED_BASE + idx
    cfg = config.make_config(dict(config.MODEL_CONFIGS[mname]), n_vocab, n_spk)
    cd = util.cfg_dict(cfg)
    sd = synth.make_state_dict(cfg, wseed)
    dsd = synth.make_duration_state_dict(cfg, dseed)
    full_sd = dict(sd, **synth.make_posterior_state_dict(cfg, SPEC, pseed), **dsd)
    net = build_reference(mname, n_vocab, n_spk, full_sd) if n_spk > 0 else build_unconditioned_reference(mname, n_vocab,
                                                                                                          full_sd)
    assert not net.training
    B, Tx = len(xls), max(xls)
    x = torch.from_numpy(ao.align_tokens(int(align["token_seed"]), n_vocab, xls))
    x_len = torch.tensor(xls, dtype=torch.long)
    sid = torch.tensor(sids, dtype=torch.long)
    w = torch.from_numpy(np.asarray(align["w"], np.float32)).unsqueeze(1)
    assert tuple(w.shape) == (B, 1, Tx)
    rs = np.random.RandomState(dseed + 40)
    e_q = torch.from_numpy(rs.randn(B, 2, Tx).astype(np.float32))
    eps_w = torch.from_numpy(rs.randn(B, 2, Tx).astype(np.float32))
    real = torch.randn
    seen = {"n": 0}

    def fake_randn(*shape, **kw):
        shp = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        if shp == (B, 2, Tx):
            seen["n"] += 1
            return (e_q if seen["n"] == 1 else eps_w).clone()
        return real(*shape, **kw)

    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()), mock.patch.object(torch, "randn", fake_randn):
        g = net.emb_g(sid).unsqueeze(-1) if n_spk > 0 else None
        xe, _, _, x_mask = net.enc_p(x, x_len, g=g)
        if net.use_sdp:  # models.py:197-201
            l_length = net.dp(xe, x_mask, w, g=g)
            l_length = l_length / torch.sum(x_mask)
            logw = net.dp(xe, x_mask, g=g, reverse=True, noise_scale=1.0)
            logw_ = torch.log(w + 1e-6) * x_mask
        else:  # :203-206
            logw_ = torch.log(w + 1e-6) * x_mask
            logw = net.dp(xe, x_mask, g=g)
            l_length = torch.sum((logw - logw_) ** 2, [1, 2]) / torch.sum(x_mask)
    assert seen["n"] == (2 if net.use_sdp else 0), seen
    keys = [(k, tuple(v.shape)) for k, v in net.dp.state_dict().items()]
    W64 = {k: v.to(torch.float64) for k, v in checkpoint.fold_weight_norm(dict(sd, **dsd)).items()}
    st = do.stages(W64, cd, x, x_len, sid, w, e_q, eps_w)
    out = dict(model=mname, n_vocab=n_vocab, n_speakers=n_spk, weight_seed=wseed, posterior_seed=pseed,
               duration_seed=dseed, token_seed=int(align["token_seed"]), x_lengths=x_len.numpy(), sid=sid.numpy(),
               blob_checksum=synth.blob_checksum(checkpoint.pack_blob(cfg, sd)),
               duration_checksum=synth.blob_checksum(checkpoint.pack_duration_blob(cfg, dsd)) if dsd else 0.0,
               e_q=e_q.numpy(), eps_w=eps_w.numpy(), w=w[:, 0].numpy(), l_length=l_length.numpy(),
               logw=logw.numpy(), logw_=logw_.numpy(), abs_total=st["abs_total"].numpy(), lens=st["lens"].numpy(),
               oracle_l_length=st["l_length"].numpy(),
               key_names=np.array([k for k, _ in keys]), key_shapes=np.array([",".join(map(str, s)) for _, s in keys]))
    path = os.path.join(OUT, "dur_" + name[len("align_"):] + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path)} bytes  l_length {l_length.numpy()}  oracle {st['l_length'].numpy()}")


def main():
    if not ref_import.available():
        raise SystemExit("reference tree not found")
    ref_import.import_reference()
    for idx, (name, spec) in enumerate(CASES.items()):
        if ONLY and name not in ONLY.split(","):
            continue
        run_case(idx, name, spec)


if __name__ == "__main__":
    main()
