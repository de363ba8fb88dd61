"""Teacher-forced reconstruction oracle (test infrastructure): float64 restatements of the four operations of
csrc/losses.hip on top of tests/align_oracle.py, and the loader of tests/golden/recon_*.npz.

Used by tests/golden/make_golden_recon.py, tests/test_cpu_recon.py (the oracle pinned to the reference's fixtures) and
tests/test_gpu_recon.py."""
import os

import numpy as np

from tests import align_oracle as ao, util

RECON_CASES = ["recon_" + n[len("align_"):] for n in ao.ALIGN_CASES]
MEL_CASES = ["recon_vits2_v1_b2", "recon_aishell3_b4x600"]  # hop 256: the mel settings of the recipes apply
# mel settings of the hop-256 recipes (examples/*/configs/*.json: filter_length, hop_length, win_length, n_mel_channels,
# mel_fmin, mel_fmax); the sampling rate is the config's
MEL = dict(filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, mel_fmin=0.0, mel_fmax=None)
# relative gate on loss_mel against the reference's fixture (tests/test_gpu_recon.py), and through its factor of ten the
# condition under which tests/golden/make_golden_recon.py writes a mel fixture.  4 x the worst relative difference
# measured on an MI355X over the two hop-256 cases (2.30e-7 and 0; profiles/recon_margins.txt); the code is
# deterministic f32, so the margin is for later compiler changes, not for noise.
MEL_GATE = 9.3e-7


def segment_of(name):
    """Frames of the decoder slice of a fixture: 8 for the two hop-256 cases, 4 for the tiny configs."""
    return 8 if name in MEL_CASES else 4


def slice_ids(u, lengths, segment):
    """commons.py:54-56 with the clamp: int64(f32(u) * f32(len - segment + 1)) truncated toward zero, clamped into
    [0, len - segment] (the clamp acts for u = 1.0 only); a row shorter than the segment gets 0.
    -> (ids int64 [B], short bool [B])."""
    u = np.asarray(u, np.float32)
    last = np.asarray(lengths, np.int64) - int(segment)
    prod = (u * (last + 1).astype(np.float32)).astype(np.float32)  # one float32 rounding, as the tensor product
    ids = np.clip(np.trunc(prod.astype(np.float64)).astype(np.int64), 0, np.maximum(last, 0))
    return np.where(last < 0, 0, ids), last < 0


def slice_segments(x, ids, segment, scale=1):
    """commons.py:41-47 (x numpy [B,C,T]) -> [B, C, segment * scale] taken at ids * scale."""
    x = np.asarray(x)
    return np.stack([x[b, :, int(i) * scale:(int(i) + segment) * scale] for b, i in enumerate(np.asarray(ids))])


def kl_terms(z_p, logs_q, m_p, logs_p, mask):
    """The masked terms of losses.py:56-58 in float64 -> [B, I, T]; mask [B, T]."""
    z_p, logs_q, m_p, logs_p = (np.asarray(a, np.float64) for a in (z_p, logs_q, m_p, logs_p))
    kl = logs_p - logs_q - 0.5 + 0.5 * (z_p - m_p) ** 2 * np.exp(-2.0 * logs_p)
    return kl * np.asarray(mask, np.float64)[:, None, :]


def kl_loss(z_p, logs_q, m_p, logs_p, mask):
    """-> dict(total, per_utt [B], abs_total = sum|terms| / sum(mask), abs_per_utt [B]) in float64."""
    t = kl_terms(z_p, logs_q, m_p, logs_p, mask)
    n = np.asarray(mask, np.float64).sum(-1)
    return dict(total=t.sum() / n.sum(), per_utt=t.sum((1, 2)) / n, abs_total=np.abs(t).sum() / n.sum(),
                abs_per_utt=np.abs(t).sum((1, 2)) / n)


def l1_loss(a, b):
    """F.l1_loss (mean) in float64 -> dict(total, per_utt [B])."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).reshape(len(a), -1)
    return dict(total=d.mean(), per_utt=d.mean(-1))


def shifted_ids(ids, lengths, segment):
    """Every id moved by one frame, forward where the slice still fits and back otherwise: the off-by-one slice the mel
    gate has to be able to see."""
    ids, last = np.asarray(ids, np.int64), np.asarray(lengths, np.int64) - int(segment)
    return np.where(ids + 1 <= last, ids + 1, ids - 1)


def load_recon_case(name):
    """A fixture of make_golden_recon.py joined with the alignment fixture it extends (inputs rebuilt from seeds)."""
    c = ao.load_align_case("align_" + name[len("recon_"):])
    d = np.load(os.path.join(util.GOLDEN, name + ".npz"))
    assert int(d["noise_seed"]) == int(c["noise_seed"]), "recon fixture was generated from another alignment fixture"
    c.update({k: d[k] for k in d.files})
    return c
