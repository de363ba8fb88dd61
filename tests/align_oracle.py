"""Forced-alignment oracle (test infrastructure): the teacher-forced pass up to the expanded prior composed from
oracle/vits_oracle.py's stages at a chosen precision, the alignment scores in float64, the reference's four-term f32
expression of the same scores (the yardstick of the scores kernel's error), and the loader of tests/golden/align_*.npz.

Used by tests/golden/make_golden_align.py (path stability of a fixture), tests/test_cpu_align.py (the oracle pinned to
the reference's fixtures) and tests/test_gpu_align.py."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vits_oracle as vo
from tests import util, vc_input
from wetts_amd import config

SPEC = vc_input.SPEC
ALIGN_CASES = ["align_tiny_b3", "align_vits2_v1_b2", "align_tiny_preconv2_spk_b3", "align_tiny_mono_post_b2",
               "align_tiny_mono_inter_b3", "align_tiny_vocos_b2", "align_tiny_dp_b2", "align_tiny_nospk_b2",
               "align_aishell3_b4x600"]
STAGES = ("z", "z_p", "m_p", "logs_p", "m_q", "logs_q")
LOG2PI = math.log(2.0 * math.pi)


def neg_cent_f64(z_p, m_p, logs_p):
    """sum_c ( -1/2 log 2pi - logs_p - 1/2 (z_p - m_p)^2 exp(-2 logs_p) ) in float64 -> [B, Ty, Tx]; z_p [B,I,Ty],
    m_p / logs_p [B,I,Tx] (unexpanded)."""
    z, m, ls = z_p.double(), m_p.double(), logs_p.double()
    r = torch.exp(-2.0 * ls)
    const = (-0.5 * LOG2PI - ls - 0.5 * m * m * r).sum(1, keepdim=True)  # [B,1,Tx]
    return torch.matmul((-0.5 * z * z).transpose(1, 2), r) + torch.matmul(z.transpose(1, 2), m * r) + const


def neg_cent_four_term(z_p, m_p, logs_p):
    """The reference's expression of the scores (models.py:173-184: two column sums and two matmuls, added in its
    order) in the dtype of its inputs."""
    r = torch.exp(-2 * logs_p)
    c1 = torch.sum(-0.5 * LOG2PI - logs_p, [1], keepdim=True)
    c2 = torch.matmul(-0.5 * (z_p ** 2).transpose(1, 2), r)
    c3 = torch.matmul(z_p.transpose(1, 2), m_p * r)
    c4 = torch.sum(-0.5 * (m_p ** 2) * r, [1], keepdim=True)
    return c1 + c2 + c3 + c4


def expand(path, stat):
    """models.py:209-212: [B,Ty,Tx] path x [B,I,Tx] -> [B,I,Ty]."""
    return torch.matmul(path.to(stat.dtype), stat.transpose(1, 2)).transpose(1, 2)


def path_score(neg_cent64, path):
    """Float64 score summed along each utterance's path -> [B]."""
    return (np.asarray(neg_cent64, np.float64) * np.asarray(path, np.float64)).sum(axis=(1, 2))


def valid_mask(x_lengths, y_lengths, Tx, Ty):
    xl, yl = np.asarray(x_lengths), np.asarray(y_lengths)
    return (np.arange(Ty)[None, :, None] < yl[:, None, None]) & (np.arange(Tx)[None, None, :] < xl[:, None, None])


def check_monotonic(path, x_lengths, y_lengths):
    """A valid monotonic path per utterance: one cell per valid frame and none elsewhere, from (0, 0) to
    (t_y - 1, t_x - 1), moving 0 or +1 phonemes per frame."""
    path = np.asarray(path)
    for b, (tx, ty) in enumerate(zip(np.asarray(x_lengths), np.asarray(y_lengths))):
        tx, ty = int(tx), int(ty)
        p = path[b]
        assert p[ty:].sum() == 0 and p[:, tx:].sum() == 0, b
        assert (p[:ty].sum(1) == 1).all(), b
        idx = p[:ty].argmax(1)
        assert idx[0] == 0 and idx[-1] == tx - 1, (b, idx[0], idx[-1])
        d = np.diff(idx)
        assert ((d == 0) | (d == 1)).all(), b


def oracle_align(W, cd, x, x_lengths, y, y_lengths, sid, eps, dtype=torch.float64):
    """forward()'s computation up to models.py:212 from the oracle's stages at `dtype` (W already of that dtype);
    the scores always in float64 from those stages.  Returns a dict of tensors (path / attn as int32 numpy)."""
    with torch.no_grad():
        g = F.embedding(sid, W["emb_g.weight"]).unsqueeze(-1) if cd["n_speakers"] > 0 else None
        _, m_p, logs_p, x_mask = vo.text_encoder(W, cd, x, x_lengths, g)
        z, m_q, logs_q, y_mask = vo.posterior_encoder(W, cd, y.to(dtype), y_lengths, g, eps.to(dtype))
        z_p = vo.flow_forward(W, cd, z, y_mask, g)
        nc = neg_cent_f64(z_p, m_p, logs_p)
    path = vo.maximum_path_numpy(nc.numpy(), y_lengths.numpy(), x_lengths.numpy())
    pt = torch.from_numpy(path)
    return dict(z=z, z_p=z_p, m_q=m_q, logs_q=logs_q, m_p=expand(pt, m_p), logs_p=expand(pt, logs_p), m_p_x=m_p,
                logs_p_x=logs_p, x_mask=x_mask, y_mask=y_mask, neg_cent=nc, path=path,
                w=torch.from_numpy(path.sum(1).astype(np.float32)))


def align_noise(seed, shape):
    """The frozen standard-normal stream injected as the posterior draw (as make_golden_vc.py:vc_noise)."""
    return np.random.RandomState(int(seed)).standard_normal(shape).astype(np.float32)


def align_tokens(seed, n_vocab, x_lengths):
    """Seeded phoneme ids [B, max(x_lengths)], zero beyond each row's length."""
    rs = np.random.RandomState(int(seed))
    x = np.zeros((len(x_lengths), max(x_lengths)), np.int64)
    for b, n in enumerate(x_lengths):
        x[b, :n] = rs.randint(0, n_vocab, size=n)
    return x


def load_align_case(name):
    """A fixture of make_golden_align.py with its inputs rebuilt: the spectrogram from tests/vc_input.py (held to the
    recorded sums), the token ids and the injected draw from their seeds."""
    d = np.load(os.path.join(util.GOLDEN, name + ".npz"))
    c = {k: d[k] for k in d.files}
    frames = [int(v) for v in c["y_lengths"]]
    y = vc_input.make_input(frames, int(c["sampling_rate"]), int(c["input_seed"]))
    for got, ref in zip(vc_input.input_sums(y), c["y_sums"]):
        assert abs(got - float(ref)) <= 1e-6 * abs(float(ref)), "rebuilt input differs from the fixture's"
    c["y"] = y.numpy()
    c["x"] = align_tokens(int(c["token_seed"]), int(c["n_vocab"]), [int(v) for v in c["x_lengths"]])
    I = config.MODEL_CONFIGS[str(c["model"])]["inter_channels"]
    c["eps"] = align_noise(c["noise_seed"], (len(frames), I, max(frames)))
    return c


def case_tensors(c):
    """(x, x_lengths, y, y_lengths, sid, eps) of a loaded fixture as CPU tensors."""
    return (torch.from_numpy(c["x"]), torch.from_numpy(c["x_lengths"]), torch.from_numpy(c["y"]),
            torch.from_numpy(c["y_lengths"]), torch.from_numpy(c["sid"]), torch.from_numpy(c["eps"]))
