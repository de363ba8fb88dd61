"""The generator-side losses of the reference's training loop that need no discriminator (losses.kl_loss,
losses.py:45-60, the mel L1 of train.py:486 and the duration loss of train.py:485) as evaluation metrics on the device,
and `teacher_forced_losses`, which does for one batch what train.py:400-432,485-488 does with
SynthesizerTrn.reconstruct() and SynthesizerTrn.duration_loss()'s stages in the place of forward().  No gradients; torch
allocates and takes views, the arithmetic is the HIP kernels of csrc/losses.hip and csrc/duration_loss.hip.

Every sum is formed in a fixed order without floating-point atomics (csrc/losses.hip): results repeat bit for bit, and
an utterance's per-utterance value is the same alone and inside a padded batch, which is what makes it usable for
finding the bad transcript or the clipped recording in a corpus.  The duration loss (`l_length`, models.py:198-207: the
stochastic duration predictor's nll + logq, or the DurationPredictor's squared error) divides by the whole batch's
phoneme count as the reference does; `dur_per_utt` is each utterance's own sum over its own phoneme count.
"""
import torch

from . import _lib, commons
from .mel_processing import mel_spectrogram_torch, spec_to_mel_torch


def _f32(t, name, dim, device=None):
    if not torch.is_tensor(t) or t.dim() != dim:
        raise ValueError(f"{name} must be a {dim}-d tensor, got {getattr(t, 'shape', type(t))}")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be on a HIP device (there is no CPU path)")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    return t.to(dtype=torch.float32).contiguous()


def kl_loss(z_p, logs_q, m_p, logs_p, z_mask, *, per_utterance=False):
    """losses.py:45-60: sum(kl * z_mask) / sum(z_mask) with kl = logs_p - logs_q - 1/2 + 1/2 (z_p - m_p)^2
    exp(-2 logs_p); tensors [B, I, T], z_mask [B, 1, T] or [B, T].  The divisor counts frames, as the reference's does.
    Returns the loss as a 0-d device tensor, or (loss, per_utt [B]) with `per_utterance=True`: each utterance's own
    masked sum over its own frame count."""
    total, per_utt = _kl(z_p, logs_q, m_p, logs_p, z_mask, 1.0)
    return (total[0], per_utt) if per_utterance else total[0]


def _kl(z_p, logs_q, m_p, logs_p, z_mask, weight):
    """kl_loss -> (total [2] = (loss, weight * loss), per_utt [B])."""
    z_p = _f32(z_p, "z_p", 3)
    B, I, T = z_p.shape
    ts = [_f32(t, n, 3, z_p.device) for t, n in ((logs_q, "logs_q"), (m_p, "m_p"), (logs_p, "logs_p"))]
    for t, n in zip(ts, ("logs_q", "m_p", "logs_p")):
        if tuple(t.shape) != (B, I, T):
            raise ValueError(f"{n} must be [{B},{I},{T}], got {tuple(t.shape)}")
    if not torch.is_tensor(z_mask) or tuple(z_mask.shape) not in ((B, 1, T), (B, T)):
        raise ValueError(f"z_mask must be [{B},1,{T}] or [{B},{T}], got {getattr(z_mask, 'shape', type(z_mask))}")
    mask = _f32(z_mask.reshape(B, T), "z_mask", 2, z_p.device)
    if B < 1:
        raise ValueError("kl_loss of an empty batch")
    partials = torch.empty(2, B, dtype=torch.float32, device=z_p.device)
    per_utt = torch.empty(B, dtype=torch.float32, device=z_p.device)
    total = torch.empty(2, dtype=torch.float32, device=z_p.device)
    with torch.cuda.device(z_p.device):
        _lib.check(_lib.load().wetts_kl_loss(_lib.ptr(z_p), _lib.ptr(ts[0]), _lib.ptr(ts[1]), _lib.ptr(ts[2]),
                                             _lib.ptr(mask), B, I, T, float(weight), _lib.ptr(partials),
                                             _lib.ptr(per_utt), _lib.ptr(total), _lib.current_stream_ptr()), "kl_loss")
    return total, per_utt


def l1_loss(a, b, *, per_utterance=False):
    """F.l1_loss(a, b) with its default mean, for two equally shaped tensors whose first dimension is the batch.
    Returns a 0-d device tensor, or (loss, per_utt [B]) with `per_utterance=True`: each row's own mean."""
    total, per_utt = _l1(a, b, 1.0)
    return (total[0], per_utt) if per_utterance else total[0]


def _l1(a, b, weight):
    """l1_loss -> (total [2] = (loss, weight * loss), per_utt [B])."""
    if not torch.is_tensor(a) or not torch.is_tensor(b) or a.dim() < 1 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"a and b must be equally shaped tensors, got {getattr(a, 'shape', type(a))} and "
                         f"{getattr(b, 'shape', type(b))}")
    a = _f32(a, "a", a.dim())
    b = _f32(b, "b", b.dim(), a.device)
    B = a.shape[0]
    N = a.numel() // B if B else 0
    if B < 1 or N < 1:
        raise ValueError("l1_loss of an empty tensor")
    partials = torch.empty(B, dtype=torch.float32, device=a.device)
    per_utt = torch.empty(B, dtype=torch.float32, device=a.device)
    total = torch.empty(2, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().wetts_l1_loss(_lib.ptr(a), _lib.ptr(b), B, N, float(weight), _lib.ptr(partials),
                                             _lib.ptr(per_utt), _lib.ptr(total), _lib.current_stream_ptr()), "l1_loss")
    return total, per_utt


def _flag(section, key):
    return key in section.keys() and bool(section[key])


def teacher_forced_losses(net_g, hps, x, x_lengths, spec, spec_lengths, sid=None, with_duration=False, e_q=None,
                          eps_w=None, **reconstruct_kwargs):
    """train.py:400-432,486-488 for one batch, without gradients: net_g.reconstruct(...) in the place of net_g(...), the
    target mel (`spec` itself for a mel posterior encoder, else spec_to_mel_torch(spec)) sliced at ids_slice, the mel
    spectrogram of the decoded slice, and
        loss_mel = l1_loss(y_mel, y_hat_mel) * hps.train.c_mel
        loss_kl = kl_loss(z_p, logs_q, m_p, logs_p, z_mask) * hps.train.c_kl.
    `reconstruct_kwargs` go to reconstruct() (segment_size in frames -- default: the model's --, ids_slice, eps_q).

    Returns a dict of device tensors: loss_mel, loss_kl (weighted scalars), mel, kl (unweighted scalars), mel_per_utt,
    kl_per_utt [B] (unweighted; an utterance's value does not depend on the batch it is scored in), y_hat
    [B, 1, segment * hop], ids_slice [B], y_mel and y_hat_mel [B, n_mel, segment].  The weights are applied by the
    reduction kernels (their `weight` argument), so no torch arithmetic runs.

    `with_duration=True` adds the duration loss of train.py:485 on the alignment reconstruct() found: the duration
    predictor's stages of SynthesizerTrn.duration_loss() on reconstruct()'s own w, x_enc, x_mask and g (no second text
    encoder pass; `e_q` / `eps_w` [B,2,Tx] inject its draws), and the entries loss_dur (sum_b l_length[b], weighted by
    hps.train.c_dur where the recipe has one, else 1), dur (unweighted) and dur_per_utt [B].  It costs one more
    read-back of the status word."""
    d = hps.data
    if int(net_g.hop_length) != int(d.hop_length):
        raise ValueError(f"the model produces {net_g.hop_length} samples per frame but hps.data.hop_length is "
                         f"{d.hop_length}: the mel spectrogram of the decoded slice would not line up with the target")
    o, ids_slice, attn, x_mask, z_mask, (z, z_p, m_p, logs_p, m_q, logs_q) = net_g.reconstruct(
        x, x_lengths, spec, spec_lengths, sid=sid, **reconstruct_kwargs)
    seg = o.shape[2] // int(net_g.hop_length)
    spec = _f32(spec.to(o.device) if torch.is_tensor(spec) else torch.as_tensor(spec).to(o.device), "spec", 3)
    if _flag(hps.model, "use_mel_posterior_encoder") or _flag(d, "use_mel_posterior_encoder"):
        mel = spec
    else:
        mel = spec_to_mel_torch(spec, d.filter_length, d.n_mel_channels, d.sampling_rate, d.mel_fmin, d.mel_fmax)
    y_mel = commons.slice_segments(mel, ids_slice, seg)
    y_hat_mel = mel_spectrogram_torch(o[:, 0], d.filter_length, d.n_mel_channels, d.sampling_rate, d.hop_length,
                                      d.win_length, d.mel_fmin, d.mel_fmax)
    if tuple(y_hat_mel.shape) != tuple(y_mel.shape):
        raise ValueError(f"mel of the decoded slice is {tuple(y_hat_mel.shape)}, the target slice {tuple(y_mel.shape)}: "
                         "filter_length / hop_length / win_length do not give one frame per hop")
    mel_total, mel_per_utt = _l1(y_mel, y_hat_mel, float(hps.train.c_mel))
    kl_total, kl_per_utt = _kl(z_p, logs_q, m_p, logs_p, z_mask, float(hps.train.c_kl))
    out = dict(loss_mel=mel_total[1], loss_kl=kl_total[1], mel=mel_total[0], kl=kl_total[0], mel_per_utt=mel_per_utt,
               kl_per_utt=kl_per_utt, y_hat=o, ids_slice=ids_slice, y_mel=y_mel, y_hat_mel=y_hat_mel)
    if with_duration:
        c_dur = float(hps.train.c_dur) if "c_dur" in hps.train.keys() else 1.0
        dur = net_g._duration_from_recon(e_q, eps_w, c_dur)
        out.update(loss_dur=dur["total"][1], dur=dur["total"][0], dur_per_utt=dur["per_utt"])
    return out
