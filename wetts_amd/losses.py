"""The losses of the reference's training loop -- losses.kl_loss (losses.py:45-60), the mel L1 of train.py:486, the
duration loss of train.py:485, and the adversarial terms discriminator_loss / generator_loss / feature_loss
(losses.py:6-42, csrc/discriminator.hip) -- as evaluation metrics on the device, and `teacher_forced_losses`, which does for one batch what train.py:400-432,485-488 does with
SynthesizerTrn.reconstruct() and SynthesizerTrn.duration_loss()'s stages in the place of forward().  No gradients; torch
allocates and takes views, the arithmetic is the HIP kernels of csrc/losses.hip and csrc/duration_loss.hip.

Every sum is formed in a fixed order without floating-point atomics (csrc/losses.hip): results repeat bit for bit, and
an utterance's per-utterance value is the same alone and inside a padded batch, which is what makes it usable for
finding the bad transcript or the clipped recording in a corpus.  The duration loss (`l_length`, models.py:198-207: the
stochastic duration predictor's nll + logq, or the DurationPredictor's squared error) divides by the whole batch's
phoneme count as the reference does; `dur_per_utt` is each utterance's own sum over its own phoneme count.
"""
import ctypes as C

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


def _rows(t, like=None):
    """-> (tensor kept alive, batch stride, N): utterance b of `t` [B, ...] owns N contiguous floats at
    data_ptr + b * stride.  A permuted view whose utterances are contiguous blocks (the period stacks' feature maps) is
    taken as it lies -- a sum over an utterance does not care in which order the block is laid out, as long as real and
    generated agree (`like`: the partner's strides); anything else is copied."""
    B = t.shape[0]
    N = t.numel() // B
    if t.dtype == torch.float32 and (like is None or like == t.stride()):
        order = sorted(range(1, t.dim()), key=lambda i: -t.stride(i))
        if t.permute(0, *order).is_contiguous():
            return t, N, N
    return t.to(torch.float32).contiguous(), N, N


MAX_ITEMS = 128  # WETTS_DISC_LOSSES_MAX_ITEMS: the MPMRD's 93 feature maps fit


def _disc_reduce(kind, reals, gens, scale, what):
    """wetts_disc_losses over the tensor pairs -> (total [1], item_a [n], item_g [n], per_utt [B])."""
    reals = list(reals)
    gens = list(gens) if gens is not None else None
    n = len(reals)
    if n < 1 or n > MAX_ITEMS or (gens is not None and len(gens) != n):
        raise ValueError(f"{what}: needs 1 .. {MAX_ITEMS} tensors (and as many generated as real), got {n}")
    dev, B = None, None
    a, g = [], []
    for i in range(n):
        pair = (reals[i],) if gens is None else (reals[i], gens[i])
        for t in pair:
            if not torch.is_tensor(t) or t.dim() < 1 or t.numel() < 1:
                raise ValueError(f"{what}: item {i} must be a non-empty tensor whose first dimension is the batch")
            if t.device.type != "cuda":
                raise ValueError(f"{what}: item {i} must be on a HIP device (there is no CPU path)")
            dev, B = (t.device, t.shape[0]) if dev is None else (dev, B)
            if t.device != dev or t.shape[0] != B:
                raise ValueError(f"{what}: item {i} is [{t.shape[0]}, ...] on {t.device}, expected [{B}, ...] on {dev}")
        if gens is not None and tuple(pair[0].shape) != tuple(pair[1].shape):
            raise ValueError(f"{what}: item {i}: {tuple(pair[0].shape)} against {tuple(pair[1].shape)}")
        same = gens is None or pair[0].stride() == pair[1].stride()
        a.append(_rows(pair[0]) if same else _rows(pair[0].contiguous()))
        if gens is not None:
            g.append(_rows(pair[1], a[-1][0].stride()))
    P, I64 = C.c_void_p * n, C.c_int64 * n
    sums = torch.empty(2 * n * B, dtype=torch.float64, device=dev)
    item_a = torch.empty(n, dtype=torch.float32, device=dev)
    item_g = torch.empty(n, dtype=torch.float32, device=dev)
    per_utt = torch.empty(B, dtype=torch.float32, device=dev)
    total = torch.empty(1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().wetts_disc_losses(
            kind, n, P(*[t.data_ptr() for t, _, _ in a]), P(*[t.data_ptr() for t, _, _ in g]) if g else None,
            I64(*[s for _, s, _ in a]), I64(*[s for _, s, _ in g]) if g else None, I64(*[N for _, _, N in a]), B,
            float(scale), _lib.ptr(sums), _lib.ptr(item_a), _lib.ptr(item_g), _lib.ptr(per_utt), _lib.ptr(total),
            _lib.current_stream_ptr()), what)
    return total, item_a, item_g, per_utt


def feature_loss(fmap_r, fmap_g, *, per_utterance=False):
    """losses.py:6-14: 2 * sum over every layer of every discriminator of mean |real - generated|.  Returns a 0-d
    device tensor, or (loss, per_utt [B]) with `per_utterance=True`: the same from each utterance's own elements."""
    total, _, _, per_utt = _feature(fmap_r, fmap_g)
    return (total[0], per_utt) if per_utterance else total[0]


def _feature(fmap_r, fmap_g):
    """feature_loss -> (total [1], per-layer mean |r - g| [n], unused, per_utt [B])."""
    return _disc_reduce(0, [l for d in fmap_r for l in d], [l for d in fmap_g for l in d], 2.0, "feature_loss")


def discriminator_loss(disc_real_outputs, disc_generated_outputs, *, per_utterance=False):
    """losses.py:17-30: sum over the discriminators of mean (1 - dr)^2 + mean dg^2.  Returns (loss, r_losses, g_losses)
    -- a 0-d device tensor and two device tensors [n] (the reference's lists of floats, without the read-back) --,
    with `per_utterance=True` also per_utt [B]."""
    total, r, g, per_utt = _disc_reduce(1, disc_real_outputs, disc_generated_outputs, 1.0, "discriminator_loss")
    return (total[0], r, g, per_utt) if per_utterance else (total[0], r, g)


def generator_loss(disc_outputs, *, per_utterance=False):
    """losses.py:33-42: sum over the discriminators of mean (1 - dg)^2.  Returns (loss, gen_losses [n]), with
    `per_utterance=True` also per_utt [B]."""
    total, gl, _, per_utt = _disc_reduce(2, disc_outputs, None, 1.0, "generator_loss")
    return (total[0], gl, per_utt) if per_utterance else (total[0], gl)


def _duration_disc_losses(net_dur_disc, x_enc, x_mask, logw_, logw):
    """train.py:441-453,481-495 on one call of the duration discriminator -> the entries teacher_forced_losses adds.
    The reference's zip over what the class returns decides the terms: DurationDiscriminatorV1 hands back two tensors,
    so discriminator_loss / generator_loss iterate over their BATCH ROWS -- B terms, each a mean over one utterance's Tx
    padded positions, summed: B x the one-mean value, which the reducer's `scale` carries.  DurationDiscriminatorV2
    hands back two one-element lists: one term over B * Tx."""
    B, _, Tx = x_enc.shape
    prob_r, prob_g = net_dur_disc._probs(x_enc, x_mask.reshape(B, 1, Tx), logw_.reshape(B, 1, Tx), logw.reshape(B, 1, Tx))
    mask = _f32(x_mask.reshape(B, Tx), "x_mask", 2, prob_r.device)
    r_rows, g_rows, gen_rows, disc_pu, gen_pu = (torch.empty(B, dtype=torch.float32, device=prob_r.device)
                                                 for _ in range(5))
    with torch.cuda.device(prob_r.device):
        _lib.check(_lib.load().wetts_durdisc_row_means(_lib.ptr(prob_r), _lib.ptr(prob_g), _lib.ptr(mask), B, Tx,
                                                       _lib.ptr(r_rows), _lib.ptr(g_rows), _lib.ptr(gen_rows),
                                                       _lib.ptr(disc_pu), _lib.ptr(gen_pu), _lib.current_stream_ptr()),
                   "durdisc_row_means")
    per_row = getattr(net_dur_disc, "VERSION", 2) == 1
    scale = float(B) if per_row else 1.0
    disc, r1, g1, _ = _disc_reduce(1, [prob_r], [prob_g], scale, "duration discriminator_loss")
    gen, n1, _, _ = _disc_reduce(2, [prob_g], None, scale, "duration generator_loss")
    return dict(loss_dur_disc=disc[0], losses_dur_disc_r=r_rows if per_row else r1,
                losses_dur_disc_g=g_rows if per_row else g1, loss_dur_gen=gen[0],
                losses_dur_gen=gen_rows if per_row else n1, dur_disc_per_utt=disc_pu, dur_gen_per_utt=gen_pu)


def _flag(section, key):
    return key in section.keys() and bool(section[key])


def teacher_forced_losses(net_g, hps, x, x_lengths, spec, spec_lengths, sid=None, with_duration=False, e_q=None,
                          eps_w=None, net_d=None, y=None, net_dur_disc=None, wl=None, **reconstruct_kwargs):
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
    read-back of the status word.

    `net_d` (a MultiPeriodDiscriminator or a MultiPeriodMultiResolutionDiscriminator) with `y`, the batch's waveform [B, 1, T_wav], adds the adversarial terms of
    train.py:431-439,480-491: y is sliced at ids_slice * hop, net_d(y_slice, y_hat) runs once, and the entries are
    loss_disc, loss_gen, loss_fm (scalars), loss_disc_per_utt, loss_gen_per_utt, loss_fm_per_utt [B], losses_disc_r,
    losses_disc_g and losses_gen (one per discriminator), and y_slice [B, 1, segment * hop].  Without `net_d` nothing changes.

    `net_dur_disc` (a DurationDiscriminatorV1 or V2; needs `with_duration=True`, whose stage supplies x_enc, x_mask,
    logw_ and logw) adds train.py:441-453,481-495: net_dur_disc(x_enc, x_mask, logw_, logw) runs once, and the entries
    are loss_dur_disc, loss_dur_gen (scalars), losses_dur_disc_r, losses_dur_disc_g, losses_dur_gen -- the reference's
    values for the class in use: B terms and their sum for V1, whose two returned tensors the reference's zip walks row
    by row (each term a mean over ALL Tx positions, as train.py:446 notes), one term for V2 -- and dur_disc_per_utt,
    dur_gen_per_utt [B]: each utterance's mean over its own phonemes, which does not depend on the batch (NaN for an
    utterance without any).  Without `net_dur_disc` nothing changes.

    `wl` (a WavLMLoss; needs `y`, which may then come without `net_d`) adds train.py:467-471,496-498 on y_slice and
    y_hat: loss_slm = wl.discriminator(y_slice, y_hat), loss_lm = wl(y_slice, y_hat), loss_lm_gen = wl.generator(y_hat)
    (scalars) and loss_slm_per_utt, loss_lm_per_utt, loss_lm_gen_per_utt [B], from ONE WavLM pass over the 2B rows.
    Without `wl` nothing changes."""
    d = hps.data
    if net_dur_disc is not None and not with_duration:
        raise ValueError("net_dur_disc needs with_duration=True: its inputs are that stage's x_enc, x_mask, logw_ and logw")
    if wl is None and (net_d is None) != (y is None):
        raise ValueError("net_d and y (the batch's waveform [B, 1, T_wav]) go together")
    if wl is not None and y is None:
        raise ValueError("wl needs y (the batch's waveform [B, 1, T_wav]): its terms compare y's slice with y_hat")
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
        if net_dur_disc is not None:
            out.update(_duration_disc_losses(net_dur_disc, net_g._last_recon["x_enc"], dur["x_mask"], dur["logw_"],
                                             dur["logw"]))
    if net_d is not None:
        y_slice = commons.slice_segments(y, ids_slice, seg, scale=int(net_g.hop_length))
        y_d_r, y_d_g, fmap_r, fmap_g = net_d(y_slice, o)
        loss_disc, r_losses, g_losses, disc_pu = discriminator_loss(y_d_r, y_d_g, per_utterance=True)
        loss_gen, gen_losses, gen_pu = generator_loss(y_d_g, per_utterance=True)
        loss_fm, fm_pu = feature_loss(fmap_r, fmap_g, per_utterance=True)
        out.update(loss_disc=loss_disc, loss_gen=loss_gen, loss_fm=loss_fm, loss_disc_per_utt=disc_pu,
                   loss_gen_per_utt=gen_pu, loss_fm_per_utt=fm_pu, losses_disc_r=r_losses, losses_disc_g=g_losses,
                   losses_gen=gen_losses, y_slice=y_slice)
    if wl is not None:
        out.update(wl.all_terms(commons.slice_segments(y, ids_slice, seg, scale=int(net_g.hop_length)), o))
    return out


class WavLMLoss:
    """losses.py:63-153 as an evaluation module on the device: `model` a transformers WavLM directory (config.json and
    pytorch_model.bin; nothing is downloaded) or a wetts_amd.wavlm.WavLM, `wd` a WavLMDiscriminator (None: only
    __call__ works), `model_sr` / `slm_sr` the rates of the resampler in front of WavLM -- a stand-in for
    torchaudio.transforms.Resample, see wetts_amd/wavlm.py.  Waveforms are [B, L] or [B, 1, L] device tensors.

        wl(wav, y_rec)                sum over the hidden states of mean |h(wav) - h(y_rec)|          (loss_lm)
        wl.generator(y_rec)           mean (1 - wd(h(y_rec)))^2                                       (loss_lm_gen)
        wl.discriminator(wav, y_rec)  mean (1 - wd(h(wav)))^2 + mean wd(h(y_rec))^2                   (loss_slm)
        wl.discriminator_forward(wav) wd(h(wav)) [B, T]

    Each returns a 0-d device tensor, or (loss, per_utt [B]) with `per_utterance=True`: the same from each utterance's
    own elements.  wav and y_rec run through the resampler and WavLM as ONE batch of 2B rows; a row's values do not
    depend on the batch, so the halves equal two calls bit for bit.  B = 1 works: the reference's `.squeeze()` drops the
    batch dimension there and its WavLM call fails.  No gradients."""

    def __init__(self, model, wd, model_sr, slm_sr=16000):
        from . import wavlm
        self.wavlm = model if isinstance(model, wavlm.WavLM) else wavlm.load_wavlm(model)
        self.wd = wd
        self.resample = wavlm.Resample(model_sr, slm_sr)
        if wd is not None and (wd.slm_layers != self.wavlm.num_layers + 1 or wd.slm_hidden != self.wavlm.hidden_size):
            raise ValueError(f"wd expects {wd.slm_layers} hidden states of {wd.slm_hidden} channels, WavLM gives "
                             f"{self.wavlm.num_layers + 1} of {self.wavlm.hidden_size}")

    def to(self, device):
        self.wavlm.to(device)
        if self.wd is not None:
            self.wd.to(device)
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))

    def eval(self):
        return self

    @staticmethod
    def _rows(t, name):
        if not torch.is_tensor(t) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[1] != 1):
            raise ValueError(f"{name} must be a [B, L] or [B, 1, L] tensor, got {getattr(t, 'shape', type(t))}")
        if t.device.type != "cuda":
            raise ValueError(f"{name} must be on a HIP device (there is no CPU path)")
        t = t.to(torch.float32)
        return t.reshape(t.shape[0], t.shape[-1])

    def hidden(self, *waves):
        """The waveforms ([B, L] or [B, 1, L], one shape) as one batch -> [layers + 1, rows, T, hidden]."""
        rows = [self._rows(w, "waveform") for w in waves]
        for r in rows[1:]:
            if tuple(r.shape) != tuple(rows[0].shape) or r.device != rows[0].device:
                raise ValueError(f"the waveforms must have one shape and device, got {tuple(rows[0].shape)} and {tuple(r.shape)}")
        x = rows[0] if len(rows) == 1 else torch.cat(rows, 0)
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"empty waveform {tuple(x.shape)}")
        n = self.resample.output_length(x.shape[1]) if self.resample.orig_freq != self.resample.new_freq else x.shape[1]
        if self.wavlm.num_frames(n) < 1:  # before the resampler's launches
            raise ValueError(f"{x.shape[1]} samples ({n} at the WavLM rate) are shorter than one WavLM frame")
        if self.resample.orig_freq != self.resample.new_freq:
            buf, n = self.resample._run(x)
            x = buf[:, :n]
        return self.wavlm._hidden(x)

    def _need_wd(self):
        if self.wd is None:
            raise ValueError("this WavLMLoss has no discriminator (wd=None)")

    def _lm(self, h, B):
        total, _, _, pu = _disc_reduce(0, [l[:B] for l in h.unbind(0)], [l[B:] for l in h.unbind(0)], 1.0, "WavLM loss")
        return total[0], pu

    def forward(self, wav, y_rec, *, per_utterance=False):
        h = self.hidden(wav, y_rec)
        loss, pu = self._lm(h, h.shape[1] // 2)
        return (loss, pu) if per_utterance else loss

    __call__ = forward

    def generator(self, y_rec, *, per_utterance=False):
        self._need_wd()
        total, _, pu = generator_loss([self.wd.on_hidden(self.hidden(y_rec))], per_utterance=True)
        return (total, pu) if per_utterance else total

    def discriminator(self, wav, y_rec, *, per_utterance=False):
        self._need_wd()
        d = self.wd.on_hidden(self.hidden(wav, y_rec))
        B = d.shape[0] // 2
        total, _, _, pu = discriminator_loss([d[:B]], [d[B:]], per_utterance=True)
        return (total, pu) if per_utterance else total

    def discriminator_forward(self, wav):
        self._need_wd()
        return self.wd.on_hidden(self.hidden(wav))

    def all_terms(self, wav, y_rec):
        """The three terms of a training step from one pass over the 2B rows -> dict loss_slm, loss_lm, loss_lm_gen and
        their _per_utt [B]."""
        self._need_wd()
        h = self.hidden(wav, y_rec)
        B = h.shape[1] // 2
        lm, lm_pu = self._lm(h, B)
        d = self.wd.on_hidden(h)
        slm, _, _, slm_pu = discriminator_loss([d[:B]], [d[B:]], per_utterance=True)
        gen, _, gen_pu = generator_loss([d[B:]], per_utterance=True)
        return dict(loss_slm=slm, loss_lm=lm, loss_lm_gen=gen, loss_slm_per_utt=slm_pu, loss_lm_per_utt=lm_pu,
                    loss_lm_gen_per_utt=gen_pu)
