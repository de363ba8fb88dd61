"""SynthesizerTrn -- drop-in for the reference's inference surface
(wetts/vits/model/models.py:14-363) running on hand-written gfx950 HIP kernels through the
C ABI in include/wetts_hip.h.  PyTorch is used for device memory, streams and nothing else:
there is no eager / CPU fallback anywhere in this module.

Same constructor arguments, same `infer` / `infer_encoder` / `export_*` / `voice_conversion` signatures and
return tuples as the reference; training (`forward`) is out of scope and raises.  The posterior
encoder (`enc_q`) is loaded when the checkpoint carries it and runs only inside `voice_conversion` and `align`
(forced alignment: forward()'s computation up to the expanded prior, models.py:161-212).

Extra, optional keyword arguments (not in the reference): `eps_w` / `eps_z` inject the two
standard-normal draws the reference makes with torch.randn (duration_predictors.py:257,
models.py:267) so results can be compared bit-for-noise with a CPU run.  Without them the draws
come from the library's Philox kernel (`wetts_randn`), driven by the device generator's (seed, offset) so
that torch.manual_seed() makes a run reproducible the way it does for the reference.

One host synchronisation per infer(): y_lengths and the device status word (errors the reference
raises from inside its modules: IndexError of nn.Embedding, the spline's discriminant assert) come
back in ONE D2H copy.
"""
import ctypes as C
import os

import torch

from . import _lib, checkpoint, commons, config as _config


class _Workspace:
    """Grow-only device scratch (one per model; the kernels themselves never allocate).

    Grows with 25 % headroom: the frame count of a batch is data dependent (durations are sampled), so a
    buffer sized to the request would be re-allocated every time a batch sets a new maximum -- a multi-GB
    hipMalloc in the middle of serving (seen as 75-88 ms bench steps instead of 73 on a fresh process)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = None  # release the old block to the caching allocator first
            self.buf = torch.empty(int(nbytes) + int(nbytes) // 4, dtype=torch.uint8, device=device)
        return self.buf


class _FoldedPart:
    """`net_g.dec` / `net_g.flow` as far as the reference's export prelude touches them (export_onnx.py:79-81): weight
    norm is folded into the weights when a checkpoint is loaded (checkpoint.fold_weight_norm), so removing it is a
    no-op here."""

    def remove_weight_norm(self):
        return None


class SynthesizerTrn:
    """Inference-only synthesizer with the reference's constructor signature (models.py:19-51)."""

    def __init__(self, n_vocab, spec_channels, segment_size, inter_channels, hidden_channels,
                 filter_channels, n_heads, n_layers, kernel_size, p_dropout, resblock,
                 resblock_kernel_sizes, resblock_dilation_sizes, upsample_rates,
                 upsample_initial_channel, upsample_kernel_sizes, n_speakers=0, gin_channels=0,
                 use_sdp=True, vocoder_type="hifigan", **kwargs):
        self.n_vocab = n_vocab
        self.spec_channels = spec_channels
        self.segment_size = segment_size
        self.inter_channels = inter_channels
        self.hidden_channels = hidden_channels
        self.n_speakers = n_speakers
        self.gin_channels = gin_channels
        self.use_sdp = use_sdp
        self.upsample_rates = list(upsample_rates)
        model = dict(inter_channels=inter_channels, hidden_channels=hidden_channels,
                     filter_channels=filter_channels, n_heads=n_heads, n_layers=n_layers,
                     kernel_size=kernel_size, p_dropout=p_dropout, resblock=resblock,
                     resblock_kernel_sizes=resblock_kernel_sizes,
                     resblock_dilation_sizes=resblock_dilation_sizes,
                     upsample_rates=upsample_rates,
                     upsample_initial_channel=upsample_initial_channel,
                     upsample_kernel_sizes=upsample_kernel_sizes, gin_channels=gin_channels,
                     use_sdp=use_sdp, vocoder_type=vocoder_type, **kwargs)
        self.cfg = _config.make_config(model, n_vocab, n_speakers)
        self.vocoder_type = vocoder_type
        self.is_onnx = bool(self.cfg.is_onnx)  # models.py:50,111: the Vocos head's iSTFT (see set_is_onnx)
        self.hop_length = 1
        for u in upsample_rates:
            self.hop_length *= int(u)
        if vocoder_type == "vocos":  # samples per frame = the iSTFT hop (decoders.py:279,304)
            self.hop_length = int(self.cfg.istft_hop_length)
        self.device = torch.device("cpu")
        self._blob = None      # CPU float32 blob (weights live here until .to(device))
        self._post_blob = None  # CPU float32 blob of enc_q.* (voice conversion), when the checkpoint carries it
        self._post_on_device = False  # uploaded by the first voice_conversion() call (wetts_load_posterior_encoder)
        self._dur_blob = None  # CPU float32 blob of dp.flows.1.* / dp.post_* (duration_loss), when the checkpoint has them
        self._dur_on_device = False  # uploaded by the first duration_loss() call (wetts_load_duration_posterior)
        self._handle = None    # wetts_model_t*
        self._ws = _Workspace()
        self._ws_dec = _Workspace()  # the decoder's own scratch in overlap mode (see set_overlap)
        self._enc_stream = None
        self.overlap = False
        self._debug_overlap = bool(os.environ.get("WETTS_DEBUG_OVERLAP"))  # check the overlap contract on every call
        self.dec = _FoldedPart()
        self.flow = _FoldedPart()
        self.quiet = True      # the reference prints stage timers on every call (:273-279)
        self.last_status = 0

    # ---- nn.Module-shaped plumbing the reference's callers use -------------------------------
    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("training is out of scope of the MI355X inference path")
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device != self.device:
            self._destroy()
            self.device = device
            if self._blob is not None and device.type == "cuda":
                self._create()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def set_decoder_dtype(self, dtype, fused=True, serial=False):
        """HiFi-GAN arithmetic: torch.float32 (default, parity-gated), torch.bfloat16 or
        torch.float16 (16-bit activations/weights, f32 accumulation; encoder / duration / flow stay f32).
        `fused=False` runs every ResBlock1 (c1, c2) pair as two conv launches instead of the fused
        LDS-resident kernel -- bit-identical, for diagnostics.  `serial=True` keeps the f32 decoder's launches on the
        caller's stream one after the other instead of running a stage's three ResBlock chains on three streams --
        bit-identical; the form in which a kernel trace's per-kernel durations do not overlap."""
        prec = {torch.float32: 0, "f32": 0, "fp32": 0, torch.bfloat16: 1, "bf16": 1,
                torch.float16: 2, "f16": 2, "fp16": 2,
                # the `export_onnx.py --quant` variant (export_onnx.py:149-157): uint8 dynamic quantisation
                torch.uint8: 3, torch.quint8: 3, "uint8": 3, "u8": 3}[dtype]
        if not fused:
            prec |= 0x10  # WETTS_DECODER_UNFUSED
        if serial:
            prec |= 0x20  # WETTS_DECODER_SERIAL: one launch after the other on the caller's stream (measurement)
        self._decoder_precision = prec
        if self._handle is not None:
            _lib.check(_lib.load().wetts_set_decoder_precision(self._handle, prec),
                       "set_decoder_precision")
        return self

    def set_is_onnx(self, on=True):
        """The `is_onnx` ctor flag of the reference (models.py:50,111) on a live model: which iSTFT a Vocos head ends in
        (decoders.py:300-304).  False: torchaudio's InverseSpectrogram == torch.istft -- what `infer()` of the PyTorch CLI
        (inference.py) computes.  True: OnnxSTFT.inverse (utils/stft.py:325-340; conv_transpose1d with
        pinv(scale * basis)^T * hann, no window-envelope division) -- what every graph export_onnx.py writes computes,
        because that script forces hps.model.is_onnx = True (export_onnx.py:59).  At hop = n_fft / 4 the interior of
        the two differs by the factor 0.375, the first / last n_fft/2 samples also in shape.  HiFi-GAN models take the
        flag without effect, like the reference.  The ORT-shaped sessions (session.py) switch to True for their calls."""
        self.is_onnx = bool(on)
        self.cfg.is_onnx = int(self.is_onnx)
        if self._handle is not None:
            _lib.check(_lib.load().wetts_set_istft_mode(self._handle, int(self.is_onnx)), "set_istft_mode")
        return self

    def set_flow_dtype(self, dtype):
        """Arithmetic of the flow's WaveNet layers: torch.float32 (default, parity-gated),
        torch.bfloat16 or torch.float16 (16-bit activations / weights, f32 accumulation, f32 skip
        sum).  BASELINE.json configs[2] precision for the flow."""
        prec = {torch.float32: 0, "f32": 0, "fp32": 0, torch.bfloat16: 1, "bf16": 1,
                torch.float16: 2, "f16": 2, "fp16": 2}[dtype]
        self._flow_precision = prec
        if self._handle is not None:
            _lib.check(_lib.load().wetts_set_flow_precision(self._handle, prec),
                       "set_flow_precision")
        return self

    def set_overlap(self, on=True):
        """Back-to-back calls as a two-stage pipeline (not in the reference).  With overlap on, the encoder stages of
        an infer() call -- text encoder, durations, flow: a few hundred small launches that cannot fill the chip --
        run on a side stream and therefore BESIDE whatever the caller's stream still holds, in a serving loop the
        previous call's decoder; the decoder waits for them by an event and runs on the caller's stream with its own
        workspace.  Results are identical; every returned tensor is safe to use on the caller's stream.  Contract: the
        input tensors of a call must already be materialised when it is made -- they are read on the side stream
        without waiting for the caller's stream (waiting would put the call behind the previous decoder again).  Device
        tensors that exist before the serving loop starts, or that come from `upload()`, satisfy it."""
        if bool(on) != self.overlap and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)  # the two modes share the encoder workspace differently: drain first
        self.overlap = bool(on)
        return self

    def _new_enc_stream(self):
        """The side stream of overlap mode (stream priorities were measured in round 5: not a lever)."""
        return torch.cuda.Stream(device=self.device)

    def upload(self, t, dtype=None, consumer="encoder", non_blocking=False):
        """Host tensor / array -> device tensor on the stream that will read it.  `consumer="encoder"` (ids, lengths,
        speaker ids: what infer() / infer_encoder() read): the caller's stream, or in overlap mode the encoder's side
        stream, whose work is NOT ordered behind the caller's stream (see set_overlap).  `consumer="decoder"` (a z chunk
        for export_decoder_forward / hifigan): always the caller's stream, where the decoder runs in either mode.
        `non_blocking=True` (opt-in, pinned sources only): the call returns before the copy has finished -- the copy is
        stream-ordered in front of its reader, but the CALLER must not refill the pinned buffer until that stream has
        passed it (a serving loop that reuses one staging buffer would otherwise overwrite ids still in flight); the
        default waits for the copy, like `tensor.to(device)` of a pageable source.  The wetts_amd hosts (sessions,
        batching, CLI) put their inputs on the device through this."""
        t = torch.as_tensor(t)
        nb = bool(non_blocking and t.device.type == "cpu" and t.is_pinned())
        if consumer != "encoder" or not (self.overlap and self.device.type == "cuda"):
            return t.to(device=self.device, dtype=dtype, non_blocking=nb)
        if self._enc_stream is None:
            self._enc_stream = self._new_enc_stream()
        with torch.cuda.stream(self._enc_stream):
            out = t.to(device=self.device, dtype=dtype, non_blocking=nb)
        if not nb and t.device.type == "cpu" and t.is_pinned():
            self._enc_stream.synchronize()  # (a pinned source is copied asynchronously on a non-default stream)
        return out

    def blob_layout(self):
        return checkpoint.blob_layout(self.cfg)

    def load_state_dict(self, state_dict, strict=True):
        """Accepts the reference's `G_*.pth["model"]` dict (weight-norm pairs folded here).  The posterior encoder's
        `enc_q.*` tensors are kept (as a host blob, uploaded by the first voice_conversion() call) when the dict carries
        all of them; a dict without them loads as before and voice_conversion() then raises."""
        self._blob = checkpoint.pack_blob(self.cfg, state_dict, strict=strict)
        self._post_blob = None
        if checkpoint.has_posterior(self.cfg, self.spec_channels, state_dict):
            self._post_blob = checkpoint.pack_posterior_blob(self.cfg, self.spec_channels, state_dict)
        self._dur_blob = None  # the SDP's forward-only tensors, kept the same way for duration_loss()
        if checkpoint.has_duration(self.cfg, state_dict):
            self._dur_blob = checkpoint.pack_duration_blob(self.cfg, state_dict)
        self._destroy()
        if self.device.type == "cuda":
            self._create()
        return self

    def state_dict(self):
        """The module's tensors under the reference's `state_dict()` keys (utils/task.py:59-76 saves
        `model.state_dict()`), read back from the model's own memory.  Weight-norm pairs are stored folded, so
        `dec.ups.0.weight` stands where the reference has `weight_g` / `weight_v` -- the spelling
        `remove_weight_norm()` leaves (decoders.py:84-88) and `load_state_dict` accepts.  Tensors live on the
        module's device (views of one blob), like nn.Module.state_dict()."""
        from collections import OrderedDict
        n = checkpoint.blob_numel(self.cfg)
        if self._handle is not None:
            blob = torch.empty(n, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().wetts_get_blob(self._handle, _lib.ptr(blob), n, _lib.current_stream_ptr()),
                           "get_blob")
        elif self._blob is not None:
            blob = self._blob
        else:
            raise _lib.WettsError("no weights loaded: call load_state_dict(...) first")
        sd = OrderedDict((name, blob[off:off + numel].view(shape))
                         for name, off, numel, shape in checkpoint.blob_layout(self.cfg))
        if self.is_onnx and self.vocoder_type == "vocos":
            # the two buffers OnnxSTFT registers (utils/stft.py:289-290); constants of the config, not of the checkpoint
            fwd, inv = _onnx_stft_bases(int(self.cfg.istft_n_fft), int(self.cfg.istft_hop_length))
            sd["dec.stft.forward_basis"] = fwd.to(blob.device)
            sd["dec.stft.inverse_basis"] = inv.to(blob.device)
        if self._post_blob is not None:  # enc_q.* (folded), only when the loaded checkpoint carried them
            pb = self._post_blob.to(blob.device)
            for name, off, numel, shape in checkpoint.posterior_layout(self.cfg, self.spec_channels):
                sd[name] = pb[off:off + numel].view(shape)
        if self._dur_blob is not None:  # dp.flows.1.* / dp.post_*, only when the loaded checkpoint carried them
            db = self._dur_blob.to(blob.device)
            for name, off, numel, shape in checkpoint.duration_layout(self.cfg):
                sd[name] = db[off:off + numel].view(shape)
        return sd

    def load_blob(self, blob):
        """Adopts an already packed float32 blob (CPU or device tensor), e.g. after a broadcast."""
        n = checkpoint.blob_numel(self.cfg)
        if blob.dtype != torch.float32 or blob.numel() != n:
            raise ValueError(f"blob must be float32[{n}]")
        self._destroy()
        if blob.device.type == "cuda":
            self.device = blob.device
            self._blob = None
            self._create(dev_blob=blob.contiguous())
        else:
            self._blob = blob.contiguous()
            if self.device.type == "cuda":
                self._create()
        return self

    def _create(self, dev_blob=None):
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.WettsError("no HIP device visible; the product path has no CPU fallback")
        with torch.cuda.device(self.device):
            if dev_blob is None:
                dev_blob = self._blob.to(self.device)
            h = C.c_void_p()
            rc = lib.wetts_create(C.byref(self.cfg), _lib.ptr(dev_blob), dev_blob.numel(),
                                  _lib.current_stream_ptr(), C.byref(h))
            _lib.check(rc, "wetts_create")
            self._handle = h
            if getattr(self, "_decoder_precision", 0):
                _lib.check(lib.wetts_set_decoder_precision(h, self._decoder_precision),
                           "set_decoder_precision")
            if getattr(self, "_flow_precision", 0):
                _lib.check(lib.wetts_set_flow_precision(h, self._flow_precision),
                           "set_flow_precision")

    def _destroy(self):
        if self._handle is not None:
            _lib.load().wetts_destroy(self._handle)
            self._handle = None
        self._post_on_device = False
        self._dur_on_device = False

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _require(self):
        if self._handle is None:
            raise _lib.WettsError(
                "model is not on a HIP device with weights loaded: call load_state_dict(...) and "
                ".to('cuda') first (there is no CPU path)")
        return _lib.load()

    def _workspace(self, B, Tx, Ty):
        lib = _lib.load()
        n = lib.wetts_workspace_bytes(self._handle, B, Tx, Ty)
        if n < 0:
            raise _lib.WettsError("workspace_bytes failed")
        return self._ws.get(n, self.device), n

    # ---- out-of-scope training surface ---------------------------------------------------------
    def forward(self, *a, **k):
        raise NotImplementedError("SynthesizerTrn.forward (training, models.py:161-226) is out of "
                                  "scope; this is the inference hot path only")

    def __call__(self, *a, **k):
        # through the instance, like nn.Module: the reference's export scripts assign `net_g.forward =
        # net_g.export_forward` (export_onnx.py:82,94,127) and then call the module
        return self.forward(*a, **k)

    # ---- voice conversion (models.py:369-376) ------------------------------------------------------
    def _require_posterior(self):
        """The posterior encoder on the device: uploaded on first use, so a model used only for infer() holds no copy."""
        lib = self._require()
        if self._post_blob is None:
            raise _lib.WettsError("voice_conversion needs the posterior encoder, but the loaded checkpoint has no "
                                  "enc_q.* tensors")
        if not self._post_on_device:
            with torch.cuda.device(self.device):
                dev = self._post_blob.to(self.device)
                _lib.check(lib.wetts_load_posterior_encoder(self._handle, int(self.spec_channels), _lib.ptr(dev),
                                                            dev.numel(), _lib.current_stream_ptr()),
                           "load_posterior_encoder")
            self._post_on_device = True
        return lib

    def _flow_pass(self, z, y_mask, g, reverse, ws, nws):
        """flow(z, y_mask, g, reverse) on [B, inter, Ty] / [B, Ty] device tensors -> a new tensor."""
        lib = _lib.load()
        B, _, Ty = z.shape
        out = torch.empty_like(z)
        fn = lib.wetts_flow_reverse if reverse else lib.wetts_flow_forward
        _lib.check(fn(self._handle, _lib.ptr(z), _lib.ptr(y_mask), _lib.ptr(g), B, Ty, _lib.ptr(out), _lib.ptr(ws), nws,
                      _lib.current_stream_ptr()), "flow_reverse" if reverse else "flow_forward")
        return out

    def voice_conversion(self, y, y_lengths, sid_src, sid_tgt, eps_q=None):
        """models.py:369-376: the utterance in linear spectrogram `y` [B, spec_channels, Ty] (the reference's
        `spectrogram_torch(audio, filter_length, sampling_rate, hop_length, win_length)`), spoken by `sid_src`, in the
        voice of `sid_tgt`.  Returns (o_hat [B,1,Ty*hop], y_mask [B,1,Ty], (z, z_p, z_hat) [B,inter,Ty]).

        Stages: emb_g -> posterior encoder (g_src) -> flow (g_src) -> flow^-1 (g_tgt) -> dec(z_hat * y_mask, g_tgt),
        all on the caller's stream.  `eps_q` (optional, not in the reference) injects the torch.randn_like draw of the
        posterior sample (encoders.py:98); without it the draw comes from the library's Philox kernel on the device
        generator's stream, so torch.manual_seed makes a call reproducible as it does for infer().  Speaker ids outside
        the table raise IndexError after the call's one host read-back of the status word."""
        if self.n_speakers <= 0:  # the reference has no emb_g then (models.py:159-160)
            raise AttributeError("'SynthesizerTrn' object has no attribute 'emb_g'")
        lib = self._require_posterior()
        y = self._f32(y)
        if y.dim() != 3 or y.shape[1] != self.spec_channels:
            raise ValueError(f"y must be [B, {self.spec_channels}, Ty], got {tuple(y.shape)}")
        B, _, Ty = y.shape
        I = self.inter_channels
        y_lengths = self._ids(y_lengths)
        f32 = dict(dtype=torch.float32, device=self.device)
        if eps_q is None:
            eps_q = self._randn(B, I, Ty)
        else:
            eps_q = self._f32(eps_q)
            if tuple(eps_q.shape) != (B, I, Ty):
                raise ValueError(f"eps_q must be [{B},{I},{Ty}], got {tuple(eps_q.shape)}")
        # the decoder's own workspace in overlap mode (the encoder side stream may still be using self._ws)
        nws = max(int(lib.wetts_posterior_workspace_bytes(self._handle, B, Ty)),
                  int(lib.wetts_workspace_bytes(self._handle, B, 0, Ty)))
        ws = (self._ws_dec if self.overlap else self._ws).get(nws, self.device)
        s = _lib.current_stream_ptr()
        status = torch.empty(1, dtype=torch.int64, device=self.device)
        _lib.check(lib.wetts_set_status_word(self._handle, _lib.ptr(status), s), "set_status_word")
        try:
            sids = torch.stack([self._ids(sid_src).reshape(B), self._ids(sid_tgt).reshape(B)])
            g = torch.empty(2, B, self.gin_channels, **f32)
            _lib.check(lib.wetts_speaker_embedding(self._handle, _lib.ptr(sids), 2 * B, _lib.ptr(g), s),
                       "speaker_embedding")
        finally:
            lib.wetts_set_status_word(self._handle, None, s)
        g_src, g_tgt = g[0], g[1]
        z, m_q, logs_q = (torch.empty(B, I, Ty, **f32) for _ in range(3))
        y_mask = torch.empty(B, Ty, **f32)
        _lib.check(lib.wetts_posterior_encoder(self._handle, _lib.ptr(y), _lib.ptr(y_lengths), _lib.ptr(g_src),
                                               _lib.ptr(eps_q), B, Ty, _lib.ptr(z), _lib.ptr(m_q), _lib.ptr(logs_q),
                                               _lib.ptr(y_mask), _lib.ptr(ws), nws, s), "posterior_encoder")
        z_p = self._flow_pass(z, y_mask, g_src, False, ws, nws)
        z_hat = self._flow_pass(z_p, y_mask, g_tgt, True, ws, nws)
        o_hat = self._decode(z_hat, g_tgt, y_mask, Ty)
        self.last_status = int(status.cpu().item()) & 0xFFFFFFFF  # the call's one host sync
        if self.last_status & _lib.STATUS_SPEAKER_ID_RANGE:
            raise IndexError("index out of range in self (sid outside emb_g, models.py:370-371)")
        self._last_vc = dict(z=z, m_q=m_q, logs_q=logs_q, z_p=z_p, z_hat=z_hat, y_mask=y_mask, g_src=g_src,
                             g_tgt=g_tgt)
        return o_hat, y_mask.unsqueeze(1), (z, z_p, z_hat)

    # ---- forced alignment (models.py:161-212, the teacher-forced pass up to the expanded prior) -------------------
    def align(self, x, x_lengths, y, y_lengths, sid=None, eps_q=None):
        """Which frames of the recording `y` belong to which phoneme of `x`: forward()'s own computation up to
        models.py:212, without gradients.  x [B,Tx] phoneme ids, y [B, spec_channels, Ty] the spectrogram
        `posterior_spectrogram` returns, lengths [B].  Returns (attn [B,1,Ty,Tx], w [B,1,Tx], x_mask [B,1,Tx],
        y_mask [B,1,Ty], (z, z_p, m_p, logs_p, m_q, logs_q)) under forward()'s names and shapes, m_p / logs_p expanded
        to [B,inter,Ty]; w = attn.sum(2) are the phoneme durations in frames, exact integers.

        Stages, all on the caller's stream: emb_g -> text encoder -> posterior encoder (g) -> forward flow (g) ->
        alignment scores (models.py:173-184, one MFMA GEMM per utterance) -> monotonic alignment search -> path to
        durations -> length regulation.  One host read-back per call (the status word).  `eps_q` (optional, not in the
        reference) injects the posterior draw as in voice_conversion; without it the draw comes from the Philox kernel
        under torch.manual_seed.  With n_speakers == 0 no sid is needed (g = None), as in forward().

        `use_noise_scaled_mas` (models.py:186-189) anneals noise into the scores during training; this is the
        deterministic search and ignores it.  An utterance with more phonemes than frames has no monotonic alignment:
        the reference's search returns a meaningless path for it, here the call raises ValueError.  Ids outside their
        tables raise IndexError.  `infer(x, x_lengths, sid, durations=w)` resynthesises with the recording's timing."""
        x, y, B, Tx, Ty = self._align_args(x, x_lengths, y, y_lengths, sid, eps_q)
        status, st = self._align_stages(self._require_posterior(), x, x_lengths, y, y_lengths, sid, eps_q, B, Tx, Ty)
        self.last_status = int(status.cpu().item()) & 0xFFFFFFFF  # the call's one host sync
        self._align_raise()
        self._last_align = st
        return (st["attn"].unsqueeze(1), st["w"].unsqueeze(1), st["x_mask"].unsqueeze(1), st["y_mask"].unsqueeze(1),
                (st["z"], st["z_p"], st["m_p"], st["logs_p"], st["m_q"], st["logs_q"]))

    def _align_args(self, x, x_lengths, y, y_lengths, sid, eps_q):
        """The argument checks of align() / reconstruct(), before anything is launched -> (x, y, B, Tx, Ty)."""
        x = torch.as_tensor(x)
        y = torch.as_tensor(y)
        if x.dim() != 2:
            raise ValueError(f"x must be [B, Tx], got {tuple(x.shape)}")
        if y.dim() != 3 or y.shape[1] != self.spec_channels or y.shape[0] != x.shape[0]:
            raise ValueError(f"y must be [{x.shape[0]}, {self.spec_channels}, Ty], got {tuple(y.shape)}")
        B, Tx = x.shape
        Ty = y.shape[2]
        for name, t in (("x_lengths", x_lengths), ("y_lengths", y_lengths)):
            if tuple(torch.as_tensor(t).shape) != (B,):
                raise ValueError(f"{name} must be [{B}], got {tuple(torch.as_tensor(t).shape)}")
        if self.n_speakers > 0 and sid is None:
            raise ValueError("sid is required when n_speakers > 0")
        if eps_q is not None and tuple(eps_q.shape) != (B, self.inter_channels, Ty):
            raise ValueError(f"eps_q must be [{B},{self.inter_channels},{Ty}], got {tuple(eps_q.shape)}")
        return x, y, B, Tx, Ty

    def _align_stages(self, lib, x, x_lengths, y, y_lengths, sid, eps_q, B, Tx, Ty):
        """The launches of align() on checked arguments, without its read-back -> (status word tensor, stage dict).
        Shared by align() and reconstruct(); the status word stays readable until the caller fetches it."""
        I = self.inter_channels
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        x, x_lengths, y, y_lengths = self._ids(x), self._ids(x_lengths), self._f32(y), self._ids(y_lengths)
        eps_q = self._randn(B, I, Ty) if eps_q is None else self._f32(eps_q)
        nws = max(int(lib.wetts_workspace_bytes(self._handle, B, Tx, 0)),
                  int(lib.wetts_posterior_workspace_bytes(self._handle, B, Ty)),
                  int(lib.wetts_workspace_bytes(self._handle, B, 0, Ty)))
        ws = (self._ws_dec if self.overlap else self._ws).get(nws, dev)  # as voice_conversion: the side stream owns _ws
        s = _lib.current_stream_ptr()
        H = self.hidden_channels
        g_buf = torch.empty(B, max(1, self.gin_channels), **f32)
        g = g_buf if self.n_speakers > 0 else None
        x_enc, stats, x_mask = torch.empty(B, H, Tx, **f32), torch.empty(B, 2 * I, Tx, **f32), torch.empty(B, Tx, **f32)
        t_xs, t_ys = torch.empty(B, **i32), torch.empty(B, **i32)
        status = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.wetts_set_status_word(self._handle, _lib.ptr(status), s), "set_status_word")
        try:
            _lib.check(lib.wetts_speaker_embedding(self._handle, _lib.ptr(self._ids(sid)) if g is not None else None, B,
                                                   _lib.ptr(g_buf), s), "speaker_embedding")
            _lib.check(lib.wetts_text_encoder(self._handle, _lib.ptr(x), _lib.ptr(x_lengths), _lib.ptr(g), B, Tx,
                                              _lib.ptr(x_enc), _lib.ptr(stats), _lib.ptr(x_mask), _lib.ptr(ws), nws, s),
                       "text_encoder")
            _lib.check(lib.wetts_align_lengths(self._handle, _lib.ptr(x_lengths), _lib.ptr(y_lengths), B, Tx, Ty,
                                               _lib.ptr(t_xs), _lib.ptr(t_ys), s), "align_lengths")
        finally:
            lib.wetts_set_status_word(self._handle, None, s)
        z, m_q, logs_q = (torch.empty(B, I, Ty, **f32) for _ in range(3))
        y_mask = torch.empty(B, Ty, **f32)
        _lib.check(lib.wetts_posterior_encoder(self._handle, _lib.ptr(y), _lib.ptr(y_lengths), _lib.ptr(g),
                                               _lib.ptr(eps_q), B, Ty, _lib.ptr(z), _lib.ptr(m_q), _lib.ptr(logs_q),
                                               _lib.ptr(y_mask), _lib.ptr(ws), nws, s), "posterior_encoder")
        z_p = self._flow_pass(z, y_mask, g, False, ws, nws)
        # caller-owned, as in monotonic_align.maximum_path: the scores, the search's value table and the int32 path
        neg_cent = torch.empty(B, Ty, Tx, **f32)
        values = torch.empty(max(1, B * Ty * Tx), **f32)
        path = torch.empty(B, Ty, Tx, **i32)
        _lib.check(lib.wetts_align_scores(self._handle, _lib.ptr(z_p), _lib.ptr(stats), B, Tx, Ty, _lib.ptr(neg_cent), s),
                   "align_scores")
        _lib.check(lib.wetts_mas(_lib.ptr(neg_cent), _lib.ptr(t_ys), _lib.ptr(t_xs), B, Ty, Tx, _lib.ptr(path),
                                 _lib.ptr(values), values.numel() * 4, s), "wetts_mas")
        w, cum = torch.empty(B, Tx, **f32), torch.empty(B, Tx, **f32)
        f2p = torch.empty(B, Ty, **i32)
        attn = torch.empty(B, Ty, Tx, **f32)
        _lib.check(lib.wetts_path_to_durations(_lib.ptr(path), _lib.ptr(t_ys), _lib.ptr(t_xs), B, Tx, Ty, _lib.ptr(w),
                                               _lib.ptr(cum), _lib.ptr(f2p), _lib.ptr(attn), s), "path_to_durations")
        # models.py:209-212 through the kernel infer() expands the prior with: noise_scale = 0, its z_p output unused
        m_p, logs_p, unused = (torch.empty(B, I, Ty, **f32) for _ in range(3))
        f2p_lr, y_mask_lr = torch.empty(B, Ty, **i32), torch.empty(B, Ty, **f32)
        _lib.check(lib.wetts_length_regulate(self._handle, _lib.ptr(stats), _lib.ptr(cum), _lib.ptr(x_mask),
                                             _lib.ptr(y_lengths), _lib.ptr(z_p), I * Ty, Ty, 0.0, B, Tx, Ty,
                                             _lib.ptr(f2p_lr), _lib.ptr(y_mask_lr), None, _lib.ptr(m_p),
                                             _lib.ptr(logs_p), _lib.ptr(unused), s), "length_regulate")
        st = dict(g=g, x_enc=x_enc, stats=stats, x_mask=x_mask, y_mask=y_mask, z=z, m_q=m_q, logs_q=logs_q,
                  z_p=z_p, neg_cent=neg_cent, path=path, t_xs=t_xs, t_ys=t_ys, w=w, cum=cum,
                  frame2phone=f2p, attn=attn, m_p=m_p, logs_p=logs_p)
        return status, dict(st, y_lengths=y_lengths)

    def _align_raise(self):
        """What align() raises from the status word it read back (self.last_status)."""
        if self.last_status & _lib.STATUS_PHONE_ID_RANGE:
            raise IndexError("index out of range in self (phoneme id outside emb, encoders.py:48)")
        if self.last_status & _lib.STATUS_SPEAKER_ID_RANGE:
            raise IndexError("index out of range in self (sid outside emb_g, models.py:163)")
        if self.last_status & _lib.STATUS_ALIGN_TEXT_LONGER:
            raise ValueError("align: an utterance has more phonemes than frames (x_lengths[b] > y_lengths[b]); no "
                             "monotonic alignment exists")

    # ---- teacher-forced reconstruction (models.py:161-226 without the duration loss) ---------------------------------
    def reconstruct(self, x, x_lengths, y, y_lengths, sid=None, segment_size=None, ids_slice=None, eps_q=None):
        """How well the checkpoint reconstructs the recording `y` from its transcript `x`: forward()'s teacher-forced
        computation without gradients and without the duration loss.  Arguments as align(); returns (o [B,1,segment*hop],
        ids_slice [B] int64, attn [B,1,Ty,Tx], x_mask, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q)) -- forward()'s tuple
        without `l_length` and its eighth element.  wetts_amd.losses.teacher_forced_losses turns it into the
        reconstruction losses of train.py.

        Stages, all on the caller's stream: align()'s stages -> slice ids (commons.rand_slice_segments, models.py:214)
        -> slice z -> the decoder on the slice with no mask (models.py:216), in the precision set_decoder_dtype
        selected.  One host read-back per call (the status word, at the end).

        `segment_size` (frames) defaults to the constructor's.  `ids_slice` [B] (optional, not in the reference)
        gives the slice starts; without it they are drawn as the reference draws them, u * (len - segment + 1)
        truncated, with u from the Philox kernel under torch.manual_seed, and clamped to len - segment.  `eps_q` as
        in align().

        segment_size > Ty or a wrong shape raises ValueError before anything is launched; an utterance shorter than
        the segment, or a given id outside [0, len - segment], raises ValueError after the read-back.  align()'s
        IndexError / ValueError conditions carry over."""
        x, y, B, Tx, Ty = self._align_args(x, x_lengths, y, y_lengths, sid, eps_q)
        seg = int(self.segment_size if segment_size is None else segment_size)
        if seg < 1 or seg > Ty:
            raise ValueError(f"segment_size must be in [1, Ty={Ty}], got {seg}")
        if ids_slice is not None and tuple(torch.as_tensor(ids_slice).shape) != (B,):
            raise ValueError(f"ids_slice must be [{B}], got {tuple(torch.as_tensor(ids_slice).shape)}")
        lib = self._require_posterior()
        status, st = self._align_stages(lib, x, x_lengths, y, y_lengths, sid, eps_q, B, Tx, Ty)
        I = self.inter_channels
        s = _lib.current_stream_ptr()
        ids = torch.empty(B, dtype=torch.int64, device=self.device)
        u = ids_in = None
        if ids_slice is None:
            u = self._rand(B)
        else:
            ids_in = self._ids(torch.as_tensor(ids_slice))
        _lib.check(lib.wetts_slice_ids(_lib.ptr(u), _lib.ptr(ids_in), _lib.ptr(st["y_lengths"]), B, Ty, seg,
                                       _lib.ptr(ids), _lib.ptr(status), s), "slice_ids")
        z_slice = torch.empty(B, I, seg, dtype=torch.float32, device=self.device)
        _lib.check(lib.wetts_slice_segments(_lib.ptr(st["z"]), I * Ty, Ty, _lib.ptr(ids), B, I, Ty, seg, 1,
                                            _lib.ptr(z_slice), s), "slice_segments")
        o = self._decode(z_slice, st["g"], None, seg)
        self.last_status = int(status.cpu().item()) & 0xFFFFFFFF  # the call's one host sync
        self._align_raise()
        if self.last_status & _lib.STATUS_SEGMENT_LONGER:
            raise ValueError(f"reconstruct: an utterance is shorter than the segment of {seg} frames, or a given "
                             "ids_slice lies outside [0, y_lengths[b] - segment_size]")
        self._last_recon = dict(st, u=u, ids_slice=ids, z_slice=z_slice, o=o, segment_size=seg)
        return (o, ids, st["attn"].unsqueeze(1), st["x_mask"].unsqueeze(1), st["y_mask"].unsqueeze(1),
                (st["z"], st["z_p"], st["m_p"], st["logs_p"], st["m_q"], st["logs_q"]))

    # ---- duration loss (models.py:196-206) ---------------------------------------------------------------------------
    def _require_duration(self):
        """The SDP's forward-only tensors on the device: uploaded on first use, like the posterior encoder.  A
        DurationPredictor model needs none."""
        lib = self._require()
        if not self.use_sdp:
            return lib
        if self._dur_blob is None:
            names = [n for n, _, _, _ in checkpoint.duration_layout(self.cfg)]
            raise _lib.WettsError("duration_loss needs the stochastic duration predictor's forward-only tensors, but the "
                                  f"loaded checkpoint does not carry all of them: {names[0]} ... {names[-1]} "
                                  "(dp.flows.1.*, dp.post_pre, dp.post_proj, dp.post_convs.*, dp.post_flows.*)")
        if not self._dur_on_device:
            with torch.cuda.device(self.device):
                dev = self._dur_blob.to(self.device)
                _lib.check(lib.wetts_load_duration_posterior(self._handle, _lib.ptr(dev), dev.numel(),
                                                             _lib.current_stream_ptr()), "load_duration_posterior")
            self._dur_on_device = True
        return lib

    def duration_loss(self, x, x_lengths, w, sid=None, e_q=None, eps_w=None):
        """How plausible the durations `w` are for the transcript `x` under the checkpoint's duration predictor:
        forward()'s `l_length` (models.py:196-206) without gradients.  x [B,Tx] phoneme ids, x_lengths [B], w [B,1,Tx]
        or [B,Tx] frame counts per phoneme -- what align() returns as `w`.  Returns (l_length [B], (x_enc [B,H,Tx],
        logw [B,1,Tx], logw_ [B,1,Tx])): forward()'s second and eighth elements.

        SDP models: l_length = dp(x, x_mask, w, g) / sum(x_mask), the variational bound nll + logq of
        duration_predictors.py:206-253 per utterance over the WHOLE batch's phoneme count, logw the predictor's own
        sample at noise_scale 1.0, logw_ = log(w + 1e-6) * x_mask.  DurationPredictor models: logw = dp(x, x_mask, g),
        l_length = sum((logw - logw_)^2) / sum(x_mask).  train.py:485 sums l_length into loss_dur; the per-utterance
        values that do not depend on the batch are kept in `_last_duration` (nll, logq, per_utt).

        Stages on the caller's stream: emb_g -> text encoder -> the SDP forward (or DP and its squared error) -> for
        SDP models the reverse pass for logw -> the totals.  One host read-back (the status word, at the end).  `e_q`
        and `eps_w` [B,2,Tx] (optional, not in the reference) inject the torch.randn draws of :229 and :257; without
        them they come from the Philox kernel under torch.manual_seed, e_q first.

        Shape errors raise ValueError before anything is launched; a negative or non-finite w under the mask raises
        ValueError after the read-back; ids outside their tables raise IndexError.  An utterance of length 0 divides
        0 by 0: its `_last_duration["per_utt"]` is NaN (and every l_length, if no utterance has a phoneme).  An SDP checkpoint without the
        forward-only tensors (dp.flows.1.*, dp.post_*) raises a RuntimeError naming them."""
        x = torch.as_tensor(x)
        if x.dim() != 2:
            raise ValueError(f"x must be [B, Tx], got {tuple(x.shape)}")
        B, Tx = x.shape
        if tuple(torch.as_tensor(x_lengths).shape) != (B,):
            raise ValueError(f"x_lengths must be [{B}], got {tuple(torch.as_tensor(x_lengths).shape)}")
        w = torch.as_tensor(w)
        if tuple(w.shape) not in ((B, 1, Tx), (B, Tx)):
            raise ValueError(f"w must be [{B},1,{Tx}] or [{B},{Tx}], got {tuple(w.shape)}")
        if self.n_speakers > 0 and sid is None:
            raise ValueError("sid is required when n_speakers > 0")
        for name, t in (("e_q", e_q), ("eps_w", eps_w)):
            if t is not None and tuple(t.shape) != (B, 2, Tx):
                raise ValueError(f"{name} must be [{B},2,{Tx}], got {tuple(t.shape)}")
        if B < 1 or Tx < 1:
            raise ValueError("duration_loss of an empty batch")
        lib = self._require_duration()
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        H, I = self.hidden_channels, self.inter_channels
        x, x_lengths = self._ids(x), self._ids(x_lengths)
        nws = int(lib.wetts_workspace_bytes(self._handle, B, Tx, 0))
        ws = (self._ws_dec if self.overlap else self._ws).get(nws, dev)
        s = _lib.current_stream_ptr()
        g_buf = torch.empty(B, max(1, self.gin_channels), **f32)
        g = g_buf if self.n_speakers > 0 else None
        x_enc, stats, x_mask = torch.empty(B, H, Tx, **f32), torch.empty(B, 2 * I, Tx, **f32), torch.empty(B, Tx, **f32)
        status = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.wetts_set_status_word(self._handle, _lib.ptr(status), s), "set_status_word")
        try:
            _lib.check(lib.wetts_speaker_embedding(self._handle, _lib.ptr(self._ids(sid)) if g is not None else None, B,
                                                   _lib.ptr(g_buf), s), "speaker_embedding")
            _lib.check(lib.wetts_text_encoder(self._handle, _lib.ptr(x), _lib.ptr(x_lengths), _lib.ptr(g), B, Tx,
                                              _lib.ptr(x_enc), _lib.ptr(stats), _lib.ptr(x_mask), _lib.ptr(ws), nws, s),
                       "text_encoder")
            st = self._duration_stages(lib, x_enc, x_mask, g, w, e_q, eps_w, status, 1.0)
        finally:
            lib.wetts_set_status_word(self._handle, None, s)
        self.last_status = int(status.cpu().item()) & 0xFFFFFFFF  # the call's one host sync
        self._duration_raise()
        self._last_duration = st
        return st["l_length"], (x_enc, st["logw"].unsqueeze(1), st["logw_"].unsqueeze(1))

    def _duration_stages(self, lib, x_enc, x_mask, g, w, e_q, eps_w, status, weight):
        """The launches of duration_loss() behind the text encoder on device tensors x_enc [B,H,Tx], x_mask [B,Tx], g
        [B,gin] or None, without the read-back -> stage dict.  `status` is the registered status word.  Shared with
        losses.teacher_forced_losses(with_duration=True), which feeds reconstruct()'s tensors."""
        B, H, Tx = x_enc.shape
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        s = _lib.current_stream_ptr()
        w = self._f32(torch.as_tensor(w)).reshape(B, Tx)
        logw, logw_ = torch.empty(B, Tx, **f32), torch.empty(B, Tx, **f32)
        rows, per_utt, l_length = (torch.empty(B, **f32) for _ in range(3))
        total = torch.empty(2, **f32)
        nws = max(int(lib.wetts_workspace_bytes(self._handle, B, Tx, 0)),
                  int(lib.wetts_duration_loss_workspace_bytes(self._handle, B, Tx)))
        ws = (self._ws_dec if self.overlap else self._ws).get(nws, dev)
        st = dict(x_mask=x_mask, w=w, nll=None, logq=None, e_q=None, eps_w=None)
        if self.use_sdp:
            e_q = self._randn(B, 2, Tx) if e_q is None else self._f32(e_q)
            eps_w = self._randn(B, 2, Tx) if eps_w is None else self._f32(eps_w)
            nll, logq = torch.empty(B, **f32), torch.empty(B, **f32)
            z_q, z = torch.empty(B, 2, Tx, **f32), torch.empty(B, 2, Tx, **f32)
            nll_terms, logq_terms = torch.empty(B, Tx, **f32), torch.empty(B, Tx, **f32)
            _lib.check(lib.wetts_duration_sdp_forward(self._handle, _lib.ptr(x_enc), _lib.ptr(x_mask), _lib.ptr(g),
                                                      _lib.ptr(w), _lib.ptr(e_q), B, Tx, _lib.ptr(nll), _lib.ptr(logq),
                                                      _lib.ptr(rows), _lib.ptr(per_utt), _lib.ptr(z_q), _lib.ptr(z), _lib.ptr(nll_terms),
                                                      _lib.ptr(logq_terms), _lib.ptr(status), _lib.ptr(ws), nws, s),
                       "duration_sdp_forward")
            # models.py:200: logw = dp(x, x_mask, g=g, reverse=True, noise_scale=1.0)
            _lib.check(lib.wetts_duration_sdp(self._handle, _lib.ptr(x_enc), _lib.ptr(x_mask), _lib.ptr(g),
                                              _lib.ptr(eps_w), 1.0, B, Tx, _lib.ptr(logw), _lib.ptr(status), _lib.ptr(ws),
                                              nws, s), "duration_sdp")
            # logw_ = log(w + 1e-6) * x_mask (models.py:201)
            _lib.check(lib.wetts_duration_logw_target(_lib.ptr(w), _lib.ptr(x_mask), B, Tx, _lib.ptr(logw_), s),
                       "duration_logw_target")
            st.update(nll=nll, logq=logq, z_q=z_q, z=z, nll_terms=nll_terms, logq_terms=logq_terms, e_q=e_q, eps_w=eps_w)
        else:
            _lib.check(lib.wetts_duration_dp(self._handle, _lib.ptr(x_enc), _lib.ptr(x_mask), _lib.ptr(g), B, Tx,
                                             _lib.ptr(logw), _lib.ptr(ws), nws, s), "duration_dp")
            _lib.check(lib.wetts_duration_dp_loss(self._handle, _lib.ptr(logw), _lib.ptr(w), _lib.ptr(x_mask), B, Tx,
                                                  _lib.ptr(logw_), _lib.ptr(rows), _lib.ptr(per_utt), s),
                       "duration_dp_loss")
        _lib.check(lib.wetts_duration_loss_total(_lib.ptr(rows), _lib.ptr(x_mask), B, Tx, float(weight),
                                                 _lib.ptr(l_length), _lib.ptr(total), s), "duration_loss_total")
        st.update(rows=rows, per_utt=per_utt, l_length=l_length, total=total, logw=logw, logw_=logw_)
        return st

    def _duration_from_recon(self, e_q, eps_w, weight):
        """The duration stages on what the last reconstruct() computed (losses.teacher_forced_losses)."""
        lib = self._require_duration()
        rc = self._last_recon
        B, _, Tx = rc["x_enc"].shape
        for name, t in (("e_q", e_q), ("eps_w", eps_w)):
            if t is not None and tuple(t.shape) != (B, 2, Tx):
                raise ValueError(f"{name} must be [{B},2,{Tx}], got {tuple(t.shape)}")
        s = _lib.current_stream_ptr()
        status = torch.empty(1, dtype=torch.int64, device=self.device)
        _lib.check(lib.wetts_set_status_word(self._handle, _lib.ptr(status), s), "set_status_word")
        try:
            st = self._duration_stages(lib, rc["x_enc"], rc["x_mask"], rc["g"], rc["w"], e_q, eps_w, status, weight)
        finally:
            lib.wetts_set_status_word(self._handle, None, s)
        self.last_status = int(status.cpu().item()) & 0xFFFFFFFF
        self._duration_raise()
        self._last_duration = st
        return st

    def _duration_raise(self):
        """What duration_loss() raises from the status word it read back (self.last_status)."""
        if self.last_status & _lib.STATUS_PHONE_ID_RANGE:
            raise IndexError("index out of range in self (phoneme id outside emb, encoders.py:48)")
        if self.last_status & _lib.STATUS_SPEAKER_ID_RANGE:
            raise IndexError("index out of range in self (sid outside emb_g, models.py:163)")
        if self.last_status & _lib.STATUS_DURATION_NEGATIVE:
            raise ValueError("duration_loss: w holds a negative duration")
        if self.last_status & _lib.STATUS_DURATION_NONFINITE:
            raise ValueError("duration_loss: w holds a NaN or infinite duration")
        if self.last_status & _lib.STATUS_SPLINE_DOMAIN:
            raise AssertionError("spline inverse: negative discriminant (transforms.py:171)")

    # ---- stages ----------------------------------------------------------------------------------
    def _ids(self, t):
        return t.to(device=self.device, dtype=torch.int64).contiguous()

    def _f32(self, t):
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def _speaker(self, sid, B):
        lib = self._require()
        gin = max(1, self.gin_channels)
        g = torch.empty(B, gin, dtype=torch.float32, device=self.device)
        if self.n_speakers > 0:
            if sid is None:
                raise ValueError("sid is required when n_speakers > 0")
            sid = self._ids(sid)
        else:
            sid = None
        _lib.check(lib.wetts_speaker_embedding(self._handle, _lib.ptr(sid), B, _lib.ptr(g),
                                               _lib.current_stream_ptr()), "speaker_embedding")
        return g if self.n_speakers > 0 else None

    def _encode(self, x, x_lengths, sid, noise_scale, length_scale, noise_scale_w, eps_w, eps_z, durations=None):
        """Everything of infer() up to and including flow^-1 (== infer_encoder, models.py:282-331).
        Returns a dict of stage tensors."""
        lib = self._require()
        x = self._ids(x)
        x_lengths = self._ids(x_lengths)
        if durations is not None:
            return self._encode_stages_given(lib, x, x_lengths, sid, noise_scale, self._ids(durations), eps_z)
        return self._encode_stages(lib, x, x_lengths, sid, noise_scale, length_scale, noise_scale_w, eps_w, eps_z)

    def _randn(self, *shape):
        """Standard-normal tensor from the library's Philox kernel (replaces torch.randn).

        The (seed, offset) pair is the device generator's own -- torch.cuda.default_generators[device] -- read
        and advanced here exactly as an ATen kernel would: torch.manual_seed(s) therefore rewinds the stream
        (also when s is the seed already in use: the reference's `manual_seed(0); a = infer(); manual_seed(0);
        b = infer()` gives a == b, and so does this), successive calls continue it, and no ATen kernel runs."""
        return self._randn_into(torch.empty(*shape, dtype=torch.float32, device=self.device))

    def _randn_into(self, out):
        """Fills a contiguous float32 device tensor from the same stream (see _randn)."""
        lib = self._require()
        gen = torch.cuda.default_generators[self.device.index]
        seed = gen.initial_seed() & 0xFFFFFFFFFFFFFFFF
        offset = int(gen.get_offset())
        assert out.is_contiguous() and out.dtype == torch.float32
        n = out.numel()
        _lib.check(lib.wetts_randn(_lib.ptr(out), n, seed, offset, _lib.current_stream_ptr()), "randn")
        used = (n + 3) // 4  # Philox counters consumed (4 normals each)
        gen.set_offset(offset + (used + 3) // 4 * 4)  # ATen keeps the offset a multiple of 4
        return out

    def _rand(self, n):
        """Uniform [0, 1) float32 [n] from the same stream (replaces torch.rand, commons.py:54); see _randn."""
        self._require()
        return commons.rand(n, self.device)

    # The encoder call in two halves around its one host synchronisation.  Each half is (a) a set of device buffers
    # and (b) stream-ordered launches that touch nothing else -- so a half can also be captured once into a HIP graph
    # and replayed (session.GraphedEncoder), which is why the buffers are explicit.
    def _pre_buffers(self, B, Tx, own=False):
        """Buffers of the first half: speaker vector -> text encoder -> duration predictor -> durations.  `own`: also the
        input tensors and a private workspace (a captured graph bakes every pointer in)."""
        dev = self.device
        H, I = self.hidden_channels, self.inter_channels
        f32 = dict(dtype=torch.float32, device=dev)
        pb = dict(
            B=B, Tx=Tx, g=torch.empty(B, max(1, self.gin_channels), **f32),
            x_enc=torch.empty(B, H, Tx, **f32), stats=torch.empty(B, 2 * I, Tx, **f32),
            x_mask=torch.empty(B, Tx, **f32), logw=torch.empty(B, Tx, **f32), w_ceil=torch.empty(B, Tx, **f32),
            cum=torch.empty(B, Tx, **f32), eps_w=None, sid=None,
            # [B] y_lengths + one word of WETTS_STATUS_* bits: read back together, one sync
            meta=torch.empty(B + 1, dtype=torch.int64, device=dev))
        if own:
            nws = int(_lib.load().wetts_workspace_bytes(self._handle, B, Tx, 0))
            pb.update(x=torch.zeros(B, Tx, dtype=torch.int64, device=dev),
                      x_lengths=torch.zeros(B, dtype=torch.int64, device=dev),
                      sid=torch.zeros(B, dtype=torch.int64, device=dev), eps_w=torch.zeros(B, 2, Tx, **f32),
                      ws=torch.empty(max(nws, 16), dtype=torch.uint8, device=dev), nws=nws)
        return pb

    def _launch_pre(self, lib, pb, length_scale, noise_scale_w):
        B, Tx = pb["B"], pb["Tx"]
        s = _lib.current_stream_ptr()
        status_ptr = C.c_void_p(pb["meta"].data_ptr() + 8 * B)
        _lib.check(lib.wetts_set_status_word(self._handle, status_ptr, s), "set_status_word")
        try:
            g = pb["g"] if self.n_speakers > 0 else None
            _lib.check(lib.wetts_speaker_embedding(self._handle, _lib.ptr(pb["sid"]) if self.n_speakers > 0 else None, B,
                                                   _lib.ptr(pb["g"]), s), "speaker_embedding")
            _lib.check(lib.wetts_text_encoder(self._handle, _lib.ptr(pb["x"]), _lib.ptr(pb["x_lengths"]), _lib.ptr(g), B,
                                              Tx, _lib.ptr(pb["x_enc"]), _lib.ptr(pb["stats"]), _lib.ptr(pb["x_mask"]),
                                              _lib.ptr(pb["ws"]), pb["nws"], s), "text_encoder")
            if self.use_sdp:
                _lib.check(lib.wetts_duration_sdp(self._handle, _lib.ptr(pb["x_enc"]), _lib.ptr(pb["x_mask"]), _lib.ptr(g),
                                                  _lib.ptr(pb["eps_w"]), float(noise_scale_w), B, Tx, _lib.ptr(pb["logw"]),
                                                  status_ptr, _lib.ptr(pb["ws"]), pb["nws"], s), "duration_sdp")
            else:
                _lib.check(lib.wetts_duration_dp(self._handle, _lib.ptr(pb["x_enc"]), _lib.ptr(pb["x_mask"]), _lib.ptr(g), B,
                                                 Tx, _lib.ptr(pb["logw"]), _lib.ptr(pb["ws"]), pb["nws"], s), "duration_dp")
            _lib.check(lib.wetts_durations_to_lengths(_lib.ptr(pb["logw"]), _lib.ptr(pb["x_mask"]), float(length_scale), B,
                                                      Tx, _lib.ptr(pb["w_ceil"]), _lib.ptr(pb["cum"]), _lib.ptr(pb["meta"]),
                                                      status_ptr, s), "durations_to_lengths")
        finally:
            lib.wetts_set_status_word(self._handle, None, s)

    def _launch_pre_given(self, lib, pb, counts):
        """_launch_pre with the duration predictor replaced by the caller's frame counts [B,Tx] int64."""
        B, Tx = pb["B"], pb["Tx"]
        s = _lib.current_stream_ptr()
        status_ptr = C.c_void_p(pb["meta"].data_ptr() + 8 * B)
        _lib.check(lib.wetts_set_status_word(self._handle, status_ptr, s), "set_status_word")
        try:
            g = pb["g"] if self.n_speakers > 0 else None
            _lib.check(lib.wetts_speaker_embedding(self._handle, _lib.ptr(pb["sid"]) if self.n_speakers > 0 else None, B,
                                                   _lib.ptr(pb["g"]), s), "speaker_embedding")
            _lib.check(lib.wetts_text_encoder(self._handle, _lib.ptr(pb["x"]), _lib.ptr(pb["x_lengths"]), _lib.ptr(g), B,
                                              Tx, _lib.ptr(pb["x_enc"]), _lib.ptr(pb["stats"]), _lib.ptr(pb["x_mask"]),
                                              _lib.ptr(pb["ws"]), pb["nws"], s), "text_encoder")
            _lib.check(lib.wetts_counts_to_lengths(_lib.ptr(counts), _lib.ptr(pb["x_mask"]), B, Tx, _lib.ptr(pb["w_ceil"]),
                                                   _lib.ptr(pb["cum"]), _lib.ptr(pb["meta"]), status_ptr, s),
                       "counts_to_lengths")
        finally:
            lib.wetts_set_status_word(self._handle, None, s)

    def _encode_stages_given(self, lib, x, x_lengths, sid, noise_scale, counts, eps_z):
        """_encode_stages for infer(durations=): no duration predictor and no eps_w draw; everything behind the
        y_lengths read-back is _encode_stages' own second half."""
        B, Tx = x.shape
        I = self.inter_channels
        if self.n_speakers > 0 and sid is None:
            raise ValueError("sid is required when n_speakers > 0")
        pb = self._pre_buffers(B, Tx)
        pb["x"], pb["x_lengths"] = x, x_lengths
        if self.n_speakers > 0:
            pb["sid"] = self._ids(sid)
        pb["ws"], pb["nws"] = self._workspace(B, Tx, 0)
        self._launch_pre_given(lib, pb, counts)
        y_host, Ty = self._read_lengths(pb)
        if self.last_status & _lib.STATUS_DURATION_NEGATIVE:
            raise ValueError("durations must not be negative")
        qb = self._post_buffers(B, Tx, Ty)
        qb["eps_z"] = self._randn(B, I, Ty) if eps_z is None else self._f32(eps_z)
        if tuple(qb["eps_z"].shape) != (B, I, Ty):
            raise ValueError(f"eps_z must be [{B},{I},{Ty}], got {tuple(qb['eps_z'].shape)}")
        qb["ws"], qb["nws"] = self._workspace(B, Tx, Ty)
        self._launch_post(lib, pb, qb, noise_scale)
        return self._stage_dict(pb, qb, y_host, Ty)

    def _read_lengths(self, pb):
        """The one host sync of infer(): y_lengths and the status word in one D2H copy (the output length is data
        dependent, commons.py:114-115); raises what the reference raises from inside its modules."""
        B = pb["B"]
        meta_host = pb["meta"].cpu()
        y_host = meta_host[:B]
        self.last_status = int(meta_host[B].item()) & 0xFFFFFFFF
        if self.last_status & _lib.STATUS_PHONE_ID_RANGE:
            raise IndexError("index out of range in self (phoneme id outside emb, encoders.py:48)")
        if self.last_status & _lib.STATUS_SPEAKER_ID_RANGE:
            raise IndexError("index out of range in self (sid outside emb_g, models.py:239)")
        if self.last_status & (_lib.STATUS_SPLINE_DOMAIN | _lib.STATUS_DURATION_NONFINITE):
            # the reference dies on `assert (discriminant >= 0).all()` (transforms.py:171)
            raise AssertionError("spline inverse: negative discriminant (transforms.py:171)")
        return y_host, (int(y_host.max().item()) if B > 0 else 0)

    def _post_buffers(self, B, Tx, Ty, own=False):
        """Buffers of the second half: length regulation -> prior sampling -> flow^-1, for Ty frames."""
        dev = self.device
        I = self.inter_channels
        f32 = dict(dtype=torch.float32, device=dev)
        qb = dict(B=B, Tx=Tx, Ty=Ty, eps_z=None,
                  f2p=torch.empty(B, Ty, dtype=torch.int32, device=dev), y_mask=torch.empty(B, Ty, **f32),
                  attn=torch.empty(B, Ty, Tx, **f32), m_p=torch.empty(B, I, Ty, **f32),
                  logs_p=torch.empty(B, I, Ty, **f32), z_p=torch.empty(B, I, Ty, **f32), z=torch.empty(B, I, Ty, **f32))
        if own:
            nws = int(_lib.load().wetts_workspace_bytes(self._handle, B, Tx, Ty))
            qb.update(eps_z=torch.zeros(B, I, Ty, **f32), ws=torch.empty(max(nws, 16), dtype=torch.uint8, device=dev),
                      nws=nws)
        return qb

    def _launch_post(self, lib, pb, qb, noise_scale):
        B, Tx, Ty = qb["B"], qb["Tx"], qb["Ty"]
        I = self.inter_channels
        s = _lib.current_stream_ptr()
        g = pb["g"] if self.n_speakers > 0 else None
        _lib.check(lib.wetts_length_regulate(self._handle, _lib.ptr(pb["stats"]), _lib.ptr(pb["cum"]),
                                             _lib.ptr(pb["x_mask"]), _lib.ptr(pb["meta"]), _lib.ptr(qb["eps_z"]), I * Ty, Ty,
                                             float(noise_scale), B, Tx, Ty, _lib.ptr(qb["f2p"]), _lib.ptr(qb["y_mask"]),
                                             _lib.ptr(qb["attn"]), _lib.ptr(qb["m_p"]), _lib.ptr(qb["logs_p"]),
                                             _lib.ptr(qb["z_p"]), s), "length_regulate")
        _lib.check(lib.wetts_flow_reverse(self._handle, _lib.ptr(qb["z_p"]), _lib.ptr(qb["y_mask"]), _lib.ptr(g), B, Ty,
                                          _lib.ptr(qb["z"]), _lib.ptr(qb["ws"]), qb["nws"], s), "flow_reverse")

    def _encode_stages(self, lib, x, x_lengths, sid, noise_scale, length_scale, noise_scale_w, eps_w, eps_z):
        B, Tx = x.shape
        I = self.inter_channels
        if self.n_speakers > 0 and sid is None:
            raise ValueError("sid is required when n_speakers > 0")
        pb = self._pre_buffers(B, Tx)
        pb["x"], pb["x_lengths"] = x, x_lengths
        if self.n_speakers > 0:
            pb["sid"] = self._ids(sid)
        pb["ws"], pb["nws"] = self._workspace(B, Tx, 0)
        if self.use_sdp:
            pb["eps_w"] = self._randn(B, 2, Tx) if eps_w is None else self._f32(eps_w)
            if tuple(pb["eps_w"].shape) != (B, 2, Tx):
                raise ValueError(f"eps_w must be [{B},2,{Tx}]")
        self._launch_pre(lib, pb, length_scale, noise_scale_w)
        y_host, Ty = self._read_lengths(pb)
        qb = self._post_buffers(B, Tx, Ty)
        qb["eps_z"] = self._randn(B, I, Ty) if eps_z is None else self._f32(eps_z)
        if tuple(qb["eps_z"].shape) != (B, I, Ty):
            raise ValueError(f"eps_z must be [{B},{I},{Ty}], got {tuple(qb['eps_z'].shape)}")
        qb["ws"], qb["nws"] = self._workspace(B, Tx, Ty)
        self._launch_post(lib, pb, qb, noise_scale)
        return self._stage_dict(pb, qb, y_host, Ty)

    def _stage_dict(self, pb, qb, y_host, Ty):
        B = pb["B"]
        return dict(g=pb["g"] if self.n_speakers > 0 else None, x_enc=pb["x_enc"], stats=pb["stats"], x_mask=pb["x_mask"],
                    logw=pb["logw"], w_ceil=pb["w_ceil"], y_lengths=pb["meta"][:B], y_lengths_host=y_host,
                    frame2phone=qb["f2p"], y_mask=qb["y_mask"], attn=qb["attn"], m_p=qb["m_p"], logs_p=qb["logs_p"],
                    z_p=qb["z_p"], z=qb["z"], B=B, Tx=pb["Tx"], Ty=Ty)

    def ragged_supported(self):
        """True when the decoder can run a batch ragged (`infer(..., ragged=True)`): float32 ResBlock1 HiFi-GAN."""
        lib = self._require()
        return bool(lib.wetts_hifigan_ragged_supported(self._handle))

    def _decode(self, z, g, y_mask, L, y_lengths=None):
        """dec((z * y_mask)[:, :, :L], g) without materialising the masked / sliced copy.  With `y_lengths`
        (int64 device tensor [B]) the batch is decoded ragged: every utterance over its own frames, as if alone."""
        lib = self._require()
        B = z.shape[0]
        if B == 0 or L == 0:  # (z * y_mask)[:, :, :0] -> empty audio, nothing to launch
            return torch.empty(B, 1, 0, dtype=torch.float32, device=self.device)
        if z.shape[2] > 1 and z.stride(2) != 1:
            # the C entry takes a batch and a channel stride and reads time at stride 1: a time-major view (an ORT
            # [B, L, inter] tensor transposed) would be read as garbage without an error
            z = z.contiguous()
        if self.overlap:  # the next call's encoder stages may be using self._ws on the side stream by now
            nws = lib.wetts_workspace_bytes(self._handle, B, 0, L)
            if nws < 0:
                raise _lib.WettsError("workspace_bytes failed")
            ws = self._ws_dec.get(nws, self.device)
        else:
            ws, nws = self._workspace(B, 0, L)
        audio = torch.empty(B, 1, L * self.hop_length, dtype=torch.float32, device=self.device)
        if y_lengths is not None:
            _lib.check(lib.wetts_hifigan_ragged(self._handle, _lib.ptr(z), z.stride(0), z.stride(1),
                                                _lib.ptr(y_lengths), _lib.ptr(g), B, L, _lib.ptr(audio),
                                                _lib.ptr(ws), nws, _lib.current_stream_ptr()), "hifigan_ragged")
            return audio
        _lib.check(lib.wetts_hifigan(self._handle, _lib.ptr(z), z.stride(0), z.stride(1),
                                     _lib.ptr(y_mask),
                                     y_mask.stride(0) if y_mask is not None else 0,
                                     _lib.ptr(g), B, L, _lib.ptr(audio), _lib.ptr(ws), nws,
                                     _lib.current_stream_ptr()), "hifigan")
        return audio

    # ---- the reference's public inference API ----------------------------------------------------
    def infer(self, x, x_lengths, sid=None, noise_scale=1, length_scale=1, noise_scale_w=1.0,
              max_len=None, eps_w=None, eps_z=None, ragged=False, durations=None):
        """models.py:228-280.  Returns (o [B,1,Ty*hop], attn [B,1,Ty,Tx], y_mask [B,1,Ty],
        (z, z_p, m_p, logs_p) [B,inter,Ty]); z is unmasked, as in the reference.

        `durations` (not in the reference): frames per phoneme, an integer tensor [B,Tx] or [B,1,Tx] (a float tensor
        of whole numbers such as align()'s `w` is converted), masked by x_lengths.  The duration predictor is then
        skipped and these counts are w_ceil; `length_scale`, `noise_scale_w` and `eps_w` are ignored.  Everything
        behind the y_lengths read-back is unchanged.  A negative count raises ValueError.

        `ragged=True` (not in the reference): the generator has no masks, so the reference decodes every row of a
        padded batch to the longest utterance; ragged decodes row b over its own y_lengths[b] frames -- the audio
        the reference returns when that utterance is synthesised alone (its CLI's call shape) -- and writes zeros
        behind it.  The masked stages (encoder, durations, flow) are batch independent either way."""
        if durations is not None:
            durations = self._check_durations(x, durations)
            st = self._encode_ordered(x, x_lengths, sid, noise_scale, 1.0, 1.0, None, eps_z, durations=durations)
        else:
            st = self._encode_ordered(x, x_lengths, sid, noise_scale, length_scale, noise_scale_w, eps_w, eps_z)
        Ty = st["Ty"]
        L = Ty if max_len is None else max(0, min(Ty, int(max_len)))
        o = self._decode(st["z"], st["g"], st["y_mask"], L, st["y_lengths"] if ragged else None)
        self._last = st
        return (o, st["attn"].unsqueeze(1), st["y_mask"].unsqueeze(1),
                (st["z"], st["z_p"], st["m_p"], st["logs_p"]))

    @staticmethod
    def _check_durations(x, durations):
        """infer(durations=) argument check, before anything is launched: -> [B,Tx] tensor."""
        d = torch.as_tensor(durations)
        B, Tx = tuple(torch.as_tensor(x).shape)
        if d.dim() == 3 and d.shape[1] == 1:
            d = d[:, 0]
        if tuple(d.shape) != (B, Tx):
            raise ValueError(f"durations must be [{B},{Tx}] or [{B},1,{Tx}], got {tuple(torch.as_tensor(durations).shape)}")
        if d.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise ValueError(f"durations must be an integer tensor, got {d.dtype}")
        return d

    def _encode_ordered(self, x, x_lengths, sid, noise_scale, length_scale, noise_scale_w, eps_w, eps_z, durations=None):
        """_encode for the public entry points (infer, infer_encoder, export_encoder_forward, the sessions): on the
        caller's stream, or -- overlap mode -- on the side stream with the result ordered in front of whatever the
        caller's stream does next.  EVERY entry point goes through here, so in overlap mode the encoder workspace
        (self._ws) is only ever touched on the side stream: mixing infer() with infer_encoder() / the encoder session
        cannot race on it.  WETTS_DEBUG_OVERLAP=1 checks the one contract of the mode on every call (see set_overlap):
        it compares what the side stream reads of the id tensors NOW with their contents once the caller's stream has
        drained, and raises if a device op that produces them was still pending (it serialises the pipeline: debug only)."""
        if not (self.overlap and self.device.type == "cuda"):
            return self._encode(x, x_lengths, sid, float(noise_scale), float(length_scale),
                                float(noise_scale_w), eps_w, eps_z, durations)
        main = torch.cuda.current_stream(self.device)
        if self._enc_stream is None:
            self._enc_stream = self._new_enc_stream()
        if self._debug_overlap:
            ins = [t for t in (x, x_lengths, sid, eps_w, eps_z, durations) if isinstance(t, torch.Tensor) and t.is_cuda]
            with torch.cuda.stream(self._enc_stream):
                seen = [t.clone() for t in ins]  # what the side stream reads at this point of the caller's stream
            main.synchronize()
            self._enc_stream.synchronize()
            for a, b in zip(seen, ins):
                if not torch.equal(a, b):
                    raise RuntimeError(
                        "overlap mode: an input tensor was still being produced on the caller's stream when the call "
                        "was made; the encoder stages read inputs on a side stream WITHOUT waiting for the caller's "
                        "stream (SynthesizerTrn.set_overlap).  Materialise inputs first (upload(), or synchronise), "
                        "or call set_overlap(False).")
        with torch.cuda.stream(self._enc_stream):
            st = self._encode(x, x_lengths, sid, float(noise_scale), float(length_scale),
                              float(noise_scale_w), eps_w, eps_z, durations)
            done = torch.cuda.Event()
            done.record(self._enc_stream)
        main.wait_event(done)
        for v in st.values():  # allocated on the side stream, consumed (and later freed) on the caller's
            if isinstance(v, torch.Tensor) and v.is_cuda:
                v.record_stream(main)
        return st

    def infer_encoder(self, x, x_lengths, sid=None, noise_scale=1, length_scale=1,
                      noise_scale_w=1.0, eps_w=None, eps_z=None):
        """models.py:282-331.  Returns (attn, y_mask, (z*y_mask, z_p, m_p, logs_p), g)."""
        st = self._encode_ordered(x, x_lengths, sid, noise_scale, length_scale, noise_scale_w, eps_w, eps_z)
        z = torch.empty_like(st["z"])
        _lib.check(_lib.load().wetts_mask_rows(_lib.ptr(st["z"]), _lib.ptr(st["y_mask"]), st["B"],
                                               self.inter_channels, st["Ty"], _lib.ptr(z),
                                               _lib.current_stream_ptr()), "mask_rows")
        g = st["g"].unsqueeze(-1) if st["g"] is not None else None
        return (st["attn"].unsqueeze(1), st["y_mask"].unsqueeze(1),
                (z, st["z_p"], st["m_p"], st["logs_p"]), g)

    def export_forward(self, x, x_lengths, scales, sid):
        """models.py:333-344: row 0 of `scales` [B,3] = (noise_scale, length_scale, noise_scale_w)
        applies to the whole batch."""
        sc = torch.as_tensor(scales).detach().cpu().to(torch.float32)
        audio, *_ = self.infer(x, x_lengths, sid, noise_scale=float(sc[0][0]),
                               length_scale=float(sc[0][1]), noise_scale_w=float(sc[0][2]))
        return audio

    def export_encoder_forward(self, x, x_lengths, scales, sid):
        """models.py:346-358: returns z [B, L, inter] (time-major so callers slice chunks)."""
        sc = torch.as_tensor(scales).detach().cpu().to(torch.float32)
        _, _, (z, _, _, _), _ = self.infer_encoder(x, x_lengths, sid, noise_scale=float(sc[0][0]),
                                                   length_scale=float(sc[0][1]),
                                                   noise_scale_w=float(sc[0][2]))
        return z.transpose(1, 2)

    def export_decoder_forward(self, z, sid):
        """models.py:360-363: z [B, L, inter] -> audio [B,1,L*hop]."""
        z = self._f32(z).transpose(1, 2).contiguous()
        g = self._speaker(sid, z.shape[0])
        return self._decode(z, g, None, z.shape[2])

    def hifigan(self, z, g=None):
        """Generator.forward(z, g) (decoders.py:63-82) on [B,inter,L]; g is [B,gin] or [B,gin,1]."""
        z = self._f32(z)
        if g is not None:
            g = self._f32(g).reshape(z.shape[0], -1)
        return self._decode(z, g, None, z.shape[2])

    def audio_to_int16(self, audio, lengths_samples=None):
        """inference.py:100-110 scaling on the device; audio [B,1,L] or [B,L] -> int16 [B,L]."""
        lib = self._require()
        a = self._f32(audio)
        if a.dim() == 3:
            a = a[:, 0].contiguous()
        B, L = a.shape
        pcm = torch.empty(B, L, dtype=torch.int16, device=self.device)
        ln = self._ids(lengths_samples) if lengths_samples is not None else None
        _lib.check(lib.wetts_audio_to_int16(_lib.ptr(a), _lib.ptr(ln), B, L, _lib.ptr(pcm),
                                            _lib.current_stream_ptr()), "audio_to_int16")
        return pcm


def _onnx_stft_bases(n_fft, hop):
    """OnnxSTFT's `forward_basis` / `inverse_basis` buffers [n_fft + 2, 1, n_fft] (utils/stft.py:266-290, hann window,
    win_length == n_fft) for state_dict().  The device kernels build their own copy of the inverse one in closed form
    (kernels.hip: istft_basis_kernel); this host restatement serves the state_dict surface only."""
    import numpy as np
    n = np.arange(n_fft)
    k = np.arange(n_fft // 2 + 1)
    ang = 2.0 * np.pi * ((k[:, None] * n[None, :]) % n_fft) / n_fft
    basis = np.vstack([np.cos(ang), -np.sin(ang)])  # real and imaginary rows of fft(eye)[:cutoff]
    win = torch.from_numpy(0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)).float()  # scipy get_window("hann", fftbins=True)
    fwd = torch.from_numpy(basis[:, None, :]).float() * win
    inv = torch.from_numpy(np.linalg.pinv((n_fft / hop) * basis).T[:, None, :]).float() * win
    return fwd, inv


def load_checkpoint(checkpoint_path, model, optimizer=None):
    """task.load_checkpoint (utils/task.py:31-56) for the drop-in model: reads `G_*.pth`, folds
    weight norm, uploads.  Returns (model, optimizer, learning_rate, iteration) like the
    reference."""
    sd, iteration, lr = checkpoint.load_state_dict_file(checkpoint_path)
    # strict: a tensor the config asks for and the checkpoint lacks means the two do not belong
    # together (wrong n_layers / flow type / vocoder); the reference would keep a random init value
    # for it (task.py:44-49) and synthesise noise, here the blob slot would stay zero -- refuse.
    model.load_state_dict(sd, strict=True)
    return model, optimizer, lr, iteration
