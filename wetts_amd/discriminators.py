"""MultiPeriodDiscriminator (model/discriminators.py:228-254: one DiscriminatorS and DiscriminatorP for the periods 2, 3,
5, 7, 11, all weight-normed) as a drop-in evaluation module on the device.  No gradients.  torch allocates the feature
maps and takes views; the arithmetic is the HIP kernels of csrc/discriminator.hip.

y and y_hat run as one batch of 2B utterances, so every weight is read once; the results do not depend on the pairing
(an utterance's maps are a function of that utterance alone, bit for bit).  A period stack's feature map is computed as
[2B, p, C, H] and handed back as the permuted view [2B, C, H, p] -- the reference's shape, no copy -- split into its real
and generated halves.

MultiPeriodMultiResolutionDiscriminator (model/discriminators.py:256-283, the `use_mrd_disc` recipes) follows below with
the same surface: three DiscriminatorR stacks (csrc/mrd.hip) in front of the same five period stacks.

DurationDiscriminatorV1 / DurationDiscriminatorV2 (model/discriminators.py:287-449, the `use_duration_discriminator`
recipes) close the file: csrc/duration_disc.hip, four launches per call."""
import ctypes as C

import torch

from . import _lib, checkpoint

PERIODS = (2, 3, 5, 7, 11)
N_FMAPS = 37  # DiscriminatorS: 6 convs + conv_post; each DiscriminatorP: 5 convs + conv_post
# F.pad(x, (0, n_pad), "reflect") needs n_pad < T.  n_pad = p - T % p for the periods that do not divide T: at T = 5,
# period 11 would pad 6 samples (illegal); from T = 6 on every pad is shorter than the input (checked for every T up to
# 11 * 11 in tests/test_cpu_disc.py; beyond that n_pad <= 10 < T).
MIN_SAMPLES = 6


class MultiPeriodDiscriminator:
    def __init__(self, use_spectral_norm=False):
        if use_spectral_norm:
            raise NotImplementedError("use_spectral_norm=True is not supported: folding spectral norm needs the "
                                      "power-iteration state (weight_u / weight_v); no checked-in recipe sets it")
        self.use_spectral_norm = False
        self.periods = PERIODS
        self.training = False
        self._blob = None      # folded float32 CPU blob (checkpoint.disc_layout order)
        self._handle = None
        self._device = None
        self._shapes = {}      # (B, T) -> [(rows, C, H, p)] * 37

    # ---- nn.Module-like surface ----
    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("this discriminator is evaluation only (no gradients)")
        return self

    def load_state_dict(self, state_dict, strict=True):
        """Reference-keyed state_dict (`discriminators.N.convs.M.{bias,weight_g,weight_v}`, either weight-norm spelling,
        or already folded `weight`s).  Every tensor must be present: there is no init value to fall back to."""
        self._blob = checkpoint.pack_disc_blob(state_dict)
        if self._device is not None:
            self._create()
        return self

    def state_dict(self):
        """The folded tensors (weight norm collapsed), reference-keyed."""
        self._require_blob()
        return {name: self._blob[off:off + numel].reshape(shape).clone()
                for name, off, numel, shape in checkpoint.disc_layout()}

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("MultiPeriodDiscriminator runs on a HIP device only (there is no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._device = device
        if self._blob is not None:
            self._create()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))

    def _require_blob(self):
        if self._blob is None:
            raise RuntimeError("no weights: call load_state_dict() (or models.load_checkpoint on a D_*.pth) first")

    def _create(self):
        self._destroy()
        lib = _lib.load()
        with torch.cuda.device(self._device):
            dev = self._blob.to(self._device)
            h = C.c_void_p()
            _lib.check(lib.wetts_disc_create(_lib.ptr(dev), dev.numel(), _lib.current_stream_ptr(), C.byref(h)),
                       "disc_create")
        self._handle = h

    def _destroy(self):
        if self._handle is not None:
            _lib.load().wetts_disc_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _require(self):
        self._require_blob()
        if self._handle is None:
            raise RuntimeError("the discriminator is not on a device: call .to('cuda') / .cuda() first")

    # ---- forward ----
    @staticmethod
    def fmap_shapes(B, T):
        """[(rows, C, H, p)] of the 37 feature maps as the device computes them (wetts_disc_fmap_shape)."""
        lib = _lib.load()
        out, shp = [], (C.c_int64 * 4)()
        for i in range(N_FMAPS):
            _lib.check(lib.wetts_disc_fmap_shape(int(B), int(T), i, C.byref(shp)), "disc_fmap_shape")
            out.append(tuple(int(v) for v in shp))
        return out

    def _check(self, y, y_hat):
        for t, n in ((y, "y"), (y_hat, "y_hat")):
            if not torch.is_tensor(t) or t.dim() != 3 or t.shape[1] != 1:
                raise ValueError(f"{n} must be a [B, 1, T] tensor, got {getattr(t, 'shape', type(t))}")
            if t.device.type != "cuda":
                raise ValueError(f"{n} must be on a HIP device (there is no CPU path)")
        if tuple(y.shape) != tuple(y_hat.shape):
            raise ValueError(f"y {tuple(y.shape)} and y_hat {tuple(y_hat.shape)} must have one shape")
        if y.shape[0] < 1:
            raise ValueError("empty batch")
        if y.shape[2] < MIN_SAMPLES:
            raise ValueError(f"T = {y.shape[2]} samples: the reflect pad of discriminators.py:81-84 needs at least "
                             f"{MIN_SAMPLES}")
        self._require()
        if y.device != self._device or y_hat.device != self._device:
            raise ValueError(f"y is on {y.device}, y_hat on {y_hat.device}, the discriminator on {self._device}")

    def _run(self, y, y_hat):
        """-> (buffers [37] as the device wrote them, B): S maps [2B, C, T'], P maps [2B, p, C, H], P conv_post maps
        [2B, 1, H, p]; all slices of one torch-owned allocation made for this call."""
        self._check(y, y_hat)
        y = y.to(torch.float32).contiguous()
        y_hat = y_hat.to(torch.float32).contiguous()
        B, _, T = y.shape
        shapes = self._shapes.get((B, T))
        if shapes is None:
            shapes = self._shapes[(B, T)] = self.fmap_shapes(B, T)
        offs, total = [], 0
        for rows, Cc, H, p in shapes:
            offs.append(total)
            total += (rows * Cc * H + 63) // 64 * 64
        flat = torch.empty(total, dtype=torch.float32, device=y.device)
        bufs = []
        for i, ((rows, Cc, H, p), off) in enumerate(zip(shapes, offs)):
            t = flat[off:off + rows * Cc * H]
            post = i >= 7 and (i - 7) % 6 == 5
            bufs.append(t.view(2 * B, 1, H, p) if post else (t.view(2 * B, p, Cc, H) if i >= 7 else t.view(2 * B, Cc, H)))
        ptrs = (C.c_void_p * N_FMAPS)(*[b.data_ptr() for b in bufs])
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().wetts_disc_forward(self._handle, _lib.ptr(y), _lib.ptr(y_hat), B, T, ptrs,
                                                      _lib.current_stream_ptr()), "disc_forward")
        return bufs, B

    def forward(self, y, y_hat):
        """discriminators.py:241-254 -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs): six [B, N_d] outputs each, and six lists of
        feature maps in the reference's shapes ([B, C, T'] for DiscriminatorS, [B, C, H, p] for the period stacks)."""
        bufs, B = self._run(y, y_hat)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        i = 0
        for d in range(6):
            n = 7 if d == 0 else 6
            maps = [b if (d == 0 or k == n - 1) else b.permute(0, 2, 3, 1) for k, b in enumerate(bufs[i:i + n])]
            i += n
            fmap_rs.append([m[:B] for m in maps])
            fmap_gs.append([m[B:] for m in maps])
            y_d_rs.append(maps[-1][:B].reshape(B, -1))
            y_d_gs.append(maps[-1][B:].reshape(B, -1))
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs

    __call__ = forward


# ---- MultiPeriodMultiResolutionDiscriminator ----------------------------------------------------------------------------
MRD_WINDOWS = (2048, 1024, 512)
MRD_MIN_SAMPLES = 1025  # torch.stft(center=True) reflect-pads n_fft / 2 = 1024 samples on each side: T must exceed that
MRD_N_FMAPS = 93  # three DiscriminatorR: 5 bands x layers 1..4 + conv_post; five DiscriminatorP: 5 convs + conv_post
_MRD_R_MAPS = 21


class MultiPeriodMultiResolutionDiscriminator(MultiPeriodDiscriminator):
    """model/discriminators.py:256-283 (the `use_mrd_disc` recipes, e.g. vits2_vocos_v1): DiscriminatorR for the window
    lengths 2048, 1024, 512 (discriminators.py:127-225, no embedding) followed by DiscriminatorP for the periods 2, 3, 5,
    7, 11; there is no DiscriminatorS.  The same evaluation-only surface as MultiPeriodDiscriminator; the arithmetic is
    csrc/mrd.hip, csrc/stft.hip's complex STFT and the period kernels of csrc/discriminator.hip.  `use_spectral_norm`
    only ever reached the period stacks and is refused as it is there."""
    MIN_SAMPLES = MRD_MIN_SAMPLES

    def __init__(self, use_spectral_norm=False):
        super().__init__(use_spectral_norm)
        self.windows = MRD_WINDOWS

    def load_state_dict(self, state_dict, strict=True):
        """Reference-keyed state_dict (`discriminators.{0,1,2}.band_convs.B.L.*` / `.conv_post.*`,
        `discriminators.{3..7}.convs.M.*` / `.conv_post.*`; either weight-norm spelling, or folded weights)."""
        self._blob = checkpoint.pack_mrd_blob(state_dict)
        if self._device is not None:
            self._create()
        return self

    def state_dict(self):
        self._require_blob()
        return {name: self._blob[off:off + numel].reshape(shape).clone()
                for name, off, numel, shape in checkpoint.mrd_layout()}

    def _create(self):
        self._destroy()
        lib = _lib.load()
        with torch.cuda.device(self._device):
            dev = self._blob.to(self._device)
            h = C.c_void_p()
            _lib.check(lib.wetts_mrd_create(_lib.ptr(dev), dev.numel(), _lib.current_stream_ptr(), C.byref(h)),
                       "mrd_create")
        self._handle = h

    def _destroy(self):
        if self._handle is not None:
            _lib.load().wetts_mrd_destroy(self._handle)
            self._handle = None

    @staticmethod
    def fmap_shapes(B, T):
        """The 93 maps as the device computes them (wetts_mrd_fmap_shape): (2B, C, frames, F) for the DiscriminatorR
        maps, which is the reference's own shape; (rows, C, H, p) for the period stacks."""
        lib = _lib.load()
        out, shp = [], (C.c_int64 * 4)()
        for i in range(MRD_N_FMAPS):
            _lib.check(lib.wetts_mrd_fmap_shape(int(B), int(T), i, C.byref(shp)), "mrd_fmap_shape")
            out.append(tuple(int(v) for v in shp))
        return out

    def _check(self, y, y_hat):
        if torch.is_tensor(y) and y.dim() == 3 and y.shape[2] < self.MIN_SAMPLES:
            raise ValueError(f"T = {y.shape[2]} samples: the centring reflect pad of the 2048-sample window "
                             f"(torch.stft, center=True) needs at least {self.MIN_SAMPLES}")
        super()._check(y, y_hat)

    def _run(self, y, y_hat):
        """-> (buffers [93] as the device wrote them, B): DiscriminatorR maps [2B, C, frames, F], period maps
        [2B, p, C, H] and [2B, 1, H, p]; maps and workspace are slices of one torch-owned allocation made for this call."""
        self._check(y, y_hat)
        y = y.to(torch.float32).contiguous()
        y_hat = y_hat.to(torch.float32).contiguous()
        B, _, T = y.shape
        shapes = self._shapes.get((B, T))
        if shapes is None:
            shapes = self._shapes[(B, T)] = self.fmap_shapes(B, T)
        lib = _lib.load()
        offs, total = [], 0
        for s in shapes:
            offs.append(total)
            total += (s[0] * s[1] * s[2] * (s[3] if len(offs) <= 3 * _MRD_R_MAPS else 1) + 63) // 64 * 64
        ws_bytes = int(lib.wetts_mrd_workspace_bytes(B, T))
        if ws_bytes < 0:
            raise _lib.WettsError(f"mrd_workspace_bytes: {_lib.last_error()}")
        flat = torch.empty(total + ws_bytes // 4, dtype=torch.float32, device=y.device)
        bufs = []
        for i, (s, off) in enumerate(zip(shapes, offs)):
            if i < 3 * _MRD_R_MAPS:
                bufs.append(flat[off:off + s[0] * s[1] * s[2] * s[3]].view(*s))
                continue
            rows, Cc, H, p = s
            t = flat[off:off + rows * Cc * H]
            bufs.append(t.view(2 * B, 1, H, p) if (i - 3 * _MRD_R_MAPS) % 6 == 5 else t.view(2 * B, p, Cc, H))
        ws = flat[total:]
        ptrs = (C.c_void_p * MRD_N_FMAPS)(*[b.data_ptr() for b in bufs])
        with torch.cuda.device(y.device):
            _lib.check(lib.wetts_mrd_forward(self._handle, _lib.ptr(y), _lib.ptr(y_hat), B, T, ptrs, _lib.ptr(ws), ws_bytes,
                                             _lib.current_stream_ptr()), "mrd_forward")
        return bufs, B

    def forward(self, y, y_hat):
        """discriminators.py:270-283 -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs): eight entries each.  A DiscriminatorR's
        output stays 4-D, [B, 1, frames, sum F'], as the reference returns it; a period stack's is [B, N_d]."""
        bufs, B = self._run(y, y_hat)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        i = 0
        for d in range(8):
            n = _MRD_R_MAPS if d < 3 else 6
            maps = [b if (d < 3 or k == n - 1) else b.permute(0, 2, 3, 1) for k, b in enumerate(bufs[i:i + n])]
            i += n
            fmap_rs.append([m[:B] for m in maps])
            fmap_gs.append([m[B:] for m in maps])
            y_d_rs.append(maps[-1][:B] if d < 3 else maps[-1][:B].reshape(B, -1))
            y_d_gs.append(maps[-1][B:] if d < 3 else maps[-1][B:].reshape(B, -1))
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs

    __call__ = forward


def from_hparams(hps):
    """train.py:196-203: MultiPeriodMultiResolutionDiscriminator where hps.model.use_mrd_disc is set, else
    MultiPeriodDiscriminator; both with hps.model.use_spectral_norm."""
    model = hps.model
    keys = model.keys() if hasattr(model, "keys") else model
    sn = bool(model["use_spectral_norm"]) if "use_spectral_norm" in keys else False
    mrd = "use_mrd_disc" in keys and bool(model["use_mrd_disc"])
    return (MultiPeriodMultiResolutionDiscriminator if mrd else MultiPeriodDiscriminator)(sn)


# ---- VITS2 duration discriminators ------------------------------------------------------------------------------------
AVAILABLE_DURATION_DISCRIMINATOR_TYPES = ("dur_disc_1", "dur_disc_2")  # model/discriminators.py:15-18
DURDISC_STAGES = ("conv_1", "conv_2", "pre_out_conv_1", "pre_out_conv_2", "prob")


class DurationDiscriminatorV1:
    """model/discriminators.py:287-369 as an evaluation module on the device: conv_1 and conv_2 on hidden_x, then per
    duration dur_proj, the concatenation, pre_out_conv_1, pre_out_conv_2, Linear and sigmoid; every conv reads its
    input under x_mask and pads with zeros at Tx.  The reference's constructor signature; `p_dropout` and
    `gin_channels` are stored and unused, as there (the dropout is never applied, `cond` is commented out).  forward()
    returns the reference's [prob_r, prob_g], each [B, Tx, 1]: losses.discriminator_loss zips over that pair's batch
    rows, which losses.teacher_forced_losses(net_dur_disc=) reproduces.  `pre_out_norm_*` of a state_dict are ignored."""
    VERSION = 1

    def __init__(self, in_channels, filter_channels, kernel_size, p_dropout, gin_channels=0):
        self.in_channels = int(in_channels)
        self.filter_channels = int(filter_channels)
        self.kernel_size = int(kernel_size)
        self.p_dropout = p_dropout
        self.gin_channels = gin_channels
        self.training = False
        self._cfg = (self.VERSION, self.in_channels, self.filter_channels, self.kernel_size)
        checkpoint.durdisc_layout(*self._cfg)  # raises ValueError for a shape the kernel does not cover: no slow path
        self._blob = None
        self._handle = None
        self._device = None

    # ---- nn.Module-like surface ----
    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("this discriminator is evaluation only (no gradients)")
        return self

    def load_state_dict(self, state_dict, strict=True):
        """Reference-keyed state_dict (a `DUR_*.pth`'s "model").  Every tensor the class reads must be present."""
        self._blob = checkpoint.pack_durdisc_blob(*self._cfg, state_dict)
        if self._device is not None:
            self._create()
        return self

    def state_dict(self):
        """The tensors the class uses, reference-keyed."""
        self._require_blob()
        return {name: self._blob[off:off + numel].reshape(shape).clone()
                for name, off, numel, shape in checkpoint.durdisc_layout(*self._cfg)}

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"{type(self).__name__} runs on a HIP device only (there is no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._device = device
        if self._blob is not None:
            self._create()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))

    def _require_blob(self):
        if self._blob is None:
            raise RuntimeError("no weights: call load_state_dict() (or models.load_checkpoint on a DUR_*.pth) first")

    def _create(self):
        self._destroy()
        lib = _lib.load()
        with torch.cuda.device(self._device):
            dev = self._blob.to(self._device)
            h = C.c_void_p()
            _lib.check(lib.wetts_durdisc_create(*self._cfg, _lib.ptr(dev), dev.numel(), _lib.current_stream_ptr(),
                                                C.byref(h)), "durdisc_create")
        self._handle = h

    def _destroy(self):
        if self._handle is not None:
            _lib.load().wetts_durdisc_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _require(self):
        self._require_blob()
        if self._handle is None:
            raise RuntimeError("the discriminator is not on a device: call .to('cuda') / .cuda() first")

    # ---- forward ----
    def _check(self, x, x_mask, durs):
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError(f"x must be a [B, {self.in_channels}, Tx] tensor, got {getattr(x, 'shape', type(x))}")
        B, _, Tx = x.shape
        if B < 1 or Tx < 1:
            raise ValueError("empty batch")
        for t, n in ((x_mask, "x_mask"),) + tuple(durs):
            if not torch.is_tensor(t) or tuple(t.shape) != (B, 1, Tx):
                raise ValueError(f"{n} must be a [{B}, 1, {Tx}] tensor, got {getattr(t, 'shape', type(t))}")
        for t, n in ((x, "x"), (x_mask, "x_mask")) + tuple(durs):
            if t.device.type != "cuda":
                raise ValueError(f"{n} must be on a HIP device (there is no CPU path)")
        self._require()
        for t, n in ((x, "x"), (x_mask, "x_mask")) + tuple(durs):
            if t.device != self._device:
                raise ValueError(f"{n} is on {t.device}, the discriminator on {self._device}")

    def _run(self, x, x_mask, dur_r, dur_hat):
        """-> the five stages as the device wrote them (DURDISC_STAGES): conv_1's and conv_2's maps [B, F, Tx],
        pre_out_conv_1's and pre_out_conv_2's [2B, F, Tx] (version 2: after ReLU + LayerNorm; rows 0..B-1 belong to
        dur_r) and the probabilities [2B, Tx]; all slices of one torch-owned allocation made for this call."""
        self._check(x, x_mask, ((dur_r, "dur_r"), (dur_hat, "dur_hat")))
        x, x_mask, dur_r, dur_hat = (t.to(torch.float32).contiguous() for t in (x, x_mask, dur_r, dur_hat))
        B, _, Tx = x.shape
        F_ = self.filter_channels
        lib = _lib.load()
        nbytes = int(lib.wetts_durdisc_workspace_bytes(self._handle, B, Tx))
        if nbytes < 0:
            raise _lib.WettsError(f"durdisc_workspace_bytes: {_lib.last_error()}")
        flat = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.wetts_durdisc_forward(self._handle, _lib.ptr(x), _lib.ptr(x_mask), _lib.ptr(dur_r),
                                                 _lib.ptr(dur_hat), B, Tx, _lib.ptr(flat), nbytes,
                                                 _lib.current_stream_ptr()), "durdisc_forward")
        out, off = [], 0
        for shape in ((B, F_, Tx), (B, F_, Tx), (2 * B, F_, Tx), (2 * B, F_, Tx), (2 * B, Tx)):
            n = 1
            for v in shape:
                n *= v
            out.append(flat[off:off + n].view(*shape))
            off += (n + 63) // 64 * 64
        return out

    def _probs(self, x, x_mask, dur_r, dur_hat):
        prob = self._run(x, x_mask, dur_r, dur_hat)[4]
        B = x.shape[0]
        return prob[:B].unsqueeze(2), prob[B:].unsqueeze(2)

    def forward(self, x, x_mask, dur_r, dur_hat, g=None):
        """discriminators.py:350-369 -> [prob_r, prob_g], each [B, Tx, 1].  `g` is accepted and unused, as there."""
        return list(self._probs(x, x_mask, dur_r, dur_hat))

    def forward_probability(self, x, x_mask, dur, g=None):
        """The probabilities [B, Tx, 1] of one duration tensor.  `x` is hidden_x, as in forward(): the trunk runs here
        too (the reference's method of this name takes the trunk's output, which this module does not hand out)."""
        return self._probs(x, x_mask, dur, dur)[0]

    __call__ = forward


class DurationDiscriminatorV2(DurationDiscriminatorV1):
    """model/discriminators.py:372-449: ReLU and a channel LayerNorm (normalization.py: biased variance over the
    channels, eps 1e-5) behind each of the four convs.  forward() returns the reference's [[prob_r], [prob_g]], over
    which losses.discriminator_loss forms ONE term (the mean over B * Tx)."""
    VERSION = 2

    def forward(self, x, x_mask, dur_r, dur_hat, g=None):
        """discriminators.py:432-449 -> [[prob_r], [prob_g]], each probability tensor [B, Tx, 1]."""
        r, g_ = self._probs(x, x_mask, dur_r, dur_hat)
        return [[r], [g_]]

    __call__ = forward


def duration_discriminator_from_hparams(hps):
    """train.py:129-163: None unless hps.model.use_duration_discriminator; else the class named by
    hps.model.duration_discriminator_type (default "dur_disc_1"), built as (hidden_channels, hidden_channels, 3, 0.1,
    gin_channels = hps.model.gin_channels where hps.data.n_speakers != 0, else 0)."""
    model = hps.model
    if not ("use_duration_discriminator" in model.keys() and model["use_duration_discriminator"]):
        return None
    kind = model["duration_discriminator_type"] if "duration_discriminator_type" in model.keys() else "dur_disc_1"
    assert kind in AVAILABLE_DURATION_DISCRIMINATOR_TYPES, kind
    cls = DurationDiscriminatorV1 if kind == "dur_disc_1" else DurationDiscriminatorV2
    gin = model["gin_channels"] if hps.data["n_speakers"] != 0 else 0
    return cls(model["hidden_channels"], model["hidden_channels"], 3, 0.1, gin_channels=gin)


# ---- WavLMDiscriminator ------------------------------------------------------------------------------------------------
class WavLMDiscriminator:
    """model/discriminators.py:452-498: a 1x1 `pre` conv over the slm_layers * slm_hidden stacked WavLM hidden states,
    three k = 5 convs with leaky_relu(0.1), and conv_post to one channel, all weight-normed -- as an evaluation module on
    the device (csrc/wavlm.hip).  forward(x [B, slm_layers * slm_hidden, T]) -> [B, T] as the reference's; the WavLM loss
    calls `on_hidden`, which reads the hidden-state buffers where they lie, so the stacked tensor is never formed."""

    def __init__(self, slm_hidden=768, slm_layers=13, initial_channel=64, use_spectral_norm=False):
        if use_spectral_norm:
            raise NotImplementedError("use_spectral_norm=True is not supported: folding spectral norm needs the "
                                      "power-iteration state (weight_u / weight_v); no checked-in recipe sets it")
        self.slm_hidden, self.slm_layers, self.initial_channel = int(slm_hidden), int(slm_layers), int(initial_channel)
        self.use_spectral_norm = False
        self.training = False
        self.layout()  # raises ValueError for a shape the kernels do not cover
        self._blob = None
        self._folded = None    # the folded tensors in the reference's shapes (state_dict)
        self._handle = None
        self._device = None

    def layout(self):
        """[(name, offset, numel, shape)] of the device blob: weight norm folded, convs tap-major [Cout][k][Cin]."""
        from . import wavlm
        lib = _lib.load()
        a = (self.slm_hidden, self.slm_layers, self.initial_channel)
        n = lib.wetts_wavlm_disc_blob_num_tensors(*a)
        if n < 0:
            raise ValueError(_lib.last_error())
        return wavlm._read_layout(lambda i, *r: lib.wetts_wavlm_disc_blob_tensor_info(*a, i, *r), n)

    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("this discriminator is evaluation only (no gradients)")
        return self

    def load_state_dict(self, state_dict, strict=True):
        """Reference-keyed (`pre`, `convs.N`, `conv_post`: bias and weight_g / weight_v, either weight-norm spelling, or
        already folded weights).  Every tensor must be present."""
        sd = checkpoint.fold_weight_norm(state_dict)
        lay = self.layout()
        blob = torch.zeros(lay[-1][1] + (lay[-1][2] + 3) // 4 * 4, dtype=torch.float32)
        folded = {}
        for name, off, numel, shape in lay:
            if name not in sd:
                raise KeyError(f"{name} is missing from the state_dict")
            t = sd[name].detach().to(torch.float32)
            # the reference's shape: [Cout, Cin, k] for a weight laid out tap-major [Cout][k][Cin] (pre: [c0][Cin], k = 1)
            want = (shape[0], shape[-1], shape[1] if len(shape) == 3 else 1) if name.endswith(".weight") else tuple(shape)
            if tuple(t.shape) != want:
                raise ValueError(f"{name}: shape {tuple(t.shape)} in the state_dict, the discriminator has {want}")
            folded[name] = t.clone()
            if name.endswith(".weight"):
                t = t.permute(0, 2, 1)
            blob[off:off + numel] = t.reshape(-1)
        self._blob, self._folded = blob, folded
        if self._device is not None:
            self._create()
        return self

    def state_dict(self):
        """The folded tensors (weight norm collapsed), reference-keyed and in the reference's [Cout, Cin, k] shapes."""
        self._require_blob()
        return {k: v.clone() for k, v in self._folded.items()}

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("WavLMDiscriminator runs on a HIP device only (there is no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._device = device
        if self._blob is not None:
            self._create()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))

    def _require_blob(self):
        if self._blob is None:
            raise RuntimeError("no weights: call load_state_dict() first")

    def _create(self):
        self._destroy()
        lib = _lib.load()
        with torch.cuda.device(self._device):
            dev = self._blob.to(self._device)
            h = C.c_void_p()
            _lib.check(lib.wetts_wavlm_disc_create(self.slm_hidden, self.slm_layers, self.initial_channel, _lib.ptr(dev),
                                                   dev.numel(), _lib.current_stream_ptr(), C.byref(h)), "wavlm_disc_create")
        self._handle = h

    def _destroy(self):
        if getattr(self, "_handle", None) is not None:
            _lib.load().wetts_wavlm_disc_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _require(self):
        self._require_blob()
        if self._handle is None:
            raise RuntimeError("the discriminator is not on a device: call .to('cuda') / .cuda() first")

    def on_hidden(self, hidden):
        """hidden [slm_layers, R, T, slm_hidden] (contiguous float32, what WavLM computes) -> [R, T]."""
        self._require()
        if (not torch.is_tensor(hidden) or hidden.dim() != 4 or hidden.shape[0] != self.slm_layers or
                hidden.shape[3] != self.slm_hidden or hidden.shape[1] < 1 or hidden.shape[2] < 1):
            raise ValueError(f"hidden must be [{self.slm_layers}, rows, T, {self.slm_hidden}], got "
                             f"{getattr(hidden, 'shape', type(hidden))}")
        if hidden.device != self._device:
            raise ValueError(f"hidden is on {hidden.device}, the discriminator on {self._device}")
        hidden = hidden.to(torch.float32).contiguous()
        _, R, T, H = hidden.shape
        lib = _lib.load()
        nbytes = int(lib.wetts_wavlm_disc_workspace_bytes(self._handle, R, T))
        if nbytes < 0:
            raise _lib.WettsError(f"wavlm_disc_workspace_bytes: {_lib.last_error()}")
        with torch.cuda.device(self._device):
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self._device)
            out = torch.empty(R, T, dtype=torch.float32, device=self._device)
            _lib.check(lib.wetts_wavlm_disc_forward(self._handle, _lib.ptr(hidden), R * T * H, R, T, _lib.ptr(out),
                                                    _lib.ptr(ws), _lib.current_stream_ptr()), "wavlm_disc_forward")
        return out

    def forward(self, x):
        """discriminators.py:487-498: x [B, slm_layers * slm_hidden, T], channel layer * slm_hidden + c -> [B, T]."""
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != self.slm_layers * self.slm_hidden:
            raise ValueError(f"x must be [B, {self.slm_layers * self.slm_hidden}, T], got {getattr(x, 'shape', type(x))}")
        B, _, T = x.shape
        return self.on_hidden(x.reshape(B, self.slm_layers, self.slm_hidden, T).permute(1, 0, 3, 2).contiguous())

    __call__ = forward


def wavlm_discriminator_from_hparams(hps):
    """train.py:165-176: None unless hps.model.use_wd; else WavLMDiscriminator(slm_hidden, slm_nlayers,
    slm_initial_channel)."""
    model = hps.model
    if not ("use_wd" in model.keys() and model["use_wd"]):
        return None
    return WavLMDiscriminator(model["slm_hidden"], model["slm_nlayers"], model["slm_initial_channel"])
