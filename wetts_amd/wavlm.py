"""WavLM on the device: what the reference's WavLMLoss (losses.py:63-153) gets from
`AutoModel.from_pretrained(...)(input_values=..., output_hidden_states=True).hidden_states`, and the resampler in front
of it.

    resample = Resample(22050, 16000)
    wavlm = load_wavlm("exp/slm/wavlm-base-plus").cuda()      # config.json + pytorch_model.bin
    hidden = wavlm.hidden_states(resample(wav))               # 13 tensors [B, T, 768]

The model is transformers' WavLMModel in the `wavlm-base` / `wavlm-base-plus` architecture: feat_extract_norm "group",
no conv bias, post-norm encoder layers (do_stable_layer_norm false), GELU, no adapter, and no attention mask -- the
reference passes none, every row of a batch has one length.  Any other config raises ValueError naming the key.
Evaluation only, float32, no gradients; the arithmetic is csrc/wavlm.hip, and there is no `transformers` import.

`Resample` is a STAND-IN for torchaudio.transforms.Resample at its defaults (sinc_interp_hann, lowpass_filter_width 6,
rolloff 0.99): torchaudio is not a dependency of this project and was not available to compare against, so the class
restates the published arithmetic of its kernel -- built in float64 on the host and rounded to float32 once -- and is
pinned to a float64 restatement and to analytic facts (identity, length, DC gain, pass band, stop band), not to
torchaudio itself."""
import ctypes as C
import json
import math
import os

import torch

from . import _lib

_CONFIG_INTS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "num_conv_pos_embeddings",
                "num_conv_pos_embedding_groups", "num_buckets", "max_bucket_distance")
# key -> the one value the kernels cover (transformers' default in brackets where it differs)
_REQUIRED = (("feat_extract_norm", "group", "group"), ("do_stable_layer_norm", False, False), ("conv_bias", False, False),
             ("feat_extract_activation", "gelu", "gelu"), ("hidden_act", "gelu", "gelu"), ("add_adapter", False, False))
MAX_FRAMES = 512


# ---- the resampler -----------------------------------------------------------------------------------------------------
def resample_kernel(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """-> (kernel float32 [new, 2 width + orig], width, orig, new) with orig, new the rates over their gcd: the
    sinc_interp_hann kernel, value sinc(pi t) cos^2(pi t / (2 lowpass_filter_width)) base / orig at
    t = (-j / new + (i - width) / orig) base clamped to +-lowpass_filter_width, base = min(orig, new) rolloff;
    evaluated in float64 and rounded once."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq < 1 or new_freq < 1:
        raise ValueError(f"orig_freq = {orig_freq} and new_freq = {new_freq} must be positive")
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    base = min(o, n) * float(rolloff)
    width = int(math.ceil(lowpass_filter_width * o / base))
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, :] / o
    t = (torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx) * base
    t = t.clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / torch.where(t == 0, torch.ones_like(t), t))
    return (sinc * window * (base / o)).to(torch.float32), width, o, n


class Resample:
    """Stand-in for torchaudio.transforms.Resample(orig_freq, new_freq) at its defaults (see the module docstring),
    callable on a device tensor [..., L] -> [..., ceil(new L / orig)].  Equal rates return the input itself."""

    def __init__(self, orig_freq=16000, new_freq=16000):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.kernel, self.width, self.orig, self.new = resample_kernel(orig_freq, new_freq)
        self.taps = 2 * self.width + self.orig
        self.kernel_stride = (self.taps + 7) // 8 * 8
        self._dev = {}

    def output_length(self, L):
        return -(-self.new * int(L) // self.orig)

    def _kernel_on(self, device):
        k = self._dev.get(device)
        if k is None:
            k = torch.zeros(self.new, self.kernel_stride, dtype=torch.float32)
            k[:, :self.taps] = self.kernel
            k = self._dev[device] = k.to(device)
        return k

    def _run(self, x):
        """x [R, L] float32 on the device, rows at any stride -> (buffer [R, frames * new], valid length): the rows'
        resampled signals are buffer[:, :valid]."""
        R, L = x.shape
        if R < 1 or L < 1:
            raise ValueError(f"Resample: empty input {tuple(x.shape)}")
        if x.stride(1) != 1 or (R > 1 and x.stride(0) < L):  # a transposed, expanded or overlapping view
            x = x.contiguous()
        frames = L // self.orig + 1
        stride = ((frames - 1) * self.orig + self.kernel_stride + 3) // 4 * 4
        padded = torch.empty(R, stride, dtype=torch.float32, device=x.device)
        out = torch.empty(R, frames * self.new, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().wetts_wavlm_resample(
                _lib.ptr(x), x.stride(0) if R > 1 else L, R, L, self.orig, self.new, self.width,
                _lib.ptr(self._kernel_on(x.device)), self.kernel_stride, _lib.ptr(padded), stride, _lib.ptr(out),
                _lib.current_stream_ptr()), "wavlm_resample")
        return out, self.output_length(L)

    def __call__(self, waveform):
        if not torch.is_tensor(waveform) or waveform.dim() < 1:
            raise ValueError(f"waveform must be a tensor [..., L], got {getattr(waveform, 'shape', type(waveform))}")
        if self.orig_freq == self.new_freq:
            return waveform
        if waveform.device.type != "cuda":
            raise ValueError("Resample runs on a HIP device only (there is no CPU path)")
        shape = waveform.shape
        x = waveform.to(torch.float32).reshape(-1, shape[-1])
        out, n = self._run(x)
        return out[:, :n].reshape(*shape[:-1], n)

    forward = __call__


# ---- the model -----------------------------------------------------------------------------------------------------------
def wavlm_config(config):
    """The fields of wetts_wavlm_config_t from a transformers WavLM `config.json` (dict or path).  Raises ValueError
    naming the key for an architecture the kernels do not cover."""
    if isinstance(config, (str, os.PathLike)):
        with open(config, encoding="utf-8") as f:
            config = json.load(f)
    c = dict(config)
    for key, want, default in _REQUIRED:
        got = c.get(key, default)
        if got != want:
            raise ValueError(f"{key} = {got!r} is not supported (only {want!r}, the wavlm-base / wavlm-base-plus architecture)")
    for key in _CONFIG_INTS + ("conv_dim", "conv_kernel", "conv_stride"):
        if key not in c:
            raise ValueError(f"the WavLM config has no {key!r}")
    dims, kernels, strides = (list(c[k]) for k in ("conv_dim", "conv_kernel", "conv_stride"))
    if not (len(dims) == len(kernels) == len(strides)) or not 2 <= len(dims) <= _lib.WAVLM_MAX_CONV:
        raise ValueError(f"conv_dim, conv_kernel and conv_stride must have one length of 2 .. {_lib.WAVLM_MAX_CONV}, got "
                         f"{len(dims)}, {len(kernels)}, {len(strides)}")
    out = dict(conv_dim=[int(v) for v in dims], conv_kernel=[int(v) for v in kernels], conv_stride=[int(v) for v in strides],
               layer_norm_eps=float(c.get("layer_norm_eps", 1e-5)))
    out.update({k: int(c[k]) for k in _CONFIG_INTS})
    return out


def c_config(cfg):
    c = _lib.WavLMConfig()
    n = len(cfg["conv_dim"])
    c.num_conv_layers = n
    for i in range(n):
        c.conv_dim[i], c.conv_kernel[i], c.conv_stride[i] = cfg["conv_dim"][i], cfg["conv_kernel"][i], cfg["conv_stride"][i]
    c.hidden_size, c.num_layers, c.num_heads = cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"]
    c.intermediate_size = cfg["intermediate_size"]
    c.pos_kernel, c.pos_groups = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    c.num_buckets, c.max_bucket_distance = cfg["num_buckets"], cfg["max_bucket_distance"]
    c.layer_norm_eps = cfg["layer_norm_eps"]
    return c


def blob_layout(cfg):
    """[(name, offset, numel, shape)] of the device blob (wetts_wavlm_blob_tensor_info); ValueError for a config the
    kernels refuse."""
    lib = _lib.load()
    cc = c_config(cfg)
    n = lib.wetts_wavlm_blob_num_tensors(C.byref(cc))
    if n < 0:
        raise ValueError(_lib.last_error())
    return _read_layout(lambda i, *a: lib.wetts_wavlm_blob_tensor_info(C.byref(cc), i, *a), n)


def _read_layout(info, n):
    out = []
    name = C.create_string_buffer(256)
    off, numel, shape = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    for i in range(n):
        _lib.check(info(i, name, 256, C.byref(off), C.byref(numel), C.byref(shape)), "blob_tensor_info")
        out.append((name.value.decode(), int(off.value), int(numel.value), tuple(int(v) for v in shape if v > 0)))
    return out


def num_frames(cfg, L):
    """transformers' _get_feat_extract_output_lengths: floor((L - k) / s) + 1 per conv layer (0 below one frame)."""
    cc = c_config(cfg)
    n = int(_lib.load().wetts_wavlm_num_frames(C.byref(cc), int(L)))
    if n < 0:
        raise ValueError(_lib.last_error())
    return n


def min_samples(cfg):
    """The shortest input that leaves one frame (400 for the base architecture)."""
    n = 1
    for k, s in zip(reversed(cfg["conv_kernel"]), reversed(cfg["conv_stride"])):
        n = (n - 1) * s + k
    return n


POS_CONV = "encoder.pos_conv_embed.conv."


def fold_pos_conv(state_dict):
    """The positional conv's weight with its weight norm (dim = 2: one norm per tap, over the dims 0 and 1) folded,
    from `parametrizations.weight.original0 / original1`, the legacy `weight_g / weight_v`, or a plain `weight`."""
    for g, v in ((POS_CONV + "parametrizations.weight.original0", POS_CONV + "parametrizations.weight.original1"),
                 (POS_CONV + "weight_g", POS_CONV + "weight_v")):
        if g in state_dict and v in state_dict:
            wg, wv = state_dict[g].detach().to(torch.float32), state_dict[v].detach().to(torch.float32)
            return wv * (wg / torch.linalg.vector_norm(wv, ord=2, dim=(0, 1), keepdim=True))
    if POS_CONV + "weight" in state_dict:
        return state_dict[POS_CONV + "weight"].detach().to(torch.float32)
    raise KeyError(f"{POS_CONV}weight: neither parametrizations.weight.original0/1, weight_g/weight_v nor weight is present")


def pack_blob(cfg, state_dict):
    """The float32 CPU blob of a transformers-keyed WavLMModel state_dict (an optional `wavlm.` prefix is dropped)."""
    sd = {(k[len("wavlm."):] if k.startswith("wavlm.") else k): v for k, v in state_dict.items()}
    layout = blob_layout(cfg)
    blob = torch.zeros(layout[-1][1] + (layout[-1][2] + 3) // 4 * 4, dtype=torch.float32)
    for name, off, numel, shape in layout:
        if name == POS_CONV + "weight":
            t = fold_pos_conv(sd).permute(0, 2, 1)
        else:
            if name not in sd:
                raise KeyError(f"{name} is missing from the state_dict")
            t = sd[name].detach().to(torch.float32)
            if name.startswith("feature_extractor.conv_layers.") and name.endswith(".conv.weight"):
                t = t.reshape(t.shape[0], t.shape[2]) if t.dim() == 3 and t.shape[1] == 1 and len(shape) == 2 else t.permute(0, 2, 1)
            elif name.endswith("gru_rel_pos_const"):
                t = t.reshape(-1)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(t.shape)} in the state_dict, the config gives {tuple(shape)}")
        blob[off:off + numel] = t.reshape(-1)
    return blob


class WavLM:
    """transformers' WavLMModel (base architecture) as an evaluation module on the device.  `config`: its config.json as
    a dict or a path."""

    def __init__(self, config):
        self.config = wavlm_config(config)
        blob_layout(self.config)  # raises ValueError for a shape the kernels do not cover: no slow path
        self.hidden_size, self.num_layers = self.config["hidden_size"], self.config["num_hidden_layers"]
        self.training = False
        self._sd = None
        self._blob = None
        self._handle = None
        self._device = None

    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("WavLM is evaluation only (no gradients)")
        return self

    def parameters(self):
        return iter(())

    def load_state_dict(self, state_dict, strict=True):
        """transformers' parameter names; the positional conv's weight norm under either spelling.  Every tensor the
        model reads must be present with its shape; masked_spec_embed is ignored."""
        self._blob = pack_blob(self.config, state_dict)
        used = {n for n, *_ in blob_layout(self.config)} - {POS_CONV + "weight"}
        self._sd = {}
        for k, v in state_dict.items():
            k = k[len("wavlm."):] if k.startswith("wavlm.") else k
            if k in used or k.startswith(POS_CONV):
                self._sd[k] = v.detach().to(torch.float32).clone()
        if self._device is not None:
            self._create()
        return self

    def state_dict(self):
        """The tensors the model uses, as they were loaded (names and shapes of transformers' WavLMModel)."""
        self._require_blob()
        return {k: v.clone() for k, v in self._sd.items()}

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("WavLM runs on a HIP device only (there is no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._device = device
        if self._blob is not None:
            self._create()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))

    @property
    def device(self):
        return self._device

    def _require_blob(self):
        if self._blob is None:
            raise RuntimeError("no weights: call load_state_dict() first")

    def _create(self):
        self._destroy()
        lib = _lib.load()
        with torch.cuda.device(self._device):
            dev = self._blob.to(self._device)
            h = C.c_void_p()
            cfg = c_config(self.config)
            _lib.check(lib.wetts_wavlm_create(C.byref(cfg), _lib.ptr(dev), dev.numel(), _lib.current_stream_ptr(), C.byref(h)),
                       "wavlm_create")
        self._handle = h

    def _destroy(self):
        if self._handle is not None:
            _lib.load().wetts_wavlm_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _require(self):
        self._require_blob()
        if self._handle is None:
            raise RuntimeError("WavLM is not on a device: call .to('cuda') / .cuda() first")

    def num_frames(self, L):
        return num_frames(self.config, L)

    def _hidden(self, x):
        """x [B, L] float32 on the device (rows at any stride) -> [layers + 1, B, T, hidden]."""
        self._require()
        if not torch.is_tensor(x) or x.dim() != 2:
            raise ValueError(f"input_values must be a [B, L] tensor, got {getattr(x, 'shape', type(x))}")
        B, L = x.shape
        if B < 1:
            raise ValueError("input_values: empty batch")
        T = self.num_frames(L) if L >= 1 else 0
        if T < 1:
            raise ValueError(f"input_values: {L} samples are shorter than one frame ({min_samples(self.config)} samples)")
        if T > MAX_FRAMES:
            raise ValueError(f"input_values: {L} samples give {T} frames, the kernels cover at most {MAX_FRAMES}")
        if x.device != self._device:
            raise ValueError(f"input_values is on {x.device}, WavLM on {self._device}")
        if x.dtype != torch.float32 or x.stride(1) != 1 or (B > 1 and x.stride(0) < L):
            x = x.to(torch.float32).contiguous()
        lib = _lib.load()
        nbytes = int(lib.wetts_wavlm_workspace_bytes(self._handle, B, L))
        if nbytes < 0:
            raise _lib.WettsError(f"wavlm_workspace_bytes: {_lib.last_error()}")
        with torch.cuda.device(self._device):
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self._device)
            hidden = torch.empty(self.num_layers + 1, B, T, self.hidden_size, dtype=torch.float32, device=self._device)
            _lib.check(lib.wetts_wavlm_forward(self._handle, _lib.ptr(x), x.stride(0) if B > 1 else L, B, L, _lib.ptr(hidden),
                                               _lib.ptr(ws), nbytes, _lib.current_stream_ptr()), "wavlm_forward")
        return hidden

    def hidden_states(self, input_values):
        """-> tuple of num_hidden_layers + 1 tensors [B, T, hidden]: the input of every encoder layer, then the last
        layer's output (transformers' `hidden_states` with output_hidden_states=True)."""
        return tuple(self._hidden(input_values).unbind(0))


def load_wavlm(model_dir):
    """A WavLM from a transformers model directory: config.json and pytorch_model.bin (model.safetensors is read only
    where `safetensors` imports).  Nothing is downloaded: a missing directory or file raises FileNotFoundError."""
    cfg_path, bin_path = os.path.join(model_dir, "config.json"), os.path.join(model_dir, "pytorch_model.bin")
    st_path = os.path.join(model_dir, "model.safetensors")
    if not os.path.isfile(cfg_path) or not (os.path.isfile(bin_path) or os.path.isfile(st_path)):
        raise FileNotFoundError(f"{model_dir!r} must hold config.json and pytorch_model.bin (this project downloads nothing)")
    model = WavLM(cfg_path)
    if os.path.isfile(bin_path):
        sd = torch.load(bin_path, map_location="cpu", weights_only=True)
    else:
        try:
            from safetensors.torch import load_file
        except ImportError as e:
            raise FileNotFoundError(f"{model_dir!r} has no pytorch_model.bin, and model.safetensors needs the "
                                    f"`safetensors` package ({e})") from e
        sd = load_file(st_path)
    return model.load_state_dict(sd)
