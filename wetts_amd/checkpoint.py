"""Checkpoint handling: reference `G_*.pth` state_dict -> folded float32 weight blob.

Replaces utils/task.py:31-56 (load_checkpoint) + Generator/WN.remove_weight_norm
(decoders.py:84-88, modules.py:89-95).  The blob order is owned by the C library
(wetts_blob_tensor_info); this module only fills it.
"""
import ctypes as C
import logging

import torch

from . import _lib

logger = logging.getLogger(__name__)


def blob_layout(cfg):
    """[(name, offset, numel, shape)] as the library defines it (offsets / sizes in floats)."""
    lib = _lib.load()
    n = lib.wetts_blob_num_tensors(C.byref(cfg))
    if n < 0:
        raise _lib.WettsError(f"invalid config: {_lib.last_error()}")
    out = []
    buf = C.create_string_buffer(256)
    off, num, shape = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    for i in range(n):
        _lib.check(lib.wetts_blob_tensor_info(C.byref(cfg), i, buf, 256, C.byref(off),
                                              C.byref(num), C.byref(shape)), "blob_tensor_info")
        shp = tuple(int(s) for s in shape if s > 0)
        out.append((buf.value.decode(), int(off.value), int(num.value), shp))
    return out


def blob_numel(cfg):
    n = _lib.load().wetts_blob_numel(C.byref(cfg))
    if n < 0:
        raise _lib.WettsError(f"invalid config: {_lib.last_error()}")
    return int(n)


def fold_weight_norm(state_dict):
    """Collapses old-style weight-norm pairs: w = g * v / ||v|| with the norm over every dim but 0
    (torch.nn.utils.weight_norm default dim=0; for ConvTranspose1d that is the *input*-channel dim,
    weight [Cin,Cout,k], exactly as torch._weight_norm computes it).  Also accepts the
    parametrizations spelling (`parametrizations.weight.original0/1`)."""
    out = {}
    for k, v in state_dict.items():
        if k.endswith(".weight_g") or k.endswith(".weight_v"):
            continue
        if ".parametrizations.weight.original" in k:
            continue
        out[k] = v
    for k, g in state_dict.items():
        if k.endswith(".weight_g"):
            base = k[:-len("weight_g")]
            v = state_dict[base + "weight_v"]
        elif k.endswith(".parametrizations.weight.original0"):
            base = k[:-len("parametrizations.weight.original0")]
            v = state_dict[base + "parametrizations.weight.original1"]
        else:
            continue
        g = g.detach().to(torch.float32)
        v = v.detach().to(torch.float32)
        dims = tuple(range(1, v.dim()))
        norm = torch.linalg.vector_norm(v, ord=2, dim=dims, keepdim=True)
        out[base + "weight"] = v * (g / norm)
    return out


def pack_blob(cfg, state_dict, strict=True):
    """Natural-layout float32 CPU blob from a (reference-keyed) state_dict."""
    sd = fold_weight_norm(state_dict)
    blob = torch.zeros(blob_numel(cfg), dtype=torch.float32)
    missing = []
    for name, off, numel, shape in blob_layout(cfg):
        t = sd.get(name)
        if t is None:
            missing.append(name)
            continue
        t = t.detach().to(torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != expected {shape}")
        blob[off:off + numel] = t.reshape(-1)
    if missing:
        # the reference tolerates missing keys (task.py:44-49: keeps the module's init value).  There
        # is no random init to keep here, so strict mode (the default, and what load_checkpoint uses)
        # refuses; non-strict fills the DETERMINISTIC init values of the reference (LayerNorm
        # gamma = 1, normalization.py:12; ConvNeXt scale = 1/num_layers, decoders.py:236-238), leaves
        # the randomly initialised rest at zero, and reports every name.
        msg = f"{len(missing)} tensors missing from checkpoint: {missing}"
        if strict:
            raise KeyError(msg)
        for name, off, numel, shape in blob_layout(cfg):
            if name in missing and name.endswith(".gamma"):
                blob[off:off + numel] = 1.0
            elif name in missing and name.endswith(".scale"):
                blob[off:off + numel] = 1.0 / max(1, int(cfg.vocos_num_layers))
        logger.warning(msg)
    return blob


def posterior_layout(cfg, spec_channels):
    """[(name, offset, numel, shape)] of the posterior encoder's own blob (`enc_q.*`, voice conversion), as the library
    defines it (wetts_posterior_blob_tensor_info)."""
    lib = _lib.load()
    spec = int(spec_channels)
    n = lib.wetts_posterior_blob_num_tensors(C.byref(cfg), spec)
    if n < 0:
        raise _lib.WettsError(f"invalid config: {_lib.last_error()}")
    out = []
    buf = C.create_string_buffer(256)
    off, num, shape = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    for i in range(n):
        _lib.check(lib.wetts_posterior_blob_tensor_info(C.byref(cfg), spec, i, buf, 256, C.byref(off), C.byref(num),
                                                        C.byref(shape)), "posterior_blob_tensor_info")
        shp = tuple(int(s) for s in shape if s > 0)
        out.append((buf.value.decode(), int(off.value), int(num.value), shp))
    return out


def posterior_numel(cfg, spec_channels):
    n = _lib.load().wetts_posterior_blob_numel(C.byref(cfg), int(spec_channels))
    if n < 0:
        raise _lib.WettsError(f"invalid config: {_lib.last_error()}")
    return int(n)


def has_posterior(cfg, spec_channels, state_dict):
    """True when `state_dict` carries every `enc_q.*` tensor of the layout (weight-norm pairs count as their weight)."""
    sd = fold_weight_norm({k: v for k, v in state_dict.items() if k.startswith("enc_q.")})
    return all(name in sd for name, _, _, _ in posterior_layout(cfg, spec_channels))


def pack_posterior_blob(cfg, spec_channels, state_dict):
    """Natural-layout float32 CPU blob of the posterior encoder (`enc_q.*`, weight norm folded) from a reference-keyed
    state_dict.  Every tensor must be present (there is no init value to fall back to) and have its layout shape."""
    sd = fold_weight_norm({k: v for k, v in state_dict.items() if k.startswith("enc_q.")})
    blob = torch.zeros(posterior_numel(cfg, spec_channels), dtype=torch.float32)
    missing = []
    for name, off, numel, shape in posterior_layout(cfg, spec_channels):
        t = sd.get(name)
        if t is None:
            missing.append(name)
            continue
        t = t.detach().to(torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != expected {shape}")
        blob[off:off + numel] = t.reshape(-1)
    if missing:
        raise KeyError(f"{len(missing)} posterior encoder tensors missing from checkpoint: {missing}")
    return blob


def duration_layout(cfg):
    """[(name, offset, numel, shape)] of the duration posterior's own blob (SynthesizerTrn.duration_loss): `dp.flows.1.*`,
    `dp.post_pre`, `dp.post_proj`, `dp.post_convs.*`, `dp.post_flows.*`, as the library defines it
    (wetts_duration_blob_tensor_info).  Empty for a DurationPredictor model (use_sdp = false)."""
    lib = _lib.load()
    n = lib.wetts_duration_blob_num_tensors(C.byref(cfg))
    if n < 0:
        raise _lib.WettsError(f"invalid config: {_lib.last_error()}")
    out = []
    buf = C.create_string_buffer(256)
    off, num, shape = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    for i in range(n):
        _lib.check(lib.wetts_duration_blob_tensor_info(C.byref(cfg), i, buf, 256, C.byref(off), C.byref(num),
                                                       C.byref(shape)), "duration_blob_tensor_info")
        shp = tuple(int(s) for s in shape if s > 0)
        out.append((buf.value.decode(), int(off.value), int(num.value), shp))
    return out


def duration_numel(cfg):
    n = _lib.load().wetts_duration_blob_numel(C.byref(cfg))
    if n < 0:
        raise _lib.WettsError(f"invalid config: {_lib.last_error()}")
    return int(n)


def has_duration(cfg, state_dict):
    """True when `state_dict` carries every tensor of the duration layout (and the layout has any: SDP models)."""
    lay = duration_layout(cfg)
    return bool(lay) and all(name in state_dict for name, _, _, _ in lay)


def pack_duration_blob(cfg, state_dict):
    """Natural-layout float32 CPU blob of the duration posterior from a reference-keyed state_dict.  Every tensor must be
    present (there is no init value to fall back to) and have its layout shape."""
    blob = torch.zeros(duration_numel(cfg), dtype=torch.float32)
    missing = []
    for name, off, numel, shape in duration_layout(cfg):
        t = state_dict.get(name)
        if t is None:
            missing.append(name)
            continue
        t = t.detach().to(torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != expected {shape}")
        blob[off:off + numel] = t.reshape(-1)
    if missing:
        raise KeyError(f"{len(missing)} duration predictor tensors missing from checkpoint: {missing}")
    return blob


def disc_layout():
    """[(name, offset, numel, shape)] of the MultiPeriodDiscriminator's blob (`discriminators.N.convs.M.*`,
    `discriminators.N.conv_post.*`, weight norm folded), as the library defines it (wetts_disc_blob_tensor_info).  The
    architecture has no configuration, so neither has the layout."""
    lib = _lib.load()
    out = []
    buf = C.create_string_buffer(256)
    off, num, shape = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    for i in range(lib.wetts_disc_blob_num_tensors()):
        _lib.check(lib.wetts_disc_blob_tensor_info(i, buf, 256, C.byref(off), C.byref(num), C.byref(shape)),
                   "disc_blob_tensor_info")
        shp = tuple(int(s) for s in shape if s > 0)
        out.append((buf.value.decode(), int(off.value), int(num.value), shp))
    return out


def disc_numel():
    return int(_lib.load().wetts_disc_blob_numel())


def pack_disc_blob(state_dict):
    """Natural-layout float32 CPU blob of the discriminator from a reference-keyed state_dict (a `D_*.pth`'s "model"):
    weight-norm pairs in either spelling are folded (Conv2d weights [Cout, Cin, k, 1]: the norm runs over all dims but
    0).  Every tensor must be present and have its layout shape."""
    sd = fold_weight_norm(state_dict)
    blob = torch.zeros(disc_numel(), dtype=torch.float32)
    missing = []
    for name, off, numel, shape in disc_layout():
        t = sd.get(name)
        if t is None:
            missing.append(name)
            continue
        t = t.detach().to(torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != expected {shape}")
        blob[off:off + numel] = t.reshape(-1)
    if missing:
        raise KeyError(f"{len(missing)} discriminator tensors missing from checkpoint: {missing}")
    return blob


def mrd_layout():
    """[(name, offset, numel, shape)] of the MultiPeriodMultiResolutionDiscriminator's blob: the three DiscriminatorR
    stacks (`discriminators.{0,1,2}.band_convs.B.L.*`, `.conv_post.*`) then the five period stacks
    (`discriminators.{3..7}.convs.M.*`, `.conv_post.*`), weight norm folded, as the library defines it
    (wetts_mrd_blob_tensor_info)."""
    lib = _lib.load()
    out = []
    buf = C.create_string_buffer(256)
    off, num, shape = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    for i in range(lib.wetts_mrd_blob_num_tensors()):
        _lib.check(lib.wetts_mrd_blob_tensor_info(i, buf, 256, C.byref(off), C.byref(num), C.byref(shape)),
                   "mrd_blob_tensor_info")
        shp = tuple(int(s) for s in shape if s > 0)
        out.append((buf.value.decode(), int(off.value), int(num.value), shp))
    return out


def mrd_numel():
    return int(_lib.load().wetts_mrd_blob_numel())


def pack_mrd_blob(state_dict):
    """Natural-layout float32 CPU blob of the MPMRD from a reference-keyed state_dict (a `D_*.pth`'s "model" of a recipe
    with use_mrd_disc): weight-norm pairs in either spelling are folded.  Every tensor must be present and have its
    layout shape.  A DiscriminatorR embedding (`discriminators.N.emb.weight`, num_embeddings) is not supported."""
    emb = [k for k in state_dict if k.startswith("discriminators.") and ".emb." in k]
    if emb:
        raise NotImplementedError(f"DiscriminatorR's num_embeddings conditioning is not supported (found {emb[0]})")
    sd = fold_weight_norm(state_dict)
    blob = torch.zeros(mrd_numel(), dtype=torch.float32)
    missing = []
    for name, off, numel, shape in mrd_layout():
        t = sd.get(name)
        if t is None:
            missing.append(name)
            continue
        t = t.detach().to(torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != expected {shape}")
        blob[off:off + numel] = t.reshape(-1)
    if missing:
        raise KeyError(f"{len(missing)} discriminator tensors missing from checkpoint: {missing}")
    return blob


def durdisc_layout(version, in_channels, filter_channels, kernel_size):
    """[(name, offset, numel, shape)] of a duration discriminator's blob (model/discriminators.py:287-449; version 1 =
    DurationDiscriminatorV1, 2 = DurationDiscriminatorV2), as the library defines it (wetts_durdisc_blob_tensor_info).
    Version 1 has no norm tensors: the reference constructs `pre_out_norm_*` there and never reads them.  Raises
    ValueError for a shape the kernel does not cover (channels: multiples of 32 up to 256; taps: odd, up to 7)."""
    lib = _lib.load()
    cfg = (int(version), int(in_channels), int(filter_channels), int(kernel_size))
    n = lib.wetts_durdisc_blob_num_tensors(*cfg)
    if n < 0:
        raise ValueError(_lib.last_error())
    out = []
    buf = C.create_string_buffer(256)
    off, num, shape = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    for i in range(n):
        _lib.check(lib.wetts_durdisc_blob_tensor_info(*cfg, i, buf, 256, C.byref(off), C.byref(num), C.byref(shape)),
                   "durdisc_blob_tensor_info")
        shp = tuple(int(s) for s in shape if s > 0)
        out.append((buf.value.decode(), int(off.value), int(num.value), shp))
    return out


def durdisc_numel(version, in_channels, filter_channels, kernel_size):
    n = int(_lib.load().wetts_durdisc_blob_numel(int(version), int(in_channels), int(filter_channels), int(kernel_size)))
    if n < 0:
        raise ValueError(_lib.last_error())
    return n


def pack_durdisc_blob(version, in_channels, filter_channels, kernel_size, state_dict):
    """Natural-layout float32 CPU blob of a duration discriminator from a reference-keyed state_dict (a `DUR_*.pth`'s
    "model").  Every tensor of the layout must be present and have its layout shape; tensors the version does not read
    (version 1's `pre_out_norm_*`) are ignored."""
    cfg = (version, in_channels, filter_channels, kernel_size)
    blob = torch.zeros(durdisc_numel(*cfg), dtype=torch.float32)
    missing = []
    for name, off, numel, shape in durdisc_layout(*cfg):
        t = state_dict.get(name)
        if t is None:
            missing.append(name)
            continue
        t = t.detach().to(torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != expected {shape}")
        blob[off:off + numel] = t.reshape(-1)
    if missing:
        raise KeyError(f"{len(missing)} duration discriminator tensors missing from checkpoint: {missing}")
    return blob


def frontend_c_config(cfg):
    """_lib.FrontendConfig of a frontend config dict (the fields of wetts_frontend_config_t)."""
    c = _lib.FrontendConfig()
    for name, _ in _lib.FrontendConfig._fields_:
        if name not in cfg:
            raise ValueError(f"frontend config: field {name!r} is missing")
        setattr(c, name, float(cfg[name]) if name == "layer_norm_eps" else int(cfg[name]))
    return c


def frontend_layout(cfg):
    """[(name, offset, numel, shape)] of the frontend's blob (frontend/model.py:21-73: an HF BertModel, `transform`, the
    two classifiers), as the library defines it (wetts_frontend_blob_tensor_info); the names are the reference's
    state_dict keys.  Raises ValueError for a config the kernels do not cover."""
    lib = _lib.load()
    c = frontend_c_config(cfg)
    n = lib.wetts_frontend_blob_num_tensors(C.byref(c))
    if n < 0:
        raise ValueError(_lib.last_error())
    out = []
    buf = C.create_string_buffer(256)
    off, num, shape = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    for i in range(n):
        _lib.check(lib.wetts_frontend_blob_tensor_info(C.byref(c), i, buf, 256, C.byref(off), C.byref(num), C.byref(shape)),
                   "frontend_blob_tensor_info")
        shp = tuple(int(v) for v in shape if v > 0)
        out.append((buf.value.decode(), int(off.value), int(num.value), shp))
    return out


def frontend_numel(cfg):
    c = frontend_c_config(cfg)
    n = int(_lib.load().wetts_frontend_blob_numel(C.byref(c)))
    if n < 0:
        raise ValueError(_lib.last_error())
    return n


def pack_frontend_blob(cfg, state_dict):
    """Natural-layout float32 CPU blob of the frontend from what frontend/train.py:215 saves (keys bert.*, transform.*,
    phone_classifier.*, prosody_classifier.*).  Every tensor of the layout must be present and have its layout shape;
    bert.pooler.* and bert.embeddings.position_ids are not read."""
    blob = torch.zeros(frontend_numel(cfg), dtype=torch.float32)
    missing = []
    for name, off, numel, shape in frontend_layout(cfg):
        t = state_dict.get(name)
        if t is None:
            missing.append(name)
            continue
        t = t.detach().to(torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: checkpoint shape {tuple(t.shape)} != expected {shape}")
        blob[off:off + numel] = t.reshape(-1)
    if missing:
        raise KeyError(f"{len(missing)} frontend tensors missing from checkpoint: {missing}")
    return blob


def load_state_dict_file(checkpoint_path):
    """Reads `G_*.pth` as saved by task.save_checkpoint (task.py:59-76): {"model": state_dict,
    "iteration", "optimizer", "learning_rate"}; a bare state_dict is accepted too."""
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    if isinstance(ckpt, dict) and "model" in ckpt and isinstance(ckpt["model"], dict):
        return ckpt["model"], ckpt.get("iteration"), ckpt.get("learning_rate")
    return ckpt, None, None
