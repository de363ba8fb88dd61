"""Drop-ins for the two slicing helpers of the reference's utils/commons.py (slice_segments, rand_slice_segments:
commons.py:41-58) on the device, through the HIP kernels of csrc/losses.hip.  torch allocates and nothing else; inputs
are float32 [B, C, T] tensors on a HIP device (there is no CPU path).

Differences from the reference, all deliberate:
  * the drawn id is clamped to len - segment: with u = 1.0 (torch.rand stays below it, an injected `u` need not) the
    reference's u * (len - segment + 1) is one step past the last valid start;
  * a start outside the tensor is clamped into it instead of raising (the helpers do not read back from the device;
    SynthesizerTrn.reconstruct() does, and raises);
  * `scale=` (keyword only) slices x at ids * scale over segment_size * scale steps, which is how train.py:430-431
    slices the waveform at frame ids (`slice_segments(y, ids_slice * hop_length, segment_size)`) without an
    element-wise op on the ids;
  * `u=` (keyword only) injects rand_slice_segments' uniform draw; without it the draw comes from the Philox kernel on
    the device generator's (seed, offset), so torch.manual_seed makes it reproducible.
"""
import torch

from . import _lib


def _x3(x):
    if not torch.is_tensor(x) or x.dim() != 3:
        raise ValueError(f"x must be a [B, C, T] tensor, got {getattr(x, 'shape', type(x))}")
    if x.device.type != "cuda":
        raise ValueError("x must be on a HIP device (there is no CPU path)")
    x = x.to(dtype=torch.float32)
    if x.shape[2] > 1 and x.stride(2) != 1:
        x = x.contiguous()
    return x


def _ids(ids, B, device):
    ids = torch.as_tensor(ids)
    if tuple(ids.shape) != (B,):
        raise ValueError(f"ids_str must be [{B}], got {tuple(ids.shape)}")
    return ids.to(device=device, dtype=torch.int64).contiguous()


def slice_segments(x, ids_str, segment_size=4, *, scale=1):
    """commons.py:41-47: ret[b] = x[b, :, ids_str[b] : ids_str[b] + segment_size] -> [B, C, segment_size]; with
    `scale`, x[b, :, ids_str[b] * scale : (ids_str[b] + segment_size) * scale]."""
    x = _x3(x)
    B, C, T = x.shape
    seg, scale = int(segment_size), int(scale)
    if seg < 1 or scale < 1 or seg * scale > T:
        raise ValueError(f"segment_size * scale = {seg} * {scale} must be in [1, T={T}]")
    ids = _ids(ids_str, B, x.device)
    out = torch.empty(B, C, seg * scale, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().wetts_slice_segments(_lib.ptr(x), x.stride(0), x.stride(1), _lib.ptr(ids), B, C, T, seg,
                                                    scale, _lib.ptr(out), _lib.current_stream_ptr()), "slice_segments")
    return out


def rand(n, device):
    """torch.rand([n]) from the library's Philox kernel on the device generator's (seed, offset), which it advances."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("device must be a HIP device (there is no CPU path)")
    index = torch.cuda.current_device() if device.index is None else device.index
    gen = torch.cuda.default_generators[index]
    seed = gen.initial_seed() & 0xFFFFFFFFFFFFFFFF
    offset = int(gen.get_offset())
    out = torch.empty(int(n), dtype=torch.float32, device=torch.device("cuda", index))
    with torch.cuda.device(index):
        _lib.check(_lib.load().wetts_rand(_lib.ptr(out), int(n), seed, offset, _lib.current_stream_ptr()), "rand")
    gen.set_offset(offset + ((int(n) + 3) // 4 + 3) // 4 * 4)  # ATen keeps the offset a multiple of 4
    return out


def rand_slice_segments(x, x_lengths=None, segment_size=4, *, u=None):
    """commons.py:50-58 -> (ret [B, C, segment_size], ids_str [B] int64): ids_str = (u * (x_lengths - segment_size + 1))
    truncated, clamped to x_lengths - segment_size; a row shorter than the segment gets id 0."""
    x = _x3(x)
    B, C, T = x.shape
    seg = int(segment_size)
    if seg < 1 or seg > T:
        raise ValueError(f"segment_size must be in [1, T={T}], got {seg}")
    lengths = None
    if x_lengths is not None:
        lengths = torch.as_tensor(x_lengths)
        if tuple(lengths.shape) != (B,):
            raise ValueError(f"x_lengths must be [{B}], got {tuple(lengths.shape)}")
        lengths = lengths.to(device=x.device, dtype=torch.int64).contiguous()
    if u is None:
        u = rand(B, x.device)
    else:
        u = torch.as_tensor(u)
        if tuple(u.shape) != (B,):
            raise ValueError(f"u must be [{B}], got {tuple(u.shape)}")
        u = u.to(device=x.device, dtype=torch.float32).contiguous()
    ids = torch.empty(B, dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().wetts_slice_ids(_lib.ptr(u), None, _lib.ptr(lengths), B, T, seg, _lib.ptr(ids), None,
                                               _lib.current_stream_ptr()), "slice_ids")
    return slice_segments(x, ids, seg), ids
