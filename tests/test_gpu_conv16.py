"""GPU tier: every launch of the 16-bit conv kernels held to float64, element by element (tests/conv16_oracle.py: the
reference, the gate  |got - y| <= 1/2 ulp16 + (K + 4) 2^-24 S  and the sweep; tests/test_cpu_conv16_gate.py: why zero
violations is a fair assert and what the gate sees).  The launches run through the stand-alone entries of
include/wetts_hip.h (csrc/conv16_entry.hip), which fill the launchers' parameter blocks as the decoder and the 16-bit
WaveNet do.  bf16 and f16 throughout.

Which test holds which launcher of csrc/conv_bf16.h to float64, and at which tile remainders:

* launch_conv_bf16, epilogue 0 -- test_single_conv: the five instantiations (64 -> 128, 64 -> 64, 32 -> 128, 32 -> 64,
  32 -> 32), three chunks (192 -> 512), a partial last chunk and partial m-tiles (40 -> 96, 72 -> 160), each at
  T in {1, 5, NT - 1, NT, NT + 1, 2 NT + 3} and at every (k, dilation) of {(1, 1), (3, 1), (7, 3), (11, 5), (11, 12)}
  with T = NT + 1; leaky-relu, bias, per-utterance bias (B = 3), residual, running sum, out_div 3 / 5 and `basic` each
  on and off per instantiation.  test_transposed_conv: every (rate, kernel) of config.MODEL_CONFIGS at Tin in {1, 2, 33}.
* launch_conv_bf16, epilogues 1 and 2, k_gate_cl16, k_wn_update_cl16 -- test_wavenet_layer_pieces: H = 192,
  T in {4, 124, 128, 132} (NT = 128), a ragged mask, first / middle / last layer.  The plain in_layer and res_skip
  launches are gated as convs; the gate kernel and the fused gate epilogue against tanh(a) sigmoid(b) of the device's own
  rounded xin; h and skip of k_wn_update_cl16 against float64; the fused update epilogue is bit-equal to it
  (conv_bf16.hip: "equals k_wn_update_cl16 on the stored tensor").
* k_conv_post_mfma16 (epilogue 3) and k_conv_post_bf16 -- test_conv_post: C = 32 / 64, T in {1, 6, 511, 512, 513}.
* launch_resblock_pair16, launch_resblock2_chain16, launch_resblock2_stage16 -- test_resblock_launch: every
  (C, k, dilations) of v1, v3, stress48k and tiny at C in {32, 64, 128}, T in {1, h2, NTO - 1, NTO, NTO + 1, 2 NTO,
  2 NTO + 2, 3 NTO + NTO / 2}, B in {1, 3}, running sum and out_div on and off.  Conv by conv first: c1's output
  against float64 on x, c2's against float64 on the DEVICE's intermediate; then the fused launch is bit-equal to it.
  Stages of 1, 2 and 3 chains (v3's halos 2, 12, 36: columns between a chain's halo and the common origin).
* test_garbage_behind_the_ends: a conv, a pair and a stage on views inside NaN-filled buffers.
* test_refused_shapes: the status codes for what the launchers refuse.

With WETTS_CONV16_MARGINS set the worst err / gate per kernel class goes to that file (profiles/conv16_margins.txt)."""
import ctypes as C
import os

import pytest
import torch

from tests import conv16_oracle as co
from wetts_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = sorted(co.DTYPES)
CASES = co.conv_cases()
_MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out = os.environ.get("WETTS_CONV16_MARGINS")  # the GPU run that records profiles/conv16_margins.txt sets it
    if out and _MARGINS:
        with open(out, "w") as f:
            f.write("worst err / gate per kernel class over tests/test_gpu_conv16.py (1 = at the gate; gate = 1/2 ulp16 + "
                    "(K + 4) 2^-24 S per element, tests/conv16_oracle.py)\n")
            for k in sorted(_MARGINS):
                f.write(f"{k}: {_MARGINS[k]:.4f}\n")


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _f16(dtype):
    return 1 if dtype == torch.float16 else 0


def _flags(c, dtype):
    return (_lib.CONV16_F16 * _f16(dtype) | (_lib.CONV16_TRANSPOSED if c["up"] else 0) |
            (_lib.CONV16_LRELU if c["slope"] is not None else 0) | (_lib.CONV16_ACCUM if c["prev"] else 0) |
            (_lib.CONV16_BASIC if c["basic"] else 0))


def _conv(c, d, dtype, x=None, res=None, out=None, rc_only=False):
    """One wetts_conv16 launch of case c on the tensors d (channel-first, CPU) -> channel-first CPU output.  x / res /
    out: channel-last device tensors to use instead (views inside larger buffers)."""
    lib, s = _lib.load(), _lib.current_stream_ptr()
    B, To = c["B"], co.out_len(c)
    x = _d(co.cl(d["x"])) if x is None else x
    if res is None and d["res"] is not None:
        res = _d(co.cl(d["res"]))
    if out is None:
        out = _d(co.cl(d["prev"])) if d["prev"] is not None else _nan((B, To, c["Cout"]), dtype)
    w, bias, bias_b = _d(d["w"]), _d(d["bias"]), _d(d["bias_b"])
    rc = lib.wetts_conv16(_lib.ptr(w), _lib.ptr(bias), _lib.ptr(bias_b), _lib.ptr(x), _lib.ptr(res), _lib.ptr(out), B,
                          c["Cin"], c["Cout"], c["k"], c["dil"], c["pad"], c["up"], c["T"], To, _flags(c, dtype),
                          c["slope"] or 0.0, c["div"], s)
    if rc_only:
        return rc
    _lib.check(rc, "wetts_conv16 " + co.case_id(c))
    return co.cf(out.cpu())


# ---- single convs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape", co.CONV_SHAPES, ids=lambda s: f"{s[0]}to{s[1]}")
def test_single_conv(shape, dt):
    dtype = co.DTYPES[dt]
    tile = co.conv_tile(*shape)
    cls = co.conv_class(*shape) + "_" + dt
    for c in CASES:
        if c["up"] or (c["Cin"], c["Cout"]) != shape:
            continue
        d = co.conv_data(c, dtype)
        if co.conv_refused(c):  # two 64-channel staging buffers of span 120 exceed the LDS the launcher allows itself
            assert _conv(c, d, dtype, rc_only=True) == -1 and "LDS" in _lib.last_error(), co.case_id(c)
            continue
        y, S, K = co.case_ref(c, d)
        r = co.check(co.case_id(c) + " " + dt, _conv(c, d, dtype), y, S, K, dtype, nt=tile["NT"], margins=_MARGINS, cls=cls)
        print(f"{co.case_id(c)} {dt}: worst err / gate {r:.3f}")


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("ratek", co.transposed_shapes(), ids=lambda s: f"up{s[0]}k{s[1]}")
def test_transposed_conv(ratek, dt):
    dtype, n = co.DTYPES[dt], 0
    for c in CASES:
        if (c["up"], c["k"]) != ratek:
            continue
        d = co.conv_data(c, dtype)
        y, S, K = co.case_ref(c, d)
        # the kernel's columns are input positions n = (t + pad) // up: the tile of an output sample follows from it
        co.check(co.case_id(c) + " " + dt, _conv(c, d, dtype), y, S, K, dtype, margins=_MARGINS,
                 cls=co.conv_class(c["Cin"], c["Cout"] * c["up"]) + "_transposed_" + dt)
        n += 1
    assert n == 6


# ---- WaveNet layer pieces -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("T", co.WN_T)
def test_wavenet_layer_pieces(T, dt):
    dtype, H, k, B, f16 = co.DTYPES[dt], co.WN_H, co.WN_K, 3, _f16(co.DTYPES[dt])
    lib, s = _lib.load(), _lib.current_stream_ptr()
    g = torch.Generator().manual_seed(8000 + T)
    w_in, b_in = torch.randn(2 * H, H, k, generator=g) / (H * k) ** 0.5, torch.randn(2 * H, generator=g) * 0.3
    gl = torch.randn(B, 3, 2 * H, generator=g) * 0.3  # the cond_layer output of three layers: layer 1's slice is used
    h = torch.randn(B, H, T, generator=g).to(dtype)
    mask = co.wn_mask(B, T)
    h_d, gl_d, mask_d = _d(co.cl(h)), _d(gl), _d(mask)
    # in_layer, plain launch
    c = dict(Cin=H, Cout=2 * H, k=k, dil=1, pad=k // 2, up=0, B=B, T=T, slope=None, prev=False, basic=0, div=1.0)
    d = dict(w=w_in, x=h, bias=b_in, bias_b=gl[:, 1].contiguous(), res=None, prev=None)
    xin = _conv(c, d, dtype)
    y, S, K = co.conv_ref(h, w_in, pad=k // 2, bias=b_in, bias_b=gl[:, 1])
    co.check(f"in_layer T{T} {dt}", xin, y, S, K, dtype, nt=128, margins=_MARGINS, cls="wn_in_layer_plain_" + dt)
    # the gate: the stand-alone kernel and the fused epilogue, both against the device's own rounded xin
    xin_d = _d(co.cl(xin))
    ya = co.wn_gate_ref(xin)
    acts_d = _nan((B, T, H), dtype)
    _lib.check(lib.wetts_wn16_gate(_lib.ptr(xin_d), _lib.ptr(acts_d), B * T, H, f16, s), "wn16_gate")
    acts = co.cf(acts_d.cpu())
    co.check(f"k_gate_cl16 T{T} {dt}", acts, ya, ya.abs(), 0, dtype, margins=_MARGINS, cls="wn_gate_kernel_" + dt)
    actsf_d = _nan((B, T, H), dtype)
    glv = gl_d[:, 1]  # rows 6H apart
    w_in_d, b_in_d = _d(w_in), _d(b_in)  # (named: a temporary's memory is reused by the next allocation)
    _lib.check(lib.wetts_conv16_wn_gate(_lib.ptr(w_in_d), _lib.ptr(b_in_d), _lib.ptr(glv), 6 * H, _lib.ptr(h_d),
                                        _lib.ptr(actsf_d), B, H, k, 1, T, f16, s), "conv16_wn_gate")
    co.check(f"epi_mode 1 T{T} {dt}", co.cf(actsf_d.cpu()), ya, ya.abs(), 0, dtype, nt=128,
             extra=co.GATE_FAST_REL * ya.abs(), margins=_MARGINS, cls="wn_gate_epi1_" + dt)
    # res_skip: plain launch + k_wn_update_cl16, then the fused epilogue, for a first, a middle and the last layer
    for first, last in ((1, 0), (0, 0), (0, 1)):
        RC = H if last else 2 * H
        w_rs, b_rs = torch.randn(RC, H, 1, generator=g) / H ** 0.5, torch.randn(RC, generator=g) * 0.3
        skip = torch.randn(B, H, T, generator=g)
        c2 = dict(c, Cin=H, Cout=RC, k=1, pad=0)
        rs = _conv(c2, dict(w=w_rs, x=acts, bias=b_rs, bias_b=None, res=None, prev=None), dtype)
        y, S, K = co.conv_ref(acts, w_rs, bias=b_rs)
        co.check(f"res_skip T{T} {dt}", rs, y, S, K, dtype, nt=128, margins=_MARGINS, cls="wn_res_skip_plain_" + dt)
        # (a first layer's skip is written, not read: NaN there proves it)
        skip0 = _nan((B, T, H), torch.float32) if first else _d(co.cl(skip))
        hu_d, su_d = h_d.clone(), skip0.clone()
        rs_d, w_rs_d, b_rs_d = _d(co.cl(rs)), _d(w_rs), _d(b_rs)
        _lib.check(lib.wetts_wn16_update(_lib.ptr(rs_d), _lib.ptr(hu_d), _lib.ptr(su_d), _lib.ptr(mask_d), last,
                                         first, B * T, H, f16, s), "wn16_update")
        hn, sk = co.wn_update_ref(rs, h, skip, mask, last, first)
        hu, su = co.cf(hu_d.cpu()), co.cf(su_d.cpu())
        if last:
            assert torch.equal(hu_d, h_d)
        else:
            co.check(f"h T{T} {dt}", hu, hn, h.double().abs() + rs[:, :H].double().abs(), 0, dtype, margins=_MARGINS,
                     cls="wn_update_h_" + dt)
            assert bool((hu * (1 - mask).unsqueeze(1).to(dtype) == 0).all())  # masked frames are exact zeros
        rsk = (rs if last else rs[:, H:]).double().abs()
        co.check(f"skip T{T} {dt}", su, sk, rsk if first else skip.double().abs() + rsk, 0, None, margins=_MARGINS,
                 cls="wn_update_skip_" + dt)
        hf_d, sf_d = h_d.clone(), skip0.clone()
        _lib.check(lib.wetts_conv16_wn_update(_lib.ptr(w_rs_d), _lib.ptr(b_rs_d), _lib.ptr(acts_d), _lib.ptr(hf_d),
                                              _lib.ptr(sf_d), _lib.ptr(mask_d), B, H, T, last, first, f16, s),
                   "conv16_wn_update")
        assert torch.equal(hf_d, hu_d), f"epi_mode 2 h differs from k_wn_update_cl16 (T {T}, first {first}, last {last})"
        assert torch.equal(sf_d, su_d), f"epi_mode 2 skip differs from k_wn_update_cl16 (T {T}, first {first}, last {last})"


# ---- conv_post ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("C_,mfma", ((32, 1), (32, 0), (64, 0)))
def test_conv_post(C_, mfma, dt):
    dtype, B = co.DTYPES[dt], 2
    lib, s = _lib.load(), _lib.current_stream_ptr()
    for i, T in enumerate((1, 6, 511, 512, 513)):
        g = torch.Generator().manual_seed(8100 + i)
        w, x = torch.randn(1, C_, 7, generator=g) / (C_ * 7) ** 0.5, torch.randn(B, C_, T, generator=g).to(dtype)
        out, w_d, x_d = _nan((B, T), torch.float32), _d(w), _d(co.cl(x))
        _lib.check(lib.wetts_conv16_post(_lib.ptr(w_d), _lib.ptr(x_d), _lib.ptr(out), B, C_, T, mfma,
                                         _f16(dtype), s), "conv16_post")
        # the matrix-core form reads 16-bit weights and a rounded leaky-relu; the scalar one f32 weights, f32 leaky-relu
        y, S, K = co.conv_ref(x, w, pad=3, slope=0.01, round_w=bool(mfma), round_act=bool(mfma))
        co.check(f"conv_post C{C_} mfma{mfma} T{T} {dt}", out.cpu().unsqueeze(1), torch.tanh(y), S, K, None,
                 nt=512 if mfma else 256, margins=_MARGINS, cls=f"conv_post_{'mfma' if mfma else 'scalar'}_C{C_}_{dt}")


# ---- ResBlock launches ----------------------------------------------------------------------------------------------
def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _resblock(form, fused, chains, wd, x_d, out_d, mid_d, B, C_, T, accum, div, dtype):
    lib, s = _lib.load(), _lib.current_stream_ptr()
    n = len(chains)
    ints = lambda v: (C.c_int32 * n)(*v)
    return lib.wetts_resblock16(form, fused, n, _ptrs([w[0] for w in wd]), _ptrs([w[1] for w in wd]),
                                _ptrs([w[2] for w in wd]), _ptrs([w[3] for w in wd]), ints([c[0] for c in chains]),
                                ints([c[1] for c in chains]), ints([c[2] for c in chains]), _lib.ptr(x_d), _lib.ptr(out_d),
                                _lib.ptr(mid_d), B, C_, T, accum, div, _f16(dtype), s)


def _chain_by_chain(g, rc, dtype, name):
    """The conv-by-conv form of a group, chain by chain, each conv gated against float64 on the device's own input.
    Returns the device tensors (x, weights, mids [n][B][T][C], out, the running sum it started from)."""
    form, C_, chains = g
    B, T = rc["B"], rc["T"]
    wbs = co.rb_weights(C_, chains, rc["seed"])
    x, prev = co.rb_input(B, C_, T, rc["seed"] + 1, dtype, rc["prev"])
    wd = [[_d(t) for t in wb] for wb in wbs]
    x_d, prev_d = _d(co.cl(x)), (_d(co.cl(prev)) if prev is not None else None)
    mids, run, run_d = [], prev, prev_d
    ntc, nto, _ = co.rb_geom(form, C_, chains)
    for j, ((k, d1, d2), wb) in enumerate(zip(chains, wbs)):
        div = rc["div"] if j == len(chains) - 1 else 1.0
        out_d = run_d.clone() if run_d is not None else _nan((B, T, C_), dtype)
        mid_d = _nan((1, B, T, C_), dtype)
        f1 = 0 if form == 0 else 1
        _lib.check(_resblock(f1, 0, chains[j:j + 1], wd[j:j + 1], x_d, out_d, mid_d, B, C_, T, 1 if run_d is not None else 0,
                             div, dtype), "resblock16 conv by conv")
        mid, out = co.cf(mid_d[0].cpu()), co.cf(out_d.cpu())
        cls = f"{('pair', 'chain', 'stage')[form]}_C{C_}_" + ("f16" if dtype == torch.float16 else "bf16")
        co.check(f"{name} c1[{j}]", mid, *co.rb_c1_ref(f1, x, wb, k, d1), dtype, nt=nto, margins=_MARGINS, cls=cls + "_c1")
        co.check(f"{name} c2[{j}]", out, *co.rb_c2_ref(f1, x, mid, wb, k, d2, run, div), dtype, nt=nto, margins=_MARGINS,
                 cls=cls + "_c2")
        mids.append(mid_d[0])
        run, run_d = out, out_d
    return x_d, wd, torch.stack(mids), run_d, prev_d


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("g", co.rb_groups(), ids=co.rb_id)
def test_resblock_launch(g, dt):
    form, C_, chains = g
    dtype = co.DTYPES[dt]
    for rc in co.rb_cases(form, C_, chains):
        B, T = rc["B"], rc["T"]
        name = f"{co.rb_id(g)} T{T} B{B} {dt}"
        x_d, wd, mids_d, out_d, prev_d = _chain_by_chain(g, rc, dtype, name)
        accum = 1 if prev_d is not None else 0
        fresh = lambda: prev_d.clone() if prev_d is not None else _nan((B, T, C_), dtype)
        if form == 2:  # the entry's own conv-by-conv form of the whole stage is those launches
            o2, m2 = fresh(), _nan((len(chains), B, T, C_), dtype)
            _lib.check(_resblock(2, 0, chains, wd, x_d, o2, m2, B, C_, T, 0, rc["div"], dtype), "resblock16 stage unfused")
            assert torch.equal(o2, out_d) and torch.equal(m2, mids_d), name
        if not co.rb_fused_supported(form, C_, chains):
            continue
        of = fresh()
        _lib.check(_resblock(form, 1, chains, wd, x_d, of, None, B, C_, T, accum, rc["div"], dtype), "resblock16 fused")
        if not torch.equal(of, out_d):
            ntc, nto, h = co.rb_geom(form, C_, chains)
            bad = (of.view(torch.int16) != out_d.view(torch.int16)).nonzero()
            b, t, c = [int(v) for v in bad[0]]
            raise AssertionError(f"{name}: fused != conv by conv at {len(bad)} elements, first (b, t, c) = ({b}, {t}, {c}), "
                                 f"tile {t // nto} column {t % nto} of {nto} (halo {h})")


# ---- garbage behind the ends ----------------------------------------------------------------------------------------
def _inside_nan(t, pad=4096):
    """A copy of the channel-last device tensor t as a view in the middle of a NaN-filled buffer (16-byte aligned)."""
    big = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=t.dtype, device=DEV)
    v = big[pad:pad + t.numel()].view(t.shape)
    v.copy_(t)
    return big, v


def _untouched(big, n, pad=4096):
    return bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + n:]).all())


@pytest.mark.parametrize("dt", DT)
def test_garbage_behind_the_ends(dt):
    """Rows before and behind an utterance's plane are the convs' zero padding, whatever the memory there holds: each
    launch on views inside larger NaN-filled (ordinary, in-bounds) buffers gives the bits of the plain run and leaves the
    surroundings alone."""
    dtype = co.DTYPES[dt]
    c = next(c for c in CASES if (c["Cin"], c["Cout"]) == (64, 128) and c["res"] and c["prev"] and c["T"] == 129)
    d = co.conv_data(c, dtype)
    plain = _conv(c, d, dtype)
    bx, vx = _inside_nan(_d(co.cl(d["x"])))
    br, vr = _inside_nan(_d(co.cl(d["res"])))
    bo, vo = _inside_nan(_d(co.cl(d["prev"])))
    got = _conv(c, d, dtype, x=vx, res=vr, out=vo)
    assert torch.equal(got, plain)
    assert _untouched(bx, vx.numel()) and _untouched(br, vr.numel()) and _untouched(bo, vo.numel())
    v3 = ((3, 1, 2), (5, 2, 6), (7, 3, 12))
    for form, C_, chains, T in ((0, 64, ((7, 3, 1),), 251), (2, 32, v3, 697)):
        B = 2
        wd = [[_d(t) for t in wb] for wb in co.rb_weights(C_, chains, 9901)]
        x, _ = co.rb_input(B, C_, T, 9902, dtype, False)
        x_d, out_d = _d(co.cl(x)), _nan((B, T, C_), dtype)
        _lib.check(_resblock(form, 1, chains, wd, x_d, out_d, None, B, C_, T, 0, 3.0, dtype), "resblock16 fused")
        assert bool(torch.isfinite(out_d.float()).all())
        bx, vx = _inside_nan(x_d)
        bo, vo = _inside_nan(out_d * 0)
        _lib.check(_resblock(form, 1, chains, wd, vx, vo, None, B, C_, T, 0, 3.0, dtype), "resblock16 fused, inside NaN")
        assert torch.equal(vo, out_d), (form, C_)
        assert _untouched(bx, vx.numel()) and _untouched(bo, vo.numel())


# ---- what the launchers refuse --------------------------------------------------------------------------------------
def test_refused_shapes():
    dtype = torch.bfloat16
    base = dict(Cin=32, Cout=32, k=3, dil=1, pad=1, up=0, B=1, T=8, slope=0.1, bias=True, bias_b=False, res=False,
                prev=False, div=1.0, basic=0, seed=1)
    for over in (dict(Cout=48), dict(Cin=36), dict(k=11, dil=13, pad=65)):  # Cout % 32, Cin % 8, a span of 130 > 128
        c = dict(base, **over)
        assert _conv(c, co.conv_data(c, dtype), dtype, rc_only=True) == -1, over
        assert _lib.last_error()
    c = dict(base, Cin=64, up=2, k=4, pad=1, res=True)  # a transposed conv has no residual
    assert _conv(c, co.conv_data(c, dtype), dtype, rc_only=True) == -1
    v3 = ((3, 1, 2), (5, 2, 6), (7, 3, 12))
    for form, C_, chains in ((2, 128, v3), (1, 64, v3[2:]), (0, 256, ((3, 1, 1),))):  # no fused kernel for these
        wd = [[_d(t) for t in wb] for wb in co.rb_weights(C_, chains, 3)]
        x_d, out_d = _d(torch.zeros(1, 8, C_, dtype=dtype)), _nan((1, 8, C_), dtype)
        assert _resblock(form, 1, chains, wd, x_d, out_d, None, 1, C_, 8, 0, 1.0, dtype) == -1, (form, C_)
        assert bool(torch.isnan(out_d.float()).all())
    # the plain run still works afterwards
    d = co.conv_data(base, dtype)
    co.check("after refusals", _conv(base, d, dtype), *co.case_ref(base, d), dtype)
