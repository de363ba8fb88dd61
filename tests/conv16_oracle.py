"""Shared by tests/test_cpu_conv16_gate.py and tests/test_gpu_conv16.py: the float64 reference of ONE launch of the
16-bit conv kernels (csrc/conv_bf16.hip, resblock16.hip, resblock2_stage16.hip, wn16.hip), the per-element gate it is
held to, the sweep of cases, and the kernels' tile arithmetic restated in Python (no kernel reads it).

Why per launch.  End to end the 16-bit decoder cannot be gated locally: a rounding that falls the other way is as large
as the whole precision loss and is amplified through ~60 convs (tests/test_cpu_conv16_gate.py::test_end_to_end_floor
records the figures: the bf16 simulator with f32 accumulation against the same simulator with f64 accumulation).  On
the launch's own input the error is bounded by arithmetic, so every output element gets its own bound.

The reference is the launch's operation in float64 on the 16-bit values the device reads: the activations as stored
(leaky-relu taken in f32 and rounded to the type, conv16_dev.h:lrelu_pk2), the weights rounded to the type
(pack_bf16_kernel); bias, per-utterance bias, residual, running sum and the division in float64; nothing rounded at the
end.

The gate, per output element; nothing in it is measured:

    |got - y|  <=  1/2 ulp16(max(|y|, |got|))  +  (K + 4) 2^-24 S

ulp16 = the spacing of the storage type at that magnitude (floored at its smallest subnormal): the one rounding of the
stored value.  K = Cin * taps terms are accumulated in f32 in an order of the kernel's choosing; S = the same launch on
absolute values (sum |w||x| + |bias| + |bias_b| + |res| + |sum|, divided like the output): (K + 4) 2^-24 S bounds f32
accumulation of K products and the four epilogue operations in any order.  f32 outputs (conv_post, skip) have no
first term.  The fused WaveNet gate adds 4e-6 |value| for its hardware exp / rcp ("~1e-6 relative",
conv_bf16.hip:109-110)."""
import math

import torch
import torch.nn.functional as F

from wetts_amd import config

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
_MANT = {torch.bfloat16: 7, torch.float16: 10}
_MIN_SUB = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}
U32 = 2.0 ** -24
GATE_FAST_REL = 4e-6  # conv_bf16.hip:109 "~1e-6 relative" (gate_fast: v_exp_f32, v_rcp_f32), taken fourfold


def ulp16(v, dtype):
    """Spacing of `dtype` at magnitude |v| (float64 tensor), floored at the smallest subnormal."""
    _, e = torch.frexp(v.abs().double())  # |v| = m 2^e, m in [0.5, 1)
    u = torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 1 - _MANT[dtype])
    return torch.clamp(u, min=_MIN_SUB[dtype])


def q(w, dtype):
    """Round to the storage type (round to nearest even, as pack_bf16_kernel / pk2) and widen to float64."""
    return w.to(dtype).double()


def lrelu16(x16, slope):
    """What the conv reads: leaky-relu in f32 (one f32 product), rounded back to the type."""
    if slope is None:
        return x16
    xf = x16.float()
    return torch.maximum(xf, xf * torch.tensor(slope, dtype=torch.float32)).to(x16.dtype)


def _conv(x, w, dil, pad, up):
    if up:
        return F.conv_transpose1d(x, w, stride=up, padding=pad)
    return F.conv1d(x, w, dilation=dil, padding=pad)


def conv_ref(x16, w, *, dil=1, pad=0, up=0, slope=None, bias=None, bias_b=None, res=None, prev=None, div=1.0,
             round_w=True, round_act=True):
    """(y, S, K) of one conv launch, float64, channel-first.  x16 [B, Cin, T] in the storage type; w f32 [Cout, Cin, k]
    (transposed: [Cin, Cout, k]); bias [Cout] / bias_b [B, Cout] f32; res / prev [B, Cout, Tout] in the storage type.
    round_w / round_act = False: the scalar conv_post kernel, which reads f32 weights and keeps lrelu in f32."""
    dt = x16.dtype
    if round_act:
        xq = lrelu16(x16, slope).double()
    else:
        xf = x16.float()
        xq = torch.maximum(xf, xf * torch.tensor(slope, dtype=torch.float32)).double()
    wq = q(w, dt) if round_w else w.double()
    y = _conv(xq, wq, dil, pad, up)
    S = _conv(xq.abs(), wq.abs(), dil, pad, up)
    for t, shape in ((bias, (1, -1, 1)), (bias_b, None), (res, None), (prev, None)):
        if t is None:
            continue
        t = t.double()
        t = t.reshape(shape) if shape else (t.unsqueeze(-1) if t.dim() == 2 else t)
        y = y + t
        S = S + t.abs()
    k = w.shape[2]
    K = x16.shape[1] * (-(-k // up) if up else k)
    return y / div, S / abs(div), K


def gate(y, S, K, dtype, got=None, extra=None):
    """The per-element bound.  dtype None: an f32 output (no storage rounding)."""
    g = (K + 4) * U32 * S
    if dtype is not None:
        m = y.abs() if got is None else torch.maximum(y.abs(), got.double().abs())
        g = g + 0.5 * ulp16(m, dtype)
    if extra is not None:
        g = g + extra
    return g


def ratio(got, y, S, K, dtype, extra=None):
    """err / gate per element (float64)."""
    got = got.double()
    return (got - y).abs() / gate(y, S, K, dtype, got, extra)


def check(name, got, y, S, K, dtype, nt=None, extra=None, margins=None, cls=None):
    """Asserts zero violating elements of a channel-first [B, C, T] (or [B, T]) output; names the worst one.  nt: the
    kernel's output columns per tile.  Returns the worst err / gate and records it under `cls` in `margins`."""
    assert tuple(got.shape) == tuple(y.shape), (name, tuple(got.shape), tuple(y.shape))
    assert bool(torch.isfinite(got.double()).all()), f"{name}: non-finite output"
    r = ratio(got, y, S, K, dtype, extra)
    worst = float(r.max())
    if margins is not None and cls is not None:
        margins[cls] = max(margins.get(cls, 0.0), worst)
    bad = int((r > 1.0).sum())
    if bad:
        idx = [int(i) for i in torch.unravel_index(torch.argmax(r), r.shape)]
        b, t = idx[0], idx[-1]
        c = idx[1] if len(idx) == 3 else 0
        where = f"(b, t, c) = ({b}, {t}, {c})"
        if nt:
            where += f", tile {t // nt} column {t % nt} of {nt}"
        raise AssertionError(f"{name}: {bad} of {r.numel()} elements outside the gate; worst err / gate = {worst:.3g} at "
                             f"{where}: got {float(got[tuple(idx)]):.9g}, float64 {float(y[tuple(idx)]):.9g}")
    return worst


# ---- tile arithmetic of the kernels (launch_conv_bf16, resblock16.hip:launch_pair, resblock2_stage16.hip) ---------------
def conv_tile(Cin, M):
    """The instantiation launch_conv_bf16 picks: dict(CKB, NT, MT).  M = Cout (transposed: Cout * up)."""
    if Cin >= 64:
        nt = 128 if M >= 128 else 256
        return dict(CKB=64, NT=nt, MT=128 if nt == 128 else 64)
    nt = 128 if M >= 128 else (256 if M >= 64 else 512)
    return dict(CKB=32, NT=nt, MT={128: 128, 256: 64, 512: 32}[nt])


def conv_class(Cin, M):
    t = conv_tile(Cin, M)
    return f"conv_ckb{t['CKB']}_nt{t['NT']}"


def conv_lds_bytes(Cin, M, span):
    """Dynamic LDS of the launch (conv_bf16.hip:launch_b): one staging buffer of NT + span rows in whole passes, two when
    the reduction has more than one channel chunk."""
    t = conv_tile(Cin, M)
    rs, rpp = t["CKB"] * 2 + 16, 256 // (t["CKB"] // 8)
    rows = -(-(t["NT"] + span) // rpp) * rpp
    return (2 if -(-Cin // t["CKB"]) > 1 else 1) * rows * rs


def conv_refused(c):
    """Cases of the sweep that launch_conv_bf16 refuses (WETTS_E_INVALID, "exceeds the default dynamic LDS"): span 120 at
    64-channel chunks needs 2 x 256 rows x 144 B = 72 KB once there are two chunks to double-buffer (192 -> 512,
    72 -> 160).  No model has such a conv (the widest multi-chunk span is 50); the sweep asserts the status code."""
    return not c["up"] and conv_lds_bytes(c["Cin"], c["Cout"], (c["k"] - 1) * c["dil"]) > 64 * 1024


def pair_geom(C, k):
    """ResBlock1 pair: (NTC, NTO, halo per side)."""
    ntc = 128 * (4 // (C // 32))
    return ntc, ntc - (k - 1), (k - 1) // 2


def chain_geom(C, k, dil2):
    """ResBlock2 chain: (NTC, NTO, halo per side)."""
    ntc = 128 * (8 // (C // 32))
    h2 = (k - 1) // 2 * dil2
    return ntc, ntc - 2 * h2, h2


def stage_geom(C, chains):
    """ResBlock2 stage of `chains` = [(k, d1, d2), ...]: (NTC, NTO, o); o = the widest c2 halo.  Tiles whose window
    [n0 - o, n0 - o + NTC) leaves [0, T) take the `edge` path (resblock2_stage16.hip:82), the others the interior one."""
    ntc = 32 * 3 * (8 // (C // 32))
    o = max((k - 1) // 2 * d2 for k, _, d2 in chains)
    return ntc, ntc - 2 * o, o


def stage_edge_tiles(T, ntc, nto, o):
    """[is_edge] per tile of the stage kernel."""
    return [n0 - o < 0 or n0 - o + ntc > T for n0 in range(0, T, nto)]


def tile_events(T, nto, halo):
    """What a length exercises on a kernel of `nto` output columns per tile and `halo` columns of reach: a set of
    'narrow' (last tile narrower than the halo), 'seam' (it ends exactly on one), 'past' (one column past a seam),
    'single' (a single partial tile), 'multi' (>= 3 tiles)."""
    ev, r, n = set(), T % nto, -(-T // nto)
    if n >= 2 and 0 < r < halo:
        ev.add("narrow")
    if r == 0:
        ev.add("seam")
    if n >= 2 and r == 1:
        ev.add("past")
    if n == 1 and r:
        ev.add("single")
    if n >= 3:
        ev.add("multi")
    return ev


EVENTS = {"narrow", "seam", "past", "single", "multi"}


def conv_lengths(nt):
    return (1, 5, nt - 1, nt, nt + 1, 2 * nt + 3)


def resblock_lengths(nto, h2):
    return tuple(dict.fromkeys((1, h2, nto - 1, nto, nto + 1, 2 * nto, 2 * nto + 2, 3 * nto + nto // 2)))


# ---- the sweep ----------------------------------------------------------------------------------------------------------
CONV_SHAPES = ((64, 128), (64, 64), (32, 128), (32, 64), (32, 32),  # the five instantiations
               (192, 512),  # three chunks: conv_pre
               (40, 96), (72, 160))  # a partial last chunk, partial m-tiles
KDIL = ((1, 1), (3, 1), (7, 3), (11, 5), (11, 12))  # the last: span 120 of the 128 allowed
# epilogue switches, rotated over the cases so that each is on and off at least once per instantiation:
# (leaky-relu, bias, per-utterance bias, residual, running sum, out_div, basic)
SWITCHES = ((0.1, True, False, False, False, 1.0, 0),
            (None, True, True, True, False, 3.0, 1),
            (0.1, False, False, True, True, 5.0, 0),
            (None, False, True, False, True, 1.0, 1),
            (0.1, True, True, True, True, 3.0, 0),
            (0.1, True, False, True, False, 1.0, 1))


def transposed_shapes():
    """Every distinct (rate, kernel) of config.MODEL_CONFIGS, sorted."""
    s = set()
    for m in config.MODEL_CONFIGS.values():
        s |= set(zip(m.get("upsample_rates", ()), m.get("upsample_kernel_sizes", ())))
    return tuple(sorted(s))


def conv_cases():
    """The single-conv sweep: dicts(Cin, Cout, k, dil, pad, up, B, T, slope, bias, bias_b, res, prev, div, basic, seed).
    Per shape: every length of conv_lengths at a (k, dil) and a switch set that rotate, then every (k, dil) once more
    at NT + 1 (one column past the seam, the last tile narrower than every halo); B = 3 wherever a per-utterance bias
    is on.  Then the transposed convs at Tin in {1, 2, 33}."""
    out, n = [], 0
    for Cin, Cout in CONV_SHAPES:
        nt = conv_tile(Cin, Cout)["NT"]
        # (the lengths rotate over the first four: span 120 is refused at two of the shapes, see conv_refused)
        plan = [(T, KDIL[(i + 1) % 4]) for i, T in enumerate(conv_lengths(nt))] + [(nt + 1, kd) for kd in KDIL]
        for i, (T, (k, dil)) in enumerate(plan):
            slope, bias, bias_b, res, prev, div, basic = SWITCHES[i % len(SWITCHES)]
            out.append(dict(Cin=Cin, Cout=Cout, k=k, dil=dil, pad=(k - 1) // 2 * dil, up=0, B=3 if bias_b else 1 + i % 2,
                            T=T, slope=slope, bias=bias, bias_b=bias_b, res=res, prev=prev, div=div, basic=basic,
                            seed=7000 + n))
            n += 1
    for up, k in transposed_shapes():
        for j, Tin in enumerate((1, 2, 33)):
            for Cin, Cout in ((64, 32), (128, 64)):
                out.append(dict(Cin=Cin, Cout=Cout, k=k, dil=1, pad=(k - up) // 2, up=up, B=1 + j, T=Tin,
                                slope=0.1 if j != 1 else None, bias=j != 2, bias_b=j == 1, res=False, prev=False, div=1.0,
                                basic=j % 2, seed=7000 + n))
                n += 1
    return out


def case_id(c):
    s = f"{c['Cin']}to{c['Cout']}_k{c['k']}d{c['dil']}_T{c['T']}_B{c['B']}"
    return s + (f"_up{c['up']}" if c["up"] else "")


def out_len(c):
    if c["up"]:
        return (c["T"] - 1) * c["up"] - 2 * c["pad"] + c["k"]
    return c["T"] + 2 * c["pad"] - (c["k"] - 1) * c["dil"]


def conv_data(c, dtype):
    """The tensors of a case (CPU, channel-first): w f32 scaled so that the output is O(1), x ~ N(0, 1) in the type."""
    g = torch.Generator().manual_seed(c["seed"])
    Cin, Cout, k, B, T, To = c["Cin"], c["Cout"], c["k"], c["B"], c["T"], out_len(c)
    taps = -(-k // c["up"]) if c["up"] else k
    shape = (Cin, Cout, k) if c["up"] else (Cout, Cin, k)
    d = dict(w=torch.randn(shape, generator=g) / math.sqrt(Cin * taps), x=torch.randn(B, Cin, T, generator=g).to(dtype))
    d["bias"] = torch.randn(Cout, generator=g) if c["bias"] else None
    d["bias_b"] = torch.randn(B, Cout, generator=g) if c["bias_b"] else None
    d["res"] = torch.randn(B, Cout, To, generator=g).to(dtype) if c["res"] else None
    d["prev"] = torch.randn(B, Cout, To, generator=g).to(dtype) if c["prev"] else None
    return d


def case_ref(c, d):
    return conv_ref(d["x"], d["w"], dil=c["dil"], pad=c["pad"], up=c["up"], slope=c["slope"], bias=d["bias"],
                    bias_b=d["bias_b"], res=d["res"], prev=d["prev"], div=c["div"])


def f32_model(x16, w, *, dil=1, pad=0, up=0, slope=None, bias=None, bias_b=None, res=None, prev=None, div=1.0):
    """The launch as torch computes it in f32 on the same 16-bit-valued operands, rounded once: what a correct kernel
    is allowed to be.  Returns the storage type."""
    dt = x16.dtype
    y = _conv(lrelu16(x16, slope).float(), w.to(dt).float(), dil, pad, up)
    if bias is not None:
        y = y + bias.reshape(1, -1, 1)
    if bias_b is not None:
        y = y + bias_b.unsqueeze(-1)
    if res is not None:
        y = y + res.float()
    if prev is not None:
        y = y + prev.float()
    if div != 1.0:
        y = y / torch.tensor(div, dtype=torch.float32)
    return y.to(dt)


def case_f32(c, d, **over):
    """f32_model of a case; `over` replaces operands (x, w) or switches (bias=None, res=None, div=1.0, ...)."""
    kw = dict(x=d["x"], w=d["w"], dil=c["dil"], pad=c["pad"], up=c["up"], slope=c["slope"], bias=d["bias"],
              bias_b=d["bias_b"], res=d["res"], prev=d["prev"], div=c["div"])
    kw.update(over)
    return f32_model(kw.pop("x"), kw.pop("w"), **kw)


# ---- ResBlocks ----------------------------------------------------------------------------------------------------------
RB_MODELS = ("v1", "v3", "stress48k", "tiny")


def resblock_shapes():
    """(pairs, chains, stages) that RB_MODELS put at C in {32, 64, 128}: pairs = sorted {(C, k, d)} of ResBlock1,
    chains = sorted {(C, k, d1, d2)} of ResBlock2, stages = sorted {(C, ((k, d1, d2), ...))}."""
    pairs, chains, stages = set(), set(), set()
    for name in RB_MODELS:
        m = config.MODEL_CONFIGS[name]
        ch = m["upsample_initial_channel"]
        for _ in m["upsample_rates"]:
            ch //= 2
            if ch not in (32, 64, 128):
                continue
            if str(m["resblock"]) == "1":
                for k, dils in zip(m["resblock_kernel_sizes"], m["resblock_dilation_sizes"]):
                    pairs |= {(ch, k, d) for d in dils}
            else:
                cs = tuple((k, d[0], d[1]) for k, d in zip(m["resblock_kernel_sizes"], m["resblock_dilation_sizes"]))
                chains |= {(ch,) + c for c in cs}
                stages.add((ch, cs))
    return sorted(pairs), sorted(chains), sorted(stages)


def chain_fused_supported(C, k, d1, d2):
    """resblock2_chain16_supported at max_waste_pct = 100."""
    return (k - 1) * max(d1, d2) <= (80 if C == 32 else 64) and (k - 1) * d2 <= chain_geom(C, k, d2)[0]


def stage_fused_supported(C, chains):
    """resblock2_stage16_nto > 0 at max_waste_pct = 100."""
    return C in (32, 64) and all(2 * max((k - 1) // 2 * d1, (k - 1) // 2 * d2) <= 80 for k, d1, d2 in chains)


def rb_groups():
    """[(form, C, chains)]: form 0 = ResBlock1 pair ((k, d, 1),), 1 = ResBlock2 chain ((k, d1, d2),), 2 = ResBlock2 stage of
    1, 2 and all chains of the config (v3: k = 3, 5, 7 with c2 halos 2, 12, 36, so columns between h2_j and o exist)."""
    pairs, chains, stages = resblock_shapes()
    out = [(0, C, ((k, d, 1),)) for C, k, d in pairs] + [(1, C, ((k, d1, d2),)) for C, k, d1, d2 in chains]
    for C, cs in stages:
        out += [(2, C, cs[:n]) for n in range(1, len(cs) + 1)]
    return out


def rb_geom(form, C, chains):
    """(NTC, NTO, halo per side) of the fused launch of a group."""
    k, _, d2 = chains[0]
    return pair_geom(C, k) if form == 0 else chain_geom(C, k, d2) if form == 1 else stage_geom(C, chains)


def rb_fused_supported(form, C, chains):
    k, d1, d2 = chains[0]
    if form == 0:
        return (k - 1) * d1 <= 64
    return chain_fused_supported(C, k, d1, d2) if form == 1 else stage_fused_supported(C, chains)


def rb_cases(form, C, chains):
    """The lengths of a group with B in {1, 3}, the running sum and out_div (3: the fast quotient) rotating on and off;
    a stage has no running sum and divides by its chain count.  dicts(T, B, prev, div, seed)."""
    _, nto, h = rb_geom(form, C, chains)
    out = []
    for i, T in enumerate(resblock_lengths(nto, max(h, 1))):
        out.append(dict(T=T, B=3 if i % 3 == 2 else 1, prev=form != 2 and i % 2 == 1,
                        div=float(len(chains)) if form == 2 else (3.0 if i % 4 >= 2 else 1.0),
                        seed=9000 + 131 * C + 17 * chains[0][0] + 3 * chains[0][1] + i))
    return out


def rb_id(g):
    form, C, chains = g
    return ("pair", "chain", "stage")[form] + f"_C{C}_" + "_".join(f"k{k}d{d1}x{d2}" for k, d1, d2 in chains)


def rb_weights(C, chains, seed):
    """[(w1, b1, w2, b2)] per chain, f32."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, _, _ in chains:
        s = 1.0 / math.sqrt(C * k)
        out.append((torch.randn(C, C, k, generator=g) * s, torch.randn(C, generator=g) * 0.5,
                    torch.randn(C, C, k, generator=g) * s, torch.randn(C, generator=g) * 0.5))
    return out


def rb_input(B, C, T, seed, dtype, prev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, T, generator=g).to(dtype)
    return x, (torch.randn(B, C, T, generator=g).to(dtype) if prev else None)


def rb_c1_ref(form, x, wb, k, d1):
    """float64 (y, S, K) of the first conv of a chain on x: ft = c1(lrelu(x)) (pair), t = x + c1(lrelu(x)) (ResBlock2)."""
    return conv_ref(x, wb[0], dil=d1, pad=(k - 1) // 2 * d1, slope=0.1, bias=wb[1], res=None if form == 0 else x)


def rb_c2_ref(form, x, mid, wb, k, d2, prev, div):
    """float64 (y, S, K) of the second conv on the intermediate `mid` (the DEVICE's, in the GPU tier): the residual is x
    for a pair and the intermediate itself for a ResBlock2; prev = the running sum it adds (or None)."""
    d2 = 1 if form == 0 else d2
    return conv_ref(mid, wb[2], dil=d2, pad=(k - 1) // 2 * d2, slope=0.1, bias=wb[3], res=x if form == 0 else mid,
                    prev=prev, div=div)


def rb_f32(form, x, wb, k, d1, d2, prev, div):
    """(mid, out) of one chain in torch f32, rounded where the kernels round."""
    mid = f32_model(x, wb[0], dil=d1, pad=(k - 1) // 2 * d1, slope=0.1, bias=wb[1], res=None if form == 0 else x)
    d2 = 1 if form == 0 else d2
    out = f32_model(mid, wb[2], dil=d2, pad=(k - 1) // 2 * d2, slope=0.1, bias=wb[3], res=x if form == 0 else mid,
                    prev=prev, div=div)
    return mid, out


# ---- WaveNet pieces -----------------------------------------------------------------------------------------------------
WN_H, WN_K = 192, 5  # wn16_fused(H) = H % 16 == 0 and H >= 128 distinguishes nothing else at the model's H
WN_T = (4, 124, 128, 132)


def wn_gate_ref(xin16):
    """float64 tanh(a) * sigmoid(b) of the ROUNDED conv outputs xin16 [B, 2H, T] -> [B, H, T]."""
    H = xin16.shape[1] // 2
    a, b = xin16[:, :H].double(), xin16[:, H:].double()
    return torch.tanh(a) * torch.sigmoid(b)


def wn_mask(B, T):
    """A ragged batch: utterance b keeps T - 3 b frames (at least one)."""
    m = torch.zeros(B, T)
    for b in range(B):
        m[b, :max(1, T - 3 * b)] = 1.0
    return m


def wn_update_ref(rs16, h16, skip32, mask, last, first):
    """float64 (h, skip) of modules.py:79-86 on the ROUNDED res_skip output rs16 [B, 2H or H, T]: h = (h + rs[:H]) mask
    unless last; skip (+)= rs[H:] (last: rs)."""
    H = h16.shape[1]
    if last:
        hn, sk = h16.double(), rs16.double()
    else:
        hn, sk = (h16.double() + rs16[:, :H].double()) * mask.double().unsqueeze(1), rs16[:, H:].double()
    return hn, sk if first else skip32.double() + sk


# ---- channel-last device layout -----------------------------------------------------------------------------------------
def cl(x):
    """[B, C, T] -> the kernels' channel-last [B, T, C], contiguous."""
    return x.transpose(1, 2).contiguous()


def cf(x):
    """Back: [B, T, C] -> [B, C, T]."""
    return x.transpose(1, 2)
