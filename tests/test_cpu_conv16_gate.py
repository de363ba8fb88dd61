"""CPU tier of the per-launch gate of the 16-bit conv kernels (tests/conv16_oracle.py), without a GPU.

* The reference alone stays within the gate: for EVERY case of the GPU sweep (single convs, ResBlock launches, WaveNet
  pieces, conv_post) the torch f32 computation on the same 16-bit-valued operands, rounded once, has zero violating
  elements.  That is what makes "zero" a fair assert on the device.
* Sensitivity: applied to defective restatements at the sweep's own shapes and seeds, each listed defect exceeds the
  gate by >= 10 x on at least half of the elements it touches.  A single lost (channel, tap) term is a smaller defect:
  a term is ~ 1 / sqrt(K) of an O(1) output whose storage rounding alone is 2^-9 (bf16).  At K = 1408 its median is
  0.96 x (bf16) / 1.96 x (f16) the gate, so visibility -- above the gate on at least half of the elements -- is asserted
  only where K <= 224: measured there, lowest case, 0.68 of the elements visible at a median of 2.3 x (bf16), 0.86 at
  5.5 x (f16).  Tenfold it is not: the gate does not claim to see one term of a few hundred.
* Coverage: by the restated tile arithmetic every kernel class of the sweep sees a last tile narrower than its halo, a
  last tile that ends exactly on a seam, one column past a seam, a single partial tile and >= 3 tiles; the stage kernel
  both its `edge` and its interior path.
* The end-to-end floor that rules out a local gate on the whole decoder is recomputed and printed.
* `_lib` binds the stand-alone entries and the header declares them."""
import os
import re

import pytest
import torch

from tests import conv16_oracle as co
from tests import decoder_input as di
from wetts_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wetts_hip.h")
DT = sorted(co.DTYPES)
CASES = co.conv_cases()


def _zero(name, got, y, S, K, dtype):
    return co.check(name, got, y, S, K, dtype)


# ---- the reference alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape", sorted({(c["Cin"], c["Cout"]) for c in CASES}))
def test_f32_conv_alone_is_inside_the_gate(shape, dt):
    dtype, worst, n = co.DTYPES[dt], 0.0, 0
    for c in CASES:
        if (c["Cin"], c["Cout"]) != shape:
            continue
        d = co.conv_data(c, dtype)
        y, S, K = co.case_ref(c, d)
        worst = max(worst, _zero(co.case_id(c), co.case_f32(c, d), y, S, K, dtype))
        n += y.numel()
    print(f"{shape} {dt}: 0 violations of {n} elements, worst err / gate {worst:.3f}")


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("g", co.rb_groups(), ids=co.rb_id)
def test_f32_resblock_alone_is_inside_the_gate(g, dt):
    form, C, chains = g
    dtype, worst = co.DTYPES[dt], 0.0
    for rc in co.rb_cases(form, C, chains):
        wbs = co.rb_weights(C, chains, rc["seed"])
        x, prev = co.rb_input(rc["B"], C, rc["T"], rc["seed"] + 1, dtype, rc["prev"])
        run = prev
        for j, ((k, d1, d2), wb) in enumerate(zip(chains, wbs)):
            div = rc["div"] if j == len(chains) - 1 else 1.0
            mid, out = co.rb_f32(form, x, wb, k, d1, d2, run, div)
            worst = max(worst, _zero(f"{co.rb_id(g)} T{rc['T']} c1[{j}]", mid, *co.rb_c1_ref(form, x, wb, k, d1), dtype))
            worst = max(worst, _zero(f"{co.rb_id(g)} T{rc['T']} c2[{j}]", out,
                                     *co.rb_c2_ref(form, x, mid, wb, k, d2, run, div), dtype))
            run = out
    print(f"{co.rb_id(g)} {dt}: worst err / gate {worst:.3f}")


@pytest.mark.parametrize("dt", DT)
def test_f32_wavenet_pieces_alone_are_inside_the_gate(dt):
    dtype, H, k = co.DTYPES[dt], co.WN_H, co.WN_K
    for i, T in enumerate(co.WN_T):
        B = 3
        g = torch.Generator().manual_seed(8000 + i)
        w_in, b_in = torch.randn(2 * H, H, k, generator=g) / (H * k) ** 0.5, torch.randn(2 * H, generator=g) * 0.3
        gl = torch.randn(B, 2 * H, generator=g) * 0.3
        h = torch.randn(B, H, T, generator=g).to(dtype)
        xin = co.f32_model(h, w_in, pad=k // 2, bias=b_in, bias_b=gl)
        _zero(f"in_layer T{T}", xin, *co.conv_ref(h, w_in, pad=k // 2, bias=b_in, bias_b=gl), dtype)
        a, b = xin[:, :H].float(), xin[:, H:].float()
        acts = (torch.tanh(a) * torch.sigmoid(b)).to(dtype)
        y = co.wn_gate_ref(xin)
        _zero(f"gate T{T}", acts, y, y.abs(), 0, dtype, )
        for last in (0, 1):
            RC = H if last else 2 * H
            w_rs, b_rs = torch.randn(RC, H, 1, generator=g) / H ** 0.5, torch.randn(RC, generator=g) * 0.3
            rs = co.f32_model(acts, w_rs, bias=b_rs)
            _zero(f"res_skip T{T}", rs, *co.conv_ref(acts, w_rs, bias=b_rs), dtype)
            skip, mask = torch.randn(B, H, T, generator=g), co.wn_mask(B, T)
            hn, sk = co.wn_update_ref(rs, h, skip, mask, last, 0)
            if not last:
                got_h = ((h.float() + rs[:, :H].float()) * mask.unsqueeze(1)).to(dtype)
                _zero(f"h T{T}", got_h, hn, h.double().abs() + rs[:, :H].double().abs(), 0, dtype)
            got_s = skip + (rs if last else rs[:, H:]).float()
            _zero(f"skip T{T}", got_s, sk, skip.double().abs() + (rs if last else rs[:, H:]).double().abs(), 0, None)


@pytest.mark.parametrize("dt", DT)
def test_f32_conv_post_alone_is_inside_the_gate(dt):
    dtype = co.DTYPES[dt]
    for C, mfma in ((32, True), (64, False)):
        for i, T in enumerate((1, 6, 511, 512, 513)):
            g = torch.Generator().manual_seed(8100 + i)
            w, x = torch.randn(1, C, 7, generator=g) / (C * 7) ** 0.5, torch.randn(2, C, T, generator=g).to(dtype)
            y, S, K = co.conv_ref(x, w, pad=3, slope=0.01, round_w=mfma, round_act=mfma)
            xf = x.float()
            act = co.lrelu16(x, 0.01).float() if mfma else torch.maximum(xf, xf * torch.tensor(0.01))
            got = torch.tanh(torch.nn.functional.conv1d(act, w.to(dtype).float() if mfma else w, padding=3))
            _zero(f"conv_post C{C} T{T}", got, torch.tanh(y), S, K, None)


# ---- sensitivity ----------------------------------------------------------------------------------------------------
def _touched(shape, cols):
    m = torch.zeros(shape, dtype=torch.bool)
    m[..., cols] = True
    return m


def _splice(good, alt, cols):
    out = good.clone()
    out[..., cols] = alt[..., cols]
    return out


def _defects(c, d, good, nt):
    """{name: (defective output, mask of the elements the defect touches)} for every defect the case can carry."""
    out, T, k = {}, good.shape[-1], c["k"]
    if c["up"]:
        up, w = c["up"], d["w"].clone()
        w[:, :, up - 1::up] = 0.0  # the taps of phase up - 1
        cols = [t for t in range(T) if (t + c["pad"]) % up == up - 1]
        out["transposed_last_phase"] = (_splice(good, co.case_f32(c, d, w=w), cols), _touched(good.shape, cols))
        return out
    w = d["w"].clone()
    w[:, :, (k - 1) // 2] = 0.0  # the centre tap: in range at every column
    alt = co.case_f32(c, d, w=w)
    out["tap_last_column"] = (_splice(good, alt, [T - 1]), _touched(good.shape, [T - 1]))
    if T > nt:
        out["tap_first_column_of_tile_2"] = (_splice(good, alt, [nt]), _touched(good.shape, [nt]))
        tile = list(range(nt, min(2 * nt, T)))
        if k > 1:
            x = d["x"].clone()
            x[..., nt - 1] = 0.0  # the last column of tile 1 is tile 2's first halo column
            cols = [t for t in tile if any(t - c["pad"] + j * c["dil"] == nt - 1 for j in range(k))]
            if cols:  # (a dilated conv reaches column nt - 1 only from some columns: none of them in a one-column tile)
                out["halo_column_zero_at_seam"] = (_splice(good, co.case_f32(c, d, x=x), cols),
                                                   _touched(good.shape, cols))
        if c["res"]:
            out["residual_skipped_on_a_tile"] = (_splice(good, co.case_f32(c, d, res=None), tile),
                                                 _touched(good.shape, tile))
        if c["div"] != 1.0:
            out["out_div_skipped_on_a_tile"] = (_splice(good, co.case_f32(c, d, div=1.0), tile), _touched(good.shape, tile))
    if c["bias"] and T >= 64:
        cols = list(range(32, 64))
        out["bias_lost_over_32_columns"] = (_splice(good, co.case_f32(c, d, bias=None), cols), _touched(good.shape, cols))
    if c["Cin"] * k <= 224 and T >= 64:  # (T >= 64: the term's x takes enough values for a median to mean something)
        w = d["w"].clone()
        w[:, 3, k // 2] = 0.0
        out["one_lost_term"] = (co.case_f32(c, d, w=w), torch.ones(good.shape, dtype=torch.bool))
    return out


LISTED = ("tap_last_column", "tap_first_column_of_tile_2", "halo_column_zero_at_seam", "bias_lost_over_32_columns",
          "residual_skipped_on_a_tile", "out_div_skipped_on_a_tile", "transposed_last_phase", "one_lost_term")


@pytest.mark.parametrize("dt", DT)
def test_every_defect_exceeds_the_gate_tenfold_on_half_of_what_it_touches(dt):
    """Every case of the conv sweep carries every defect it can; per defect the fraction of touched elements at >= 10 x
    the gate must be >= 1/2 in EVERY case.  one_lost_term, the smaller defect, runs only where K = Cin * k <= 224 and is
    held to visibility (>= 1 x the gate on at least half of the elements), see the module docstring."""
    dtype, seen = co.DTYPES[dt], {}
    for c in CASES:
        d = co.conv_data(c, dtype)
        y, S, K = co.case_ref(c, d)
        good = co.case_f32(c, d)
        nt = co.conv_tile(c["Cin"], c["Cout"])["NT"]
        for name, (bad, mask) in _defects(c, d, good, nt).items():
            r = co.ratio(bad, y, S, K, dtype)[mask]
            need = 1.0 if name == "one_lost_term" else 10.0
            frac, med = float((r >= need).double().mean()), float(r.median())
            e = seen.setdefault(name, [0, 1.0, float("inf")])
            e[0], e[1], e[2] = e[0] + 1, min(e[1], frac), min(e[2], med)
            assert frac >= 0.5, (name, co.case_id(c), dt, f"fraction at >= {need:g} x gate {frac:.2f}, median {med:.1f} x")
    for name in LISTED:
        assert name in seen and seen[name][0] >= 3, (name, seen.get(name))
        print(f"{dt} {name}: {seen[name][0]} cases, lowest fraction at >= {1 if name == 'one_lost_term' else 10} x "
              f"{seen[name][1]:.2f}, "
              f"lowest median {seen[name][2]:.1f} x gate")


@pytest.mark.parametrize("dt", DT)
def test_one_lost_term_is_not_always_visible_at_large_k(dt):
    """Why one_lost_term is asserted only at K <= 224: the median over the touched elements at K = 1408 (C = 128,
    k = 11), printed; the gate's accumulation term and the storage rounding of an O(1) output both exceed one term of
    size ~ 1 / sqrt(K)."""
    dtype, C, k = co.DTYPES[dt], 128, 11
    c = dict(Cin=C, Cout=C, k=k, dil=1, pad=5, up=0, B=1, T=64, slope=0.1, bias=True, bias_b=False, res=False, prev=False,
             div=1.0, basic=0, seed=7999)
    d = co.conv_data(c, dtype)
    y, S, K = co.case_ref(c, d)
    w = d["w"].clone()
    w[:, 3, k // 2] = 0.0
    r = co.ratio(co.case_f32(c, d, w=w), y, S, K, dtype)
    print(f"{dt} K = {K}: one lost term, median {float(r.median()):.2f} x gate, "
          f"{float((r >= 10).double().mean()):.2f} of the elements at >= 10 x")
    assert float((r >= 10.0).double().mean()) < 0.5


# ---- coverage -------------------------------------------------------------------------------------------------------
def test_every_conv_instantiation_sees_every_tile_event_and_switch():
    ev, sw = {}, {}
    for c in CASES:
        if c["up"] or co.conv_refused(c):
            continue
        cls = co.conv_class(c["Cin"], c["Cout"])
        nt = co.conv_tile(c["Cin"], c["Cout"])["NT"]
        assert co.out_len(c) == c["T"]
        ev.setdefault(cls, set()).update(co.tile_events(c["T"], nt, (c["k"] - 1) * c["dil"]))
        s = sw.setdefault(cls, {n: set() for n in ("slope", "bias", "bias_b", "res", "prev", "div", "basic", "B", "kd")})
        for n in ("bias", "bias_b", "res", "prev", "div", "basic", "B"):
            s[n].add(c[n])
        s["slope"].add(c["slope"] is not None)
        s["kd"].add((c["k"], c["dil"]))
    assert len(ev) == 5, sorted(ev)
    # what the launcher refuses of the sweep (its LDS budget, restated): span 120 where two 64-channel chunks are staged
    assert {co.case_id(c) for c in CASES if co.conv_refused(c)} == {"192to512_k11d12_T129_B3", "72to160_k11d12_T129_B3"}
    for cls in ev:
        assert ev[cls] == co.EVENTS, (cls, co.EVENTS - ev[cls])
        for n in ("slope", "bias", "bias_b", "res", "prev", "basic"):
            assert sw[cls][n] == {False, True} or sw[cls][n] == {0, 1}, (cls, n, sw[cls][n])
        assert {1.0, 3.0, 5.0} <= sw[cls]["div"] and 3 in sw[cls]["B"] and sw[cls]["kd"] == set(co.KDIL), (cls, sw[cls])
    ups = {(c["up"], c["k"]) for c in CASES if c["up"]}
    assert ups == set(co.transposed_shapes()) and (5, 9) in ups and (3, 5) in ups  # tiny_oddrate's included
    for u in ups:
        assert {c["T"] for c in CASES if (c["up"], c["k"]) == u} == {1, 2, 33}


def test_every_resblock_kernel_sees_every_tile_event():
    groups = co.rb_groups()
    # (v3's C = 128 stage has no fused kernel: its conv-by-conv form is still swept)
    assert {(f, C) for f, C, _ in groups} == {(f, C) for f in (0, 1, 2) for C in (32, 64, 128)}
    assert len([g for g in groups if g[0] == 0]) == 27 and len([g for g in groups if g[0] == 1]) == 9
    ev, paths = {}, {}
    for form, C, chains in groups:
        if not co.rb_fused_supported(form, C, chains):
            continue
        ntc, nto, h = co.rb_geom(form, C, chains)
        for rc in co.rb_cases(form, C, chains):
            ev.setdefault((form, C), set()).update(co.tile_events(rc["T"], nto, h))
            if form == 2:
                paths.setdefault(C, set()).update(co.stage_edge_tiles(rc["T"], ntc, nto, h))
        e = {(rc["B"], rc["prev"], rc["div"]) for rc in co.rb_cases(form, C, chains)}
        assert {b for b, _, _ in e} == {1, 3}
        assert form == 2 or ({p for _, p, _ in e} == {False, True} and {v for _, _, v in e} == {1.0, 3.0})
    assert set(ev) == {(0, 32), (0, 64), (0, 128), (1, 32), (1, 64), (1, 128), (2, 32), (2, 64)}
    for key, e in ev.items():
        assert e == co.EVENTS, (key, co.EVENTS - e)
    assert paths == {32: {False, True}, 64: {False, True}}
    # the stage with all of v3's chains has columns between a chain's own halo and the common origin
    assert any(form == 2 and len({(k - 1) // 2 * d2 for k, _, d2 in chains}) == 3 for form, _, chains in groups)


def test_tile_arithmetic_restated():
    assert [co.conv_tile(*s) for s in co.CONV_SHAPES[:5]] == [
        dict(CKB=64, NT=128, MT=128), dict(CKB=64, NT=256, MT=64), dict(CKB=32, NT=128, MT=128),
        dict(CKB=32, NT=256, MT=64), dict(CKB=32, NT=512, MT=32)]
    assert [co.pair_geom(C, 7)[:2] for C in (32, 64, 128)] == [(512, 506), (256, 250), (128, 122)]
    assert [co.chain_geom(C, 5, 6)[:2] for C in (32, 64, 128)] == [(1024, 1000), (512, 488), (256, 232)]
    v3 = ((3, 1, 2), (5, 2, 6), (7, 3, 12))
    assert co.stage_geom(32, v3) == (768, 696, 36) and co.stage_geom(64, v3) == (384, 312, 36)
    assert co.stage_geom(32, v3[:1]) == (768, 764, 2)


# ---- the end-to-end floor -------------------------------------------------------------------------------------------
def test_end_to_end_floor(monkeypatch):
    """Why the decoder is not gated locally end to end.  The bf16 numerics simulator (vits_oracle.hifigan_bf16sim: the
    same rounding points as the device) on `tiny`'s own weights with f32 accumulation, against itself with float64
    accumulation: a rounding that falls the other way is amplified through the ~20 convs of `tiny`, so even two correct
    implementations differ by a relative RMS and a largest element (printed) that are orders of magnitude above a
    dropped tap's effect on the audio.  Recorded, not gated: the only assert is that the floor is far above f32's
    2^-24, i.e. that it is indeed rounding flips and not accumulation noise."""
    vo = di.vo()
    cfg, sd, cd, W32, W64 = di.weights("tiny")
    worst = [0.0, 0.0]
    for i, (B, L) in enumerate(((1, 1), (2, 5), (1, 37))):
        z, g = di.inputs(W32, B, L, 1000 + i)
        with torch.no_grad():
            monkeypatch.setattr(vo, "_q", lambda x: x.to(torch.bfloat16).to(torch.float32))
            a = vo.hifigan_bf16sim(W32, cd, z, g)
            monkeypatch.setattr(vo, "_q", lambda x: x.to(torch.bfloat16).to(torch.float64))
            b = vo.hifigan_bf16sim(W64, cd, z.double(), g.double())
        rel, loc = di.gates(a, b)
        print(f"tiny bf16 {B} x {L}: simulator f32 vs f64 accumulation rel RMS {rel:.3g}, max|d| / rms {loc:.3g}")
        worst = [max(worst[0], rel), max(worst[1], loc)]
    print(f"tiny bf16 end-to-end floor: rel {worst[0]:.3g}, local {worst[1]:.3g}")
    assert worst[0] > 1e-5 and worst[1] > 1e-4


# ---- bindings -------------------------------------------------------------------------------------------------------
ENTRIES = ("wetts_conv16", "wetts_conv16_wn_gate", "wetts_conv16_wn_update", "wetts_wn16_gate", "wetts_wn16_update",
           "wetts_conv16_post", "wetts_resblock16")


def test_lib_binds_the_entries_and_the_header_declares_them():
    src = open(HEADER).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert nargs == len(_lib.SIGNATURES[name][1]), (name, nargs, len(_lib.SIGNATURES[name][1]))
    flags = dict(re.findall(r"#define WETTS_CONV16_([A-Z0-9]+) (\d+)", src))
    assert {k: int(v) for k, v in flags.items()} == dict(F16=_lib.CONV16_F16, TRANSPOSED=_lib.CONV16_TRANSPOSED,
                                                         LRELU=_lib.CONV16_LRELU, ACCUM=_lib.CONV16_ACCUM,
                                                         BASIC=_lib.CONV16_BASIC, TAG=_lib.CONV16_TAG)
    assert re.search(r"#define WETTS_ABI_VERSION 12\b", src) and _lib.ABI_VERSION == 12  # additive entries
