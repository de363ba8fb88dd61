"""The F(2,3) ResBlock pair kernel (wetts_amd/csrc/resblock_chain_f23.hip) restated in numpy.  No GPU.

* chain_f23_geometry() of the launcher, restated: coverage without holes, every stored column of every tile depends on
  valid inputs only (found by brute force over the tile's columns, not by the formula), tiles abut, every column a conv
  reads or writes fits the staged width.
* The pair tile by tile in float64, pairs taken by TILE COLUMN (base q + d (q / d), partner + d; c2: 2q, 2q + 1), equals
  direct64 of c1 -> lrelu -> c2 + residual, the sequence ends and a length that is no multiple of NTO included.
* The f32 accumulation chains of the kernel's order against resblock_chain32_kernel's (C = 32).

    python -m tests.test_cpu_chain_pair_f23     prints the numerics table kept as profiles/chain_pair_f23_numerics.txt
"""
import numpy as np
import pytest

from tests.test_cpu_conv_f23 import direct64, lrelu, transformed_weights

STRIDE = {32: 320}  # chain_f23_stride(C): LDS row stride of the built kernels (NP = 128)


def geometry(NP, k, dils):
    """chain_f23_geometry: dict(S_left, S_right, NTO, Mmin, Wst) of a tile of NP pairs"""
    hk, big = (k - 1) // 2, 1 << 20
    vlo, vhi, m, r = -big, big, 0, 0
    for d in dils:
        h1 = hk * d
        cov = 2 * d * (NP // d) + NP % d
        last = (NP - 1) + d * ((NP - 1) // d) + d
        vlo, vhi = max(vlo + h1, 0), min(vhi - h1, cov)
        m, r = max(m, h1), max(r, last + h1)
        vlo, vhi = vlo + hk, min(vhi - hk, 2 * NP)
        m, r = max(m, hk), max(r, 2 * NP - 1 + hk)
    S_left = (vlo + 1) & ~1
    NTO = (vhi - S_left) & ~1
    return dict(S_left=S_left, NTO=NTO, S_right=2 * NP - S_left - NTO, Mmin=m, Wst=(m + 3 + r + 1 + 3) & ~3)


def pair_columns(NP, d):
    """(bases, partners) of the NP pairs of a conv at dilation d, by tile column"""
    q = np.arange(NP)
    base = q + d * (q // d)
    return base, base + d


def dil_sets(d, npairs):
    return [(d,)] if npairs == 1 else [(d, d, d), (1, 3, 5), (5, 3, 1)]


GEOM_CASES = [(k, d, NP, n) for k in (3, 7, 11) for d in (1, 3, 5) for NP in (32, 64, 128) for n in (1, 3)]


@pytest.mark.parametrize("k,d,NP,npairs", GEOM_CASES)
def test_geometry_coverage_validity_and_fit(k, d, NP, npairs):
    hk = (k - 1) // 2
    # coverage: the columns [0, cov) are each produced exactly once, partners behind cov lie behind a hole
    base, part = pair_columns(NP, d)
    cols = np.concatenate([base, part])
    assert len(set(cols.tolist())) == 2 * NP
    cov = 2 * d * (NP // d) + NP % d
    assert set(range(cov)) <= set(cols.tolist())
    if cov < 2 * NP:
        assert cov not in set(cols.tolist())
    assert 2 * NP - cov <= 6
    for dils in dil_sets(d, npairs):
        g = geometry(NP, k, dils)
        if g["NTO"] <= 0:
            continue  # the launcher refuses the shape (small tiles under a three-pair halo)
        assert g["S_left"] % 2 == 0 and g["NTO"] % 2 == 0 and g["S_right"] >= 0
        # brute force: which tile columns hold exact values after each conv.  Staged x is exact on the whole window.
        lo, hi = -(g["Mmin"]), g["Wst"] - (g["Mmin"] + 3)  # columns staged whatever the margin (M in Mmin .. Mmin + 3)
        valid = set(range(lo, hi))
        for dd in dils:
            for (dc, cs) in ((dd, np.concatenate(pair_columns(NP, dd))), (1, np.arange(2 * NP))):
                reads = [(i - hk) * dc for i in range(k)]
                # every column read or written lies inside the staged width, for every left margin
                assert cs.min() + min(reads) >= lo and cs.max() + max(reads) < hi, (dils, dc)
                valid = {int(c) for c in cs if all(c + o in valid for o in reads)}
        stored = set(range(g["S_left"], g["S_left"] + g["NTO"]))
        assert stored <= valid, (k, dils, NP, sorted(stored - valid)[:8])
        # and the run of valid columns around them is at most two columns longer (the rounding to even)
        lo_run, hi_run = g["S_left"], g["S_left"] + g["NTO"]
        while lo_run - 1 in valid:
            lo_run -= 1
        while hi_run in valid:
            hi_run += 1
        assert g["S_left"] - lo_run <= 1 and hi_run - (g["S_left"] + g["NTO"]) <= 1, (k, dils, NP, lo_run, hi_run)
        # tiles abut: tile n stores the times [n NTO, (n + 1) NTO)
        for n in range(3):
            t0 = n * g["NTO"] - g["S_left"]
            assert t0 % 2 == 0 and t0 + g["S_left"] == n * g["NTO"]
            M = g["Mmin"] + ((t0 - g["Mmin"]) & 3)
            assert (t0 - M) % 4 == 0 and g["Mmin"] <= M <= g["Mmin"] + 3
    if npairs == 1 and k in (7, 11) and NP == 128:
        assert geometry(NP, k, (d,))["Wst"] <= STRIDE[32]


def f23_columns(tile, w, d, base, off0, init0, init3, dt=np.float64, chains=False):
    """One conv of the kernel on a tile: tile[c, L] is LDS column L; pair p reads a_j = tile[:, base[p] + off0 + j d],
    j = 0 .. k.  Returns (y at the bases, y at the partners).  chains: every m_q one sequential f32 fma chain in the
    kernel's order: 16-channel chunk -> channel pair -> groups -> leftover taps -> the pair's two channels."""
    O, C, k = w.shape
    ng = k // 3
    col = lambda j: tile[:, base + off0 + j * d].astype(dt)
    m = [init0.astype(dt), np.zeros(init0.shape, dt), np.zeros(init0.shape, dt), (-init3).astype(dt)]
    slots = []
    for g, Gs in enumerate(transformed_weights(w)):
        a0, a1, a2, a3 = (col(3 * g + j) for j in range(4))
        V = (a0 - a2, a1 + a2, a2 - a1, a1 - a3)
        for q in range(4):
            slots.append((q, Gs[q].astype(dt), V[q].astype(dt)))
    i = 3 * ng
    if k % 3 == 1:  # one leftover tap on m0 and m3
        wi = w[:, :, i].astype(dt)
        slots += [(0, wi, col(i)), (3, -wi, col(i + 1))]
    elif k % 3 == 2:  # the F(2,2) tail on m0, m1, m3
        a0, a1, a2 = col(i), col(i + 1), col(i + 2)
        w0, w1 = w[:, :, i].astype(np.float64), w[:, :, i + 1].astype(np.float64)
        slots += [(0, w0.astype(dt), (a0 - a1).astype(dt)), (1, (w0 + w1).astype(dt), a1), (3, w1.astype(dt), (a1 - a2).astype(dt))]
    if not chains:
        for q, Wm, X in slots:
            m[q] = m[q] + Wm @ X
    else:
        for c0 in range(0, C, 16):
            for ks in range(8):
                for q, Wm, X in slots:
                    for c in (c0 + 2 * ks, c0 + 2 * ks + 1):
                        m[q] = (m[q].astype(np.float64) + Wm[:, c:c + 1].astype(np.float64) * X[c:c + 1].astype(np.float64)).astype(dt)
    return ((m[0] + m[1]).astype(dt) + m[2]).astype(dt), ((m[1] - m[2]).astype(dt) - m[3]).astype(dt)


def pair_by_tiles(x, w1, b1, w2, b2, d, NP, dt=np.float64, chains=False, prev=None):
    """out = x + c2(lrelu(c1(lrelu(x)))) [+ prev] as the kernel computes it: tile by tile, pairs by tile column, zeros
    outside [0, T) at both stages, the residual (and the running sum) in c2's accumulator init."""
    C, T = x.shape
    k = w1.shape[2]
    hk = (k - 1) // 2
    g = geometry(NP, k, (d,))
    out = np.full((C, T), np.nan, dt)
    b1c, b2c = b1.astype(dt)[:, None], b2.astype(dt)[:, None]
    for n in range(-(-T // g["NTO"])):
        t0 = n * g["NTO"] - g["S_left"]
        M = g["Mmin"] + ((t0 - g["Mmin"]) & 3)
        tx0 = t0 - M
        tt = tx0 + np.arange(g["Wst"])
        inside = (tt >= 0) & (tt < T)
        tile = np.zeros((C, g["Wst"]), dt)
        tile[:, inside] = lrelu(x[:, tt[inside]]).astype(dt)
        base1, part1 = pair_columns(NP, d)
        ones = np.ones((C, NP), dt)
        y0, y1 = f23_columns(tile, w1, d, M + base1, -hk * d, b1c * ones, b1c * ones, dt, chains)
        tile[:, M + base1] = np.where(inside[M + base1], lrelu(y0), 0).astype(dt)  # holes keep lrelu(x): never read by a stored column
        tile[:, M + part1] = np.where(inside[M + part1], lrelu(y1), 0).astype(dt)
        c2 = 2 * np.arange(NP)
        ok = (c2 >= g["S_left"]) & (c2 < g["S_left"] + g["NTO"]) & (t0 + c2 < T)
        r0, r1 = np.zeros((C, NP), dt), np.zeros((C, NP), dt)
        r0[:, ok], r1[:, ok] = x[:, t0 + c2[ok]], x[:, t0 + c2[ok] + 1]
        if prev is not None:
            r0[:, ok] = (r0[:, ok] + prev[:, t0 + c2[ok]]).astype(dt)
            r1[:, ok] = (r1[:, ok] + prev[:, t0 + c2[ok] + 1]).astype(dt)
        z0, z1 = f23_columns(tile, w2, 1, M + c2, -hk, (r0 + b2c).astype(dt), (r1 + b2c).astype(dt), dt, chains)
        assert np.isnan(out[:, t0 + c2[ok]]).all()  # tiles abut: nothing is stored twice
        out[:, t0 + c2[ok]], out[:, t0 + c2[ok] + 1] = z0[:, ok], z1[:, ok]
    assert not np.isnan(out).any()  # ... and nothing is left out
    return out


def pair_direct64(x, w1, b1, w2, b2, d, prev=None):
    ft = lrelu(direct64(lrelu(x), w1, d, b1))
    y = direct64(ft, w2, 1, b2, x)
    return y if prev is None else y + prev


@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_pair_by_tile_columns_equals_direct_pair(k, d):
    """float64, small tiles (NP = 32: NTO of 40 - 60 columns): the sequence ends, one tile reaching past the end, the
    first seam, several tiles, lengths that are no multiple of NTO.  T is even, as every stage length of a decoder is."""
    rng = np.random.default_rng(10 * k + d)
    NP, C = 32, 4
    nto = geometry(NP, k, (d,))["NTO"]
    assert nto > 0
    for T in (2, 8, nto - 2, nto, nto + 2, 2 * nto + 18, 5 * nto - 4):
        x = rng.standard_normal((C, T))
        w1, w2 = (rng.standard_normal((C, C, k)).astype(np.float32) * 0.3 for _ in range(2))
        b1, b2 = rng.standard_normal(C), rng.standard_normal(C)
        prev = rng.standard_normal((C, T))
        for pv in (None, prev):
            ref = pair_direct64(x, w1, b1, w2, b2, d, pv)
            got = pair_by_tiles(x, w1, b1, w2, b2, d, NP, prev=pv)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            assert err <= 1e-12, (k, d, T, pv is not None, err)


def pair_direct_chains(x, w1, b1, w2, b2, d):
    """resblock_chain32_kernel's f32 order: per conv 16-channel chunk -> tap -> channel, one rounding per fma; c1 from
    zero, bias behind the sum; c2 accumulates into the residual, bias behind the sum."""
    f32, f64 = np.float32, np.float64

    def chain(a, w, dd, acc):
        C, T = a.shape
        k = w.shape[2]
        p = (k - 1) // 2 * dd
        ap = np.zeros((C, T + 2 * p), f32)
        ap[:, p:p + T] = a
        for c0 in range(0, C, 16):
            for i in range(k):
                for c in range(c0, c0 + 16):
                    acc = (acc.astype(f64) + w[:, c:c + 1, i].astype(f64) * ap[c:c + 1, i * dd:i * dd + T].astype(f64)).astype(f32)
        return acc
    ft = lrelu(chain(lrelu(x).astype(f32), w1, d, np.zeros(x.shape, f32)) + b1.astype(f32)[:, None]).astype(f32)
    return (chain(ft, w2, 1, x.astype(f32)) + b2.astype(f32)[:, None]).astype(f32)


def numerics_case(k, d, T=300, seed=1):
    """(rel RMS, max / rms) of the direct chain order and of the new order against float64, C = 32, one pair"""
    C = 32
    rng = np.random.default_rng(seed + 10 * k + d)
    x = rng.standard_normal((C, T)).astype(np.float32)
    w1, w2 = ((rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float32) for _ in range(2))
    b1, b2 = (0.1 * rng.standard_normal(C)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    ref = pair_direct64(x.astype(np.float64), w1, b1.astype(np.float64), w2, b2.astype(np.float64), d)
    r = np.sqrt((ref ** 2).mean())
    ed = pair_direct_chains(x, w1, b1, w2, b2, d).astype(np.float64) - ref
    ef = pair_by_tiles(x, w1, b1, w2, b2, d, 128, dt=np.float32, chains=True).astype(np.float64) - ref
    return np.sqrt((ed ** 2).mean()) / r, np.abs(ed).max() / r, np.sqrt((ef ** 2).mean()) / r, np.abs(ef).max() / r


NUMERICS_CASES = [(k, d) for k in (7, 11) for d in (1, 3, 5)]
# The table (profiles/chain_pair_f23_numerics.txt): the new order is closer to float64 than the direct chain kernel's in
# every case -- worst rel-RMS ratio 0.68, worst ratio of the maxima 0.74.  Here both are held to 1.0; the device test
# (tests/test_gpu_chain_pair_f23.py) asserts rel RMS <= the direct kernel's and, for the maximum over a sweep of a few
# thousand samples, 1.5 x (what test_gpu_conv_f23.py took for an emulated 0.77).
RMS_RATIO_BOUND, MAX_RATIO_BOUND = 1.0, 1.0


@pytest.mark.parametrize("k,d", NUMERICS_CASES)
def test_pair_f32_chains_against_the_direct_chain_kernel(k, d):
    rd, md, rf, mf = numerics_case(k, d)
    print(f"C=32 k={k} d={d}: rel RMS direct {rd:.3e} F(2,3) {rf:.3e} ratio {rf / rd:.2f}; max/rms direct {md:.3e} F(2,3) {mf:.3e} ratio {mf / md:.2f}")
    assert rf <= RMS_RATIO_BOUND * rd and mf <= MAX_RATIO_BOUND * md


if __name__ == "__main__":
    print("one ResBlock1 pair x + c2(lrelu(c1(lrelu(x)))) at C = 32, T = 300, N(0,1) inputs, weights N(0, 1 / (C k)), f32 accumulation")
    print("chains in kernel order against float64.  direct (resblock_chain32_kernel): chunk -> tap -> channel, residual in c2's")
    print("accumulator, bias behind the sum.  F(2,3) (resblock_chain_f23_kernel, tiles of 128 pairs): chunk -> channel pair -> groups ->")
    print("leftover taps -> channel, bias and residual in the accumulator init, pairs by tile column")
    print(f"{'k':>3} {'d':>2}  {'direct rel RMS':>15} {'direct max/rms':>15}  {'F23 rel RMS':>12} {'F23 max/rms':>12}  {'RMS ratio':>9} {'max ratio':>9}")
    for k, d in NUMERICS_CASES:
        rd, md, rf, mf = numerics_case(k, d)
        print(f"{k:3d} {d:2d}  {rd:15.3e} {md:15.3e}  {rf:12.3e} {mf:12.3e}  {rf / rd:9.2f} {mf / md:9.2f}", flush=True)
