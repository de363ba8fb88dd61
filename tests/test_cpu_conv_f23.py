"""The F(2,3) minimal-filtering form of the f32 MRF convs (wetts_amd/csrc/conv_mfma.hip: conv_f23_body), restated in
numpy: the algebra in float64 against the direct conv, and the kernel's f32 accumulation chains against the direct
kernel's.  No GPU.

    python tests/test_cpu_conv_f23.py     prints the numerics table kept as profiles/conv_f23_numerics.txt
"""
import numpy as np
import pytest


def lrelu(x):
    return np.where(x > 0, x, 0.1 * x)


def direct64(a, w, d, bias=None, res=None):
    """y[o, t] = bias[o] + res[o, t] + sum_{c, i} w[o, c, i] a[c, t + (i - (k-1)/2) d], a zero outside [0, T); float64."""
    C, T = a.shape
    O, _, k = w.shape
    p = (k - 1) // 2 * d
    ap = np.zeros((C, T + 2 * p))
    ap[:, p:p + T] = a
    y = np.zeros((O, T))
    for i in range(k):
        y += w[:, :, i].astype(np.float64) @ ap[:, i * d:i * d + T]
    if bias is not None:
        y += bias[:, None]
    if res is not None:
        y += res
    return y


def pair_bases(T, d):
    """bases of the pairs (t, t + d), by absolute time: (t mod 2d) < d; one pair index P <-> t = P + d (P // d)"""
    n = (T // (2 * d)) * d + min(T % (2 * d), d)
    P = np.arange(n)
    t = P + d * (P // d)
    assert np.array_equal(t, np.array([u for u in range(T) if u % (2 * d) < d], dtype=t.dtype))
    return t


def transformed_weights(w):
    """per group g: G0 = w0, G1 = (w0 + w1 + w2) / 2, G2 = (w0 - w1 + w2) / 2, G3 = w2: float64 from the f32 weights"""
    w = w.astype(np.float64)
    k = w.shape[2]
    G = []
    for g in range(k // 3):
        w0, w1, w2 = w[:, :, 3 * g], w[:, :, 3 * g + 1], w[:, :, 3 * g + 2]
        G.append((w0, (w0 + w1 + w2) / 2, (w0 - w1 + w2) / 2, w2))
    return G


def f23_conv(a, w, d, bias=None, res=None, dt=np.float64, chains=False):
    """The kernel's form.  dt = float64: the algebra alone.  dt = float32 with chains=True: every m_q one sequential fma
    chain in the kernel's order (16-channel chunk -> channel pair -> group -> leftover taps -> the pair's two
    channels), each fma rounded once; transformed weights and input differences rounded once to f32."""
    C, T = a.shape
    O, _, k = w.shape
    ng, p = k // 3, (k - 1) // 2 * d
    tb = pair_bases(T, d)
    ap = np.zeros((C, T + 2 * p + 2 * d), dt)  # room for the partner's taps behind the end
    ap[:, p:p + T] = a
    col = lambda j: ap[:, tb + j * d]  # a[t + off_0 + j d] for every pair
    init = np.zeros((O, T + d))
    if bias is not None:
        init[:, :T] += bias[:, None]
    if res is not None:
        init[:, :T] += res
    m = [init[:, tb].astype(dt), np.zeros((O, len(tb)), dt), np.zeros((O, len(tb)), dt), (-init[:, tb + d]).astype(dt)]
    # the slots of one k-step, in issue order: (accumulator, weight [O, C], B operand [C, pairs])
    slots = []
    for g, Gs in enumerate(transformed_weights(w)):
        a0, a1, a2, a3 = (col(3 * g + j) for j in range(4))
        V = (a0 - a2, a1 + a2, a2 - a1, a1 - a3)
        for q in range(4):
            slots.append((q, Gs[q].astype(dt), V[q].astype(dt)))
    for i in range(3 * ng, k):  # leftover taps: w_i a[t + off_i] into m0, (-w_i) a[t + d + off_i] into m3
        wi = w[:, :, i].astype(dt)
        slots.append((0, wi, col(i)))
        slots.append((3, -wi, col(i + 1)))
    if not chains:
        for q, Wm, X in slots:
            m[q] += Wm @ X
    else:
        for c0 in range(0, C, 16):
            for ks in range(8):
                for q, Wm, X in slots:
                    for c in (c0 + 2 * ks, c0 + 2 * ks + 1):
                        if c < C:  # one fma: exact product and sum in float64 (24-bit operands), one rounding
                            m[q] = (m[q].astype(np.float64) + Wm[:, c:c + 1].astype(np.float64) * X[c:c + 1].astype(np.float64)).astype(dt)
    y = np.zeros((O, T + d), dt)
    y[:, tb] = (m[0] + m[1]) + m[2]
    y[:, tb + d] = (m[1] - m[2]) - m[3]
    return y[:, :T]  # a partner at or behind T is computed and not stored


def direct_chains(a, w, d):
    """the direct kernel's f32 chain: 16-channel chunk -> tap -> channel, one rounding per fma"""
    C, T = a.shape
    O, _, k = w.shape
    p = (k - 1) // 2 * d
    ap = np.zeros((C, T + 2 * p), np.float32)
    ap[:, p:p + T] = a
    y = np.zeros((O, T), np.float32)
    for c0 in range(0, C, 16):
        for i in range(k):
            for c in range(c0, min(c0 + 16, C)):
                y = (y.astype(np.float64) + w[:, c:c + 1, i].astype(np.float64) * ap[c:c + 1, i * d:i * d + T].astype(np.float64)).astype(np.float32)
    return y


@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_f23_algebra_equals_direct_conv(k, d):
    rng = np.random.default_rng(100 * k + d)
    for T in (1, 2, 2 * d - 1, 2 * d, 2 * d + 1, 4 * d + 3):
        C, O = 6, 5
        a = lrelu(rng.standard_normal((C, T)))
        w = rng.standard_normal((O, C, k)).astype(np.float32)
        bias, res = rng.standard_normal(O), rng.standard_normal((O, T))
        ref = direct64(a, w, d, bias, res)
        got = f23_conv(a, w, d, bias, res)
        assert got.shape == ref.shape
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
        assert err <= 1e-12, (k, d, T, err)
        # no residual / bias: m0 and m3 start at zero
        err0 = np.abs(f23_conv(a, w, d) - direct64(a, w, d)).max() / max(np.abs(direct64(a, w, d)).max(), 1e-300)
        assert err0 <= 1e-12, (k, d, T, err0)


def test_pairs_cover_every_output_once():
    for d in (1, 3, 5):
        for T in range(1, 4 * d + 4):
            tb = pair_bases(T, d)
            both = np.concatenate([tb, tb + d])
            assert len(set(both.tolist())) == len(both)
            assert set(range(T)) <= set(both.tolist())
            assert both.max() < T + d


def chain_case(C, k, d, O=32, T=240, seed=1):
    rng = np.random.default_rng(seed + 1000 * C + 10 * k + d)
    a = lrelu(rng.standard_normal((C, T))).astype(np.float32)
    w = (rng.standard_normal((O, C, k)) * 0.01).astype(np.float32)
    ref = direct64(a.astype(np.float64), w, d)
    r = np.sqrt((ref ** 2).mean())
    ed = direct_chains(a, w, d).astype(np.float64) - ref
    ef = f23_conv(a, w, d, dt=np.float32, chains=True).astype(np.float64) - ref
    return (np.sqrt((ed ** 2).mean()) / r, np.abs(ed).max() / r, np.sqrt((ef ** 2).mean()) / r, np.abs(ef).max() / r)


CHAIN_CASES = [(C, k, d) for C in (256, 128) for k in (3, 7, 11) for d in (1, 5)]


@pytest.mark.parametrize("C,k,d", CHAIN_CASES)
def test_f23_f32_chains_no_worse_than_direct(C, k, d):
    rd, _, rf, _ = chain_case(C, k, d)
    print(f"C={C} k={k} d={d}: rel RMS direct {rd:.3e}  F(2,3) {rf:.3e}  ratio {rf / rd:.2f}")
    assert rf <= rd


if __name__ == "__main__":
    print("f32 accumulation chains in kernel order, O = 32, T = 240, lrelu'd N(0,1) inputs, weights N(0, 0.01^2); reference float64")
    print("direct: 16-channel chunk -> tap -> channel.  F(2,3): chunk -> channel pair -> group -> leftover taps -> channel")
    print(f"{'C':>4} {'k':>3} {'d':>2}  {'direct rel RMS':>15} {'direct max/rms':>15}  {'F23 rel RMS':>12} {'F23 max/rms':>12}  {'RMS ratio':>9} {'max ratio':>9}")
    for C, k, d in CHAIN_CASES:
        rd, md, rf, mf = chain_case(C, k, d)
        print(f"{C:4d} {k:3d} {d:2d}  {rd:15.3e} {md:15.3e}  {rf:12.3e} {mf:12.3e}  {rf / rd:9.2f} {mf / md:9.2f}", flush=True)
