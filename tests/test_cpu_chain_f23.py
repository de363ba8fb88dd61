"""The F(2,2) tail of the k = 11 F(2,3) convs (wetts_amd/csrc/conv_mfma.hip: conv_f23_body, NL == 2), restated in
numpy: taps 9 and 10 as a 2-tap minimal-filtering group on the accumulators of the three 3-tap groups.  The algebra in
float64 against the direct conv, and the kernel's f32 accumulation chains against the direct kernel's.  No GPU.

    python -m tests.test_cpu_chain_f23     prints the numerics table kept as profiles/chain_f23_numerics.txt
"""
import numpy as np
import pytest

from tests.test_cpu_conv_f23 import direct64, direct_chains, lrelu, pair_bases, transformed_weights


def f23_tail_conv(a, w, d, bias=None, res=None, dt=np.float64, chains=False):
    """The kernel's form for k mod 3 == 2.  dt = float64: the algebra alone.  dt = float32 with chains=True: every m_q
    one sequential fma chain in the kernel's order (16-channel chunk -> channel pair -> groups -> tail -> the pair's two
    channels), each fma rounded once; transformed weights and input differences rounded once to f32."""
    C, T = a.shape
    O, _, k = w.shape
    assert k % 3 == 2
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
    # the tail: m0 += w9 (a9 - a10), m1 += (w9 + w10) a10, m3 += w10 (a10 - a11); the sum in float64, rounded once
    i = 3 * ng
    a0, a1, a2 = col(i), col(i + 1), col(i + 2)
    w0, w1 = w[:, :, i].astype(np.float64), w[:, :, i + 1].astype(np.float64)
    slots.append((0, w0.astype(dt), (a0 - a1).astype(dt)))
    slots.append((1, (w0 + w1).astype(dt), a1))
    slots.append((3, w1.astype(dt), (a1 - a2).astype(dt)))
    assert len(slots) == 4 * ng + 3
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


@pytest.mark.parametrize("d", [1, 3, 5])
def test_f22_tail_algebra_equals_direct_conv(d):
    k = 11
    rng = np.random.default_rng(100 * k + d)
    for T in (1, 2, 2 * d - 1, 2 * d, 2 * d + 1, 4 * d + 3):
        C, O = 6, 5
        a = lrelu(rng.standard_normal((C, T)))
        w = rng.standard_normal((O, C, k)).astype(np.float32)
        bias, res = rng.standard_normal(O), rng.standard_normal((O, T))
        for bb, rr in ((bias, res), (None, None), (bias, None), (None, res)):
            ref = direct64(a, w, d, bb, rr)
            got = f23_tail_conv(a, w, d, bb, rr)
            assert got.shape == ref.shape
            err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
            assert err <= 1e-12, (d, T, bb is not None, rr is not None, err)


def test_f22_tail_alone_is_the_two_tap_conv():
    """the tail's three products by themselves: (m0 + m1, m1 - m3) = the 2-tap conv at t and t + d, for any weights"""
    rng = np.random.default_rng(7)
    w9, w10 = rng.standard_normal(2)
    a9, a10, a11 = rng.standard_normal((3, 50))
    m0, m1, m3 = w9 * (a9 - a10), (w9 + w10) * a10, w10 * (a10 - a11)
    assert np.abs((m0 + m1) - (w9 * a9 + w10 * a10)).max() <= 1e-14
    assert np.abs((m1 - m3) - (w9 * a10 + w10 * a11)).max() <= 1e-14


def chain_case(C, d, k=11, O=32, T=240, seed=1):
    rng = np.random.default_rng(seed + 1000 * C + 10 * k + d)
    a = lrelu(rng.standard_normal((C, T))).astype(np.float32)
    w = (rng.standard_normal((O, C, k)) * 0.01).astype(np.float32)
    ref = direct64(a.astype(np.float64), w, d)
    r = np.sqrt((ref ** 2).mean())
    ed = direct_chains(a, w, d).astype(np.float64) - ref
    ef = f23_tail_conv(a, w, d, dt=np.float32, chains=True).astype(np.float64) - ref
    return (np.sqrt((ed ** 2).mean()) / r, np.abs(ed).max() / r, np.sqrt((ef ** 2).mean()) / r, np.abs(ef).max() / r)


CHAIN_CASES = [(C, d) for C in (256, 128, 32) for d in (1, 5)]


@pytest.mark.parametrize("C,d", CHAIN_CASES)
def test_f22_tail_f32_chains_no_worse_than_direct(C, d):
    rd, _, rf, _ = chain_case(C, d)
    print(f"C={C} k=11 d={d}: rel RMS direct {rd:.3e}  F(2,3) + F(2,2) tail {rf:.3e}  ratio {rf / rd:.2f}")
    assert rf <= rd


if __name__ == "__main__":
    print("f32 accumulation chains in kernel order, k = 11, O = 32, T = 240, lrelu'd N(0,1) inputs, weights N(0, 0.01^2); reference float64")
    print("direct: 16-channel chunk -> tap -> channel.  F(2,3) + F(2,2) tail: chunk -> channel pair -> groups -> tail -> channel")
    print(f"{'C':>4} {'k':>3} {'d':>2}  {'direct rel RMS':>15} {'direct max/rms':>15}  {'F23 rel RMS':>12} {'F23 max/rms':>12}  {'RMS ratio':>9} {'max ratio':>9}")
    for C, d in CHAIN_CASES:
        rd, md, rf, mf = chain_case(C, d)
        print(f"{C:4d} {11:3d} {d:2d}  {rd:15.3e} {md:15.3e}  {rf:12.3e} {mf:12.3e}  {rf / rd:9.2f} {mf / md:9.2f}", flush=True)
