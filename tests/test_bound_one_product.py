"""The one-product bound tile (csrc/hscmp_mfma.h bound_tile, derived in csrc/hscmp_bound.h), restated in numpy.

The tile rounds every float32 sample and dictionary entry to bf16 once (bf16_rn_bits), sums the products xh * dh, and
adds kBoundEps1 * ||xh_win|| * ||d_k|| as slack.  Here the products are summed in float64 (the matrix core's own error
has its own term in the derivation and is far below the margin), and the constant read from the header is put
against the score the engine pins: the float32 fmaf chain over the taps in ascending order.  In every case
|chain_k - sum_w xh_w dh_kw| <= kBoundEps1 * ||xh_win|| * ||d_k||."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'hierarchical-sparse-coding_amd', 'csrc', 'hscmp_mfma.h')
W = 64


def _header_constant(name):
    """A `constexpr float name = <product of hex / decimal float literals and one parenthesised sum>;` of the header, in float32."""
    text = open(HEADER).read()
    expr = re.search(r'constexpr\s+float\s+%s\s*=\s*([^;]+);' % name, text).group(1)
    assert re.fullmatch(r'[0-9a-fA-FxXpP.+\-*() ]+', expr), expr

    def lit(m):
        s = m.group(0).rstrip('fF')
        return 'np.float32(%r)' % (float.fromhex(s) if s.lower().startswith('0x') else float(s))
    return np.float32(eval(re.sub(r'0[xX][0-9a-fA-F.]+[pP][+-]?\d+[fF]?|\d+\.\d*[fF]?', lit, expr), {'np': np}))


def _rn_bf16(v):
    """bf16_rn_bits on float32 values: the bf16 value as a float32."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)


def _fmaf(x, d, acc):
    """rn32(x * d + acc), x, d, acc float32: the product is exact in float64, the sum is rounded to odd there
    (TwoSum gives the part the float64 sum lost), and a float64 rounded to odd rounds to float32 as the exact sum does."""
    p = x.astype(np.float64) * d.astype(np.float64)
    a = acc.astype(np.float64)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    bits = s.view(np.int64).copy()
    fix = (err != 0.0) & ((bits & 1) == 0)
    up = (err > 0.0) == (s > 0.0)                             # the neighbour towards the lost part: larger magnitude or smaller
    bits[fix & up] += 1
    bits[fix & ~up] -= 1
    return bits.view(np.float64).astype(np.float32)


def _check(x, d):
    """x, d: [N, W] float32 (window n against atom n).  Returns max over n of |chain - sum xh dh| / (||xh|| ||d||)."""
    acc = np.zeros(x.shape[0], dtype=np.float32)
    for w in range(x.shape[1]):
        acc = _fmaf(x[:, w], d[:, w], acc)
    xh, dh = _rn_bf16(x).astype(np.float64), _rn_bf16(d).astype(np.float64)
    tile = np.sum(xh * dh, axis=1)
    scale = np.sqrt(np.sum(xh * xh, axis=1)) * np.sqrt(np.sum(d.astype(np.float64) ** 2, axis=1))
    live = scale > 0.0
    assert live.any()
    return float(np.max(np.abs(acc.astype(np.float64) - tile)[live] / scale[live]))


def _under_midpoint(rs, shape, literal):
    """Magnitudes just under a bf16 rounding midpoint, times a power of two.  literal: m (1 + 2^-8 - 2^-22) for a random 8-bit
    significand m in 128..255 (under the midpoint for m = 128, past it for larger m); else (m + 1/2)(1 - 2^-22) for every m."""
    m = rs.randint(128, 256, size=shape).astype(np.float64)
    v = m * (1.0 + 2.0 ** -8 - 2.0 ** -22) if literal else (m + 0.5) * (1.0 - 2.0 ** -22)
    return (v * np.exp2(rs.randint(-12, -4, size=shape))).astype(np.float32)


def test_header_constant_is_the_derived_one():
    eps1 = _header_constant('kBoundEps1')
    assert eps1 == np.float32(2.0 ** -7 * (1.0 + 2.0 ** -6))
    u, u1, u2 = 2.0 ** -8, 2.0 ** -23, 2.0 ** -24
    gamma = lambda n, e: n * e / (1.0 - n * e)
    eps_1 = u * (2.0 + u) + gamma(64, u1) * (1.0 + u) ** 2 + gamma(64, u2)
    need = (1.0 + u2) * eps_1 / (1.0 - u)
    assert abs(eps_1 - 7.83926e-3) < 1e-8 and abs(need - 7.87001e-3) < 1e-8
    assert 1.008 < float(eps1) / need < 1.009                  # the stated margin of 0.82 %


def test_random_windows():
    eps1 = float(_header_constant('kBoundEps1'))
    rs = np.random.RandomState(1)
    x = rs.standard_normal((100000, W)).astype(np.float32)
    d = rs.standard_normal((100000, W)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    worst = _check(x, d)
    print('random: worst |chain - tile| / (||xh|| ||d||) = %.4g of %.4g' % (worst, eps1))
    assert worst <= eps1


def test_exponent_spreads():
    eps1 = float(_header_constant('kBoundEps1'))
    rs = np.random.RandomState(2)
    for spread in (4, 20, 40):
        x = (rs.standard_normal((20000, W)) * np.exp2(rs.randint(-spread // 2, spread // 2 + 1, size=(20000, W)))).astype(np.float32)
        d = (rs.standard_normal((20000, W)) * np.exp2(rs.randint(-spread // 4, spread // 4 + 1, size=(20000, W)))).astype(np.float32)
        worst = _check(x, d)
        print('spread 2^%d: worst %.4g of %.4g' % (spread, worst, eps1))
        assert worst <= eps1


def test_adversarial_family():
    """Every entry just under a rounding midpoint and every product positive: all the dropped terms line up."""
    eps1 = float(_header_constant('kBoundEps1'))
    rs = np.random.RandomState(3)
    for literal in (True, False):
        d = _under_midpoint(rs, (20000, W), literal) * rs.choice(np.float32([-1.0, 1.0]), size=(20000, W))
        x = _under_midpoint(rs, (20000, W), literal) * np.sign(d)
        worst = _check(x, d)
        print('adversarial (%s): worst %.4g of %.4g' % ('m (1 + 2^-8 - 2^-22)' if literal else '(m + 1/2)(1 - 2^-22)', worst, eps1))
        assert worst <= eps1


def test_a_halved_constant_is_caught():
    """The check is not vacuous: with every significand 128 just under its midpoint (the largest relative rounding error) and the
    window a multiple of the atom (Cauchy-Schwarz tight), the error is 0.98 of the constant, and half the constant fails."""
    eps1 = float(_header_constant('kBoundEps1'))
    rs = np.random.RandomState(4)
    d = (np.float32(128.5 * (1.0 - 2.0 ** -22) / 256.0) * rs.choice(np.float32([-1.0, 1.0]), size=(100, W))).astype(np.float32)
    worst = _check(np.float32(4.0) * d, d)
    print('tight case: worst %.4g of %.4g' % (worst, eps1))
    assert 0.95 * eps1 < worst <= eps1
