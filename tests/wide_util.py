"""What the wide-loop test files share (tests/test_gpu_wide*.py): an encode under forced loops, the bit-for-bit comparisons between
loops and against the CPU oracle, and the two inputs most cases start from."""
import numpy as np
import pytest


def _encode(xs, D, wide, rp, monkeypatch, **kw):
    from hsc_amd.modeling import ConvolutionalMatchingPursuit
    for name, value in (('HSCMP_WIDE', wide), ('HSCMP_RP', rp)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return ConvolutionalMatchingPursuit().computeCoefficientsBatch(xs, D, **kw)


def _same(a, b, B):
    for i in range(B):
        for u, v in zip(a.events[i], b.events[i]):
            assert np.array_equal(u, v), i
        assert np.array_equal(a.residuals[i], b.residuals[i]), i
    assert np.array_equal(a.stats, b.stats)
    assert np.array_equal(a.energies, b.energies)


def _against_oracle(res, i, x, D, **kw):
    from oracle import hsc_oracle as orc
    coef, r, info = orc.cmp_encode(x, D, **kw)
    t, k, c = res.events[i]
    assert np.array_equal(t, info['t']) and np.array_equal(k, info['k']) and np.array_equal(c, info['c']), i
    assert np.array_equal(np.squeeze(res.residuals[i]), r), i
    assert res.stop_reasons()[i] == info['stop']
    return info


def _all_loops(xs, D, monkeypatch, rp_applies=True, oracle=(0,), **kw):
    """wide against the sequential loop and (where it runs) the round-parallel one; the signals of `oracle` against the CPU."""
    B = xs.shape[0]
    wide = _encode(xs, D, '1', None, monkeypatch, **kw)
    assert wide.variant.endswith('_wide'), wide.variant
    seq = _encode(xs, D, '0', '0', monkeypatch, **kw)
    assert seq.variant == 'mfma_init+mfma_loop_f32', seq.variant
    _same(wide, seq, B)
    rp = _encode(xs, D, '0', '1', monkeypatch, **kw)
    assert rp.variant.endswith('_rp') == rp_applies, rp.variant
    _same(wide, rp, B)
    infos = [_against_oracle(wide, i, xs[i], D, **kw) for i in oracle]
    return wide, infos


def _edge_windows(t, T, W):
    """events whose 3W-2 window of touched samples crosses a signal end"""
    t = np.asarray(t)
    off = (W - 1) // 2
    return int(np.sum((t - off - (W - 1) < 0) | (t + W // 2 + (W - 1) > T - 1)))


def _planted(D, T, B, seed=70, nb_atoms=None):
    import hsc_amd.synth as synth
    return np.stack([synth.make_signal(D, T, i, kind='planted', nb_atoms=nb_atoms or T // 40, noise=0.03, seed=seed) for i in range(B)])


@pytest.fixture(scope='module')
def d32x16():
    import hsc_amd.synth as synth
    return synth.make_dictionary(32, 16, seed=70)


@pytest.fixture(scope='module')
def xs16k(d32x16):
    xs = _planted(d32x16, 16384, 3)
    xs.setflags(write=False)
    return xs
