"""Seeded random sweep of the wide loop (csrc/hscmp_wide.h, HSCMP_WIDE=1) against the CPU oracle, bit for bit; the cases whose
rounds fit the round-parallel workgroup (at most 512 candidates) go through the forced round-parallel loop (HSCMP_RP=1) as well.
tests/test_gpu_fuzz.py draws through the default dispatch, which takes neither loop at its sizes.

The draw covers every width the two loops are built for (2, 4 or 8 chunks of eight taps, odd widths included), signals from
the shortest the plan admits (3W - 2) on, blocks from a few samples (shorter than an atom) to thousands, weights, the
null-coefficient filter on and off, and batches with a silent or a faint member.  test_the_draw_covers_the_loop runs without a
GPU: it takes the oracle over all draws and counts what the sweep reaches."""
import os

import numpy as np
import pytest

from tests.wide_util import _encode

N_CASES = int(os.environ.get("HSCMP_WIDE_FUZZ_CASES", "400"))
OFFSET = int(os.environ.get("HSCMP_WIDE_FUZZ_OFFSET", "0"))           # soak runs explore other seeds

WIDTHS = [9, 12, 13, 15, 16, 25, 31, 32, 57, 63, 64]
SIZES = [1, 2, 5, 16, 31, 32, 33, 48, 70]


def _signal(rs, D, T):
    K, W = D.shape
    x = rs.standard_normal(T).astype(np.float32)
    if rs.rand() < 0.5:                                       # planted structure on top of weak noise
        x *= np.float32(0.05)
        for _ in range(max(1, T // (2 * W))):
            k = rs.randint(0, K); t = rs.randint(0, max(1, T - W)); n = min(W, T - t)
            x[t:t + n] += (rs.uniform(0.5, 2.0) * D[k][:n]).astype(np.float32)
    return x


def _draw(i):
    """(signals [B, T], dictionary [K, W], keywords) of case i"""
    rs = np.random.RandomState(77000 + i)
    W = int(rs.choice(WIDTHS))
    K = int(rs.choice(SIZES))
    T = int(rs.randint(3 * W - 2, 60 * W + 50))
    D = rs.standard_normal((K, W)).astype(np.float32)
    D /= np.sqrt(np.sum(np.square(D), axis=1, keepdims=True))
    B = int(rs.randint(2, 5)) if i % 4 == 3 else 1
    xs = np.stack([_signal(rs, D, T) for _ in range(B)])
    if B > 1:                                                 # a silent or a faint member (never the first signal)
        b = int(rs.randint(1, B))
        xs[b] = np.zeros(T, dtype=np.float32) if rs.rand() < 0.5 else xs[0] * np.float32(1e-3)
    kw = {}
    rule = rs.randint(0, 3)
    if rule == 0:
        kw['nbNonzeroCoefs'] = int(rs.randint(1, 40))
    elif rule == 1:
        kw['toleranceSnr'] = float(rs.uniform(3.0, 25.0)); kw['nbNonzeroCoefs'] = 150
    else:
        kw['nbNonzeroCoefs'] = int(rs.randint(1, 25)); kw['toleranceSnr'] = 30.0
    mode = rs.randint(0, 3)
    if mode == 0:
        kw['nbBlocks'] = 'auto'
    elif mode == 1:
        kw['nbBlocks'] = int(rs.randint(2, 9))
    else:
        kw['nbBlocks'] = int(rs.randint(2, T // 4 + 1))        # down to blocks of four samples: shorter than an atom
    if rs.rand() < 0.3:
        kw['weights'] = rs.uniform(0.5, 1.0, size=K).astype(np.float32)
    u = rs.rand()
    if u < 0.15:
        kw['minCoefficients'] = None
    elif u < 0.35:
        kw['minCoefficients'] = float(rs.uniform(0.05, 0.6))
    return xs, D, kw


def _block_size(T, W, nbBlocks):
    bs = 4 * W if nbBlocks == 'auto' else T // nbBlocks
    return bs + (bs & 1)


def _plan(xs, D, kw):
    from hsc_amd import _native
    params = _native.make_params(eps=float(np.finfo(np.float32).eps), **{a: b for a, b in kw.items() if a != 'weights'})
    return _native.wide_plan(D.shape[0], D.shape[1], 1, np.float32, 'weights' in kw, xs.shape[0], xs.shape[1], params)


def _references(xs, D, kw):
    from oracle import hsc_oracle as orc
    return [orc.cmp_encode(x, D, maxEvents=1 << 17, **kw) for x in xs]


def _outside(refs):
    """a member that the oracle could not follow to a stop, or whose residual overflowed: no full comparison (test_gpu_fuzz.py)"""
    return any(r[2]['stop'] == 'capacity' or not np.all(np.isfinite(r[1])) for r in refs)


def _check(res, refs, tag):
    for b, (coef, r, info) in enumerate(refs):
        t, k, c = res.events[b]
        assert np.array_equal(t, info['t']) and np.array_equal(k, info['k']), (tag, b)
        assert np.array_equal(c, info['c']), (tag, b)
        assert np.array_equal(res.residuals[b], r), (tag, b)
        assert (res.coefficients[b] != coef).nnz == 0, (tag, b)
        assert res.stop_reasons()[b] == info['stop'], (tag, b)
        assert [int(v) for v in res.stats[b, :3]] == [info['nnz'], info['duplicates'], info['rounds']], (tag, b)
        assert int(res.stats[b, 4]) == info['iterations'], (tag, b)
        assert res.energies[b, 0] == info['energy_signal'] and res.energies[b, 1] == info['energy_residual'], (tag, b)


def _run(xs, D, kw, refs, wide, rp, suffix, tag, monkeypatch):
    # NB none of the default 400 draws ends in `capacity` or diverges (the census: outside 0), so the three branches for such
    # cases below -- those of test_gpu_fuzz.py -- run only when HSCMP_WIDE_FUZZ_OFFSET moves the sweep to other seeds
    from hsc_amd._native import HscmpError
    tag = tag + (suffix,)
    if xs.shape[0] > 1 and _outside(refs):
        return                                                # non-terminating / diverging member: the single-signal cases cover it
    info, r = refs[0][2], refs[0][1]
    if info['stop'] == 'capacity':
        # more selections than the oracle was allowed to follow: nothing to compare, the encode must just end
        try:
            res = _encode(xs, D, wide, rp, monkeypatch, **kw)
            assert res.variant.endswith(suffix), (tag, res.variant)
        except HscmpError as ex:
            assert 'does not converge' in str(ex), tag
        return
    diverged = not np.all(np.isfinite(r))
    try:
        res = _encode(xs, D, wide, rp, monkeypatch, **kw)
    except HscmpError as ex:
        # only a diverging pursuit may end like this (after the overflow the stop tests see inf / NaN)
        assert diverged and 'does not converge' in str(ex), tag
        return
    assert res.variant.endswith(suffix), (tag, res.variant)
    if diverged:
        # identical up to the overflow; the order of inf / NaN comparisons after it is not pinned
        t, k, c = res.events[0]
        huge = np.where(~(np.abs(info['c']) < 1e30))[0]
        n = min(len(t), len(info['t']), int(huge[0]) if len(huge) else 1 << 30) - 2
        assert n > 0 and np.array_equal(t[:n], info['t'][:n]) and np.array_equal(k[:n], info['k'][:n]) and np.array_equal(c[:n], info['c'][:n]), tag
        return
    _check(res, refs, tag)


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(N_CASES))
def test_random_configuration_vs_oracle(i, monkeypatch):
    xs, D, kw = _draw(i + OFFSET)
    plan = _plan(xs, D, kw)
    assert plan['can_run'], (i, plan)
    refs = _references(xs, D, kw)
    tag = (i, xs.shape, D.shape, plan['candidates'], {a: b for a, b in kw.items() if a != 'weights'})
    _run(xs, D, kw, refs, '1', None, '_wide', tag, monkeypatch)
    if plan['candidates'] <= 512:
        _run(xs, D, kw, refs, '0', '1', '_rp', tag, monkeypatch)


def test_the_draw_covers_the_loop():
    """The oracle over all draws (no GPU): what the sweep reaches, and how few cases fall outside the full comparison."""
    n = dict(outside=0, nnz=0, snr=0, empty=0, short_blocks=0, long_blocks=0, below_width=0, duplicates=0, round_parallel=0, batches=0)
    for i in range(400):                                      # (the default sweep, whatever a soak run's environment says)
        xs, D, kw = _draw(i)
        plan = _plan(xs, D, kw)
        assert plan['can_run'], (i, plan)                     # every draw has a wide form
        T, W = xs.shape[1], D.shape[1]
        bs = _block_size(T, W, kw['nbBlocks'])
        assert plan['candidates'] == -(-T // bs) + 1, (i, plan, bs)
        refs = _references(xs, D, kw)
        n['batches'] += xs.shape[0] > 1
        n['round_parallel'] += plan['candidates'] <= 512
        n['short_blocks'] += bs <= 256
        n['long_blocks'] += bs > 256
        n['below_width'] += bs < W
        if _outside(refs):
            n['outside'] += 1
            continue
        info = refs[0][2]
        if info['stop'] in ('nnz', 'snr', 'empty'):
            n[info['stop']] += 1
        n['duplicates'] += any(r[2]['duplicates'] > 0 for r in refs)
    print('wide sweep census over 400 draws: %s' % ', '.join('%s %d' % kv for kv in sorted(n.items())))
    assert n['outside'] <= 20, n                              # 5 %
    assert min(n['nnz'], n['snr'], n['empty']) >= 20, n
    assert n['short_blocks'] >= 10 and n['long_blocks'] >= 10 and n['below_width'] >= 10, n
    assert n['duplicates'] >= 30, n
