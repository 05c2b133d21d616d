"""The wide loop (csrc/hscmp_wide.h) on equal values: candidates of bit-equal |c| in a round -- the bitonic sort of wide_select
must give argsort(|c|)[::-1], the later entry first among equals, whatever the sign -- and equal maxima inside a block, spread
over the slices of the two-stage arg-max (bs > 256) or over the four loads of a lane (bs <= 256): the lowest position wins.

The signals are periodic with the block length, so every block of a round holds the same values: planted atoms in noise never
tie.  Every case states the ties it relies on as an assertion on the oracle's trace."""
import numpy as np
import pytest

from tests.wide_util import _all_loops, _against_oracle, _encode, _same

pytestmark = pytest.mark.gpu

W, PERIOD, REPEATS = 16, 64, 40
T = PERIOD * REPEATS


def _tied(c):
    """events whose |c| is, bit for bit, that of another event"""
    _, counts = np.unique(np.abs(np.asarray(c, dtype=np.float32)).view(np.uint32), return_counts=True)
    return int(counts[counts > 1].sum())


@pytest.fixture(scope='module')
def D():
    import hsc_amd.synth as synth
    return synth.make_dictionary(32, W, seed=70)


@pytest.fixture(scope='module')
def periodic(D):
    """one period of 64 samples (the block of nbBlocks='auto'): +2 D[3] at [10, 26), -1.5 D[9] at [40, 56); 40 periods"""
    one = np.zeros(PERIOD, dtype=np.float32)
    one[10:10 + W] += np.float32(2.0) * D[3]
    one[40:40 + W] += np.float32(-1.5) * D[9]
    x = np.tile(one, REPEATS)
    x.setflags(write=False)
    return x


@pytest.fixture(scope='module')
def negated(periodic):
    """the second half negated (the cut falls between two periods): the same |c|, the other sign"""
    x = periodic.copy()
    x[T // 2:] *= np.float32(-1.0)
    x.setflags(write=False)
    return x


@pytest.fixture(scope='module')
def shifted(periodic):
    """seven samples later (the last seven samples of a period are zero: nothing is lost at the end)"""
    assert not np.any(periodic[-7:])
    x = np.concatenate((np.zeros(7, dtype=np.float32), periodic[:-7]))
    x.setflags(write=False)
    return x


def test_equal_coefficients_keep_the_later_entry_first(D, periodic, monkeypatch):
    """Two rounds of 41 candidates, nearly all of them tied: round one runs from the last block to the first, and the nnz rule
    fires inside the tied group of round two (the prefix cuts a run of equal keys)."""
    from oracle import hsc_oracle as orc
    kw = dict(nbBlocks='auto', nbNonzeroCoefs=57)
    wide, (info,) = _all_loops(periodic[np.newaxis], D, monkeypatch, **kw)
    assert info['rounds'] == 2 and info['stop'] == 'nnz' and len(info['t']) == 57, (info['rounds'], info['stop'], len(info['t']))
    assert _tied(info['c']) >= 30, _tied(info['c'])
    assert [int(t) for t in info['t'][:3]] == [2513, 2449, 2385], info['t'][:3]          # later first: descending positions
    # the stop falls inside a tied group: one atom more would have been the next of the same round with the same |c|
    _, _, more = orc.cmp_encode(periodic, D, nbBlocks='auto', nbNonzeroCoefs=58)
    assert more['rounds'] == 2 and np.array_equal(more['t'][:57], info['t'])
    assert np.abs(more['c'][57]) == np.abs(more['c'][56]) == np.abs(info['c'][56])


def test_the_sort_key_ignores_the_sign(D, negated, monkeypatch):
    kw = dict(nbBlocks='auto', nbNonzeroCoefs=57)
    wide, (info,) = _all_loops(negated[np.newaxis], D, monkeypatch, **kw)
    assert _tied(info['c']) >= 30, _tied(info['c'])
    c = np.asarray(info['c'])
    both = set(np.abs(c[c > 0]).view(np.uint32).tolist()) & set(np.abs(c[c < 0]).view(np.uint32).tolist())
    assert both, 'no |c| occurs with both signs'
    # ... and inside a round: a positive and a negative coefficient of equal |c| next to each other in the trace
    same = np.abs(c[1:]) == np.abs(c[:-1])
    assert np.any(same & (np.sign(c[1:]) != np.sign(c[:-1])))


@pytest.mark.parametrize('max_events', [None, 4])
def test_batch_of_tied_signals(D, periodic, negated, shifted, max_events, monkeypatch):
    """Three signals of ties in one call; with an event list of 4 the rounds resume after growth in the same order."""
    xs = np.stack([periodic, negated, shifted])
    kw = dict(nbBlocks='auto', nbNonzeroCoefs=57)
    full, infos = _all_loops(xs, D, monkeypatch, oracle=(0, 1, 2), **kw)
    for info in infos:
        assert _tied(info['c']) >= 30, _tied(info['c'])
    if max_events is not None:
        short = _encode(xs, D, '1', None, monkeypatch, maxEvents=max_events, **kw)
        assert short.variant.endswith('_wide'), short.variant
        _same(full, short, 3)
        for i in range(3):
            _against_oracle(short, i, xs[i], D, **kw)


def test_equal_maxima_over_the_slices_of_a_long_block(D, periodic, monkeypatch):
    """nbBlocks=2: blocks of 1280 positions, reduced in two stages (a slice of 80 positions per wave).  Every block holds 20
    equal maxima in different slices: the lowest position is the block's candidate."""
    kw = dict(nbBlocks=2, nbNonzeroCoefs=30)
    wide, (info,) = _all_loops(periodic[np.newaxis], D, monkeypatch, **kw)
    assert info['rounds'] == 12 and info['stop'] == 'nnz', (info['rounds'], info['stop'])
    assert [int(t) for t in info['t'][:4]] == [1297, 17, 1937, 657], info['t'][:4]
    assert _tied(info['c']) >= 28, _tied(info['c'])


def test_equal_maxima_over_the_loads_of_a_lane(D, periodic, monkeypatch):
    """nbBlocks=10: blocks of 256 positions, one wave each with four loads per lane (rp_range_argmax4).  A block holds four
    periods: four equal maxima, 64 positions apart -- one per load of the same lane."""
    kw = dict(nbBlocks=10, nbNonzeroCoefs=30)
    wide, (info,) = _all_loops(periodic[np.newaxis], D, monkeypatch, **kw)
    t = np.asarray(info['t'])
    assert info['stop'] == 'nnz' and info['rounds'] >= 2, (info['rounds'], info['stop'])
    assert _tied(info['c']) >= 20, _tied(info['c'])
    # round one: the first of the four equal maxima of every block, i.e. positions inside the block's first period
    first = t[:10]
    assert np.all(first % 256 < PERIOD) and len(set((first // 256).tolist())) == 10, first
