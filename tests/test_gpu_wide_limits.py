"""The wide loop (csrc/hscmp_wide.h) at the limits of its plan, bit for bit against the CPU oracle and the other loops: the
sort with 16 384 candidates, with more than half and with all of its 16 384 entries in use, and one candidate past the cap, blocks on both sides of the switch between the two arg-max paths (256
positions) with odd signal lengths, the shortest signal the plan admits, odd widths, the even-width atom at T-1-W, rounds that
the null-coefficient filter empties, weights with four and eight chunks of taps, the default dispatch at its batch limit, and the
two ways a caller stops a signal between rounds (a stopCondition callback, Engine.stop_signal).

Every case states the edge it is about as an assertion on the oracle's trace: an input that misses it fails."""
import numpy as np
import pytest

from tests.wide_util import _all_loops, _against_oracle, _edge_windows, _encode, _planted, _same, d32x16, xs16k  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)


def _plan(D, B, T, weights=False, **kw):
    from hsc_amd import _native
    return _native.wide_plan(D.shape[0], D.shape[1], 1, np.float32, weights, B, T, _native.make_params(eps=EPS, **kw))


def _interior(t, T, W):
    """RpMfma::is_interior: the 3W-2 window of touched samples inside the signal, and not the even-width atom at T-1-W"""
    t = np.asarray(t)
    off = (W - 1) // 2
    inside = (t - off - (W - 1) >= 0) & (t + W // 2 + (W - 1) <= T - 1)
    return inside & ~((W % 2 == 0) & (t == T - 1 - W))


# ---- the sort at its cap ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def d40x12():
    import hsc_amd.synth as synth
    return synth.make_dictionary(40, 12, seed=73)


@pytest.fixture(scope='module')
def at_cap(d40x12):
    x = _planted(d40x12, 16383 * 8, 1, seed=73)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize('kw', [dict(nbNonzeroCoefs=3000), dict(toleranceSnr=15.0)])
def test_sort_at_its_cap(d40x12, at_cap, kw, monkeypatch):
    """16 383 blocks of 8 positions (shorter than the 12 taps): 16 384 candidates with the half-block offset -- the candidates
    kernel's widest grid, 17 passes of every compaction over them, and the control workgroup launched with its 128 KiB of sort
    keys.  Most neighbouring candidates lie closer than W, so the interference filter leaves the sort a few thousand entries
    only: the sort itself at its cap is test_sort_with_more_than_half_its_entries and test_sort_of_a_full_round_of_equal_keys.
    The nnz rule stops inside round one; the snr rule runs 47 rounds until the weak-atom filter leaves nothing."""
    T = at_cap.shape[1]
    kw = dict(kw, nbBlocks=16383)
    plan = _plan(d40x12, 1, T, **kw)
    assert plan['candidates'] == 16384 and plan['can_run'], plan
    wide, (info,) = _all_loops(at_cap, d40x12, monkeypatch, rp_applies=False, **kw)
    if 'nbNonzeroCoefs' in kw:
        assert info['stop'] == 'nnz' and info['rounds'] == 1 and len(info['t']) == 3000, (info['stop'], info['rounds'])
    else:
        assert (info['stop'], info['rounds'], len(info['t']), info['duplicates']) == ('empty', 47, 7833, 275), \
            (info['stop'], info['rounds'], len(info['t']), info['duplicates'])


@pytest.fixture(scope='module')
def one_atom_per_block(d40x12):
    """16 383 blocks of W = 12 positions, each holding D[5] with an amplitude of its own: neighbouring candidates lie about W
    apart, so most of them pass the interference filter"""
    rs = np.random.RandomState(7300)
    amp = (rs.uniform(0.5, 4.0, size=16383) * rs.choice([-1.0, 1.0], size=16383)).astype(np.float32)
    x = (amp[:, None] * d40x12[5][None, :]).reshape(1, -1).astype(np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize('kw, expected', [(dict(nbNonzeroCoefs=12000), ('nnz', 2, 12000, 0)), (dict(toleranceSnr=15.0), ('snr', 4, 23544, 3199))])
def test_sort_with_more_than_half_its_entries(d40x12, one_atom_per_block, kw, expected, monkeypatch):
    """The sort of wide_select with 11 086 keys in round one: 16 384 entries, so the passes k = 8192 and 16 384 of the bitonic
    network and the keys beyond the first 64 KiB of LDS do their work.  The nnz rule stops in round two, the snr rule in round
    four, with thousands of duplicates."""
    from oracle import hsc_oracle as orc
    x = one_atom_per_block
    kw = dict(kw, nbBlocks=16383)
    plan = _plan(d40x12, 1, x.shape[1], **kw)
    assert plan['candidates'] == 16384 and plan['can_run'], plan
    _, _, first = orc.cmp_encode(x[0], d40x12, maxRounds=1, **kw)
    assert first['stop'] == 'running' and len(first['t']) == 11086 > 8192, (first['stop'], len(first['t']))      # the sorted entries of round one
    wide, (info,) = _all_loops(x, d40x12, monkeypatch, rp_applies=False, **kw)
    assert (info['stop'], info['rounds'], len(info['t']), info['duplicates']) == expected, \
        (info['stop'], info['rounds'], len(info['t']), info['duplicates'])


def test_sort_of_a_full_round_of_equal_keys(d40x12, monkeypatch):
    """A signal of period 8 under blocks of 8: every candidate but the one at the signal's start has the same |c|, and no two neighbours lie W apart, so the
    interference filter is skipped and all 16 383 candidates of round one reach the sort -- which must then hand them out from
    the last block to the first (the later entry first among equals) -- and the control workgroup applies them one by one."""
    from oracle import hsc_oracle as orc
    x = np.tile(np.float32(2.0) * d40x12[5][:8], 16383)[np.newaxis]
    kw = dict(nbBlocks=16383, nbNonzeroCoefs=600)
    plan = _plan(d40x12, 1, x.shape[1], **kw)
    assert plan['candidates'] == 16384 and plan['can_run'], plan
    _, _, first = orc.cmp_encode(x[0], d40x12, maxRounds=1, nbBlocks=16383, nbNonzeroCoefs=1 << 20)
    assert len(first['t']) == 16383 > 8192, len(first['t'])
    tied = np.abs(first['c']).view(np.uint32) == np.abs(first['c'][:1]).view(np.uint32)
    assert int(tied.sum()) >= 16380, int(tied.sum())                  # (the block at the signal's start sees a clipped atom)
    assert np.all(np.diff(first['t'][tied]) == -8), first['t'][:8]
    wide, (info,) = _all_loops(x, d40x12, monkeypatch, rp_applies=False, **kw)
    assert (info['stop'], info['rounds'], len(info['t'])) == ('nnz', 1, 600), (info['stop'], info['rounds'], len(info['t']))
    assert np.array_equal(info['t'], first['t'][:600])


def test_one_candidate_past_the_cap_keeps_todays_loop(d40x12, monkeypatch):
    T = 16384 * 8
    x = _planted(d40x12, T, 1, seed=73)
    kw = dict(nbBlocks=16384, nbNonzeroCoefs=500)
    plan = _plan(d40x12, 1, T, **kw)
    assert plan['candidates'] == 16385 and not plan['can_run'], plan
    res = _encode(x, d40x12, '1', None, monkeypatch, **kw)
    assert '_wide' not in res.variant, res.variant
    info = _against_oracle(res, 0, x[0], d40x12, **kw)
    assert info['stop'] == 'nnz' and len(info['t']) == 500


# ---- blocks of 256 and 258 positions, odd T -----------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(nbNonzeroCoefs=45), dict(toleranceSnr=18.0)])
@pytest.mark.parametrize('W', [16, 31])
@pytest.mark.parametrize('T, bs', [(2311, 256), (2323, 258)])
def test_blocks_on_both_sides_of_the_argmax_switch(T, bs, W, kw, monkeypatch):
    """nbBlocks=9: blocks of 256 positions (one wave, four loads per lane) leave a tenth block of 7 samples, blocks of 258 (the
    two-stage reduction) one of a single sample.  An atom centred on the last sample makes that block's candidate an event of
    round one."""
    import hsc_amd.synth as synth
    from oracle import hsc_oracle as orc
    D = synth.make_dictionary(32, W, seed=80 + W)
    x = _planted(D, T, 1, seed=81)
    lo = T - 1 - (W - 1) // 2
    x[0, lo:] += np.float32(5.0) * D[7][:T - lo]
    assert T // 9 + (T // 9) % 2 == bs and T - 9 * bs in (7, 1)
    kw = dict(kw, nbBlocks=9)
    assert _plan(D, 1, T, **kw)['candidates'] == 11
    wide, (info,) = _all_loops(x, D, monkeypatch, **kw)
    assert info['rounds'] >= 2 and info['stop'] == ('nnz' if 'nbNonzeroCoefs' in kw else 'snr'), (info['rounds'], info['stop'])
    _, _, first = orc.cmp_encode(x[0], D, maxRounds=1, **kw)
    assert np.any(first['t'] >= 9 * bs), first['t']                   # the short last block gave an atom of round one


# ---- the shortest signal: T = 3W - 2 ------------------------------------------------------------------------------------------
def _shortest(W, centre):
    """T = 3W-2: one position -- the centre, whose window of touched samples is the whole signal -- is interior, every other atom
    is applied by the control workgroup.  Atoms planted towards both ends (and, on request, a dominant one at the centre); the
    noise is drawn from a stream with which no selection of the first kind of signal lands on the centre (the tests assert it)."""
    import hsc_amd.synth as synth
    T = 3 * W - 2
    D = synth.make_dictionary(24, W, seed=90 + W)
    rs = np.random.RandomState(12900 + W)
    x = (0.03 * rs.standard_normal(T)).astype(np.float32)
    off = (W - 1) // 2
    atoms = [(off + 1, 3, 2.5), (T - W // 2 - 2, 7, -2.0), (off + W // 3, 11, 1.5)]
    if centre:
        atoms.append((off + W - 1, 5, 6.0))
    for p, k, c in atoms:
        x[p - off:p - off + W] += np.float32(c) * D[k]
    return x[np.newaxis], D, T


@pytest.mark.parametrize('nb', ['auto', 4])
@pytest.mark.parametrize('W', [12, 13, 16, 31, 32, 63, 64])
def test_shortest_signal_of_the_plan(W, nb, monkeypatch):
    x, D, T = _shortest(W, centre=False)
    kw = dict(nbBlocks=nb, nbNonzeroCoefs=10)
    assert _plan(D, 1, T, **kw)['can_run'] and not _plan(D, 1, T - 1, **kw)['can_run']
    wide, (info,) = _all_loops(x, D, monkeypatch, **kw)
    assert info['rounds'] >= 3 and len(info['t']) >= 10, (info['rounds'], len(info['t']))
    assert not np.any(_interior(info['t'], T, W)), info['t']          # nothing went to the grid
    assert _edge_windows(info['t'], T, W) == len(info['t'])


@pytest.mark.parametrize('W', [12, 13, 32, 63])
def test_shortest_signal_with_its_one_interior_atom(W, monkeypatch):
    """... and the one atom of such a signal that the grid applies, between atoms of the control workgroup"""
    x, D, T = _shortest(W, centre=True)
    kw = dict(nbBlocks=4, nbNonzeroCoefs=10)
    wide, (info,) = _all_loops(x, D, monkeypatch, **kw)
    inner = _interior(info['t'], T, W)
    assert np.any(inner) and not np.all(inner), info['t']
    assert set(np.asarray(info['t'])[inner].tolist()) == {(W - 1) // 2 + W - 1}


# ---- odd widths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W', [9, 13, 25, 31, 57, 63])
def test_odd_widths_with_atoms_at_both_ends(W, monkeypatch):
    """2, 4 and 8 chunks of eight taps with the last chunk partly (9, 25, 57: almost wholly) padding"""
    import hsc_amd.synth as synth
    T = 40 * W + 1
    D = synth.make_dictionary(32, W, seed=100 + W)
    x = _planted(D, T, 1, seed=101)
    x[0, :2 * W] *= 6.0
    x[0, -2 * W:] *= 6.0
    wide, (info,) = _all_loops(x, D, monkeypatch, nbBlocks='auto', toleranceSnr=18.0)
    assert info['rounds'] >= 2 and _edge_windows(info['t'], T, W) >= 3, (info['rounds'], _edge_windows(info['t'], T, W))


# ---- the even-width atom at T-1-W ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W', [12, 16, 32, 64])
def test_even_width_atom_at_the_stale_edge_position(W, monkeypatch):
    """An atom at p = T-1-W (even W) changes r[T-1-W/2], which row T-1 sees through the reflection, without re-correlating that
    row: RpMfma::is_interior makes it an atom of the control workgroup, and wide_subtract_kernel relies on never getting it.
    (Its window of touched samples also crosses the signal's end, as that of every atom right of T - 3W/2.)
    Signal 0 has a dominant atom there; signal 1 a second one a position to the left, and a third at the last interior position,
    which goes to the grid.
    The whole residual (rows T-1 and T-1-W/2 with it) and the selections that follow at the signal's end equal the oracle's."""
    import hsc_amd.synth as synth
    T = 24 * W
    D = synth.make_dictionary(32, W, seed=110 + W)
    xs = _planted(D, T, 2, seed=111)
    xs[:, -2 * W:] *= 3.0
    off = (W - 1) // 2
    p = T - 1 - W
    last = T - 1 - (W // 2 + W - 1)                                       # the last position whose window ends inside the signal
    xs[:, p - off:p - off + W] += np.float32(14.0) * D[4]
    xs[1, p - 1 - off:p - 1 - off + W] += np.float32(-11.0) * D[26]
    xs[1, last - off:last - off + W] += np.float32(9.0) * D[13]
    assert not _interior(p, T, W) and _interior(last, T, W) and not _interior(last + 1, T, W)
    kw = dict(nbBlocks='auto', nbNonzeroCoefs=40)
    wide, infos = _all_loops(xs, D, monkeypatch, oracle=(0, 1), **kw)
    for i, info in enumerate(infos):
        t = np.asarray(info['t'])
        assert p in t, (i, t)
        at = int(np.where(t == p)[0][0])
        assert np.any(t[at + 1:] + W // 2 + (W - 1) > T - 1), (i, t)      # later atoms whose rows reach the right end
    assert p - 1 in infos[1]['t'] and last in infos[1]['t'], infos[1]['t']


# ---- rounds that the filters empty --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def x4k(d32x16):
    x = _planted(d32x16, 4096, 1, nb_atoms=100)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize('minc, stop, rounds, events', [(0.3, 'empty', 13, 145), (1.0, 'empty', 6, 87), (100.0, 'empty', 1, 0), (None, 'nnz', None, None)])
def test_null_coefficient_filter_empties_a_round(d32x16, x4k, minc, stop, rounds, events, monkeypatch):
    kw = dict(nbBlocks='auto', nbNonzeroCoefs=5000, minCoefficients=minc)
    wide, (info,) = _all_loops(x4k, d32x16, monkeypatch, **kw)
    assert info['stop'] == stop, info['stop']
    if rounds is not None:
        assert (info['rounds'], len(info['t'])) == (rounds, events), (info['rounds'], len(info['t']))
    else:
        assert info['rounds'] >= 10 and info['duplicates'] > 0, (info['rounds'], info['duplicates'])
    assert int(wide.stats[0, 2]) == info['rounds'] and int(wide.stats[0, 5]) == len(info['t'])


@pytest.mark.parametrize('kw', [dict(nbNonzeroCoefs=200), dict(toleranceSnr=18.0)])
def test_all_zero_signal(d32x16, kw, monkeypatch):
    """No candidate survives the null-coefficient filter: `empty` in round one, alone and between two signals that go on"""
    xs = _planted(d32x16, 4096, 3)
    xs[1] = 0.0
    kw = dict(kw, nbBlocks='auto')
    wide, (info,) = _all_loops(xs[1:2], d32x16, monkeypatch, **kw)
    assert (info['stop'], info['rounds'], len(info['t'])) == ('empty', 1, 0), info
    wide, infos = _all_loops(xs, d32x16, monkeypatch, oracle=(0, 1, 2), **kw)
    assert (infos[1]['stop'], infos[1]['rounds'], len(infos[1]['t'])) == ('empty', 1, 0), infos[1]
    assert infos[0]['rounds'] >= 2 and infos[2]['rounds'] >= 2
    assert not np.any(wide.residuals[1]) and wide.energies[1, 0] == 0.0


# ---- weights with four and eight chunks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('K, W', [(48, 32), (64, 64)])
def test_weights_with_four_and_eight_chunks(K, W, monkeypatch):
    import hsc_amd.synth as synth
    from oracle import hsc_oracle as orc
    T = 40 * W
    D = synth.make_dictionary(K, W, seed=120 + W)
    xs = _planted(D, T, 2, seed=121)
    w = np.random.RandomState(122).uniform(0.6, 1.0, size=K).astype(np.float32)
    kw = dict(nbBlocks='auto', nbNonzeroCoefs=80)
    wide, infos = _all_loops(xs, D, monkeypatch, oracle=(0, 1), weights=w, **kw)
    for i, info in enumerate(infos):
        assert info['rounds'] >= 5 and info['stop'] == 'nnz', (info['rounds'], info['stop'])
        _, _, plain = orc.cmp_encode(xs[i], D, **kw)
        assert not (np.array_equal(plain['t'], info['t']) and np.array_equal(plain['k'], info['k'])), 'the weights changed no selection'


# ---- the default dispatch at its batch limit ----------------------------------------------------------------------------------
def test_default_dispatch_at_the_batch_limit(d32x16, monkeypatch):
    """16 signals of 1025 candidates per round go wide with nothing forced, 17 keep the one-atom loop; either equals the forced
    sequential loop, and two rows the oracle."""
    T = 65536
    xs = _planted(d32x16, T, 17)
    kw = dict(nbBlocks='auto', nbNonzeroCoefs=300)
    assert _plan(d32x16, 16, T, **kw)['by_default'] and not _plan(d32x16, 17, T, **kw)['by_default']
    seq = _encode(xs, d32x16, '0', '0', monkeypatch, **kw)
    assert seq.variant == 'mfma_init+mfma_loop_f32', seq.variant
    res16 = _encode(xs[:16], d32x16, None, None, monkeypatch, **kw)
    assert res16.variant.endswith('_wide'), res16.variant
    for i in range(16):
        for u, v in zip(res16.events[i], seq.events[i]):
            assert np.array_equal(u, v), i
        assert np.array_equal(res16.residuals[i], seq.residuals[i]), i
    assert np.array_equal(res16.stats, seq.stats[:16]) and np.array_equal(res16.energies, seq.energies[:16])
    res17 = _encode(xs, d32x16, None, None, monkeypatch, **kw)
    assert '_wide' not in res17.variant, res17.variant
    _same(res17, seq, 17)
    for i in (5, 15):                                                  # (the oracle on two rows; the others through the sequential loop)
        info = _against_oracle(res16, i, xs[i], d32x16, **kw)
        assert info['stop'] == 'nnz' and len(info['t']) == 300


# ---- stopping a signal between rounds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_events', [None, 4])
def test_stop_condition_callback(d32x16, xs16k, max_events, monkeypatch):
    """One round per call (hscmp_continue): the callback stops signal 1 after two rounds and the others after four; each is the
    oracle's run of that many rounds.  With an event list of 4 the rounds are also resumed after growth."""
    from hsc_amd.modeling import ConvolutionalMatchingPursuit
    from oracle import hsc_oracle as orc
    kw = dict(nbBlocks='auto', toleranceSnr=18.0)
    wanted = [4, 2, 4]
    seen = [0, 0, 0]

    def stop(sequence, residual, coefficients):
        b = [i for i in range(3) if np.array_equal(sequence[:, 0], xs16k[i])]
        assert len(b) == 1
        seen[b[0]] += 1
        return seen[b[0]] >= wanted[b[0]]

    monkeypatch.setenv('HSCMP_WIDE', '1')
    monkeypatch.delenv('HSCMP_RP', raising=False)
    extra = {} if max_events is None else dict(maxEvents=max_events)
    res = ConvolutionalMatchingPursuit().computeCoefficientsBatch(xs16k, d32x16, stopCondition=stop, **dict(kw, **extra))
    assert res.variant.endswith('_wide'), res.variant
    assert seen == wanted
    assert res.stop_reasons() == ['callback'] * 3
    for i in range(3):
        coef, r, info = orc.cmp_encode(xs16k[i], d32x16, maxRounds=wanted[i], **kw)
        assert info['stop'] == 'running' and info['rounds'] == wanted[i] and len(info['t']) > 100
        t, k, c = res.events[i]
        assert np.array_equal(t, info['t']) and np.array_equal(k, info['k']) and np.array_equal(c, info['c']), i
        assert np.array_equal(res.residuals[i], r), i
        assert (res.coefficients[i] != coef).nnz == 0, i
        assert [int(v) for v in res.stats[i, :3]] == [info['nnz'], info['duplicates'], info['rounds']], i
        assert res.energies[i, 0] == info['energy_signal'] and res.energies[i, 1] == info['energy_residual'], i


def test_stop_signal_between_continued_rounds(d32x16, xs16k, monkeypatch):
    """Engine.stop_signal on the raw engine: the wide loop's next call finds the signal stopped and leaves its state alone"""
    from hsc_amd import _native
    from oracle import hsc_oracle as orc
    monkeypatch.setenv('HSCMP_WIDE', '1')
    monkeypatch.delenv('HSCMP_RP', raising=False)
    kw = dict(toleranceSnr=18.0, nbBlocks='auto')
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(d32x16[:, :, None])
        x = np.ascontiguousarray(xs16k[:, :, None])
        eng.encode_batch(x, _native.make_params(eps=EPS, maxEvents=4096, maxRounds=1, **kw))
        assert eng.last_variant().endswith('_wide')
        eng.continue_rounds(1)
        eng.stop_signal(1)
        before = [a[1].copy() for a in (eng.fetch_stats(),) + eng.fetch_events() + (eng.fetch_residual(), eng.fetch_energies())]
        assert int(before[0][_native.STAT_STOP]) != _native.STOP_RUNNING and int(before[0][2]) == 2
        eng.continue_rounds(2)
        after = [a[1].copy() for a in (eng.fetch_stats(),) + eng.fetch_events() + (eng.fetch_residual(), eng.fetch_energies())]
        for u, v in zip(before, after):
            assert np.array_equal(u, v)
        stats = eng.fetch_stats()
        ev_t, ev_k, ev_c = eng.fetch_events()
        residual = eng.fetch_residual()
        for i, rounds in ((0, 4), (1, 2), (2, 4)):
            _, r, info = orc.cmp_encode(xs16k[i], d32x16, maxRounds=rounds, **kw)
            assert info['stop'] == 'running' and info['rounds'] == rounds
            assert [int(v) for v in stats[i, :3]] == [info['nnz'], info['duplicates'], rounds] and int(stats[i, 4]) == info['iterations']
            n = len(info['t'])
            assert int(stats[i, 5]) == n
            assert np.array_equal(ev_t[i, :n], info['t']) and np.array_equal(ev_k[i, :n], info['k']) and np.array_equal(ev_c[i, :n], info['c'])
            assert np.array_equal(residual[i, :, 0], r), i
        assert int(stats[0, _native.STAT_STOP]) == _native.STOP_RUNNING and int(stats[2, _native.STAT_STOP]) == _native.STOP_RUNNING
    finally:
        eng.close()
