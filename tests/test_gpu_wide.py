"""The wide loop (csrc/hscmp_wide.h: a blocked round's atoms spread over the whole chip as plain kernel launches in stream
order) against the round-parallel loop, the one-atom-at-a-time loop and the CPU oracle, bit for bit.

HSCMP_WIDE=1 / 0 force / forbid the loop (read at every encode); unset, the dispatcher picks it for few long signals whose
rounds hold more candidates than the round-parallel workgroup takes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


from tests.wide_util import _all_loops, _against_oracle, _edge_windows, _encode, _planted, _same, d32x16, xs16k  # noqa: F401 (fixtures)


@pytest.mark.parametrize('kw, rounds_at_least', [(dict(nbNonzeroCoefs=700), 4), (dict(toleranceSnr=18.0), 4)])
def test_many_blocks_per_round(d32x16, xs16k, kw, rounds_at_least, monkeypatch):
    """256 blocks per round, B = 3; the nnz rule stops inside a round (the prefix cuts the group handed to the grid), the snr
    rule after five rounds.  Duplicates: the slot chains are followed across launches."""
    kw = dict(kw, nbBlocks='auto')
    wide, (info,) = _all_loops(xs16k, d32x16, monkeypatch, oracle=(2,), **kw)
    assert info['rounds'] >= rounds_at_least and info['duplicates'] > 0, info
    assert info['stop'] == ('nnz' if 'nbNonzeroCoefs' in kw else 'snr')
    assert int(wide.stats[2, 2]) == info['rounds'] and int(wide.stats[2, 1]) == info['duplicates']


def test_beyond_the_round_parallel_cap_and_default_dispatch(d32x16, monkeypatch):
    """1024 blocks per round: more candidates than the round-parallel workgroup holds.  Unforced, one such signal goes wide."""
    x = _planted(d32x16, 65536, 3)[2:3]
    kw = dict(nbBlocks='auto', toleranceSnr=18.0)
    wide, (info,) = _all_loops(x, d32x16, monkeypatch, rp_applies=False, **kw)
    assert info['rounds'] >= 4 and len(info['t']) > 2000, (info['rounds'], len(info['t']))
    default = _encode(x, d32x16, None, None, monkeypatch, **kw)
    assert default.variant.endswith('_wide'), default.variant
    _same(wide, default, 1)


@pytest.mark.parametrize('T, rp_applies', [(16384, True), (65536, False)])
def test_atoms_at_both_signal_ends(d32x16, T, rp_applies, monkeypatch):
    """Energy piled at both ends: atoms whose windows cross them form groups of their own inside the rounds, applied by the
    control workgroup, and the edge record travels between the launches."""
    W = 16
    x = _planted(d32x16, T, 3)[2:3].copy()
    x[0, :2 * W] *= 6.0
    x[0, -2 * W:] *= 6.0
    wide, (info,) = _all_loops(x, d32x16, monkeypatch, rp_applies=rp_applies, nbBlocks='auto', toleranceSnr=18.0)
    assert _edge_windows(info['t'], T, W) >= 3, _edge_windows(info['t'], T, W)


def test_w64_long_signal_with_scaled_ends(monkeypatch):
    import hsc_amd.synth as synth
    K, W, T = 64, 64, 262144
    D = synth.make_dictionary(K, W, seed=70)
    x = _planted(D, T, 3, nb_atoms=T // 200)[2:3].copy()
    x[0, :2 * W] *= 6.0
    x[0, -2 * W:] *= 6.0
    wide, (info,) = _all_loops(x, D, monkeypatch, rp_applies=False, nbBlocks='auto', toleranceSnr=15.0)
    assert info['rounds'] >= 4 and len(info['t']) > 2000 and _edge_windows(info['t'], T, W) >= 3


def test_w32_fixed_block_count(monkeypatch):
    import hsc_amd.synth as synth
    D = synth.make_dictionary(48, 32, seed=72)
    xs = _planted(D, 20000, 2, seed=72)
    xs[1, :64] *= 5.0
    wide, (info,) = _all_loops(xs, D, monkeypatch, oracle=(1,), nbBlocks=200, toleranceSnr=20.0)
    assert info['rounds'] >= 2 and len(info['t']) > 200 and _edge_windows(info['t'], 20000, 32) >= 1, info['rounds']


def test_w12_weights_and_long_blocks(monkeypatch):
    """W = 12 (two chunks, zero-padded taps) with per-atom weights; nbBlocks=5 makes blocks of thousands of positions: the
    candidates kernel reduces such a block in two stages."""
    import hsc_amd.synth as synth
    K = 40
    D = synth.make_dictionary(K, 12, seed=73)
    xs = _planted(D, 9000, 2, seed=73)
    w = np.random.RandomState(73).uniform(0.6, 1.0, size=K).astype(np.float32)
    for nb, l0, rounds in (('auto', 400, 2), (5, 150, 20)):
        wide, (info,) = _all_loops(xs, D, monkeypatch, oracle=(1,), nbBlocks=nb, nbNonzeroCoefs=l0, weights=w)
        assert info['rounds'] >= rounds and info['stop'] == 'nnz', (nb, info['rounds'], info['stop'])


def test_three_chunk_width_keeps_todays_loop(monkeypatch):
    import hsc_amd.synth as synth
    D = synth.make_dictionary(24, 20, seed=74)
    xs = _planted(D, 4000, 1, seed=74)
    res = _encode(xs, D, '1', None, monkeypatch, nbBlocks='auto', nbNonzeroCoefs=60)
    assert '_wide' not in res.variant, res.variant
    _against_oracle(res, 0, xs[0], D, nbBlocks='auto', nbNonzeroCoefs=60)


@pytest.mark.parametrize('W', [12, 16, 32])
def test_round_whose_interference_filter_is_skipped(W, monkeypatch):
    """The three two-atom signals of tests/test_gpu_round_parallel.py: no gap qualifies, the filter is skipped, and the
    overlapping atoms are applied one by one by the control workgroup with the energies of their turn."""
    import hsc_amd.synth as synth
    K, T = 24, 64 * W
    D = synth.make_dictionary(K, W, seed=50 + W)
    xs = np.zeros((3, T), dtype=np.float32)
    for i, (gap, nbk) in enumerate([(3, 2), (W - 1, 4), (W // 2, 8)]):
        edge = (T // nbk) * (nbk // 2)
        for p, k, c in ((edge - gap // 2 - 1, 3, 2.5), (edge + gap - gap // 2 - 1, 7, -1.75)):
            lo = p - (W - 1) // 2
            xs[i, lo:lo + W] += c * D[k]
    for i, nbk in enumerate([2, 4, 8]):
        wide, (info,) = _all_loops(xs[i:i + 1], D, monkeypatch, nbBlocks=nbk, nbNonzeroCoefs=12)
        # the precondition: the first round applied both planted atoms although they lie closer than W (no filter ran)
        t = np.asarray(info['t'])
        assert len(t) >= 2 and 0 < abs(int(t[0]) - int(t[1])) < W, t[:4]


def test_resumes_after_event_list_growth(d32x16, xs16k, monkeypatch):
    kw = dict(nbBlocks='auto', toleranceSnr=18.0)
    full, (info,) = _all_loops(xs16k, d32x16, monkeypatch, oracle=(2,), **kw)     # (both other loops and the oracle)
    assert len(info['t']) > 64                                                     # an event list of 4 is grown several times
    short = _encode(xs16k, d32x16, '1', None, monkeypatch, maxEvents=4, **kw)     # grown in place, the loop resumed several times
    assert short.variant.endswith('_wide')
    _same(full, short, 3)


def test_max_rounds_is_honoured(d32x16, xs16k, monkeypatch):
    """Two rounds, then two more through hscmp_continue: the counters after either equal the oracle's with maxRounds."""
    from hsc_amd import _native
    from oracle import hsc_oracle as orc
    monkeypatch.setenv('HSCMP_WIDE', '1')
    eps = float(np.finfo(np.float32).eps)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(d32x16[:, :, None])
        x = np.ascontiguousarray(xs16k[:, :, None])
        eng.encode_batch(x, _native.make_params(toleranceSnr=18.0, nbBlocks='auto', eps=eps, maxEvents=4096, maxRounds=2))
        assert eng.last_variant().endswith('_wide')
        for rounds in (2, 4):
            stats = eng.fetch_stats()
            ev_t, ev_k, ev_c = eng.fetch_events()
            for i in (0, 2):
                _, _, info = orc.cmp_encode(xs16k[i], d32x16, toleranceSnr=18.0, nbBlocks='auto', maxRounds=rounds)
                assert info['stop'] == 'running' and info['rounds'] == rounds
                assert [int(v) for v in stats[i, :5]] == [info['nnz'], info['duplicates'], rounds, 0, info['iterations']]
                n = len(info['t'])
                assert int(stats[i, 5]) == n and np.array_equal(ev_t[i, :n], info['t']) and np.array_equal(ev_c[i, :n], info['c'])
            eng.continue_rounds(2)
    finally:
        eng.close()


def test_small_batch_with_uneven_progress(monkeypatch):
    import hsc_amd.synth as synth
    D = synth.make_dictionary(32, 16, seed=75)
    T = 8192
    xs = np.stack([synth.make_signal(D, T, i, kind='noise' if i in (1, 3) else 'planted', nb_atoms=T // (20 + 30 * i), noise=0.03, seed=75)
                   for i in range(5)])
    wide, infos = _all_loops(xs, D, monkeypatch, oracle=(0, 1, 4), nbBlocks='auto', toleranceSnr=12.0, nbNonzeroCoefs=900)
    assert len(set(int(r) for r in wide.stats[:, 2])) > 1, wide.stats[:, 2]          # the signals stop in different rounds


def test_hierarchy_level0_goes_wide(monkeypatch):
    import scipy.sparse
    import hsc_amd.synth as synth
    from hsc_amd.hierarchical import HierarchicalConvolutionalMatchingPursuit
    mld = synth.make_hierarchy(K0=32, W0=16, K1=16, W1=16, size=3, seed=9)
    mlds = mld.withSingletonBases()
    xs = synth.make_hierarchy_batch(mld, 16384, 0, 1, seed=9)
    kw = dict(toleranceSnr=[20.0, 25.0], nbBlocks='auto', singletonWeight=0.95)
    out = {}
    energy = {}
    for wide, rp in (('1', None), ('0', '0'), ('0', '1')):
        monkeypatch.setenv('HSCMP_WIDE', wide)
        if rp is None:
            monkeypatch.delenv('HSCMP_RP', raising=False)
        else:
            monkeypatch.setenv('HSCMP_RP', rp)
        gpu = HierarchicalConvolutionalMatchingPursuit(method='cmp')
        out[wide + str(rp)] = gpu.computeCoefficientsBatch(xs, mlds, **kw)
        energy[wide + str(rp)] = gpu.computeCoefficientsBatch(xs, mlds, residuals='energy', **kw)[1]
        gpu.close()
    assert out['1None'][2][0]['variant'].endswith('_wide'), out['1None'][2][0]['variant']
    assert out['00'][2][0]['variant'] == 'mfma_init+mfma_loop_f32' and out['01'][2][0]['variant'].endswith('_rp')
    for other in ('00', '01'):
        for l in range(2):
            assert (scipy.sparse.csc_matrix(out['1None'][0][0][l]) != scipy.sparse.csc_matrix(out[other][0][0][l])).nnz == 0, (other, l)
        assert np.array_equal(out['1None'][1][0], out[other][1][0]), other
        assert np.array_equal(np.asarray(energy['1None']), np.asarray(energy[other])), other
    # the host logic with the CPU oracle as level coder (the arrangement of tests/test_baseline_shapes.py)
    from oracle import hsc_oracle as orc

    class OracleLevelCoder(object):
        def __init__(self, D):
            self.D = D

        def encode(self, X, **k):
            coefficients, residual, _ = orc.cmp_encode(np.asarray(X), self.D, **k)
            return coefficients, residual
    ref = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    monkeypatch.setattr(ref, '_level_coder', lambda D: OracleLevelCoder(D))
    exp_c, exp_r = ref.computeCoefficients(xs[0], mlds, **kw)
    for l in range(2):
        assert (scipy.sparse.csc_matrix(out['1None'][0][0][l]) != scipy.sparse.csc_matrix(exp_c[l])).nnz == 0, l
    assert np.array_equal(out['1None'][1][0], exp_r)
    out['1'], out['0'] = out['1None'], out['00']
    for l in range(2):
        assert (scipy.sparse.csc_matrix(out['1'][0][0][l]) != scipy.sparse.csc_matrix(out['0'][0][0][l])).nnz == 0, l
    assert np.array_equal(out['1'][1][0], out['0'][1][0])
    assert out['1'][0][0][0].nnz > 100


def test_three_runs_bit_for_bit(d32x16, xs16k, monkeypatch):
    kw = dict(nbBlocks='auto', nbNonzeroCoefs=700)
    first, (info,) = _all_loops(xs16k, d32x16, monkeypatch, oracle=(2,), **kw)    # (both other loops and the oracle)
    assert info['duplicates'] > 0
    for _ in range(2):
        again = _encode(xs16k, d32x16, '1', None, monkeypatch, **kw)
        assert again.variant.endswith('_wide')
        _same(first, again, 3)
