"""Stop rules per signal through the level kernels: multi-feature float64 inputs on the sparse plans, and
K-SVD learning over a ragged corpus with an nbNonzeroCoefs per signal.

The problems are those of tests/test_gpu_ragged_levels.py at its shapes (F = 24, K = 36, W = 8, lengths from W to 512) with denser
inputs, so that the longer signals need tens of atoms and stop at different places under the values below.  Per signal and bit for
bit, the rules batch must equal the same engine's encode of the signal alone with its scalars, and the CPU oracle."""
import numpy as np
import pytest

from tests.test_gpu_ragged_levels import F64, LENGTHS, W8, _all_results, _check_against_oracle, _level_dictionary, _level_input, _padded, _same

pytestmark = pytest.mark.gpu

L0 = [1, 3, 2, 20, 60, 33]
SNR = [12.0, 5.0, 8.0, 25.0, 12.0, 5.0]
GATHERED = {'HSCMP_NO_DICT_LISTS': '1', 'HSCMP_FORCE_GATHERED': '1'}

# name: (env, the shared arguments, the arguments per signal)
ROWS = {
    'plain_l0': ({}, {}, dict(nbNonzeroCoefs=L0)),
    'plain_blocked_snr': ({}, dict(nbBlocks=4), dict(toleranceSnr=SNR)),
    'packed_l0': ({'HSCMP_SPARSE_PACKED': '1'}, {}, dict(nbNonzeroCoefs=L0)),
    'not_packed_l0': ({'HSCMP_SPARSE_PACKED': '0'}, {}, dict(nbNonzeroCoefs=L0)),
    'packed_blocked_snr': ({'HSCMP_SPARSE_PACKED': '1', 'HSCMP_RP': '0'}, dict(nbBlocks=4), dict(toleranceSnr=SNR)),
    'not_packed_blocked_snr': ({'HSCMP_SPARSE_PACKED': '0', 'HSCMP_RP': '0'}, dict(nbBlocks=4), dict(toleranceSnr=SNR)),
    'rp_blocked_snr': ({'HSCMP_RP': '1'}, dict(nbBlocks=4), dict(toleranceSnr=SNR)),
    'rp_auto_blocks_l0_and_snr': ({'HSCMP_RP': '1'}, dict(nbBlocks='auto'), dict(nbNonzeroCoefs=L0, toleranceSnr=SNR)),
    'no_rp_blocked_l0_and_snr': ({'HSCMP_RP': '0'}, dict(nbBlocks=4), dict(nbNonzeroCoefs=L0, toleranceSnr=SNR)),
    'gathered_l0': (GATHERED, {}, dict(nbNonzeroCoefs=L0)),
    'gathered_blocked_snr': (GATHERED, dict(nbBlocks=4), dict(toleranceSnr=SNR)),
}

_PROBLEM = []


def _problem():
    if not _PROBLEM:
        D = _level_dictionary(1, 24, 12, W8, F64)
        _PROBLEM.append(([_level_input(100 + b, n, D, density=0.25) for b, n in enumerate(LENGTHS)], D))
    return _PROBLEM[0]


def _signal_kw(name, b):
    _, shared, per_signal = ROWS[name]
    kw = dict(shared)
    kw.update((key, vals[b]) for key, vals in per_signal.items())
    return kw


def test_rules_level_rows(monkeypatch):
    """Every row above, each under its own environment; every failing row is named at the end."""
    failed = []
    for name in sorted(ROWS):
        with monkeypatch.context() as m:
            try:
                _rules_level_row(name, m)
            except AssertionError as e:
                failed.append('%s: %s' % (name, (str(e).splitlines() or [repr(e)])[0]))
    assert not failed, '%d of %d rows failed:\n%s' % (len(failed), len(ROWS), '\n'.join(failed))


def _rules_level_row(name, monkeypatch):
    from hsc_amd import _native
    from oracle import hsc_oracle as orc
    env, shared, per_signal = ROWS[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    xs, D = _problem()
    x, lens = _padded(xs)
    eps = float(np.finfo(F64).eps)
    K = D.shape[0]
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D)
        eng.encode_batch_ragged(x, lens, _native.make_params(eps=eps, maxEvents=2048, **_signal_kw(name, 3)))
        ragged_variant = eng.last_variant()
        assert ragged_variant.startswith(('sparse_init', 'dictlist_init')) and ragged_variant.endswith('_ragged')
        if 'HSCMP_RP' in env:
            assert ragged_variant.endswith('_rp_ragged') == (env['HSCMP_RP'] == '1')
        assert ('gathered' in ragged_variant) == (env is GATHERED)
        eng.encode_batch_rules(x, lens, _native.make_rules(len(xs), **per_signal), _native.make_params(eps=eps, maxEvents=2048, **shared))
        assert eng.last_variant() == ragged_variant + '_rules'
        got, raw = _all_results(eng, lens)
        for b, Tb in enumerate(lens):
            assert not raw[b, Tb:].any(), 'the residual above the signal length is not zero'
        assert len(set(len(g['t']) for g in got[3:])) == 3, 'the three long signals stop at the same place'
        for b, s in enumerate(xs):
            kw = _signal_kw(name, b)
            eng.encode_batch(s[np.newaxis], _native.make_params(eps=eps, maxEvents=2048, **kw))
            one, _ = _all_results(eng, [len(s)])
            _same(got[b], one[0])
            _check_against_oracle(got[b], orc.cmp_encode(s, D, **kw), len(s), K)
    finally:
        eng.close()


def test_ksvd_train_corpus_with_an_l0_per_signal():
    """trainCorpus(method='cmp', nbNonzeroCoefs=[...]) on a ragged corpus of three signals: the dictionary of a hand-written loop
    that encodes every signal alone with its scalar and calls update_corpus, bit for bit."""
    import hsc_amd.synth as synth
    from hsc_amd import ksvd
    from hsc_amd.ksvd import ConvolutionalKSVDLearner
    from hsc_amd.modeling import ConvolutionalMatchingPursuit
    K, W, iterations = 6, 16, 2
    D_true = synth.make_dictionary(K, W, seed=3, dtype=F64)
    lengths = [600, 251, 400]
    l0 = np.array([n // 25 for n in lengths])             # L0 follows the length: 24, 10, 16
    xs = [synth.make_signal(D_true, n, i, kind='planted', nb_atoms=n // 20, noise=0.05, seed=3, dtype=F64) for i, n in enumerate(lengths)]

    np.random.seed(7)
    learner = ConvolutionalKSVDLearner(K, W)
    D = learner.trainCorpus(xs, method='cmp', maxIterations=iterations, nbNonzeroCoefs=l0, toleranceSnr=40.0)
    assert all(s['variant'].endswith('_ragged_rules') for s in learner.lastStats) and len(learner.lastStats) == iterations

    np.random.seed(7)
    by_hand = ConvolutionalKSVDLearner(K, W)
    D_ref = by_hand._initial_D(np.concatenate(xs), by_hand.rng)
    single = ConvolutionalMatchingPursuit()
    nnz = []
    for it in range(iterations):
        codes = [single.computeCoefficients(x, D_ref, nbNonzeroCoefs=int(l0[b]), toleranceSnr=40.0)[0] for b, x in enumerate(xs)]
        # (the rule is each signal's own: on the drawn dictionary every signal stops on ITS nbNonzeroCoefs, far from the 40 dB)
        assert it > 0 or [c.nnz for c in codes] == list(l0)
        D_ref, updated = ksvd.update_corpus(D_ref, codes, False, 0)[:2]
        nnz.append(sum(c.nnz for c in updated))
    assert np.array_equal(D, D_ref)
    assert [s['nnz'] for s in learner.lastStats] == nnz
