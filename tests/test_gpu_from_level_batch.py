"""computeCoefficientsFromLevelBatch on the GPU: a hierarchy encoded one level at a time -- level 0 by computeCoefficientsBatch,
every further level from the coefficients in hand -- equals the uninterrupted computeCoefficientsBatch byte for byte:
matrices, residuals, residual energies, event records.  Shapes of tests/test_gpu_multilevel.py."""
import numpy as np
import pytest

import hsc_amd.synth as synth
from hsc_amd.dataset import MultilevelDictionary
from hsc_amd.modeling import (HierarchicalConvolutionalMatchingPursuit, HierarchicalConvolutionalSparseCoder,
                              MultilevelDictionaryLearner)

pytestmark = pytest.mark.gpu

COUNTS, SCALES = [4, 3, 3], [8, 12, 20]
KMEANS = dict(nbRandomWindows=200, maxIterations=3, tolerance=0.0, resetMethod='random_samples')
ENCODE = dict(toleranceSnr=10, nbBlocks=4, singletonWeight=0.95)
B, T = 3, 512


def _corpus(dtype=np.float64, seed=2):
    D = synth.make_dictionary(4, 8, seed=seed, dtype=dtype)
    return synth.make_batch(D, T, 0, B, kind='planted', nb_atoms=max(8, T // 12), seed=seed, dtype=dtype)


def _first_levels(mld, n):
    """The first n levels with the SAME raw dictionaries (upToLevel(n - 1) rebuilds those of the levels >= 1 from the
    decompositions, equal only to rounding: an encode with them is another encode)."""
    if n == 1:
        return mld.upToLevel(0)
    return MultilevelDictionary.fromRawDictionaries(mld.dictionaries[:n], np.asarray(mld.scales)[:n], hasSingletonBases=True)


@pytest.fixture(scope='module')
def case():
    """(corpus, 3-level dictionary learnt from it without the resumed path, one coder per method, cache of uninterrupted runs)"""
    x = _corpus()
    learner = MultilevelDictionaryLearner(COUNTS, SCALES, method='cmp', rng=np.random.RandomState(6))
    mld = learner.trainCorpus(x, resume=False, **dict(KMEANS, **ENCODE))
    assert mld.getNbLevels() == 3 and [mld.getRawDictionary(l).shape[0] for l in range(3)] == [4, 7, 10]
    for n in (1, 2):
        assert all(np.array_equal(_first_levels(mld, n).getRawDictionary(l), mld.getRawDictionary(l)) for l in range(n))
    coders = {m: HierarchicalConvolutionalMatchingPursuit(method=m) for m in ('cmp', 'locomp')}
    yield x, mld, coders, {}
    for c in coders.values():
        c.close()


def _uninterrupted(case, method, distributed, residuals='samples', mld=None):
    x, full, coders, cache = case
    key = (method, distributed, residuals, id(mld))
    if key not in cache:
        cache[key] = coders[method].computeCoefficientsBatch(x, mld or full, returnDistributed=distributed, returnEvents=True,
                                                             residuals=residuals, **ENCODE)
    return cache[key]


def _stepwise_inputs(case, method):
    """(level-0 coefficients, coefficients of levels 0..1 resumed from them), returnDistributed=False as the learner hands them on."""
    x, mld, coders, cache = case
    key = ('steps', method)
    if key not in cache:
        c0 = coders[method].computeCoefficientsBatch(x, mld.upToLevel(0), returnDistributed=False, **ENCODE)[0]
        c1, second, tm = coders[method].computeCoefficientsFromLevelBatch(x, c0, _first_levels(mld, 2), returnDistributed=False, **ENCODE)
        assert second is None and tm[0]['variant'] == 'loaded' and tm[1]['variant'] not in ('', 'loaded')
        cache[key] = (c0, c1)
    return cache[key]


def _same_matrices(got, exp):
    assert len(got) == len(exp) == B
    for b in range(B):
        assert len(got[b]) == len(exp[b])
        for l, (a, e) in enumerate(zip(got[b], exp[b])):
            a, e = a.tocsc(), e.tocsc()
            assert a.shape == e.shape and a.dtype == e.dtype, (b, l)
            assert np.array_equal(a.indptr, e.indptr) and np.array_equal(a.indices, e.indices), (b, l)
            assert a.data.tobytes() == e.data.tobytes(), (b, l)


def _same_events(got, exp):
    for b in range(B):
        assert got[b].dtype == exp[b].dtype and got[b].tobytes() == exp[b].tobytes(), b


@pytest.mark.parametrize('distributed', [True, False], ids=['distributed', 'last_level'])
@pytest.mark.parametrize('method', ['cmp', 'locomp'])
def test_level_by_level_equals_uninterrupted(case, method, distributed):
    x, mld, coders, _ = case
    c0, c1 = _stepwise_inputs(case, method)
    assert all(len(c) == 1 for c in c0) and all(len(c) == 2 and c[1].nnz > 0 for c in c1)
    # the intermediate hand-over is what an uninterrupted 2-level encode returns
    _same_matrices(c1, _uninterrupted(case, method, False, mld=_first_levels(mld, 2))[0])
    exp = _uninterrupted(case, method, distributed)
    got = coders[method].computeCoefficientsFromLevelBatch(x, c1, mld, returnDistributed=distributed, residuals='samples', returnEvents=True,
                                                           **ENCODE)
    _same_matrices(got[0], exp[0])
    assert got[1].shape == (B, T) and got[1].dtype == np.float64 and got[1].tobytes() == exp[1].tobytes()
    _same_events(got[3], exp[3])
    assert [t['variant'] for t in got[2][:2]] == ['loaded', 'loaded'] and got[2][2]['variant'] == exp[2][2]['variant']
    assert all(v == 0.0 for t in got[2][:2] for v in t['kernel_ms']) and got[2][2]['selections'] == exp[2][2]['selections'] > 0
    # the energies, summed on the device; and nothing but coefficients when no residuals are asked for
    energy = coders[method].computeCoefficientsFromLevelBatch(x, c1, mld, returnDistributed=distributed, residuals='energy', **ENCODE)[1]
    assert energy.tobytes() == _uninterrupted(case, method, distributed, residuals='energy')[1].tobytes()
    plain = coders[method].computeCoefficientsFromLevelBatch(x, c1, mld, returnDistributed=distributed, **ENCODE)
    assert len(plain) == 3 and plain[1] is None
    _same_matrices(plain[0], exp[0])


@pytest.mark.parametrize('method', ['cmp', 'locomp'])
def test_from_level_one_straight_to_the_last(case, method):
    """Two levels resumed at once: level 0 in hand, levels 1 and 2 encoded."""
    x, mld, coders, _ = case
    c0, _ = _stepwise_inputs(case, method)
    exp = _uninterrupted(case, method, True)
    got = coders[method].computeCoefficientsFromLevelBatch(x, c0, mld, residuals='samples', returnEvents=True, **ENCODE)
    _same_matrices(got[0], exp[0])
    assert got[1].tobytes() == exp[1].tobytes()
    _same_events(got[3], exp[3])
    assert [t['variant'] == 'loaded' for t in got[2]] == [True, False, False]


@pytest.mark.parametrize('kw', [dict(memoryBudget=1), dict(epilogue='host')], ids=['chunks_of_one', 'host_epilogue'])
def test_chunks_and_host_epilogue(case, kw):
    x, mld, coders, _ = case
    c0, c1 = _stepwise_inputs(case, 'cmp')
    exp = _uninterrupted(case, 'cmp', True)
    for given in (c0, c1):
        got = coders['cmp'].computeCoefficientsFromLevelBatch(x, given, mld, residuals='samples', returnEvents=True, **dict(ENCODE, **kw))
        _same_matrices(got[0], exp[0])
        assert np.asarray(got[1]).tobytes() == exp[1].tobytes()
        _same_events(got[3], exp[3])
        if 'memoryBudget' in kw:
            assert got[2][2]['chunks'] == B


def test_every_level_given_returns_the_postprocessed_input(case):
    x, mld, coders, _ = case
    last_only = _uninterrupted(case, 'cmp', False)
    exp = _uninterrupted(case, 'cmp', True)
    got = coders['cmp'].computeCoefficientsFromLevelBatch(x, last_only[0], mld, returnDistributed=True, residuals='samples', returnEvents=True,
                                                          **ENCODE)
    _same_matrices(got[0], exp[0])
    assert np.array_equal(got[1], exp[1])                 # (host residual: the same sums in the same order)
    _same_events(got[3], exp[3])
    assert [t['variant'] for t in got[2]] == ['loaded'] * 3


def test_signal_zero_equals_the_per_signal_entry(case):
    x, mld, coders, _ = case
    _, c1 = _stepwise_inputs(case, 'cmp')
    coder = HierarchicalConvolutionalSparseCoder(mld, coders['cmp'])
    batch = coder.encodeFromLevelBatch(x, c1, **ENCODE)[0]
    one = coder.encodeFromLevel(x[0], c1[0], **ENCODE)
    _same_matrices([batch[0]] * B, [one] * B)
    _same_matrices(batch, _uninterrupted(case, 'cmp', True)[0])
    _same_matrices(coder.encodeBatch(x, **ENCODE)[0], _uninterrupted(case, 'cmp', True)[0])


def test_float32_corpus_runs_level_zero_in_float32(case):
    x, mld, coders, _ = case
    x32 = _corpus(dtype=np.float32)
    mld32 = MultilevelDictionary.fromRawDictionaries([mld.dictionaries[0].astype(np.float32)] + list(mld.dictionaries[1:]), np.asarray(SCALES),
                                                     hasSingletonBases=True)
    hcmp = coders['cmp']
    exp = hcmp.computeCoefficientsBatch(x32, mld32, returnEvents=True, **ENCODE)
    assert hcmp._engines[0].dtype == np.float32
    c0 = hcmp.computeCoefficientsBatch(x32, mld32.upToLevel(0), returnDistributed=False, **ENCODE)[0]
    got = hcmp.computeCoefficientsFromLevelBatch(x32, c0, mld32, residuals='samples', returnEvents=True, **ENCODE)
    assert hcmp._engines[0].dtype == np.float32 and hcmp._engines[1].dtype == np.float64
    _same_matrices(got[0], exp[0])
    assert got[1].tobytes() == exp[1].tobytes()
    _same_events(got[3], exp[3])
