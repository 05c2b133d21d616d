"""MultilevelDictionaryLearner on the GPU, bit for bit against the same level loop written out from
the existing pieces with the dense hand-off: over a corpus (dense trainCorpus on .toarray() of every signal's last-level
matrix, then the batch hierarchical encode), and over one signal (the sequence of tools/learn_mlcsc.py: train,
encode / encodeFromLevel, todense)."""
import numpy as np
import pytest

import hsc_amd.synth as synth
from hsc_amd.dataset import MultilevelDictionary, addSingletonBases, scalesToWindowSizes
from hsc_amd.kmeans import ConvolutionalKMeansLearner
from hsc_amd.modeling import (HierarchicalConvolutionalMatchingPursuit, HierarchicalConvolutionalSparseCoder,
                              MultilevelDictionaryLearner)

pytestmark = pytest.mark.gpu

COUNTS, SCALES = [4, 3, 3], [8, 12, 20]
KMEANS = dict(nbRandomWindows=200, maxIterations=3, tolerance=0.0, resetMethod='random_samples')
ENCODE = dict(toleranceSnr=10, nbBlocks=4, singletonWeight=0.95)


def _corpus(B, T, dtype=np.float64, seed=2):
    D = synth.make_dictionary(4, 8, seed=seed, dtype=dtype)
    return synth.make_batch(D, T, 0, B, kind='planted', nb_atoms=max(8, T // 12), seed=seed, dtype=dtype)


def _dictionary_so_far(dictionaries, scales):
    if len(dictionaries) > 1:
        return MultilevelDictionary.fromRawDictionaries(addSingletonBases(dictionaries), np.asarray(scales)[:len(dictionaries)], hasSingletonBases=True)
    return MultilevelDictionary.fromRawDictionaries(dictionaries, np.asarray(scales)[:1])


def stepwise_corpus(sequences, method, seed):
    """The level loop with the dense hand-off.  Returns (raw dictionaries, nnz [level][signal] of the representations)."""
    rng = np.random.RandomState(seed)
    widths = scalesToWindowSizes(np.asarray(SCALES))
    hcmp = HierarchicalConvolutionalMatchingPursuit(method=method)
    dictionaries, nnz, inputs = [], [], sequences
    try:
        for level, (k, w) in enumerate(zip(COUNTS, widths)):
            dictionaries.append(ConvolutionalKMeansLearner(k, int(w), rng=rng).trainCorpus(inputs, **KMEANS))
            if level < len(COUNTS) - 1:
                mld = _dictionary_so_far(dictionaries, SCALES)
                coefficients = hcmp.computeCoefficientsBatch(sequences, mld, returnDistributed=False, **ENCODE)[0]
                nnz.append([c[-1].nnz for c in coefficients])
                inputs = [c[-1].toarray() for c in coefficients]
    finally:
        hcmp.close()
    return dictionaries, nnz


def stepwise_signal(signal, seed):
    """tools/learn_mlcsc.py with the device k-means and method='cmp', its generator handed over instead of seeded globally."""
    rng = np.random.RandomState(seed)
    widths = scalesToWindowSizes(np.asarray(SCALES))
    dictionaries, inp, coefficients = [], signal, None
    for level, (k, w) in enumerate(zip(COUNTS, widths)):
        dictionaries.append(ConvolutionalKMeansLearner(k, int(w), rng=rng).train(inp, **KMEANS))
        mld = _dictionary_so_far(dictionaries, SCALES)
        hcsc = HierarchicalConvolutionalSparseCoder(mld, HierarchicalConvolutionalMatchingPursuit(method='cmp'))
        if level == 0:
            coefficients, _ = hcsc.encode(signal, returnDistributed=False, **ENCODE)
        elif level < len(COUNTS) - 1:
            coefficients = hcsc.encodeFromLevel(signal, coefficients, returnDistributed=False, **ENCODE)
        inp = np.asarray(coefficients[-1].todense())
    return dictionaries


def _assert_dictionaries_equal(got, exp):
    assert len(got) == len(exp) == len(COUNTS)
    for level, (a, b) in enumerate(zip(got, exp)):
        assert a.dtype == b.dtype and a.shape == b.shape, level
        assert np.array_equal(a, b), level


@pytest.mark.parametrize('method', ['cmp', 'locomp'])
def test_corpus_equals_stepwise_pipeline_with_dense_handoff(method):
    x = _corpus(3, 512)
    learner = MultilevelDictionaryLearner(COUNTS, SCALES, method=method, rng=np.random.RandomState(6))
    mld = learner.trainCorpus(x, **dict(KMEANS, **ENCODE))
    exp, nnz = stepwise_corpus(x, method, 6)
    assert all(n > 0 for level in nnz for n in level) and [len(level) for level in nnz] == [3, 3]
    _assert_dictionaries_equal(learner.lastDictionaries, exp)
    ref = _dictionary_so_far(exp, SCALES)
    assert mld.getNbLevels() == 3
    for level in range(3):
        a, b = mld.getRawDictionary(level), ref.getRawDictionary(level)
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # the shapes of the reference's loop: level l >= 1 learns on the level below with its singleton bases
    assert [D.shape for D in exp] == [(4, 8), (3, 5, 4), (3, 9, 7)]
    stats = learner.lastStats
    assert len(stats) == 3 and [s['input_shape'] for s in stats] == [(3, 512), (3, 512, 4), (3, 512, 7)]
    assert [s['input_nnz'] for s in stats] == [None, sum(nnz[0]), sum(nnz[1])]
    assert [s['encode_nnz'] for s in stats] == [sum(nnz[0]), sum(nnz[1]), None]
    assert all(len(s['kmeans']) == 3 and s['setup_s'] > 0.0 and s['learn_s'] >= s['setup_s'] for s in stats)
    assert stats[0]['encode_s'] > 0.0 and stats[1]['encode_s'] > 0.0 and stats[2]['encode_s'] is None


def test_one_signal_equals_corpus_of_it_and_the_script_sequence():
    x = _corpus(1, 2000)[0]
    args = dict(KMEANS, **ENCODE)
    one = MultilevelDictionaryLearner(COUNTS, SCALES, method='cmp', rng=np.random.RandomState(3))
    one.train(x, **args)
    many = MultilevelDictionaryLearner(COUNTS, SCALES, method='cmp', rng=np.random.RandomState(3))
    many.trainCorpus(x[np.newaxis], **args)
    _assert_dictionaries_equal(one.lastDictionaries, many.lastDictionaries)
    _assert_dictionaries_equal(one.lastDictionaries, stepwise_signal(x, 3))
    assert all(s['encode_nnz'] > 0 for s in one.lastStats[:2])


def test_deterministic_and_float32_corpus():
    x = _corpus(2, 512, dtype=np.float32, seed=4)
    runs = []
    for _ in range(2):
        learner = MultilevelDictionaryLearner(COUNTS, SCALES, method='cmp', rng=np.random.RandomState(9))
        mld = learner.trainCorpus(x, **dict(KMEANS, **ENCODE))
        runs.append((learner.lastDictionaries, mld))
    _assert_dictionaries_equal(runs[0][0], runs[1][0])
    for level in range(3):
        assert np.array_equal(runs[0][1].getRawDictionary(level), runs[1][1].getRawDictionary(level))
    exp, nnz = stepwise_corpus(x, 'cmp', 9)
    _assert_dictionaries_equal(runs[0][0], exp)
    assert [D.dtype for D in exp] == [np.float32, np.float64, np.float64]
    assert all(n > 0 for level in nnz for n in level)
