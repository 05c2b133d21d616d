"""MultilevelDictionaryLearner.trainCorpus(resume=True): from level 1 on the hand-off encode carries on from the previous
pass's coefficients and runs the new level only.  The dictionaries equal those of resume=False (every level below encoded
again) bit for bit, and the resumed encodes report the levels below as not run."""
import numpy as np
import pytest

import hsc_amd.synth as synth
from hsc_amd.modeling import MultilevelDictionaryLearner

pytestmark = pytest.mark.gpu

KMEANS = dict(nbRandomWindows=200, maxIterations=3, tolerance=0.0, resetMethod='random_samples')
ENCODE = dict(toleranceSnr=10, nbBlocks=4, singletonWeight=0.95)
SHAPES = {'three_levels': ([4, 3, 3], [8, 12, 20], 512), 'four_levels': ([4, 3, 3, 3], [8, 12, 20, 28], 768)}


def _corpus(B, T, seed=2):
    D = synth.make_dictionary(4, 8, seed=seed, dtype=np.float64)
    return synth.make_batch(D, T, 0, B, kind='planted', nb_atoms=max(8, T // 12), seed=seed, dtype=np.float64)


@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('method', ['cmp', 'locomp'])
def test_resumed_learner_equals_the_full_reencode(method, shape):
    counts, scales, T = SHAPES[shape]
    n = len(counts)
    x = _corpus(3, T)
    runs = {}
    for resume in (True, False):
        learner = MultilevelDictionaryLearner(counts, scales, method=method, rng=np.random.RandomState(6))
        mld = learner.trainCorpus(x, resume=resume, **dict(KMEANS, **ENCODE))
        runs[resume] = (learner.lastDictionaries, mld, learner.lastStats)
    (da, ma, sa), (db, mb, sb) = runs[True], runs[False]
    assert len(da) == len(db) == n and ma.getNbLevels() == mb.getNbLevels() == n
    for level in range(n):
        assert da[level].dtype == db[level].dtype and np.array_equal(da[level], db[level]), level
        a, b = ma.getRawDictionary(level), mb.getRawDictionary(level)
        assert a.dtype == b.dtype and np.array_equal(a, b), level
    assert [s['encode_nnz'] for s in sa] == [s['encode_nnz'] for s in sb] and all(v > 0 for v in [s['encode_nnz'] for s in sa][:-1])
    assert sorted(sa[0]) == sorted(sb[0])                   # the same keys either way
    for level in range(n - 1):
        ta, tb = sa[level]['encode_timings'], sb[level]['encode_timings']
        assert len(ta) == len(tb) == level + 1 and sa[level]['encode_s'] > 0.0
        # resumed: the levels below are not run again; the full re-encode runs every level
        assert [t['variant'] == 'loaded' for t in ta] == [l < level for l in range(level + 1)]
        assert all(t['variant'] != 'loaded' and t['selections'] > 0 for t in tb)
        assert all(sum(t['kernel_ms']) == 0.0 and t['selections'] == 0 for t in ta[:level])
        assert ta[level]['selections'] == tb[level]['selections'] > 0
    assert sa[n - 1]['encode_timings'] is None and sa[n - 1]['encode_s'] is None


def test_resume_is_the_default():
    import inspect
    assert inspect.signature(MultilevelDictionaryLearner.trainCorpus).parameters['resume'].default is True
