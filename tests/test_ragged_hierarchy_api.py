"""The ragged entry points of the hierarchy on the CPU: argument checks raised before any device call, the C ABI of
hscmp_load_level_ragged, and the old entry points' refusals.  The GPU side is tests/test_gpu_ragged_levels.py and
tests/test_gpu_ragged_hierarchy.py."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse

from hsc_amd import _native
from hsc_amd.dataset import MultilevelDictionary, addSingletonBases
from hsc_amd.modeling import (HierarchicalConvolutionalMatchingPursuit, HierarchicalConvolutionalSparseCoder,
                              MultilevelDictionaryLearner)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _DeviceTouched(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise _DeviceTouched()
    monkeypatch.setattr(_native, 'load_library', touched)
    monkeypatch.setattr(_native, 'default_engine', touched)
    monkeypatch.setattr(_native, 'Engine', touched)


def _dictionary():
    rs = np.random.RandomState(1)
    raw = [rs.standard_normal((4, 8)), rs.standard_normal((3, 5, 4)), rs.standard_normal((3, 9, 7))]
    return MultilevelDictionary.fromRawDictionaries(addSingletonBases(raw), np.asarray([8, 12, 20]), hasSingletonBases=True)


def _signals(lengths, seed=0):
    rs = np.random.RandomState(seed)
    return [rs.standard_normal(n) for n in lengths]


def _levels(mld, L, T, seed=0):
    rs = np.random.RandomState(seed)
    return [scipy.sparse.random(T, mld.getRawDictionary(l).shape[0], density=0.05, format='csc', random_state=rs) for l in range(L)]


def test_declared_exported_and_named():
    header = open(os.path.join(ROOT, 'include', 'hscmp.h')).read()
    assert 'int hscmp_load_level_ragged(hscmp_ctx* ctx, const void* x, int B, int T, const int32_t* lengths, const int64_t* offsets,' in header
    assert 'hscmp_load_level_ragged' in _native.EXPORTS
    if not os.path.isfile(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _native.load_library()
    fn = lib.hscmp_load_level_ragged
    assert len(fn.argtypes) == 9
    assert fn(*[0 if t is ctypes.c_int else None for t in fn.argtypes]) == _native.ERR_INVALID
    assert lib.hscmp_last_error(None).decode() == 'hscmp_load_level_ragged: ctx is NULL'
    # the uniform entry keeps its own name in its messages
    fn = lib.hscmp_load_level
    assert fn(*[0 if t is ctypes.c_int else None for t in fn.argtypes]) == _native.ERR_INVALID
    assert lib.hscmp_last_error(None).decode() == 'hscmp_load_level: ctx is NULL'


def test_ragged_batch_checks_before_any_native_call(no_device):
    mld = _dictionary()
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    xs = _signals([96, 40, 9])
    with pytest.raises(ValueError, match='uniform batch: use computeCoefficientsBatch'):
        hcmp.computeCoefficientsRaggedBatch(np.zeros((3, 96)), mld)
    # every signal at least as long as the widest filter of the levels that run (8, 5, 9): signal, length, width
    with pytest.raises(ValueError, match=r'signal 2: length 8 is shorter than the filters \(W=9\)'):
        hcmp.computeCoefficientsRaggedBatch(_signals([96, 40, 8]), mld)
    with pytest.raises(ValueError, match=r'signal 1: length 7 is shorter than the filters \(W=8\)'):
        hcmp.computeCoefficientsRaggedBatch(_signals([96, 7]), mld.upToLevel(0))
    with pytest.raises(ValueError, match='lengths= goes with a padded array'):
        hcmp.computeCoefficientsRaggedBatch(xs, mld, lengths=[96, 40, 9])
    with pytest.raises(ValueError, match='signal 1: length 97 beyond the padded length 96'):
        hcmp.computeCoefficientsRaggedBatch(np.zeros((2, 96)), mld, lengths=[96, 97])
    with pytest.raises(ValueError, match='signal 0 has 2 features, the dictionary 1'):
        hcmp.computeCoefficientsRaggedBatch([np.zeros((40, 2))], mld)
    with pytest.raises(NotImplementedError, match='LoCOMP loop has no ragged form'):
        HierarchicalConvolutionalMatchingPursuit(method='locomp').computeCoefficientsRaggedBatch(xs, mld)
    with pytest.raises(_DeviceTouched):
        hcmp.computeCoefficientsRaggedBatch(xs, mld)
    with pytest.raises(_DeviceTouched):
        hcmp.computeCoefficientsRaggedBatch(np.zeros((2, 96)), mld, lengths=[96, 9])
    coder = HierarchicalConvolutionalSparseCoder(mld, hcmp)
    with pytest.raises(ValueError, match='uniform batch: use computeCoefficientsBatch'):
        coder.encodeRaggedBatch(np.zeros((3, 96)))
    with pytest.raises(_DeviceTouched):
        coder.encodeRaggedBatch(xs)


def test_ragged_from_level_checks_before_any_native_call(no_device):
    mld = _dictionary()
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    call = hcmp.computeCoefficientsFromLevelRaggedBatch
    lengths = [96, 40, 9]
    xs = _signals(lengths)
    good = [_levels(mld, 2, n, seed=b) for b, n in enumerate(lengths)]
    with pytest.raises(ValueError, match='uniform batch: use computeCoefficientsFromLevelBatch'):
        call(np.zeros((3, 96)), good, mld)
    with pytest.raises(ValueError, match='3 signals, but coefficients of 2'):
        call(xs, good[:2], mld)
    with pytest.raises(ValueError, match='signal 1 has the coefficients of 1 levels, signal 0 of 2'):
        call(xs, [good[0], good[1][:1], good[2]], mld)
    with pytest.raises(ValueError, match='signal 0 has the coefficients of 0 levels, outside 1 .. 3'):
        call(xs, [[], good[1], good[2]], mld)
    # the matrices against (T_b, K_{L-1})
    with pytest.raises(ValueError, match=r'signal 1: the matrix of level 1 must be sparse with shape \(40, 7\), got \(96, 7\)'):
        call(xs, [good[0], good[0], good[2]], mld)
    with pytest.raises(ValueError, match=r'signal 2: the matrix of level 1 must be sparse with shape \(9, 7\), got \(9, 4\)'):
        call(xs, [good[0], good[1], [good[2][0], good[2][0]]], mld)
    # only the levels that will run count for the width: level 0 in hand, levels 1 (W=5) and 2 (W=9) run
    short = _signals([96, 8])
    with pytest.raises(ValueError, match=r'signal 1: length 8 is shorter than the filters \(W=9\)'):
        call(short, [_levels(mld, 1, 96), _levels(mld, 1, 8)], mld)
    with pytest.raises(NotImplementedError, match='LoCOMP loop has no ragged form'):
        HierarchicalConvolutionalMatchingPursuit(method='locomp').computeCoefficientsFromLevelRaggedBatch(xs, good, mld)
    with pytest.raises(_DeviceTouched):
        call(xs, good, mld)
    with pytest.raises(_DeviceTouched):
        HierarchicalConvolutionalSparseCoder(mld, hcmp).encodeFromLevelRaggedBatch(xs, good)


def test_all_levels_given_needs_no_device(no_device):
    """L == nbLevels encodes nothing: the post-processed input per signal, residuals of the signals' own lengths."""
    mld = _dictionary()
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    lengths = [96, 40]
    xs = _signals(lengths)
    given = [_levels(mld, 3, n, seed=b) for b, n in enumerate(lengths)]
    coefs, residual, timings = hcmp.computeCoefficientsFromLevelRaggedBatch(xs, given, mld, residuals='samples')
    assert [t['variant'] for t in timings] == ['loaded'] * 3
    for b, n in enumerate(lengths):
        exp = hcmp._postprocessCoefficients(given[b], mld, True)
        for a, e in zip(coefs[b], exp):
            assert a.shape == e.shape and a.shape[0] == n and (a != e).nnz == 0
        assert residual[b].shape == (n,) and np.array_equal(residual[b], hcmp._calculateResidual(xs[b], coefs[b], mld))
    energy = hcmp.computeCoefficientsFromLevelRaggedBatch(xs, given, mld, residuals='energy')[1]
    assert energy.shape == (2,) and energy[1] == np.sum(np.square(residual[1]))


def test_train_ragged_corpus_checks_before_any_native_call(no_device, monkeypatch):
    import hsc_amd.kmeans as kmeans

    def touched(*a, **k):
        raise _DeviceTouched()
    monkeypatch.setattr(kmeans.ConvolutionalKMeansLearner, 'trainCorpus', touched)
    learner = MultilevelDictionaryLearner([4, 3, 3], [8, 12, 20], method='cmp')
    with pytest.raises(ValueError, match='uniform corpus: use trainCorpus'):
        learner.trainRaggedCorpus(np.zeros((3, 96)), 10)
    with pytest.raises(ValueError, match=r'signal 1: length 8 is shorter than the widest filter of the levels \(W=9\)'):
        learner.trainRaggedCorpus(_signals([96, 8]), 10)
    with pytest.raises(ValueError, match='lengths= goes with a padded array'):
        learner.trainRaggedCorpus(_signals([96, 40]), 10, lengths=[96, 40])
    with pytest.raises(NotImplementedError, match='LoCOMP loop has no ragged form'):
        MultilevelDictionaryLearner([4, 3, 3], [8, 12, 20], method='locomp').trainRaggedCorpus(_signals([96, 40]), 10)
    with pytest.raises(_DeviceTouched):
        learner.trainRaggedCorpus(_signals([96, 40]), 10)
    with pytest.raises(_DeviceTouched):
        learner.trainRaggedCorpus(np.zeros((2, 96)), 10, lengths=[96, 40])


def test_old_entry_points_still_refuse_with_their_text(no_device):
    mld = _dictionary()
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    xs = _signals([96, 40])
    with pytest.raises(NotImplementedError, match='computeCoefficientsBatch.* has no ragged form.*computeCoefficientsRaggedBatch'):
        hcmp.computeCoefficientsBatch(xs, mld)
    with pytest.raises(NotImplementedError, match='computeCoefficientsFromLevelBatch has no ragged form.*computeCoefficientsFromLevelRaggedBatch'):
        hcmp.computeCoefficientsFromLevelBatch(xs, [_levels(mld, 1, 96), _levels(mld, 1, 40)], mld)
    with pytest.raises(NotImplementedError, match='computeCoefficientsBatch.* has no ragged form.*trainRaggedCorpus'):
        MultilevelDictionaryLearner([4, 3], [8, 12], method='cmp').trainCorpus(xs, 10)


class _StubLib(object):
    def __init__(self):
        self.calls = []

    def hscmp_load_level_ragged(self, h, x, B, T, lengths, offsets, rows, cols, data):
        lens = np.ctypeslib.as_array(ctypes.cast(lengths, ctypes.POINTER(ctypes.c_int32)), shape=(B,)).copy()
        off = np.ctypeslib.as_array(ctypes.cast(offsets, ctypes.POINTER(ctypes.c_int64)), shape=(B + 1,)).copy()
        self.calls.append(dict(B=B, T=T, lengths=lens, offsets=off))
        return 0


def test_load_level_ragged_packs_per_signal_shapes():
    K = 5
    eng = _native.Engine.__new__(_native.Engine)
    eng._lib, eng._h, eng.K, eng.F, eng.dtype, eng._batch = _StubLib(), None, K, 1, np.dtype(np.float64), None
    ms = [scipy.sparse.random(n, K, density=0.3, format='csr', random_state=np.random.RandomState(n)) for n in (40, 17)]
    eng.load_level_ragged(None, 40, [40, 17], ms)
    call = eng._lib.calls[0]
    assert (call['B'], call['T']) == (2, 40) and call['lengths'].tolist() == [40, 17] and call['lengths'].dtype == np.int32
    assert call['offsets'].tolist() == [0, ms[0].nnz, ms[0].nnz + ms[1].nnz]
    assert eng._batch == (2, 40, max(m.nnz for m in ms))
    with pytest.raises(ValueError, match=r'signal 1: expected a sparse matrix of shape \(17, 5\)'):
        eng.load_level_ragged(None, 40, [40, 17], [ms[0], ms[0]])
