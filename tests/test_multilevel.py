"""Sparse corpora for the k-means learner and MultilevelDictionaryLearner on the CPU: the new
symbol of libhsckmeans.so, the refusals raised before any device work, and the host side of the sparse path (draws,
'noise' bounds, initial atoms, reset patches) against the dense path on the numpy twin of the library.  The GPU side is
tests/test_gpu_kmeans_sparse.py and tests/test_gpu_multilevel.py."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse

from hsc_amd import _native
from hsc_amd import kmeans
from hsc_amd.kmeans import ConvolutionalKMeansLearner, SparseStack
from tests import kmeans_corpus_restatement as crst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the symbol
def test_sparse_entry_point_is_exported_and_declared():
    assert 'hsckmeans_set_corpus_sparse' in kmeans.EXPORTS
    header = open(os.path.join(ROOT, 'include', 'hsckmeans.h')).read()
    assert 'int hsckmeans_set_corpus_sparse(hsckmeans_ctx* ctx, int dtype, int B, const int64_t* row_offsets, int F,' in header
    if not os.path.isfile(kmeans.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = kmeans.load_library()
    fn = lib.hsckmeans_set_corpus_sparse
    assert len(fn.argtypes) == 11
    assert fn(*[0 if t is ctypes.c_int else None for t in fn.argtypes]) == -1
    assert lib.hsckmeans_last_error(None).decode() == 'hsckmeans_set_corpus_sparse: ctx is NULL'
    version = lib.hsckmeans_version
    version.restype = ctypes.c_int
    assert version() == 1


# ------------------------------------------------------------------------------------------------ refusals
class _DeviceTouched(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise _DeviceTouched()
    monkeypatch.setattr(kmeans, 'load_library', touched)
    monkeypatch.setattr(kmeans, '_context', touched)
    monkeypatch.setattr(_native, 'default_engine', touched)
    monkeypatch.setattr(_native, 'Engine', touched)


def _sparse_signals(dtype=np.float64, F=4, lens=(300, 45, 170), density=0.05, seed=3):
    rs = np.random.RandomState(seed)
    return [scipy.sparse.csr_matrix((rs.standard_normal((T, F)) * (rs.rand(T, F) < density)).astype(dtype)) for T in lens]


def test_sparse_corpus_refusals_before_any_device_call(no_device):
    good = _sparse_signals()
    L = ConvolutionalKMeansLearner
    state = np.random.get_state()
    with pytest.raises(ValueError, match='not a mix of both'):
        L(4, 8).trainCorpus([good[0], good[1].toarray(), good[2]], 50)
    with pytest.raises(ValueError, match='not a mix of both'):
        L(4, 8).trainCorpus((good[0].toarray(), good[1]), 50)
    with pytest.raises(ValueError, match='lengths='):
        L(4, 8).trainCorpus(good, 50, lengths=[300, 45, 170])
    with pytest.raises(ValueError, match='same F'):
        L(4, 8).trainCorpus([good[0], _sparse_signals(F=5)[1]], 50)
    with pytest.raises(ValueError, match='one dtype'):
        L(4, 8).trainCorpus([good[0], good[1].astype(np.float32)], 50)
    with pytest.raises(ValueError, match='float32 or float64'):
        L(4, 8).trainCorpus([m.astype(np.int64) for m in good], 50)
    # the other checks of check_corpus_arguments apply as they are
    with pytest.raises(ValueError, match='signal 1 has 45 samples'):
        L(4, 23).trainCorpus(good, 50)
    with pytest.raises(Exception, match='Unsupported reset method'):
        L(4, 8).trainCorpus(good, 50, resetMethod='bogus')
    with pytest.raises(NotImplementedError):
        L(4, 256).trainCorpus([scipy.sparse.csr_matrix((600, 4))], 50)
    # the element limit is the window stack's: N * 2W * F
    with pytest.raises(NotImplementedError, match='window stack'):
        L(4, 8).trainCorpus(good, (2 ** 31) // (16 * 4))
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:3], state[1:3]))    # nothing drawn
    with pytest.raises(_DeviceTouched):
        L(4, 8).trainCorpus(good, (2 ** 31 - 1) // (16 * 4))
    # ... not the corpus': 2 * 2^28 rows of 4 features are refused dense (tests/test_kmeans_corpus.py) and pass sparse
    big = [scipy.sparse.csr_matrix((2 ** 28, 4), dtype=np.float32)] * 2
    with pytest.raises(_DeviceTouched):
        L(4, 16).trainCorpus(big, 50)


def test_multilevel_learner_refusals_before_any_device_call(no_device):
    from hsc_amd.modeling import MultilevelDictionaryLearner
    from hsc_amd.multilevel import MultilevelDictionaryLearner as direct
    assert MultilevelDictionaryLearner is direct
    x = np.random.RandomState(0).standard_normal((3, 400))
    M = MultilevelDictionaryLearner
    state = np.random.get_state()
    with pytest.raises(NotImplementedError, match='computeCoefficientsBatch.* has no ragged form'):
        M([4, 3], [8, 12]).trainCorpus(list(x), 50)
    with pytest.raises(NotImplementedError, match='computeCoefficientsBatch.* has no ragged form'):
        M([4, 3], [8, 12]).trainCorpus(x, 50, lengths=[400, 300, 200])
    with pytest.raises(ValueError, match='3 counts for 2 scales'):
        M([4, 3, 3], [8, 12]).trainCorpus(x, 50)
    for method in ('mptk-mp', 'mptk-cmp'):
        with pytest.raises(NotImplementedError, match="needs the external MPTK toolkit, which this engine does not bind; use method='cmp' or 'locomp'"):
            M([4, 3], [8, 12], method=method).trainCorpus(x, 50)
    with pytest.raises(Exception, match='Unsupported sparse coding method'):
        M([4, 3], [8, 12], method='bogus').trainCorpus(x, 50)
    with pytest.raises(ValueError):
        M([4, 3], [8, 12]).trainCorpus(x[0], 50)                             # a corpus is [B,T(,F)]
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:3], state[1:3]))
    with pytest.raises(_DeviceTouched):
        M([4, 3], [8, 12]).trainCorpus(x, 50)
    with pytest.raises(_DeviceTouched):
        M([4, 3], [8, 12]).train(x[0], 50)


# ------------------------------------------------------------------------------------------------ host values
class FakeSparseContext(crst.FakeCorpusContext):
    """set_corpus_sparse on the numpy twin: the densified stack through set_corpus (a step's t is relative to the window
    either way)."""

    def set_corpus_sparse(self, indptr, indices, data, F, row_offsets, starts, W):
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and indptr[0] == 0 and indptr.shape[0] == row_offsets[-1] + 1
        dense = scipy.sparse.csr_matrix((data, indices, indptr), shape=(int(row_offsets[-1]), F)).toarray()
        self.sparse_calls = getattr(self, 'sparse_calls', 0) + 1
        self.set_corpus(dense, row_offsets, starts, W)


@pytest.fixture
def restated(monkeypatch):
    ctx = FakeSparseContext()
    monkeypatch.setattr(kmeans, '_contexts', {0: ctx})
    monkeypatch.setattr(kmeans, 'load_library', lambda: None)
    return ctx


class _Recording(object):
    """A RandomState that keeps what the learner draws and the bounds it asks uniform for."""

    def __init__(self, seed):
        self.rs, self.randints, self.uniforms = np.random.RandomState(seed), [], []

    def randint(self, *a, **k):
        v = self.rs.randint(*a, **k)
        self.randints.append(np.array(v))
        return v

    def uniform(self, low, high, size):
        self.uniforms.append((low, high))
        return self.rs.uniform(low=low, high=high, size=size)


@pytest.mark.parametrize('reset', kmeans.RESET_METHODS)
@pytest.mark.parametrize('init', kmeans.INIT_METHODS)
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_sparse_path_draws_and_values_equal_dense(dtype, init, reset, restated):
    """Data and generator seed per initMethod, so that a centroid is reset whatever the init: under 'noise' the entries
    are positive (the bounds are then the implicit 0 and the largest entry) and one of the all-positive atoms loses its
    members."""
    signals = _sparse_signals(dtype, F=3, lens=(120, 30, 75), density=0.04, seed=9)
    if init == 'noise':
        signals = [abs(m) for m in signals]
    seed = {'random_samples': 0, 'noise': 5}[init]
    dense = [m.toarray() for m in signals]
    kw = dict(nbRandomWindows=60, maxIterations=3, initMethod=init, resetMethod=reset, nbAveragedPatches=3)
    ra, rb = _Recording(seed), _Recording(seed)
    a = ConvolutionalKMeansLearner(5, 6, rng=ra)
    Da = a.trainCorpus(signals, **kw)
    assert restated.sparse_calls == 1
    b = ConvolutionalKMeansLearner(5, 6, rng=rb)
    Db = b.trainCorpus(dense, **kw)
    assert restated.sparse_calls == 1                                     # dense input takes the dense path
    assert Da.dtype == Db.dtype and Da.shape == Db.shape == (5, 6, 3) and np.array_equal(Da, Db)
    assert np.array_equal(a.lastWindows[0], b.lastWindows[0]) and np.array_equal(a.lastWindows[1], b.lastWindows[1])
    assert len(ra.randints) == len(rb.randints) and all(np.array_equal(p, q) for p, q in zip(ra.randints, rb.randints))
    assert len(ra.uniforms) == len(rb.uniforms)
    for (lo, hi), (lo2, hi2) in zip(ra.uniforms, rb.uniforms):
        assert lo == lo2 and hi == hi2 and type(lo) is type(lo2)
    for s, r in zip(a.lastStats, b.lastStats):
        assert s['nbResets'] == r['nbResets'] and np.array_equal(s['counts'], r['counts'])
        assert np.array_equal(s['assignment'][0], r['assignment'][0]) and np.array_equal(s['assignment'][1], r['assignment'][1])
    assert sum(s['nbResets'] for s in a.lastStats) > 0                    # reset patches were cut from the sparse rows
    if init == 'noise':
        assert ra.uniforms[0][0] == 0.0 and ra.uniforms[0][1] == max(m.data.max() for m in signals)
    # tuples and other sparse formats are the same corpus
    Dc = ConvolutionalKMeansLearner(5, 6, rng=np.random.RandomState(seed)).trainCorpus(tuple(m.tocsc() for m in signals), **kw)
    assert Dc.dtype == Da.dtype and np.array_equal(Dc, Da)


def test_noise_bounds_count_the_implicit_zeros():
    rs = np.random.RandomState(1)
    pos = scipy.sparse.csr_matrix(np.where(rs.rand(40, 3) < 0.1, rs.rand(40, 3) + 0.5, 0.0))
    neg = scipy.sparse.csr_matrix(-pos.toarray())
    full = scipy.sparse.csr_matrix(rs.rand(20, 3) + 0.5)                   # no implicit zero: the smallest entry is the minimum
    empty = scipy.sparse.csr_matrix((30, 3), dtype=np.float64)
    for mats in ([pos], [neg], [pos, neg], [full], [full, full], [full, pos], [empty], [empty, empty]):
        dense = np.concatenate([m.toarray() for m in mats])
        lo, hi = SparseStack(mats).bounds()
        assert lo == np.min(dense) and hi == np.max(dense) and lo.dtype == dense.dtype
    assert SparseStack([pos]).bounds()[0] == 0.0 and SparseStack([neg]).bounds()[1] == 0.0
    assert SparseStack([full]).bounds()[0] >= 0.5


def test_patches_and_csr_of_a_sparse_stack():
    mats = _sparse_signals(np.float32, F=3, lens=(20, 9, 14), density=0.3, seed=2)
    # an unsorted matrix with a duplicate entry: its entries are those of toarray()
    dup = scipy.sparse.csr_matrix((np.array([1.0, 2.0, 4.0], dtype=np.float32), np.array([2, 0, 2]), np.array([0, 3] + [3] * 8)), shape=(9, 3))
    assert not dup.has_canonical_format
    seqs = kmeans.sparse_corpus_signals([mats[0], dup, mats[2].tocoo()])
    assert dup.nnz == 3 and seqs[1].nnz == 2                               # the caller's matrix is left alone
    stack = SparseStack(seqs)
    dense = np.concatenate([mats[0].toarray(), dup.toarray(), mats[2].toarray()])
    assert stack.row_offsets.tolist() == [0, 20, 29, 43] and stack.dtype == np.float32 and stack.ndim == 2
    for s, e in ((0, 5), (15, 20), (20, 29), (29, 35), (38, 43)):
        p = stack[s:e]
        assert p.dtype == dense.dtype and np.array_equal(p, dense[s:e])
    with pytest.raises(AssertionError):
        stack[18:22]                                                       # no patch straddles two signals
    indptr, indices, data = stack.csr()
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    again = scipy.sparse.csr_matrix((data, indices, indptr), shape=dense.shape)
    assert np.array_equal(again.toarray(), dense)
    assert all(np.all(np.diff(indices[indptr[r]:indptr[r + 1]]) > 0) for r in range(dense.shape[0]))
    assert kmeans.sparse_corpus_signals([dense]) is None and kmeans.sparse_corpus_signals(dense) is None
