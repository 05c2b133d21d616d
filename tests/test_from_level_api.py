"""computeCoefficientsFromLevelBatch and Engine.load_level on the CPU: the refusals raised before any native call, and the
packing of the matrices into the arguments of hscmp_load_level with the library call stubbed.  The GPU side is
tests/test_gpu_load_level.py and tests/test_gpu_from_level_batch.py."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse

from hsc_amd import _native
from hsc_amd.dataset import MultilevelDictionary, addSingletonBases
from hsc_amd.modeling import HierarchicalConvolutionalMatchingPursuit, HierarchicalConvolutionalSparseCoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 96


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


def _levels(mld, L, T=T, seed=0):
    rs = np.random.RandomState(seed)
    return [scipy.sparse.random(T, mld.getRawDictionary(l).shape[0], density=0.05, format='csc', random_state=rs) for l in range(L)]


def test_declared_exported_and_named():
    header = open(os.path.join(ROOT, 'include', 'hscmp.h')).read()
    assert 'int hscmp_load_level(hscmp_ctx* ctx, const void* x, int B, int T, const int64_t* offsets, const int32_t* rows,' in header
    assert 'HSCMP_STOP_LOADED = 10' in header
    assert 'hscmp_load_level' in _native.EXPORTS
    assert _native.STOP_LOADED == 10 and _native.STOP_NAMES[10] == 'loaded'
    if not os.path.isfile(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _native.load_library()
    fn = lib.hscmp_load_level
    assert len(fn.argtypes) == 8
    assert fn(*[0 if t is ctypes.c_int else None for t in fn.argtypes]) == _native.ERR_INVALID
    assert lib.hscmp_last_error(None).decode() == 'hscmp_load_level: ctx is NULL'


def test_refusals_before_any_native_call(no_device):
    mld = _dictionary()
    assert [mld.getRawDictionary(l).shape[0] for l in range(3)] == [4, 7, 10]
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    call = hcmp.computeCoefficientsFromLevelBatch
    x = np.random.RandomState(0).standard_normal((3, T))
    good = [_levels(mld, 2, seed=b) for b in range(3)]
    with pytest.raises(ValueError, match='3 signals, but coefficients of 2'):
        call(x, good[:2], mld)
    with pytest.raises(ValueError, match='signal 1 has the coefficients of 1 levels, signal 0 of 2'):
        call(x, [good[0], good[1][:1], good[2]], mld)
    with pytest.raises(ValueError, match='signal 0 has the coefficients of 0 levels, outside 1 .. 3'):
        call(x, [[], good[1], good[2]], mld)
    with pytest.raises(ValueError, match='signal 0 has the coefficients of 4 levels, outside 1 .. 3'):
        call(x, [g + g for g in good], mld)
    with pytest.raises(ValueError, match=r'signal 1: the matrix of level 1 must be sparse with shape \(96, 7\), got \(96, 4\)'):
        call(x, [good[0], [good[1][0], good[1][0]], good[2]], mld)
    with pytest.raises(ValueError, match=r'signal 2: the matrix of level 1 must be sparse with shape \(96, 7\), got \(95, 7\)'):
        call(x, [good[0], good[1], _levels(mld, 2, T=95)], mld)
    with pytest.raises(ValueError, match='signal 0: the matrix of level 1 must be sparse'):
        call(x, [[good[0][0], good[0][1].toarray()], good[1], good[2]], mld)
    # only the last matrix is read (modeling.py:1494-1500): a lower level of another shape is no refusal
    with pytest.raises(NotImplementedError, match='computeCoefficientsFromLevelBatch has no ragged form'):
        call(list(x), good, mld)
    with pytest.raises(_DeviceTouched):
        call(x, [[None, g[1]] for g in good], mld)
    # the coder's wrappers hand the same arguments on
    coder = HierarchicalConvolutionalSparseCoder(mld, hcmp)
    with pytest.raises(ValueError, match='3 signals, but coefficients of 2'):
        coder.encodeFromLevelBatch(x, good[:2])
    with pytest.raises(_DeviceTouched):
        coder.encodeFromLevelBatch(x, good)
    with pytest.raises(_DeviceTouched):
        coder.encodeBatch(x)


def test_all_levels_given_needs_no_device(no_device):
    """L == nbLevels encodes nothing: the post-processed input, on the host."""
    mld = _dictionary()
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    x = np.random.RandomState(0).standard_normal((2, T))
    given = [_levels(mld, 3, seed=b) for b in range(2)]
    for distributed in (True, False):
        coefs, second, timings = hcmp.computeCoefficientsFromLevelBatch(x, given, mld, returnDistributed=distributed)
        assert second is None and [t['variant'] for t in timings] == ['loaded'] * 3
        for b in range(2):
            exp = hcmp._postprocessCoefficients(given[b], mld, distributed)
            assert len(coefs[b]) == 3
            for a, e in zip(coefs[b], exp):
                assert a.shape == e.shape and (a != e).nnz == 0
    coefs, residual, _, events = hcmp.computeCoefficientsFromLevelBatch(x, given, mld, residuals='samples', returnEvents=True)
    assert residual.shape == (2, T) and len(events) == 2
    exp = hcmp._calculateResidual(x[1], coefs[1], mld)
    assert np.array_equal(residual[1], exp)
    energy = hcmp.computeCoefficientsFromLevelBatch(x, given, mld, residuals='energy', epilogue='device')[1]
    assert energy.shape == (2,) and energy[1] == np.sum(np.square(exp))


class _StubLib(object):
    """hscmp_load_level recorded instead of run."""

    def __init__(self):
        self.calls = []

    def hscmp_load_level(self, h, x, B, T, offsets, rows, cols, data):
        def arr(p, n, ct):
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape=(n,)).copy() if n else np.zeros(0)
        off = arr(offsets, B + 1, ctypes.c_int64)
        n = int(off[-1])
        self.calls.append(dict(x=x, B=B, T=T, offsets=off, rows=arr(rows, n, ctypes.c_int32), cols=arr(cols, n, ctypes.c_int32),
                               data=arr(data, n, ctypes.c_double)))
        return 0


def _stub_engine(K, F=1, dtype=np.float64):
    eng = _native.Engine.__new__(_native.Engine)
    eng._lib, eng._h, eng.K, eng.F, eng.dtype, eng._batch = _StubLib(), None, K, F, np.dtype(dtype), None
    return eng


def test_load_level_packs_canonical_csc():
    K, T_ = 5, 40
    # unsorted COO with one duplicate pair, (7, 3) twice, and an explicit zero
    rows = np.array([30, 7, 2, 7, 11, 2, 9])
    cols = np.array([4, 3, 4, 3, 0, 1, 2])
    vals = np.array([1.5, 2.0, -0.5, 0.25, 3.0, -1.0, 0.0])
    m0 = scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(T_, K))
    kept = (m0.row.copy(), m0.col.copy(), m0.data.copy())
    empty = scipy.sparse.csr_matrix((T_, K))
    m2 = scipy.sparse.lil_matrix((T_, K), dtype=np.float32)
    m2[39, 0] = 1.0; m2[0, 0] = 2.0; m2[5, 4] = -3.0
    eng = _stub_engine(K)
    eng.load_level(None, T_, [m0, empty, m2])
    assert eng._batch == (3, T_, 5)
    call = eng._lib.calls[0]
    assert call['x'] is None and (call['B'], call['T']) == (3, T_)
    assert call['offsets'].tolist() == [0, 5, 5, 8]              # the pair summed, the zero dropped; an empty range
    assert call['cols'].tolist() == [0, 1, 3, 4, 4, 0, 0, 4]
    assert call['rows'].tolist() == [11, 2, 7, 2, 30, 0, 39, 5]
    assert call['data'].tolist() == [3.0, -1.0, 2.25, -0.5, 1.5, 2.0, 1.0, -3.0]
    assert call['data'].dtype == np.float64 and call['rows'].dtype == np.int32 and call['cols'].dtype == np.int32
    for b in range(3):                                           # strictly ascending (col, row) inside every signal
        lo, hi = call['offsets'][b], call['offsets'][b + 1]
        key = call['cols'][lo:hi].astype(np.int64) * T_ + call['rows'][lo:hi]
        assert np.all(np.diff(key) > 0)
    # the caller's matrices are untouched
    assert all(np.array_equal(a, b) for a, b in zip((m0.row, m0.col, m0.data), kept)) and m2.dtype == np.float32
    # all empty: cap is 1
    eng.load_level(None, T_, [empty, empty])
    assert eng._batch == (2, T_, 1) and eng._lib.calls[1]['offsets'].tolist() == [0, 0, 0]
    # the signals travel as [B, T, F] in the engine's dtype
    eng32 = _stub_engine(K, F=1, dtype=np.float32)
    eng32.load_level(np.ones((2, T_, 1)), T_, [empty, m2])
    assert eng32._lib.calls[0]['x'] is not None and eng32._batch == (2, T_, 3)
    with pytest.raises(ValueError, match=r'signal 1: expected a sparse matrix of shape \(40, 5\)'):
        eng.load_level(None, T_, [empty, scipy.sparse.csr_matrix((T_, K + 1))])
    with pytest.raises(ValueError, match='signal 0: expected a sparse matrix'):
        eng.load_level(None, T_, [np.zeros((T_, K))])
