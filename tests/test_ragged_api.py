"""Ragged batches on the host side (no GPU): argument checks before any device call, the entry points without a ragged form,
and the C ABI of the two new entry points."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dictionary(K=8, W=16, F=1):
    rs = np.random.RandomState(0)
    D = rs.standard_normal((K, W, F)).astype(np.float32)
    D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
    return D if F > 1 else D[:, :, 0]


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to open a GPU context fails the test: the checks must come first."""
    from hsc_amd import _native

    def refuse(*a, **k):
        raise AssertionError('a device call was made before the arguments were checked')
    monkeypatch.setattr(_native, 'engine_for', refuse)
    monkeypatch.setattr(_native, 'default_engine', refuse)
    monkeypatch.setattr(_native, 'Engine', refuse)


def test_ragged_batch_pads_and_keeps_views():
    from hsc_amd.modeling import ragged_batch, is_ragged
    xs = [np.arange(20, dtype=np.float32), np.arange(33, dtype=np.float32) + 1.0]
    x, lens, seqs = ragged_batch(xs, None, np.float32, 16, 1)
    assert x.shape == (2, 33, 1) and list(lens) == [20, 33] and lens.dtype == np.int32
    assert np.array_equal(x[0, :20, 0], xs[0]) and not x[0, 20:].any()
    assert seqs[1] is not None and np.array_equal(seqs[1], xs[1])
    padded = np.full((2, 40), np.nan, dtype=np.float32)
    padded[0, :20] = xs[0]; padded[1, :33] = xs[1]
    x2, lens2, seqs2 = ragged_batch(padded, [20, 33], np.float32, 16, 1)
    assert x2.shape == (2, 33, 1) and list(lens2) == [20, 33]
    assert np.array_equal(x2, x) and not np.isnan(x2).any()   # (the padding of the caller's array is never copied)
    assert np.array_equal(seqs2[0], xs[0])
    assert is_ragged(xs) and is_ragged(tuple(xs)) and is_ragged(padded, [20, 33]) and not is_ragged(padded)


@pytest.mark.parametrize('bad, message', [
    (lambda: ([np.zeros(20, np.float32), np.zeros((30, 2), np.float32)], None), 'all be'),
    (lambda: ([np.zeros((20, 2), np.float32), np.zeros((30, 2), np.float32)], None), 'features'),
    (lambda: ([np.zeros(20, np.float32), np.zeros(15, np.float32)], None), 'signal 1'),
    (lambda: (np.zeros((2, 30), np.float32), [20, 31]), 'signal 1'),
    (lambda: (np.zeros((2, 30), np.float32), [20, 10]), 'shorter than the filters'),
    (lambda: (np.zeros((2, 30), np.float32), [20, 25, 30]), 'entries for 2 signals'),
    (lambda: ([np.zeros(20, np.float32)], [20]), 'padded array'),
    (lambda: ([], None), 'at least one'),
])
def test_checks_come_before_the_device(bad, message, no_engine):
    from hsc_amd.modeling import ConvolutionalMatchingPursuit
    seqs, lengths = bad()
    with pytest.raises(ValueError, match=message):
        ConvolutionalMatchingPursuit().computeCoefficientsBatch(seqs, _dictionary(), nbNonzeroCoefs=4, lengths=lengths)


def test_encode_batch_checks_through_the_coder(no_engine):
    from hsc_amd.modeling import ConvolutionalMatchingPursuit, ConvolutionalSparseCoder
    coder = ConvolutionalSparseCoder(_dictionary(F=3), ConvolutionalMatchingPursuit())
    with pytest.raises(ValueError, match='features'):
        coder.encodeBatch([np.zeros((40, 2), np.float32)], nbNonzeroCoefs=4)


def test_locomp_rejects_ragged(no_engine):
    from hsc_amd.locomp import LoCOMP
    xs = [np.zeros(40, np.float32), np.zeros(50, np.float32)]
    with pytest.raises(NotImplementedError, match='LoCOMP'):
        LoCOMP().computeCoefficientsBatch(xs, _dictionary(), nbNonzeroCoefs=4)
    with pytest.raises(NotImplementedError, match='LoCOMP'):
        LoCOMP().computeCoefficientsBatch(np.zeros((2, 50), np.float32), _dictionary(), nbNonzeroCoefs=4, lengths=[40, 50])


def test_hierarchical_rejects_ragged(no_engine):
    from hsc_amd.hierarchical import HierarchicalConvolutionalMatchingPursuit
    xs = [np.zeros(40, np.float32), np.zeros(50, np.float32)]
    for method in ('cmp', 'locomp'):
        with pytest.raises(NotImplementedError, match='levels >= 1'):
            HierarchicalConvolutionalMatchingPursuit(method=method).computeCoefficientsBatch(xs, None)
        with pytest.raises(NotImplementedError, match='levels >= 1'):
            HierarchicalConvolutionalMatchingPursuit(method=method).computeCoefficientsBatch(np.zeros((2, 50)), None, lengths=[40, 50])


def test_sharded_rejects_ragged(no_engine):
    from hsc_amd import parallel
    xs = [np.zeros(40, np.float32), np.zeros(50, np.float32)]
    with pytest.raises(NotImplementedError, match='gather'):
        parallel.encode_sharded(xs, _dictionary())
    with pytest.raises(NotImplementedError, match='gather'):
        parallel.encode_sharded(np.zeros((2, 50), np.float32), _dictionary(), lengths=[40, 50])


def test_batch_result_stays_compatible():
    from hsc_amd.modeling import BatchResult
    r = BatchResult([], np.zeros((0, 4)), [], None, None, 'v', [0, 0, 0, 0])
    assert r.lengths is None
    r = BatchResult([], [], [], None, None, 'v', [0, 0, 0, 0], lengths=np.array([3], np.int32))
    assert list(r.lengths) == [3]


def test_c_abi_declares_and_exports_the_ragged_entry_points():
    from hsc_amd import _native
    header = open(os.path.join(ROOT, 'include', 'hscmp.h')).read()
    for name in ('hscmp_encode_batch_ragged', 'hscmp_encode_batch_ragged_device'):
        assert name in _native.EXPORTS
        assert 'int %s(hscmp_ctx* ctx, const void* x' % name in header
    assert '#define HSCMP_VERSION 100' in header
    lib = _native.load_library()
    assert lib.hscmp_version() == 100
    x = np.zeros((2, 40, 1), np.float32)
    p = _native.make_params(nbNonzeroCoefs=4, eps=1e-7)
    # no context: an argument error, no device touched
    rc = lib.hscmp_encode_batch_ragged(None, x.ctypes.data_as(ctypes.c_void_p), 2, 40,
                                       np.array([20, 40], np.int32).ctypes.data_as(ctypes.c_void_p), ctypes.byref(p))
    assert rc == -1                                      # HSCMP_ERR_INVALID
    assert b'ctx is NULL' in lib.hscmp_last_error(None)
    rc = lib.hscmp_encode_batch_ragged_device(None, None, 2, 40, None, ctypes.byref(p))
    assert rc == -1
