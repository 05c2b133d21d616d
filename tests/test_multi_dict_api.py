"""CPU-side checks of the dictionary-per-signal surface: the new entry points of libhscmp.so and
libhscksvd.so are declared, exported and listed, answer a null context as documented, and every argument error of the Python
layer is raised before a library is touched (no GPU needed: the -m gpu tiers are tests/test_gpu_multi_dict.py and
tests/test_gpu_ksvd_batch.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {'hscmp': ('_native', ['hscmp_set_dictionaries', 'hscmp_encode_batch_multi']),
       'hscksvd': ('ksvd', ['hscksvd_update_batch'])}


def _declared_symbols(prefix):
    text = open(os.path.join(ROOT, 'include', prefix + '.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return set(re.findall(r'\b(%s_[a-z0-9_]+)\s*\(' % prefix, text))


def _module(name):
    import importlib
    mod = importlib.import_module('hsc_amd.' + name)
    if not os.path.isfile(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


@pytest.mark.parametrize('prefix', sorted(NEW))
def test_new_symbols_declared_exported_and_listed(prefix):
    module, names = NEW[prefix]
    mod = _module(module)
    lib = ctypes.CDLL(mod.LIB_PATH)
    declared = _declared_symbols(prefix)
    for name in names:
        assert name in declared, '%s is not declared in include/%s.h' % (name, prefix)
        assert hasattr(lib, name), 'lib%s.so does not export %s' % (prefix, name)
        assert name in mod.EXPORTS
    version = getattr(lib, prefix + '_version')
    version.restype = ctypes.c_int
    assert version() == (100 if prefix == 'hscmp' else 1)          # (additions only: the ABI versions stay)


@pytest.mark.parametrize('prefix', sorted(NEW))
def test_null_context_messages(prefix):
    module, names = NEW[prefix]
    lib = _module(module).load_library()
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
        args = [0 if t is ctypes.c_int else None for t in fn.argtypes]
        assert fn(*args) == -1, name                                    # *_ERR_INVALID
        assert getattr(lib, prefix + '_last_error')(None).decode() == name + ': ctx is NULL'


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load a library or to open an engine fails the test: the argument checks come first."""
    from hsc_amd import _native, ksvd

    def touched(*args, **kwargs):
        raise AssertionError('the library was touched before the arguments were checked')
    for mod, names in ((_native, ('load_library', 'load_satellite', 'multi_engine', 'default_engine', 'engine_for', 'Engine')),
                       (ksvd, ('load_library', '_context'))):
        for name in names:
            monkeypatch.setattr(mod, name, touched)


def _coders():
    from hsc_amd.modeling import ConvolutionalMatchingPursuit, LoCOMP
    return [ConvolutionalMatchingPursuit(), LoCOMP()]


def test_multibatch_argument_errors(no_library):
    rng = np.random.RandomState(0)
    x = rng.randn(3, 40)
    Ds = rng.randn(2, 4, 6)
    for coder in _coders():
        with pytest.raises(ValueError, match='share one shape'):
            coder.computeCoefficientsMultiBatch(x, [rng.randn(4, 6), rng.randn(4, 7)], [0, 1, 0])
        with pytest.raises(ValueError, match='share one dtype'):
            coder.computeCoefficientsMultiBatch(x, [rng.randn(4, 6), rng.randn(4, 6).astype(np.float32)], [0, 1, 0])
        with pytest.raises(ValueError, match='one entry per signal'):
            coder.computeCoefficientsMultiBatch(x, Ds, [0, 1])
        with pytest.raises(ValueError, match=r'signal 2 asks for dictionary 2 outside \[0, 2\)'):
            coder.computeCoefficientsMultiBatch(x, Ds, [0, 1, 2])
        with pytest.raises(ValueError, match=r'signal 0 asks for dictionary -1'):
            coder.computeCoefficientsMultiBatch(x, Ds, [-1, 1, 0])
        with pytest.raises(ValueError, match='one dictionary per signal'):
            coder.computeCoefficientsMultiBatch(x, Ds)                                  # dictionaryOf=None needs G == B
        with pytest.raises(ValueError, match=r'weights must be \[G,K\]'):
            coder.computeCoefficientsMultiBatch(x, Ds, [0, 1, 0], weights=np.ones(4))
        with pytest.raises(ValueError, match=r'weights must be \[G,K\]'):
            coder.computeCoefficientsMultiBatch(x, Ds, [0, 1, 0], weights=np.ones((3, 4)))
        with pytest.raises(ValueError, match='features'):
            coder.computeCoefficientsMultiBatch(rng.randn(3, 40, 2), Ds, [0, 1, 0])
        with pytest.raises(NotImplementedError, match='computeCoefficientsMultiBatch'):
            coder.computeCoefficientsMultiBatch([rng.randn(40), rng.randn(30)], Ds, [0, 1])
        with pytest.raises(TypeError):
            coder.computeCoefficientsMultiBatch(x, Ds, [0, 1, 0], stopCondition=lambda *a: False)   # no such parameter


def test_stack_dictionaries():
    from hsc_amd import _native
    rng = np.random.RandomState(1)
    a, b = rng.randn(4, 6), rng.randn(4, 6)
    s = _native.stack_dictionaries([a, b])
    assert s.shape == (2, 4, 6, 1) and s.flags.c_contiguous and np.array_equal(s[1, :, :, 0], b)
    assert _native.stack_dictionaries(rng.randn(3, 4, 6, 2)).shape == (3, 4, 6, 2)
    with pytest.raises(ValueError):
        _native.stack_dictionaries([])
    with pytest.raises(ValueError):
        _native.stack_dictionaries(rng.randn(4, 6))
    with pytest.raises(TypeError):
        _native.stack_dictionaries(np.zeros((2, 4, 6), dtype=np.int32))


def test_update_batch_argument_errors(no_library):
    from hsc_amd import ksvd
    rng = np.random.RandomState(2)
    c = scipy.sparse.csc_matrix((60, 4))
    with pytest.raises(ValueError, match='one shape'):
        ksvd.update_batch([rng.randn(4, 6), rng.randn(4, 7)], [c, c])
    with pytest.raises(ValueError, match='1 coefficient matrices for 2 dictionaries'):
        ksvd.update_batch(rng.randn(2, 4, 6), [c])
    with pytest.raises(ValueError, match='one shape'):
        ksvd.update_batch(rng.randn(2, 4, 6), [c, scipy.sparse.csc_matrix((50, 4))])
    with pytest.raises(NotImplementedError, match='W \\* F = 66'):
        ksvd.update_batch(rng.randn(1, 4, 33, 2), [scipy.sparse.csc_matrix((100, 4))])
    with pytest.raises(ValueError, match='usePCA'):
        ksvd.update_batch(rng.randn(1, 4, 6, 2), [c], usePCA=True)
    with pytest.raises(AssertionError):
        ksvd.update_batch(rng.randn(1, 4, 6), [scipy.sparse.csc_matrix((6, 4))])     # the signal must be longer than W


def test_train_batch_argument_errors(no_library):
    from hsc_amd.ksvd import ConvolutionalKSVDLearner
    rng = np.random.RandomState(3)
    x = rng.randn(3, 100)
    learner = ConvolutionalKSVDLearner(4, 8)
    with pytest.raises(ValueError, match='2 generators for 3 learners'):
        learner.trainBatch(x, rngs=[np.random.RandomState(0), np.random.RandomState(1)])
    with pytest.raises(NotImplementedError, match='trainBatch'):
        learner.trainBatch([rng.randn(100), rng.randn(90)])
    with pytest.raises(ValueError, match='B,T'):
        learner.trainBatch(rng.randn(100))
    with pytest.raises(NotImplementedError, match='W \\* F = 66'):
        ConvolutionalKSVDLearner(4, 33).trainBatch(rng.randn(2, 200, 2))
    with pytest.raises(ValueError, match='usePCA'):
        learner.trainBatch(rng.randn(2, 100, 2), usePCA=True)
    with pytest.raises(AssertionError):
        learner.trainBatch(rng.randn(2, 8))
    with pytest.raises(NotImplementedError, match='MPTK'):
        learner.trainBatch(x, method='mptk-cmp')
    with pytest.raises(Exception, match='Unsupported sparse coding method'):
        learner.trainBatch(x, method='omp')
