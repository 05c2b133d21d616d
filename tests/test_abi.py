"""CPU-side checks of the drop-in boundary: each C-ABI library loads and exports every symbol its header under
include/ declares, and the satellite libraries' argument and device checks fail as documented (no compute calls
here -- those are the -m gpu tests)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (header, module, version) of every C-ABI library the package loads
LIBRARIES = [('hscmp', '_native', 100), ('hscnmf', 'nmf', 2), ('hscksvd', 'ksvd', 1), ('hsckmeans', 'kmeans', 1)]
SATELLITES = LIBRARIES[1:]


def _declared_symbols(prefix):
    text = open(os.path.join(ROOT, 'include', prefix + '.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(%s_[a-z0-9_]+)\s*\(' % prefix, text)))


def _module(name):
    import importlib
    mod = importlib.import_module('hsc_amd.' + name)
    if not os.path.isfile(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.parametrize('prefix,module,version', LIBRARIES, ids=[l[0] for l in LIBRARIES])
def test_library_exports_every_declared_symbol(prefix, module, version):
    mod = _module(module)
    lib = ctypes.CDLL(mod.LIB_PATH)
    declared = _declared_symbols(prefix)
    assert len(declared) >= (18 if prefix == 'hscmp' else 5)
    for name in declared:
        assert hasattr(lib, name), 'lib%s.so does not export %s' % (prefix, name)
    assert sorted(mod.EXPORTS) == declared
    fn = getattr(lib, prefix + '_version')
    fn.restype = ctypes.c_int
    assert fn() == version


def _last_error(lib, prefix):
    return getattr(lib, prefix + '_last_error')(None).decode()


@pytest.mark.parametrize('prefix,module,version', SATELLITES, ids=[l[0] for l in SATELLITES])
def test_satellite_null_arguments(prefix, module, version):
    """create without an out pointer, every compute entry point without a context, destroy(NULL): the library's
    own checks, no device needed."""
    lib = _module(module).load_library()
    assert getattr(lib, prefix + '_create')(None, 0) == -1                # *_ERR_INVALID
    assert _last_error(lib, prefix) == prefix + '_create: out is NULL'
    generic = ('version', 'create', 'destroy', 'last_error')
    entries = [n for n in _declared_symbols(prefix) if n[len(prefix) + 1:] not in generic]
    assert entries
    for name in entries:
        fn = getattr(lib, name)
        args = [0 if t is ctypes.c_int else None for t in fn.argtypes]
        assert fn(*args) == -1, name                                    # *_ERR_INVALID
        assert _last_error(lib, prefix) == name + ': ctx is NULL'
    getattr(lib, prefix + '_destroy')(None)                             # a no-op


@pytest.mark.parametrize('prefix,module,version', SATELLITES, ids=[l[0] for l in SATELLITES])
def test_satellite_create_without_gpu(prefix, module, version):
    if not _no_gpu():
        pytest.skip('a GPU is visible')
    lib = _module(module).load_library()
    h = ctypes.c_void_p()
    assert getattr(lib, prefix + '_create')(ctypes.byref(h), 0) == -2     # *_ERR_NO_DEVICE
    assert not h.value
    assert _last_error(lib, prefix).startswith(prefix + '_create: no HIP device visible')


def test_no_gpu_fails_loudly():
    """Without a GPU the engine must raise, never fall back to a CPU path."""
    if not _no_gpu():
        pytest.skip('a GPU is visible')
    import numpy as np
    from hsc_amd import _native
    from hsc_amd.modeling import ConvolutionalMatchingPursuit
    with pytest.raises(_native.HscmpError):
        _native.Engine(0)
    with pytest.raises(_native.HscmpError):
        ConvolutionalMatchingPursuit().computeCoefficients(np.zeros(64, dtype=np.float32),
                                                           np.ones((2, 4), dtype=np.float32), nbNonzeroCoefs=1)


def test_product_does_not_reference_oracle():
    """The oracle is test infrastructure: nothing under the package may import or link it."""
    pkg = os.path.join(ROOT, 'hierarchical-sparse-coding_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.h', '.hip', '.cpp')) or f == 'Makefile':
                text = open(os.path.join(dirpath, f)).read()
                for needle in ('hsc_oracle', 'from oracle', 'import oracle', 'libhsc_oracle'):
                    assert needle not in text, '%s references the oracle (%s)' % (f, needle)
