"""The per-signal SNR table of the hierarchical coder, the part that needs no GPU: the shape and value
errors of the 2-D `toleranceSnr` come before any engine call, LoCOMP refuses it, the header and the library name the new call."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse

from tests.test_ragged_api import no_engine  # noqa: F401 (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = 3, 64


def _mld(nbLevels=2):
    """A generated two-level dictionary with its singleton bases (as tests/test_gpu_ragged_hierarchy.py makes its three levels)."""
    from hsc_amd.dataset import MultilevelDictionaryGenerator
    mld = MultilevelDictionaryGenerator(np.random.RandomState(503)).generate(
        scales=[8, 16, 36][:nbLevels], counts=[4, 3, 3][:nbLevels], decompositionSize=2, multilevelDecomposition=False,
        maxNbPatternsConsecutiveRejected=30)
    return mld.withSingletonBases()


def _entry_points(hcmp, mld, given_levels=1):
    """(name, call(toleranceSnr)) of the eight batch entry points, uniform and ragged, from the start and from a level."""
    from hsc_amd.modeling import HierarchicalConvolutionalSparseCoder
    x = np.zeros((B, T), np.float64)
    xs = [np.zeros(n, np.float64) for n in (64, 40, 50)]
    K = [int(mld.getRawDictionary(l).shape[0]) for l in range(given_levels)]
    given = [[scipy.sparse.csc_matrix((T, k)) for k in K] for _ in range(B)]
    given_r = [[scipy.sparse.csc_matrix((len(q), k)) for k in K] for q in xs]
    coder = HierarchicalConvolutionalSparseCoder(mld, hcmp)
    return [
        ('computeCoefficientsBatch', lambda snr: hcmp.computeCoefficientsBatch(x, mld, toleranceSnr=snr)),
        ('computeCoefficientsBatch unchained', lambda snr: hcmp.computeCoefficientsBatch(x, mld, toleranceSnr=snr, chained=False)),
        ('computeCoefficientsRaggedBatch', lambda snr: hcmp.computeCoefficientsRaggedBatch(xs, mld, toleranceSnr=snr)),
        ('computeCoefficientsFromLevelBatch', lambda snr: hcmp.computeCoefficientsFromLevelBatch(x, given, mld, toleranceSnr=snr)),
        ('computeCoefficientsFromLevelRaggedBatch', lambda snr: hcmp.computeCoefficientsFromLevelRaggedBatch(xs, given_r, mld, toleranceSnr=snr)),
        ('encodeBatch', lambda snr: coder.encodeBatch(x, toleranceSnr=snr)),
        ('encodeRaggedBatch', lambda snr: coder.encodeRaggedBatch(xs, toleranceSnr=snr)),
        ('encodeFromLevelBatch', lambda snr: coder.encodeFromLevelBatch(x, given, toleranceSnr=snr)),
        ('encodeFromLevelRaggedBatch', lambda snr: coder.encodeFromLevelRaggedBatch(xs, given_r, toleranceSnr=snr)),
    ]


def test_shape_and_value_errors_come_before_the_device(no_engine):  # noqa: F811
    from hsc_amd.modeling import HierarchicalConvolutionalMatchingPursuit
    mld = _mld(2)
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    good = np.array([[10.0, 12.0], [14.0, 8.0], [6.0, 20.0]])
    for name, call in _entry_points(hcmp, mld):
        # a wrong shape: signals x levels is (3, 2)
        for bad in (good.T, good[:2], good[:, :1], np.concatenate([good, good], axis=1), [[10.0, 12.0]]):
            with pytest.raises(ValueError, match=r'toleranceSnr.*\(3, 2\)'):
                call(bad)
        # a value that is NaN, infinite or negative, in a column that is read: the signal and the level are named
        for b, l, v in ((1, 1, float('nan')), (2, 1, -1.0), (0, 1, float('inf'))):
            bad = good.copy()
            bad[b, l] = v
            with pytest.raises(ValueError, match='toleranceSnr: signal %d, level %d' % (b, l)):
                call(bad)
        bad = good.copy()
        bad[2, 0] = -3.0
        if 'FromLevel' in name:
            # (column 0 lies below fromLevel = 1 and is not read: the call gets as far as the engine)
            with pytest.raises(AssertionError, match='a device call was made'):
                call(bad)
        else:
            with pytest.raises(ValueError, match='toleranceSnr: signal 2, level 0'):
                call(bad)


def test_locomp_refuses_the_table(no_engine):  # noqa: F811
    from hsc_amd.modeling import HierarchicalConvolutionalMatchingPursuit
    mld = _mld(2)
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='locomp')
    table = [[10.0, 12.0], [14.0, 8.0], [6.0, 20.0]]
    message = re.escape('the LoCOMP loop has no per-signal stop rules')
    for name, call in _entry_points(hcmp, mld):
        if 'Ragged' in name:
            continue                            # (LoCOMP has no ragged form at all: refused as before)
        with pytest.raises(NotImplementedError, match=message):
            call(table)


def test_multilevel_learner_reads_the_level_count_from_the_second_axis(no_engine):  # noqa: F811
    from hsc_amd.modeling import MultilevelDictionaryLearner
    learner = MultilevelDictionaryLearner([4, 3, 3], [8, 12, 20], method='cmp')
    x = np.zeros((2, 256))
    # two signals, three levels: the encodes run up to level 1, so two columns are enough -- and two ROWS are not two levels
    with pytest.raises(ValueError, match='toleranceSnr has shape'):
        learner._levels(x, False, 10, {}, dict(toleranceSnr=np.zeros((2, 1))), True)
    with pytest.raises(ValueError, match='toleranceSnr has shape'):
        learner._levels(x, False, 10, {}, dict(toleranceSnr=np.zeros((3, 2))), True)


def test_header_and_exports_name_the_entry_point():
    from hsc_amd import _native
    header = open(os.path.join(ROOT, 'include', 'hscmp.h')).read()
    name = 'hscmp_encode_batch_from_level_rules'
    assert re.search(r'\bint %s\(hscmp_ctx\* ctx, hscmp_ctx\* prev, int first, int count, double min_coefficients,\s*'
                     r'const hscmp_signal_rules\* rules, const hscmp_params\* params\);' % name, header)
    assert name in _native.EXPORTS
    assert '#define HSCMP_VERSION 100' in header
    lib = _native.load_library()
    assert hasattr(lib, name)
    # no device is needed for the first refusal
    params = _native.make_params(eps=1e-16)
    rules = _native.make_rules(1, toleranceSnr=[10.0])
    assert lib.hscmp_encode_batch_from_level_rules(None, None, 0, 1, ctypes.c_double(1e-16), ctypes.byref(rules), ctypes.byref(params)) == _native.ERR_INVALID
    assert b'hscmp_encode_batch_from_level_rules: NULL context' in lib.hscmp_last_error(None)
