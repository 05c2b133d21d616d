"""ConvolutionalNMF (hsc/modeling.py:662-747): the float64 restatement against the reference's goldens (CPU), and
hsc_amd.nmf on the GPU against the goldens and against itself (batch vs single calls)."""
import os

import numpy as np
import pytest

from hsc_amd import _native
from tests import nmf_restatement as rst

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nmf.npz')
STOP_NAMES = {1: 'max_iterations', 2: 'residual_scale', 3: 'snr'}


def _gpu_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _cases():
    g = np.load(GOLDEN)
    out = []
    for name in g['names']:
        name = str(name)
        c = {k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(name + '/')}
        c['name'] = name
        c['tol_rs'] = None if np.isnan(c['tol_rs']) else float(c['tol_rs'])
        c['tol_snr'] = None if np.isnan(c['tol_snr']) else float(c['tol_snr'])
        c['max_iterations'] = int(c['max_iterations'])
        out.append(c)
    return out


CASES = _cases()
IDS = [c['name'] for c in CASES]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / np.max(np.abs(np.asarray(b, np.float64))))


def _initial(c):
    """The reference's draw (hsc/modeling.py:684) for the case's seed, in the case's dtype, as float64."""
    T, K = c['x'].shape[0], c['D'].shape[0]
    np.random.seed(int(c['seed']))
    return (np.random.random((T, K)).astype(c['x'].dtype) + 2.0).astype(np.float64)


def _ref64(c):
    return (c['coef64'], c['resid64']) if 'coef64' in c else (c['coef'], c['resid'])


# ------------------------------------------------------------------------------------------------ CPU
def test_importable_from_modeling_and_no_cpu_path():
    from hsc_amd.modeling import ConvolutionalNMF, SparseApproximator
    from hsc_amd import nmf
    assert ConvolutionalNMF is nmf.ConvolutionalNMF
    assert issubclass(ConvolutionalNMF, SparseApproximator)
    if _gpu_visible():
        pytest.skip('a GPU is visible: the no-GPU error path cannot be exercised here')
    x = np.random.random(64)
    D = np.random.random((4, 8))
    with pytest.raises(_native.HscmpError):
        ConvolutionalNMF().computeCoefficients(x, D, nbMaxIterations=2)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_restatement_matches_reference_float64(c):
    x, D = c['x'].astype(np.float64), c['D'].astype(np.float64)
    coef, resid, iters, stop, _, _ = rst.nmf(x, D, _initial(c), c['max_iterations'], c['tol_rs'], c['tol_snr'])
    c64, r64 = _ref64(c)
    assert _rel(coef, c64) <= 1e-11
    assert _rel(resid.reshape(r64.shape), r64) <= 1e-11
    assert iters == int(c['iterations'])
    assert stop == int(c['stop'])


def test_fixtures_cover_the_issue_matrix():
    by = {c['name']: c for c in CASES}
    Ws = {c['D'].shape[1] for c in CASES}
    assert 2 in Ws and any(w % 2 for w in Ws) and any(w % 2 == 0 for w in Ws)
    assert any(c['D'].ndim == 3 and c['D'].shape[2] == 7 for c in CASES)
    assert {c['x'].dtype for c in CASES} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert any(c['x'].shape[0] >= 2048 for c in CASES)
    assert {int(c['stop']) for c in CASES} == {1, 2, 3}
    for c in by.values():
        if int(c['stop']) == 3:
            assert c['margin'] >= 1e-3
        elif int(c['stop']) == 2:
            assert c['margin'] >= 1e-6


def test_none_iterations_is_one():
    rs = np.random.RandomState(5)
    x, D = rs.random_sample(90), rs.random_sample((6, 7))
    A0 = rs.random_sample((90, 6)) + 2.0
    a = rst.nmf(x, D, A0, None)
    b = rst.nmf(x, D, A0, 1)
    assert a[2] == b[2] == 1
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('T,W', [(64, 1), (10, 11), (3, 8)])
def test_bad_shapes_raise_before_any_device_call(monkeypatch, T, W):
    from hsc_amd import nmf

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(nmf, '_context', no_device)
    monkeypatch.setattr(nmf, 'load_library', no_device)
    with pytest.raises(Exception) as ei:
        nmf.ConvolutionalNMF().computeCoefficients(np.random.random(T), np.random.random((4, W)), nbMaxIterations=2)
    assert not isinstance(ei.value, AssertionError)
    assert 'filter width' in str(ei.value)


# ------------------------------------------------------------------------------------------------ GPU
def _gpu_run(c):
    from hsc_amd.modeling import ConvolutionalNMF
    cnmf = ConvolutionalNMF()
    np.random.seed(int(c['seed']))
    coef, resid = cnmf.computeCoefficients(c['x'], c['D'], nbMaxIterations=c['max_iterations'],
                                           toleranceResidualScale=c['tol_rs'], toleranceSnr=c['tol_snr'])
    return coef, resid, cnmf.lastStats


@pytest.mark.gpu
@pytest.mark.parametrize('c', [c for c in CASES if c['x'].dtype == np.float64], ids=[c['name'] for c in CASES if c['x'].dtype == np.float64])
def test_gpu_float64_matches_reference(c):
    coef, resid, st = _gpu_run(c)
    assert coef.shape == c['coef'].shape and coef.dtype == np.float64
    assert resid.shape == c['resid'].shape
    assert _rel(coef, c['coef']) <= 1e-10
    assert _rel(resid, c['resid']) <= 1e-10
    assert int(st.iterations[0]) == int(c['iterations'])
    assert st.stop_reasons()[0] == STOP_NAMES[int(c['stop'])]


@pytest.mark.gpu
@pytest.mark.parametrize('c', [c for c in CASES if c['x'].dtype == np.float32], ids=[c['name'] for c in CASES if c['x'].dtype == np.float32])
def test_gpu_float32_within_reference_spread(c):
    coef, resid, st = _gpu_run(c)
    assert coef.dtype == np.float32 and resid.dtype == np.float32
    for got, r32, r64 in ((coef, c['coef'], c['coef64']), (resid, c['resid'], c['resid64'])):
        spread = np.max(np.abs(r32.astype(np.float64) - r64))
        err = np.max(np.abs(got.astype(np.float64) - r64))
        assert err <= 4.0 * spread + 1e-6 * np.max(np.abs(r64)), (c['name'], err, spread)
    assert int(st.iterations[0]) == int(c['iterations'])
    assert st.stop_reasons()[0] == STOP_NAMES[int(c['stop'])]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_gpu_batch_equals_single_calls(dtype):
    """Signals that stop at different iterations (planted and uniform signals, one SNR tolerance) in one batch give the
    per-signal results bit for bit, and whatever else is in the batch does not change a signal's result."""
    from hsc_amd.modeling import ConvolutionalNMF
    rs = np.random.RandomState(7)
    K, W, T, F = 8, 6, 300, 2
    D = rs.random_sample((K, W, F))
    D = (D / np.sqrt(np.sum(np.square(D.reshape(K, -1)), axis=1))[:, None, None]).astype(dtype)
    xs = []
    for b in range(6):
        x = 0.01 * rs.random_sample((T, F)) if b % 2 == 0 else rs.random_sample((T, F))
        if b % 2 == 0:
            for t in rs.randint(0, T - W + 1, size=30):
                x[t:t + W] += D[rs.randint(K)]
        xs.append(x)
    X = np.stack(xs).astype(dtype)
    A0 = (rs.random_sample((6, T, K)) + 2.0).astype(dtype)
    cnmf = ConvolutionalNMF()
    kw = dict(nbMaxIterations=12, toleranceSnr=9.0)
    coef, resid, st = cnmf.computeCoefficientsBatch(X, D, initialCoefficients=A0, **kw)
    assert len(set(int(i) for i in st.iterations)) > 1, st.iterations
    for b in range(6):
        c1, r1, s1 = cnmf.computeCoefficientsBatch(X[b:b + 1], D, initialCoefficients=A0[b:b + 1], **kw)
        assert np.array_equal(c1[0], coef[b]) and np.array_equal(r1[0], resid[b])
        assert int(s1.iterations[0]) == int(st.iterations[b]) and int(s1.stop[0]) == int(st.stop[b])
    # reversed order, and a small chunk budget (several chunks): the same results
    c2, r2, s2 = ConvolutionalNMF(memoryBudget=1).computeCoefficientsBatch(X[::-1], D, initialCoefficients=A0[::-1], **kw)
    assert np.array_equal(c2[::-1], coef) and np.array_equal(r2[::-1], resid)
    assert np.array_equal(s2.iterations[::-1], st.iterations) and s2.timing_ms[3] == 6


@pytest.mark.gpu
def test_gpu_global_rng_draw_matches_sequential_calls():
    from hsc_amd.modeling import ConvolutionalNMF
    rs = np.random.RandomState(3)
    X, D = rs.random_sample((3, 128)), rs.random_sample((8, 9))
    np.random.seed(11)
    coef, resid, _ = ConvolutionalNMF().computeCoefficientsBatch(X, D, nbMaxIterations=3)
    np.random.seed(11)
    for b in range(3):
        c1, r1 = ConvolutionalNMF().computeCoefficients(X[b], D, nbMaxIterations=3)
        assert np.array_equal(c1, coef[b]) and np.array_equal(r1, resid[b])


@pytest.mark.gpu
def test_gpu_reference_unittest_shapes():
    """tests/hsc/test_modeling.py:43-62 of the reference, through ConvolutionalSparseCoder."""
    from hsc_amd.modeling import ConvolutionalNMF, ConvolutionalSparseCoder
    for filterWidth in [5, 9, 16]:
        sequence = np.random.random(size=(256,))
        D = np.random.random(size=(16, filterWidth))
        D /= np.sqrt(np.sum(np.square(D), axis=1, keepdims=True))
        coefficients, residual = ConvolutionalSparseCoder(D, ConvolutionalNMF()).encode(sequence, nbMaxIterations=10)
        assert coefficients.shape == (256, 16) and residual.shape == (256,)
        assert np.sum(np.square(residual)) < np.sum(np.square(sequence))
        rec = ConvolutionalSparseCoder(D, ConvolutionalNMF()).reconstruct(coefficients)
        assert np.max(np.abs(rec + residual - sequence)) <= 1e-9
    for filterWidth in [5, 9, 16]:
        sequence = np.random.random(size=(64, 7))
        D = np.random.random(size=(16, 15, 7))
        D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
        coefficients, residual = ConvolutionalNMF().computeCoefficients(sequence, D, nbMaxIterations=10)
        assert residual.shape == (64, 7)
        assert np.sum(np.square(residual)) < np.sum(np.square(sequence))
