"""ConvolutionalKSVDLearner (the reference's ConvolutionalDictionaryLearner(algorithm='ksvd'), hsc/modeling.py:528-641,
with the dictionary update on the GPU): the float64 restatement against the reference's goldens, the argument checks
and the missing-library error (CPU); hsc_amd.ksvd against the goldens, the restatement, the host learner and itself
(GPU)."""
import os

import numpy as np
import pytest
import scipy.sparse

from hsc_amd import _native
from hsc_amd import ksvd
from hsc_amd.learning import ConvolutionalDictionaryLearner
from hsc_amd.ksvd import ConvolutionalKSVDLearner
from tests import ksvd_restatement as rst

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ksvd.npz')
EPS = np.finfo(np.float64).eps


def _cases():
    g = np.load(GOLDEN)
    out = []
    for name in g['names']:
        name = str(name)
        c = {k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(name + '/')}
        c['name'] = name
        c['method'] = str(c['method'])
        c['nbNonzeroCoefs'] = None if np.isnan(c['nbNonzeroCoefs']) else int(c['nbNonzeroCoefs'])
        for k in ('K', 'W', 'seed', 'maxIterations', 'iterations'):
            c[k] = int(c[k])
        c['usePCA'] = bool(c['usePCA'])
        for k in ('toleranceSnr', 'tolerance', 'gap'):
            c[k] = float(c[k])
        out.append(c)
    return out


CASES = _cases()
IDS = [c['name'] for c in CASES]
CMP_CASES = [c for c in CASES if c['method'] == 'cmp']


def _tol(c):
    """max(1e-10, 64 eps / gap), gap the case's smallest relative gap of the top two singular values / eigenvalues."""
    return max(1e-10, 64.0 * EPS / c['gap'])


def _draw(c):
    np.random.seed(c['seed'])
    return ConvolutionalDictionaryLearner(c['K'], c['W'], algorithm='ksvd')._init_D(c['x'], initMethod='noise')


def _err_up_to_sign(a, b):
    K = a.shape[0]
    a, b = np.asarray(a, np.float64).reshape(K, -1), np.asarray(b, np.float64).reshape(K, -1)
    return float(np.max(np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1))))


def _kw(c):
    return dict(method=c['method'], maxIterations=c['maxIterations'], tolerance=c['tolerance'],
                nbNonzeroCoefs=c['nbNonzeroCoefs'], toleranceSnr=c['toleranceSnr'], usePCA=c['usePCA'])


def _restate(c):
    return rst.learn(c['x'], _draw(c), c['nbNonzeroCoefs'], c['toleranceSnr'], c['usePCA'], c['maxIterations'],
                     c['tolerance'])


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('c', CMP_CASES, ids=[c['name'] for c in CMP_CASES])
def test_restatement_matches_reference(c):
    hist, alphas, _ = _restate(c)
    assert len(hist) == c['iterations']
    for i, D in enumerate(hist):
        assert _err_up_to_sign(D, c['D_hist'][i]) <= _tol(c), (c['name'], i)


def test_fixtures_cover_the_issue_matrix():
    by = {c['name']: c for c in CASES}
    s = by['script_cmp']
    assert (s['K'], s['W'], s['nbNonzeroCoefs'], s['toleranceSnr'], s['x'].shape[0]) == (64, 32, 100, 20.0, 4000)
    assert by['script_locomp']['method'] == 'locomp'
    assert any(c['W'] % 2 == 1 for c in CASES)
    assert any(c['x'].ndim == 2 and c['x'].shape[1] == 2 for c in CASES)
    assert by['snr_stop']['nbNonzeroCoefs'] is None
    assert by['tolerance_stop']['tolerance'] > 0.0 and by['tolerance_stop']['iterations'] < by['tolerance_stop']['maxIterations']
    assert all(c['x'].dtype == np.float64 for c in CASES)
    rules = {}
    for name in ('script_cmp', 'never_occurs', 'dense', 'pca'):
        _, _, stats = _restate(by[name])
        rules[name] = np.concatenate(stats)
    # isolated atoms of the script shape: zero patches (the e_0 rule)
    assert np.any(rules['script_cmp'][:, 3] == 3)
    # an atom that never occurs
    assert np.any(rules['never_occurs'][:, 0] == 0)
    # dense overlaps: many patches per atom
    assert np.max(rules['dense'][:, 0]) >= 30
    # usePCA: a single occurrence (P / |P|) and a zero covariance (e_{n-1})
    pca = rules['pca']
    assert np.any((pca[:, 0] == 1) & (pca[:, 3] == 2))
    assert np.any((pca[:, 0] >= 2) & (pca[:, 3] == 3))


class _DeviceTouched(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise _DeviceTouched()
    monkeypatch.setattr(ksvd, 'load_library', touched)
    monkeypatch.setattr(ksvd, '_context', touched)
    monkeypatch.setattr(_native, 'default_engine', touched)


def test_argument_checks_raise_before_any_device_call(no_device):
    x = np.random.RandomState(0).randn(500)
    with pytest.raises(NotImplementedError, match='64'):
        ConvolutionalKSVDLearner(4, 65).train(x, method='cmp')
    with pytest.raises(NotImplementedError, match='64'):
        ConvolutionalKSVDLearner(4, 33).train(np.zeros((500, 2)), method='cmp')
    with pytest.raises(AssertionError):
        ConvolutionalKSVDLearner(4, 16).train(x[:16], method='cmp')
    with pytest.raises(ValueError):
        ConvolutionalKSVDLearner(4, 16).train(np.zeros((500, 2)), method='cmp', usePCA=True)
    for m in ('mptk-mp', 'mptk-cmp'):
        with pytest.raises(NotImplementedError, match='MPTK'):
            ConvolutionalKSVDLearner(4, 16).train(x, method=m)
    with pytest.raises(Exception, match='Unsupported sparse coding method'):
        ConvolutionalKSVDLearner(4, 16).train(x, method='omp')
    # valid arguments reach the device
    with pytest.raises(_DeviceTouched):
        ConvolutionalKSVDLearner(4, 16).train(x, method='cmp')


def test_no_library_raises_hscmp_error(monkeypatch):
    monkeypatch.setattr(ksvd, '_lib', None)
    monkeypatch.setattr(ksvd, '_contexts', {})
    monkeypatch.setattr(ksvd, 'LIB_PATH', os.path.join(os.path.dirname(ksvd.LIB_PATH), 'missing', 'libhscksvd.so'))
    x = np.random.RandomState(0).randn(500)
    with pytest.raises(_native.HscmpError):
        ConvolutionalKSVDLearner(4, 16).train(x, method='cmp')
    D = np.eye(4, 16)
    with pytest.raises(_native.HscmpError):
        ksvd.update(D, scipy.sparse.csc_matrix(np.ones((500, 4))))


# ------------------------------------------------------------------------------------------------ GPU
def _random_input(T, K, W, F, nnz, seed, clusters=0):
    """Random unit atoms and nnz random coefficients; `clusters` bursts of entries packed into a few windows."""
    rs = np.random.RandomState(seed)
    D = rs.randn(K, W, F)
    D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
    t = rs.randint(0, T, nnz)
    k = rs.randint(0, K, nnz)
    for _ in range(clusters):
        c0 = rs.randint(0, T - 2 * W)
        n = 4 * K
        t = np.concatenate([t, c0 + rs.randint(0, 2 * W, n)])
        k = np.concatenate([k, rs.randint(0, K, n)])
    key = np.unique(t.astype(np.int64) * K + k)
    t, k = key // K, key % K
    c = rs.randn(len(key))
    c[rs.rand(len(key)) < 0.02] = 0.0                     # stored zeros: never occurrences, never terms
    A = scipy.sparse.csc_matrix((c, (t, k)), shape=(T, K))
    return (D[:, :, 0] if F == 1 else D), A


UPDATE_INPUTS = [
    ('small', (3000, 8, 16, 1, 200, 1, 0), False),
    ('odd_w_f2', (2000, 6, 15, 2, 150, 2, 2), False),
    ('pca', (3000, 8, 16, 1, 120, 3, 1), True),
    ('large', (1 << 16, 64, 32, 1, 6000, 4, 8), False),
]


@pytest.mark.gpu
@pytest.mark.parametrize('name,shape,pca', UPDATE_INPUTS, ids=[u[0] for u in UPDATE_INPUTS])
def test_update_matches_restatement(name, shape, pca):
    D, A = _random_input(*shape)
    D_ref, A_ref, st_ref = rst.sweep(D, A, pca)
    D_gpu, A_gpu, st_gpu, _ = ksvd.update(D, A, usePCA=pca)
    assert np.array_equal(st_gpu[:, 0], st_ref[:, 0])
    assert _err_up_to_sign(D_gpu, D_ref) <= 1e-10
    assert np.array_equal(A_gpu.indices, A_ref.indices) and np.array_equal(A_gpu.indptr, A_ref.indptr)
    scale = np.max(np.abs(A_ref.data))
    assert np.max(np.abs(A_gpu.data - A_ref.data)) <= 1e-12 * scale
    # the restatement orients by the same rule: D agrees with its signs too
    assert np.max(np.abs(D_gpu - D_ref)) <= 1e-10
    # eigenvalues of the Gram matrix (covariance for PCA)
    occ = st_ref[:, 3] == 1
    assert np.allclose(st_gpu[occ, 1], st_ref[occ, 1], rtol=1e-10, atol=1e-12 * np.max(st_ref[:, 1]))


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_train_matches_reference(c):
    np.random.seed(c['seed'])
    learner = ConvolutionalKSVDLearner(c['K'], c['W'])
    D = learner.train(c['x'], **_kw(c))
    assert D.dtype == np.float64 and D.shape == c['D_hist'].shape[1:]
    assert len(learner.lastStats) == c['iterations']
    assert _err_up_to_sign(D, c['D_hist'][c['iterations'] - 1]) <= _tol(c)


@pytest.mark.gpu
def test_rng_draws_like_the_global_generator():
    c = CASES[IDS.index('odd_w')]
    D1 = ConvolutionalKSVDLearner(c['K'], c['W'], rng=np.random.RandomState(c['seed'])).train(c['x'], **_kw(c))
    assert _err_up_to_sign(D1, c['D_hist'][c['iterations'] - 1]) <= _tol(c)


@pytest.mark.gpu
def test_locomp_matches_host_learner():
    c = CASES[IDS.index('script_locomp')]
    kw = dict(method='locomp', maxIterations=2, nbNonzeroCoefs=c['nbNonzeroCoefs'], toleranceSnr=c['toleranceSnr'])
    np.random.seed(c['seed'])
    D_host = ConvolutionalDictionaryLearner(c['K'], c['W'], algorithm='ksvd').train(c['x'], **kw)
    np.random.seed(c['seed'])
    D_gpu = ConvolutionalKSVDLearner(c['K'], c['W']).train(c['x'], **kw)
    assert _err_up_to_sign(D_gpu, D_host) <= _tol(c)


@pytest.mark.gpu
def test_two_runs_bit_identical():
    c = CASES[IDS.index('dense')]
    out = []
    for _ in range(2):
        np.random.seed(c['seed'])
        out.append(ConvolutionalKSVDLearner(c['K'], c['W']).train(c['x'], **_kw(c)))
    assert np.array_equal(out[0], out[1])
    D, A = _random_input(1 << 16, 64, 32, 1, 6000, 4, 8)
    r1, r2 = ksvd.update(D, A), ksvd.update(D, A)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1].data, r2[1].data)


@pytest.mark.gpu
def test_last_stats_and_tolerance_stop():
    c = CASES[IDS.index('tolerance_stop')]
    np.random.seed(c['seed'])
    learner = ConvolutionalKSVDLearner(c['K'], c['W'])
    learner.train(c['x'], **_kw(c))
    st = learner.lastStats
    assert len(st) == c['iterations'] < c['maxIterations']
    assert all(s['alpha'] > c['tolerance'] for s in st[:-1]) and st[-1]['alpha'] <= c['tolerance']
    _, alphas, rstats = _restate(c)
    assert np.allclose([s['alpha'] for s in st], alphas, rtol=1e-9)
    for s, r in zip(st, rstats):
        assert np.array_equal(s['n_k'], r[:, 0].astype(np.int64))
        assert s['nnz'] > 0 and s['encode_ms'] > 0.0 and s['update_ms'] > 0.0
        assert s['eigenvalues'].shape == (c['K'], 2)
