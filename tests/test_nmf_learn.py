"""ConvolutionalNMFLearner (the reference's ConvolutionalDictionaryLearner(algorithm='nmf'), hsc/modeling.py:330-417):
the float64 restatement against the reference's goldens and the draw order (CPU), and hsc_amd.nmf on the GPU against
the goldens and against itself (batch vs single calls, chunked vs whole)."""
import os

import numpy as np
import pytest

from hsc_amd import _native
from hsc_amd.learning import ConvolutionalDictionaryLearner
from hsc_amd.nmf import ConvolutionalNMFLearner
from tests import nmf_learn_restatement as rst

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nmf_learn.npz')
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
        c['init'] = str(c['init'])
        c['tol_rs'] = None if np.isnan(c['tol_rs']) else float(c['tol_rs'])
        c['tol_snr'] = None if np.isnan(c['tol_snr']) else float(c['tol_snr'])
        for k in ('K', 'W', 'max_iterations', 'iterations', 'stop', 'seed'):
            c[k] = int(c[k])
        out.append(c)
    return out


CASES = _cases()
IDS = [c['name'] for c in CASES]


def _draws(x, K, W, init, seed):
    """The reference's draws (hsc/modeling.py:331-344) under np.random.seed(seed): the initial dictionary, then the
    initial coefficients in the data's dtype."""
    np.random.seed(seed)
    D0 = ConvolutionalDictionaryLearner(K, W, algorithm='nmf')._init_D(x, init)
    A0 = np.random.random((x.shape[0], K)).astype(x.dtype) + 2.0
    return D0, A0


def _ref64(c):
    return c['D64'] if 'D64' in c else c['D']


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def _kw(c):
    return dict(initMethod=c['init'], nbMaxIterations=c['max_iterations'], toleranceResidualScale=c['tol_rs'],
                toleranceSnr=c['tol_snr'])


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_restatement_matches_reference_float64(c):
    D0, A0 = _draws(c['x'], c['K'], c['W'], c['init'], c['seed'])
    D, iters, stop, _, _ = rst.learn(c['x'].astype(np.float64), D0.astype(np.float64), A0.astype(np.float64),
                                     c['max_iterations'], c['tol_rs'], c['tol_snr'])
    ref = _ref64(c)
    assert _err(D.reshape(ref.shape), ref) <= 1e-11
    assert iters == c['iterations']
    assert stop == c['stop']


def test_fixtures_cover_the_issue_matrix():
    shapes = {(c['x'].shape[0], c['K'], c['W'], 1 if c['x'].ndim == 1 else c['x'].shape[1]) for c in CASES}
    unittest = [c for c in CASES if c['x'].shape[0] == 256 and c['K'] == 16 and c['W'] == 5 and c['max_iterations'] == 100]
    assert {1 if c['x'].ndim == 1 else c['x'].shape[1] for c in unittest} == {1, 4}
    assert {c['init'] for c in CASES} == {'noise', 'random_samples'}
    Ws = {s[2] for s in shapes}
    assert 2 in Ws and any(w % 2 == 0 and w > 2 for w in Ws) and any(w % 2 for w in Ws)
    assert any(c['K'] % 8 for c in CASES)
    assert any(s[3] == 3 for s in shapes)
    assert (4096, 16, 32, 1) in shapes
    assert {c['x'].dtype for c in CASES} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert any(c['x'].dtype == np.float32 and c['init'] == 'noise' and c['D'].dtype == np.float64 for c in CASES)
    assert {c['stop'] for c in CASES} == {1, 2, 3}
    for c in CASES:
        if c['stop'] == 3:
            assert c['margin'] >= 1e-3
        elif c['stop'] == 2:
            assert c['margin'] >= 1e-4
        if c['x'].dtype == np.float32:
            assert 'D64' in c and c['D64'].dtype == np.float64


@pytest.mark.parametrize('init', ['random_samples', 'noise'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('F', [1, 3])
def test_draw_order_and_dtypes(monkeypatch, init, dtype, F):
    """trainBatch draws D_init then A0 per learner in batch order, from the global generator or from `rng`, computes in
    _compute_dtype(data, D_init) and returns D in D_init's dtype (squeezed for [B,T] data)."""
    from hsc_amd import nmf
    captured = {}

    def fake(device, dt, x, D0, a0, energy, params):
        captured.update(dt=dt, x=x, D0=D0, a0=a0, energy=energy, max_iterations=params.max_iterations)
        st = nmf.NMFStats(np.ones(len(x), np.int32), np.ones(len(x), np.int32), np.zeros(len(x)), np.zeros(len(x)), np.zeros(5))
        return D0.copy(), st
    monkeypatch.setattr(nmf, '_call_learn', fake)
    K, W, T, B = 5, 4, 40, 3
    X = np.random.RandomState(1).random_sample((B, T) if F == 1 else (B, T, F)).astype(dtype)
    np.random.seed(17)
    D, st = ConvolutionalNMFLearner(K, W).trainBatch(X, initMethod=init, nbMaxIterations=None)
    expect_D, expect_A = [], []
    np.random.seed(17)
    for b in range(B):
        d0 = ConvolutionalDictionaryLearner(K, W, algorithm='nmf')._init_D(X[b], init)
        a0 = np.random.random((T, K)).astype(dtype) + 2.0
        expect_D.append(d0)
        expect_A.append(a0)
    expect_D, expect_A = np.stack(expect_D), np.stack(expect_A)
    dt = np.float64 if (dtype == np.float64 or init == 'noise') else np.float32
    assert captured['dt'] == dt and captured['max_iterations'] == 1
    assert captured['x'].dtype == dt and captured['D0'].dtype == dt and captured['a0'].dtype == dt
    assert captured['D0'].shape == (B, K, W, F) and captured['a0'].shape == (B, T, K)
    assert np.array_equal(captured['D0'].reshape(expect_D.shape), expect_D.astype(dt))
    assert np.array_equal(captured['a0'], expect_A.astype(dt))
    assert np.array_equal(captured['energy'], [np.sum(np.square(captured['x'][b])) for b in range(B)])
    assert D.dtype == expect_D.dtype and D.shape == expect_D.shape
    # the same draws from a seeded RandomState given as rng
    ConvolutionalNMFLearner(K, W, rng=np.random.RandomState(17)).trainBatch(X, initMethod=init, nbMaxIterations=2)
    assert np.array_equal(captured['D0'].reshape(expect_D.shape), expect_D.astype(dt))
    assert np.array_equal(captured['a0'], expect_A.astype(dt)) and captured['max_iterations'] == 2
    # train: one learner, the reference's draws
    np.random.seed(17)
    D1 = ConvolutionalNMFLearner(K, W).train(X[0], initMethod=init, nbMaxIterations=3)
    assert D1.shape == expect_D.shape[1:] and D1.dtype == expect_D.dtype
    assert np.array_equal(captured['a0'][0], expect_A[0].astype(dt)) and captured['max_iterations'] == 3


@pytest.mark.parametrize('T,W,init', [(64, 1, 'noise'), (10, 11, 'noise'), (3, 8, 'random_samples'),
                                      (8, 8, 'random_samples'), (8, 9, 'noise')])
def test_bad_shapes_raise_before_any_device_call(monkeypatch, T, W, init):
    from hsc_amd import nmf

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(nmf, '_context', no_device)
    monkeypatch.setattr(nmf, 'load_library', no_device)
    monkeypatch.setattr(nmf, '_call_learn', no_device)
    with pytest.raises(Exception) as ei:
        ConvolutionalNMFLearner(4, W).train(np.random.random(T), initMethod=init, nbMaxIterations=2)
    assert not isinstance(ei.value, AssertionError)
    assert 'filter width' in str(ei.value)


def test_noise_with_signal_as_long_as_the_filter_is_accepted(monkeypatch):
    """T == W is a valid shape for 'noise' (one coefficient row); only 'random_samples' needs T > W."""
    from hsc_amd import nmf
    seen = []

    def fake(*a):
        seen.append(a)
        return a[3].copy(), nmf.NMFStats(np.ones(1, np.int32), np.ones(1, np.int32), np.zeros(1), np.zeros(1), np.zeros(5))
    monkeypatch.setattr(nmf, '_call_learn', fake)
    D = ConvolutionalNMFLearner(4, 8).train(np.random.random(8), initMethod='noise', nbMaxIterations=2)
    assert D.shape == (4, 8) and len(seen) == 1


def test_no_cpu_path():
    if _gpu_visible():
        pytest.skip('a GPU is visible: the no-GPU error path cannot be exercised here')
    with pytest.raises(_native.HscmpError):
        ConvolutionalNMFLearner(4, 8).train(np.random.random(64), nbMaxIterations=2)
    with pytest.raises(_native.HscmpError):
        ConvolutionalNMFLearner(4, 8).trainBatch(np.random.random((2, 64, 3)), initMethod='noise', nbMaxIterations=2)


# ------------------------------------------------------------------------------------------------ GPU
def _gpu_train(c):
    learner = ConvolutionalNMFLearner(c['K'], c['W'])
    np.random.seed(c['seed'])
    D = learner.train(c['x'], **_kw(c))
    return D, learner.lastStats


def _check_stop(c, st):
    assert int(st.iterations[0]) == c['iterations']
    assert st.stop_reasons()[0] == STOP_NAMES[c['stop']]


F64 = [c for c in CASES if c['x'].dtype == np.float64]
F32 = [c for c in CASES if c['x'].dtype == np.float32 and c['D'].dtype == np.float32]
MIXED = [c for c in CASES if c['x'].dtype == np.float32 and c['D'].dtype == np.float64]


@pytest.mark.gpu
@pytest.mark.parametrize('c', F64, ids=[c['name'] for c in F64])
def test_gpu_float64_matches_reference(c):
    D, st = _gpu_train(c)
    assert D.shape == c['D'].shape and D.dtype == np.float64
    assert _err(D, c['D']) <= 1e-10, _err(D, c['D'])
    _check_stop(c, st)


@pytest.mark.gpu
@pytest.mark.parametrize('c', F32, ids=[c['name'] for c in F32])
def test_gpu_float32_within_reference_spread(c):
    D, st = _gpu_train(c)
    assert D.shape == c['D'].shape and D.dtype == np.float32
    spread = _err(c['D'], c['D64'])
    err = _err(D, c['D64'])
    assert err <= 4.0 * spread + 1e-6, (c['name'], err, spread)
    _check_stop(c, st)


@pytest.mark.gpu
@pytest.mark.parametrize('c', MIXED, ids=[c['name'] for c in MIXED])
def test_gpu_mixed_dtype_runs_in_float64(c):
    """float32 data with 'noise': a float64 D, so the learner runs in float64 (the reference keeps its coefficients in
    float32): within 1e-10 of the reference's float64 run on the same draws, and within the spread of its mixed run."""
    D, st = _gpu_train(c)
    assert D.shape == c['D'].shape and D.dtype == np.float64
    assert _err(D, c['D64']) <= 1e-10, _err(D, c['D64'])
    spread = _err(c['D'], c['D64'])
    assert _err(D, c['D']) <= 4.0 * spread + 1e-6
    _check_stop(c, st)


def _batch_inputs(dtype, B=6, T=300, K=6, W=6, F=2):
    rs = np.random.RandomState(7)
    atoms = rs.random_sample((K, W, F))
    xs = []
    for b in range(B):
        x = (0.003 * (b + 1)) * rs.random_sample((T, F))
        for t in rs.randint(0, T - W + 1, size=T // W):
            x[t:t + W] += atoms[rs.randint(K)]
        xs.append(x)
    X = np.stack(xs).astype(dtype)
    D0 = rs.random_sample((B, K, W, F))
    D0 = (D0 / np.sqrt(np.sum(np.square(D0), axis=(2, 3), keepdims=True))).astype(dtype)
    A0 = (rs.random_sample((B, T, K)) + 2.0).astype(dtype)
    return X, D0, A0


def _tolerance_with_spread_stops(learner, X, D0, A0, n=6):
    """An SNR tolerance at which the learners of the batch stop at different iterations (from their SNR after 1..n
    iterations: a learner's run does not depend on the tolerance until it stops)."""
    S = np.stack([learner.trainBatch(X, nbMaxIterations=i, initialDictionaries=D0, initialCoefficients=A0)[1].snr
                  for i in range(1, n + 1)], axis=1)
    for tol in np.sort(S.ravel()):
        reached = S >= tol
        first = np.where(reached.any(axis=1), reached.argmax(axis=1) + 1, n + 1)
        if len(set(first.tolist())) >= 3:
            return float(tol)
    raise AssertionError('no tolerance separates the learners: %s' % S)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_gpu_batch_equals_single_calls_and_chunks(dtype):
    """Learners that stop at different iterations in one batch give the single-learner results bit for bit; so do the
    reversed batch and a memory budget that forces one learner per chunk."""
    X, D0, A0 = _batch_inputs(dtype)
    B = X.shape[0]
    learner = ConvolutionalNMFLearner(6, 6)
    kw = dict(nbMaxIterations=8, toleranceSnr=_tolerance_with_spread_stops(learner, X, D0, A0))
    D, st = learner.trainBatch(X, initialDictionaries=D0, initialCoefficients=A0, **kw)
    assert len(set(int(i) for i in st.iterations)) > 1, st.iterations
    assert st.timing_ms[3] == 1
    for b in range(B):
        D1, s1 = learner.trainBatch(X[b:b + 1], initialDictionaries=D0[b:b + 1], initialCoefficients=A0[b:b + 1], **kw)
        assert np.array_equal(D1[0], D[b])
        assert int(s1.iterations[0]) == int(st.iterations[b]) and int(s1.stop[0]) == int(st.stop[b])
        assert s1.snr[0] == st.snr[b] and s1.residual_scale[0] == st.residual_scale[b]
    D2, s2 = ConvolutionalNMFLearner(6, 6, memoryBudget=1).trainBatch(X[::-1], initialDictionaries=D0[::-1],
                                                                      initialCoefficients=A0[::-1], **kw)
    assert s2.timing_ms[3] == B
    assert np.array_equal(D2[::-1], D) and np.array_equal(s2.iterations[::-1], st.iterations)
    assert np.array_equal(s2.snr[::-1], st.snr)


@pytest.mark.gpu
def test_gpu_global_rng_batch_matches_sequential_train_calls():
    rs = np.random.RandomState(3)
    X = rs.random_sample((3, 200))
    np.random.seed(11)
    D, st = ConvolutionalNMFLearner(8, 7).trainBatch(X, initMethod='random_samples', nbMaxIterations=4)
    assert D.shape == (3, 8, 7)
    np.random.seed(11)
    for b in range(3):
        assert np.array_equal(ConvolutionalNMFLearner(8, 7).train(X[b], nbMaxIterations=4), D[b])


@pytest.mark.gpu
def test_gpu_reference_unittest_shapes():
    """tests/hsc/test_modeling.py:79-90 of the reference (test_train_nmf_1d / _2d)."""
    sequence = np.random.random(size=(256,))
    D = ConvolutionalNMFLearner(k=16, windowSize=5).train(sequence, nbMaxIterations=100, initMethod='random_samples')
    assert np.array_equal(D.shape, [16, 5])
    assert np.all(np.isfinite(D)) and np.allclose(np.sum(np.square(D), axis=1), 1.0)
    nbFeatures = 4
    sequence = np.random.random(size=(256, nbFeatures))
    D = ConvolutionalNMFLearner(k=16, windowSize=5).train(sequence, nbMaxIterations=100, initMethod='random_samples')
    assert np.array_equal(D.shape, [16, 5, nbFeatures])
    assert np.all(np.isfinite(D)) and np.allclose(np.sum(np.square(D), axis=(1, 2)), 1.0)
