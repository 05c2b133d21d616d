"""ConvolutionalKMeansLearner (the reference's ConvolutionalDictionaryLearner(algorithm='kmean'), hsc/modeling.py:420-524,
with every iteration on the GPU): the numpy restatement of the device step against the reference's goldens and
numpy's own sums, the argument checks and the missing-library error (CPU); hsc_amd.kmeans against the goldens, the
host learner, hscmp_assign_windows, separate runs of the batch and itself (GPU)."""
import logging
import os
import re

import numpy as np
import pytest

import golden_util as gu
from hsc_amd import _native
from hsc_amd import kmeans
from hsc_amd.kmeans import ConvolutionalKMeansLearner
from hsc_amd.learning import ConvolutionalDictionaryLearner
from tests import kmeans_restatement as rst

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kmeans.npz')
TRAIN_ARGS = ('nbRandomWindows', 'maxIterations', 'tolerance', 'initMethod', 'resetMethod', 'nbAveragedPatches')


def _cases():
    g = np.load(GOLDEN)
    out = []
    for name in g['names']:
        name = str(name)
        c = {k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(name + '/')}
        kw = {}
        for a in TRAIN_ARGS:
            if a in c:
                v = c[a]
                kw[a] = str(v) if v.dtype.kind == 'U' else (float(v) if a == 'tolerance' else int(v))
        out.append(dict(name=name, x=c['x'], K=int(c['K']), W=int(c['W']), seed=int(c['seed']), kw=kw, D=c['D'],
                        assign_t=c['assign_t'], assign_k=c['assign_k'], nbResets=c['nbResets'],
                        iterations=int(c['iterations'])))
    return out


CASES = _cases()
LEARN = sorted(gu.LEARN_CASES)


def _train(x, K, W, seed, kw):
    np.random.seed(seed)
    learner = ConvolutionalKMeansLearner(K, W)
    return learner.train(x, **kw), learner.lastStats


def _check_case(c, D, stats):
    assert D.dtype == c['D'].dtype and D.shape == c['D'].shape
    assert np.array_equal(D, c['D'])
    assert len(stats) == c['iterations']
    for i, s in enumerate(stats):
        assert np.array_equal(s['assignment'][0], c['assign_t'][i]), (c['name'], i)
        assert np.array_equal(s['assignment'][1], c['assign_k'][i]), (c['name'], i)
        assert s['nbResets'] == c['nbResets'][i]
        assert int(np.sum(s['counts'])) == c['assign_t'].shape[1]


def _learn_case(name):
    sig, k, w, seed, kw = gu.LEARN_CASES[name]
    return gu.learn_signal(sig), k, w, seed, kw, gu.load('learn_small.npz')[name + '__D']


@pytest.fixture
def restated(monkeypatch):
    """hsc_amd.kmeans on the numpy twin of libhsckmeans.so."""
    monkeypatch.setattr(kmeans, '_contexts', {0: rst.FakeContext()})
    monkeypatch.setattr(kmeans, 'load_library', lambda: None)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('name', LEARN)
def test_restatement_matches_learn_small(name, restated):
    x, k, w, seed, kw, exp = _learn_case(name)
    D, _ = _train(x, k, w, seed, kw)
    assert D.dtype == exp.dtype and np.array_equal(D, exp)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_restatement_matches_kmeans_golden(c, restated):
    D, stats = _train(c['x'], c['K'], c['W'], c['seed'], c['kw'])
    _check_case(c, D, stats)


def test_fixtures_cover_the_issue_matrix():
    by = {c['name']: c for c in CASES}
    s = by['sparse_level']
    assert s['x'].ndim == 2 and s['x'].shape[1] == 8 and s['W'] * 8 <= 256
    assert np.mean(np.all(s['x'] == 0.0, axis=1)) > 0.5
    assert by['f32_noise']['x'].dtype == np.float32 and by['f32_noise']['kw']['initMethod'] == 'noise'
    r = by['f32_noise_reset']
    assert r['x'].dtype == np.float32 and r['D'].dtype == np.float64 and r['nbResets'].sum() > 0
    assert by['average']['kw']['resetMethod'] == 'random_samples_average'
    t = by['tolerance_stop']
    assert t['kw']['tolerance'] > 0.0 and t['iterations'] < t['kw']['maxIterations']
    w0 = by['window0_only']
    assert any(np.array_equal(np.flatnonzero(k == c), [0]) for k in w0['assign_k'] for c in range(w0['K']))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [5, 15, 16, 36, 528, 1584])
def test_pairwise_norm_and_sequential_mean_are_numpys(n, dtype):
    rs = np.random.RandomState(n)
    for F in (1, 3, 8, 48):
        if n % F:
            continue
        p = (rs.randn(40, n // F, F) * np.exp(3.0 * rs.randn(40, 1, 1))).astype(dtype)
        p[3] = 0.0
        assert np.array_equal(rst.pairwise_sum(np.square(p).reshape(40, -1)), np.sum(np.square(p), axis=(1, 2)))
        for m in (1, 2, 9, 40):
            ref = np.mean(p[:m], axis=0)
            got = rst.sequential_mean(p[:m])
            assert got.dtype == ref.dtype and np.array_equal(got, ref)


class _DeviceTouched(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise _DeviceTouched()
    monkeypatch.setattr(kmeans, 'load_library', touched)
    monkeypatch.setattr(kmeans, '_context', touched)
    monkeypatch.setattr(_native, 'default_engine', touched)


def test_argument_checks_raise_before_any_device_call(no_device):
    x = np.random.RandomState(0).randn(500)
    state = np.random.get_state()
    with pytest.raises(Exception, match='Unsupported initialization method'):
        ConvolutionalKMeansLearner(4, 16).train(x, 50, initMethod='bogus')
    with pytest.raises(Exception, match='Unsupported reset method'):
        ConvolutionalKMeansLearner(4, 16).train(x, 50, resetMethod='bogus')
    with pytest.raises(ValueError):
        ConvolutionalKMeansLearner(4, 250).train(x, 50)                    # 2W >= T
    with pytest.raises(ValueError):
        ConvolutionalKMeansLearner(0, 16).train(x, 50)
    with pytest.raises(ValueError):
        ConvolutionalKMeansLearner(4, 16).train(x, 0)
    with pytest.raises(ValueError):
        ConvolutionalKMeansLearner(4, 16).train(np.zeros((500, 2, 2)), 50)
    with pytest.raises(ValueError):
        ConvolutionalKMeansLearner(4, 16).train(x.astype(np.int64), 50)
    with pytest.raises(ValueError):
        ConvolutionalKMeansLearner(4, 16).trainBatch(x, 50)                # batch needs [B,T(,F)]
    with pytest.raises(ValueError):
        ConvolutionalKMeansLearner(4, 16).trainBatch(np.stack([x, x]), 50, rngs=[np.random.RandomState(0)])
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:3], state[1:3]))    # nothing drawn
    # valid arguments reach the device
    with pytest.raises(_DeviceTouched):
        ConvolutionalKMeansLearner(4, 16).train(x, 50)
    with pytest.raises(_DeviceTouched):
        ConvolutionalKMeansLearner(4, 16).train(np.asmatrix(x.reshape(-1, 1)), 50)


def test_no_library_raises_hscmp_error(monkeypatch):
    monkeypatch.setattr(kmeans, '_lib', None)
    monkeypatch.setattr(kmeans, '_contexts', {})
    monkeypatch.setattr(kmeans, 'LIB_PATH', os.path.join(os.path.dirname(kmeans.LIB_PATH), 'missing', 'libhsckmeans.so'))
    x = np.random.RandomState(0).randn(500)
    with pytest.raises(_native.HscmpError):
        ConvolutionalKMeansLearner(4, 16).train(x, 50)
    with pytest.raises(_native.HscmpError):
        ConvolutionalKMeansLearner(4, 16).trainBatch(np.stack([x, x]), 50)


# ------------------------------------------------------------------------------------------------ GPU
def level_data(T, F, seed, dtype=np.float64, density=2e-3):
    """Level-style input: a sparse [T, F] coefficient stream (F = 1: a sparse signal of planted bursts)."""
    rs = np.random.RandomState(seed)
    x = np.zeros((T, F))
    for c in rs.randint(0, T - 16, max(1, int(density * T * max(1, F // 4)))):
        for _ in range(rs.randint(1, 5)):
            x[c + rs.randint(0, 16), rs.randint(F)] = rs.uniform(0.5, 2.0) * rs.choice([-1.0, 1.0])
    return x.astype(dtype)


def _host(x, K, W, seed, kw):
    np.random.seed(seed)
    return ConvolutionalDictionaryLearner(K, W, algorithm='kmean').train(x, **kw)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('name', LEARN)
def test_train_matches_learn_small(name):
    x, k, w, seed, kw, exp = _learn_case(name)
    D, _ = _train(x, k, w, seed, kw)
    assert _same(D, exp)


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_train_matches_kmeans_golden(c):
    D, stats = _train(c['x'], c['K'], c['W'], c['seed'], c['kw'])
    _check_case(c, D, stats)


SCRIPT_LEVELS = [(16, 32, 1), (32, 33, 16), (64, 33, 48)]


@pytest.mark.gpu
@pytest.mark.parametrize('K,W,F', SCRIPT_LEVELS, ids=['level0', 'level1', 'level2'])
def test_script_shapes_match_host_learner(K, W, F):
    x = level_data(20000, F, seed=K)
    if F == 1:
        x = x[:, 0].astype(np.float32)
    kw = dict(nbRandomWindows=10000, maxIterations=10, tolerance=0.0, resetMethod='random_samples')
    assert _same(_train(x, K, W, 3, kw)[0], _host(x, K, W, 3, kw))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('init', ['random_samples', 'noise'])
@pytest.mark.parametrize('reset', ['random_samples', 'random_samples_average', 'noise'])
def test_methods_and_dtypes_match_host_learner(reset, init, dtype):
    x = level_data(6000, 4, seed=7, dtype=dtype)
    kw = dict(nbRandomWindows=800, maxIterations=5, tolerance=0.0, initMethod=init, resetMethod=reset, nbAveragedPatches=3)
    assert _same(_train(x, 12, 20, 11, kw)[0], _host(x, 12, 20, 11, kw))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_1d_and_single_feature_inputs_match_host_learner(dtype):
    x = (np.random.RandomState(5).randn(5000) * (np.random.RandomState(6).rand(5000) < 0.1)).astype(dtype)
    kw = dict(nbRandomWindows=600, maxIterations=4, tolerance=0.0, resetMethod='noise')
    for inp in (x, x[:, None]):
        D = _train(inp, 8, 17, 2, kw)[0]
        assert _same(D, _host(inp, 8, 17, 2, kw))
    assert _train(np.asmatrix(x[:, None]), 8, 17, 2, kw)[0].shape == (8, 17, 1)


def _windows(x, starts, W):
    return x[starts[:, None] + np.arange(2 * W)[None, :]]


@pytest.mark.gpu
@pytest.mark.parametrize('W,F,dtype', [(16, 1, np.float32), (9, 4, np.float64), (33, 16, np.float32), (33, 48, np.float64),
                                       (3, 5, np.float64)])
def test_step_assignment_matches_hscmp_assign_windows(W, F, dtype):
    rs = np.random.RandomState(W * F)
    K, N, T = 21, 700, 3000
    x = level_data(T, F, seed=W, dtype=dtype, density=2e-2)
    x[:200] = 0.0                                                         # all-zero windows: (0, 0)
    D = rs.randn(K, W, F)
    D[5] = D[2]                                                           # duplicated atoms: the lower one wins
    D[17] = -D[9]
    D = (D / np.sqrt(np.sum(D ** 2, axis=(1, 2), keepdims=True))).astype(dtype)
    starts = rs.randint(0, T - 2 * W, N).astype(np.int64)
    starts[:50] = rs.randint(0, 200 - 2 * W, 50) if W < 90 else 0
    ctx = kmeans._context(0)
    ctx.set_data(np.ascontiguousarray(x[None]), starts[None], W)
    mode = np.array([1 if dtype == np.float32 else 2], dtype=np.int32)
    t, k, count, nonzero, sums, _ = ctx.step(D.astype(np.float64)[None], mode)
    eng = _native.default_engine(0)
    eng.set_dictionary(np.ascontiguousarray(D))
    t_ref, k_ref, _ = eng.assign_windows(np.ascontiguousarray(_windows(x, starts, W)))
    assert np.array_equal(t[0], t_ref) and np.array_equal(k[0], k_ref)
    assert np.sum(count) == N and not np.any(k[0] == 5) and not np.any(k[0] == 17)
    assert t[0][0] == 0 and k[0][0] == 0
    # the sums against the restatement
    fake = rst.FakeContext()
    fake.set_data(np.ascontiguousarray(x[None]), starts[None], W)
    t2, k2, count2, nonzero2, sums2, _ = fake.step(D.astype(np.float64)[None], mode)
    assert np.array_equal(t2, t) and np.array_equal(k2, k)
    assert np.array_equal(count2, count) and np.array_equal(nonzero2, nonzero)
    assert sums.dtype == sums2.dtype and np.array_equal(sums, sums2)


@pytest.mark.gpu
def test_float32_data_under_a_float64_dictionary():
    """Assignment in float64 on widened float32 windows, sums in float32 (hscmp_assign_windows on widened windows)."""
    rs = np.random.RandomState(3)
    W, F, K, N = 12, 3, 9, 500
    x = level_data(2000, F, seed=4, dtype=np.float32, density=5e-2)
    D = rs.uniform(-1, 1, (K, W, F))
    starts = rs.randint(0, 2000 - 2 * W, N).astype(np.int64)
    ctx = kmeans._context(0)
    ctx.set_data(np.ascontiguousarray(x[None]), starts[None], W)
    t, k, count, nonzero, sums, _ = ctx.step(D[None], np.array([2], dtype=np.int32))
    eng = _native.default_engine(0)
    eng.set_dictionary(np.ascontiguousarray(D))
    t_ref, k_ref, _ = eng.assign_windows(np.ascontiguousarray(_windows(x, starts, W).astype(np.float64)))
    assert np.array_equal(t[0], t_ref) and np.array_equal(k[0], k_ref)
    assert sums.dtype == np.float32


@pytest.mark.gpu
def test_train_batch_matches_separate_trains():
    B, K, W = 4, 8, 16
    xs = np.stack([level_data(4000, 3, seed=20 + b) for b in range(B)])
    kw = dict(nbRandomWindows=500, maxIterations=8, tolerance=1.4, resetMethod='random_samples')
    learner = ConvolutionalKMeansLearner(K, W)
    Db, stats = learner.trainBatch(xs, rngs=[np.random.RandomState(100 + b) for b in range(B)], **kw)
    assert Db.shape == (B, K, W, 3)
    iters = []
    for b in range(B):
        one = ConvolutionalKMeansLearner(K, W, rng=np.random.RandomState(100 + b))
        D = one.train(xs[b], **kw)
        assert _same(Db[b], D), b
        assert len(stats[b]) == len(one.lastStats)
        assert [s['nbResets'] for s in stats[b]] == [s['nbResets'] for s in one.lastStats]
        iters.append(len(one.lastStats))
    assert len(set(iters)) > 1, iters                                     # learners stopped at different iterations
    # one shared generator: windows and D learner by learner, then the resets learner by learner
    Dg, _ = ConvolutionalKMeansLearner(K, W).trainBatch(xs[:2], rngs=np.random.RandomState(9), **kw)
    Dh, _ = ConvolutionalKMeansLearner(K, W).trainBatch(xs[:2], rngs=np.random.RandomState(9), **kw)
    assert np.array_equal(Dg, Dh)


@pytest.mark.gpu
def test_two_runs_bit_identical_and_stats(caplog):
    x = level_data(20000, 16, seed=2)
    kw = dict(nbRandomWindows=3000, maxIterations=4, tolerance=0.0, resetMethod='random_samples')
    D1, st1 = _train(x, 32, 33, 4, kw)
    D2, st2 = _train(x, 32, 33, 4, kw)
    assert np.array_equal(D1, D2)
    for a, b in zip(st1, st2):
        assert np.array_equal(a['assignment'][1], b['assignment'][1]) and a['alpha'] == b['alpha']
    with caplog.at_level(logging.DEBUG):
        _host(x, 32, 33, 4, kw)
    host_resets = [int(re.search(r'nb resets = (\d+)', r.getMessage()).group(1)) for r in caplog.records
                   if r.getMessage().startswith('K-mean iteration')]
    assert host_resets == [s['nbResets'] for s in st1]
    for s in st1:
        assert int(np.sum(s['counts'])) == 3000 and s['counts'].shape == (32,)
        assert s['step_ms'] > 0.0 and s['kernel_ms'] > 0.0 and s['assign_ms'] > 0.0
