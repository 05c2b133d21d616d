"""ConvolutionalKMeansLearner.trainCorpus (one dictionary from many signals) on the CPU: the
learner on the numpy twin of the corpus context against the reference's goldens (tests/golden/kmeans_corpus.npz), the
draw rule at its edges, the three input forms, the argument checks and the exported symbols.  The GPU side is
tests/test_gpu_kmeans_corpus.py."""
import os

import numpy as np
import pytest

from hsc_amd import _native
from hsc_amd import kmeans
from hsc_amd.kmeans import ConvolutionalKMeansLearner
from tests import kmeans_corpus_restatement as crst

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kmeans_corpus.npz')
TRAIN_ARGS = ('nbRandomWindows', 'maxIterations', 'tolerance', 'initMethod', 'resetMethod', 'nbAveragedPatches')


def golden_cases():
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
        signals = np.split(c['x'], np.cumsum(c['lengths'])[:-1])
        out.append(dict(name=name, signals=signals, form=str(c['form']), K=int(c['K']), W=int(c['W']), seed=int(c['seed']),
                        kw=kw, D=c['D'], assign_t=c['assign_t'], assign_k=c['assign_k'], nbResets=c['nbResets'],
                        iterations=int(c['iterations']), win_signal=c['win_signal'], win_start=c['win_start']))
    return out


CASES = golden_cases()


def train_case(c):
    """trainCorpus on a golden case in the form it was recorded for; returns (D, learner)."""
    np.random.seed(c['seed'])
    learner = ConvolutionalKMeansLearner(c['K'], c['W'])
    seqs = np.stack(c['signals']) if c['form'] == 'array' else list(c['signals'])
    return learner.trainCorpus(seqs, **c['kw']), learner


def check_case(c, D, learner):
    assert D.dtype == c['D'].dtype and D.shape == c['D'].shape
    stats = learner.lastStats
    assert len(stats) == c['iterations']
    for i, s in enumerate(stats):
        assert np.array_equal(s['assignment'][0], c['assign_t'][i]), (c['name'], i)
        assert np.array_equal(s['assignment'][1], c['assign_k'][i]), (c['name'], i)
        assert s['nbResets'] == c['nbResets'][i], (c['name'], i)
        assert int(np.sum(s['counts'])) == c['assign_t'].shape[1]
    assert np.array_equal(D, c['D'])
    assert np.array_equal(learner.lastWindows[0], c['win_signal']) and np.array_equal(learner.lastWindows[1], c['win_start'])


@pytest.fixture
def restated(monkeypatch):
    """hsc_amd.kmeans on the numpy twin of libhsckmeans.so."""
    monkeypatch.setattr(kmeans, '_contexts', {0: crst.FakeCorpusContext()})
    monkeypatch.setattr(kmeans, 'load_library', lambda: None)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_restatement_matches_corpus_golden(c, restated):
    D, learner = train_case(c)
    check_case(c, D, learner)


def test_fixtures_cover_the_issue_matrix():
    by = {c['name']: c for c in CASES}
    u = by['uniform_b4']
    assert u['form'] == 'array' and len(u['signals']) == 4 and u['signals'][0].dtype == np.float64
    r = by['ragged_short']
    assert min(len(q) for q in r['signals']) == 2 * r['W'] + 1
    b = int(np.argmin([len(q) for q in r['signals']]))
    assert np.any(r['win_signal'] == b) and np.all(r['win_start'][r['win_signal'] == b] == 0)     # its one admissible start, drawn
    assert by['odd_w']['W'] % 2 == 1
    s = by['sparse_level_f3']
    assert s['signals'][0].ndim == 2 and s['signals'][0].shape[1] == 3
    assert np.mean(np.all(np.concatenate(s['signals']) == 0.0, axis=1)) > 0.5
    assert by['f32_noise']['signals'][0].dtype == np.float32 and by['f32_noise']['kw']['initMethod'] == 'noise'
    p = by['f32_noise_reset']
    assert p['signals'][0].dtype == np.float32 and p['D'].dtype == np.float64 and p['nbResets'].sum() > 0
    for name, method in (('end_samples', 'random_samples'), ('end_average', 'random_samples_average')):
        e = by[name]
        assert e['kw']['resetMethod'] == method and e['nbResets'].sum() > 0
        assert max(len(q) for q in e['signals']) <= 2 * e['W'] + 4             # every patch lies next to its signal's end
    t = by['tolerance_stop']
    assert t['kw']['tolerance'] > 0.0 and t['iterations'] < t['kw']['maxIterations']
    w0 = by['window0_only']
    assert any(np.array_equal(np.flatnonzero(k == c), [0]) for k in w0['assign_k'] for c in range(w0['K']))
    for c in CASES:
        assert 40 <= min(len(q) for q in c['signals']) or c['name'] in ('ragged_short', 'end_samples', 'end_average')
        assert c['iterations'] <= 6 and 200 <= c['assign_t'].shape[1] <= 400
    assert os.path.getsize(GOLDEN) < 200 * 1024


# ------------------------------------------------------------------------------------------------ the draw rule
class _Scripted(object):
    """A generator whose randint returns the given values (and checks the call)."""

    def __init__(self, values, high):
        self.values, self.high = np.asarray(values, dtype=np.int64), high

    def randint(self, low, high, size):
        assert low == 0 and high == self.high and tuple(size) == self.values.shape
        return self.values


def test_draw_rule_edges():
    lens, width = [50, 21, 40], 20
    signals = [np.zeros(n) for n in lens]
    A = np.array(lens) - width                                        # 30, 1, 20
    C = np.cumsum(A)
    g = [0, C[0] - 1, C[0], C[1] - 1, C[1], C[2] - 1]
    sig, start = kmeans.corpus_windows(signals, len(g), width, _Scripted(g, int(C[-1])))
    assert sig.tolist() == [0, 0, 1, 1, 2, 2]
    assert start.tolist() == [0, A[0] - 1, 0, 0, 0, A[2] - 1]         # g = C[b] - 1: the last start of b; g = C[b]: start 0 of b + 1
    assert np.all(start + width < np.array(lens)[sig])                # the reference's high is exclusive: T_b - width is never a start
    sig2, start2 = crst.corpus_windows(signals, len(g), width, _Scripted(g, int(C[-1])))
    assert np.array_equal(sig, sig2) and np.array_equal(start, start2)


@pytest.mark.parametrize('seed', [0, 7])
def test_draw_rule_matches_restatement_and_train(seed):
    rs = np.random.RandomState(seed)
    signals = [np.zeros(n) for n in rs.randint(41, 400, 9)]
    a = kmeans.corpus_windows(signals, 500, 40, np.random.RandomState(seed))
    b = crst.corpus_windows(signals, 500, 40, np.random.RandomState(seed))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].min() == 0 and a[0].max() == 8
    # one signal: the starts are train's own (extractRandomWindows: randint(low=0, high=T - width, size=(nb,)))
    sig, start = kmeans.corpus_windows(signals[:1], 300, 40, np.random.RandomState(seed))
    assert not sig.any()
    assert np.array_equal(start, np.random.RandomState(seed).randint(low=0, high=len(signals[0]) - 40, size=(300,)))


def _signals(dtype=np.float64, F=None, seed=3):
    rs = np.random.RandomState(seed)
    out = []
    for T in (300, 45, 170):
        x = rs.standard_normal((T,) if F is None else (T, F)) * (rs.rand(T, *([] if F is None else [1])) < 0.3)
        out.append(x.astype(dtype))
    return out


@pytest.mark.parametrize('F', [None, 2])
def test_one_signal_corpus_is_train(F, restated):
    x = _signals(np.float32, F)[0]
    kw = dict(nbRandomWindows=60, maxIterations=3, resetMethod='noise')
    for init in ('random_samples', 'noise'):
        np.random.seed(5)
        ref = ConvolutionalKMeansLearner(5, 8).train(x, initMethod=init, **kw)
        for form in ([x], x[np.newaxis]):
            np.random.seed(5)
            D = ConvolutionalKMeansLearner(5, 8).trainCorpus(form, initMethod=init, **kw)
            assert D.dtype == ref.dtype and D.shape == ref.shape and np.array_equal(D, ref)


@pytest.mark.parametrize('F', [None, 2])
def test_list_and_padded_forms_agree(F, restated):
    signals = _signals(np.float64, F)
    kw = dict(nbRandomWindows=80, maxIterations=3, resetMethod='random_samples')
    learner = ConvolutionalKMeansLearner(5, 8, rng=np.random.RandomState(1))
    D = learner.trainCorpus(signals, **kw)
    assert D.shape == ((5, 8) if F is None else (5, 8, F))
    assert learner.lastWindows[0].shape == (80,) and set(learner.lastWindows[0]) <= {0, 1, 2}
    lens = [len(q) for q in signals]
    padded = np.full((3, max(lens)) + signals[0].shape[1:], np.nan)
    for b, q in enumerate(signals):
        padded[b, :len(q)] = q
    Dp = ConvolutionalKMeansLearner(5, 8, rng=np.random.RandomState(1)).trainCorpus(padded, lengths=lens, **kw)
    Dt = ConvolutionalKMeansLearner(5, 8, rng=np.random.RandomState(1)).trainCorpus(tuple(signals), **kw)
    assert np.array_equal(D, Dp) and np.array_equal(D, Dt) and not np.any(np.isnan(D))
    # 'noise' draws between the signals' own extremes: the padding is not read there either
    kw = dict(nbRandomWindows=80, maxIterations=2, initMethod='noise')
    Dn = ConvolutionalKMeansLearner(5, 8, rng=np.random.RandomState(2)).trainCorpus(signals, **kw)
    Dq = ConvolutionalKMeansLearner(5, 8, rng=np.random.RandomState(2)).trainCorpus(padded, lengths=lens, **kw)
    assert np.array_equal(Dn, Dq) and not np.any(np.isnan(Dn))


# ------------------------------------------------------------------------------------------------ arguments, symbols
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
    rs = np.random.RandomState(0)
    good = [rs.randn(500), rs.randn(300)]
    L = ConvolutionalKMeansLearner
    state = np.random.get_state()
    with pytest.raises(Exception, match='Unsupported initialization method'):
        L(4, 16).trainCorpus(good, 50, initMethod='bogus')
    with pytest.raises(Exception, match='Unsupported reset method'):
        L(4, 16).trainCorpus(good, 50, resetMethod='bogus')
    with pytest.raises(ValueError, match='signal 1 has 32 samples'):
        L(4, 16).trainCorpus([good[0], rs.randn(32)], 50)                     # T_b = 2W
    with pytest.raises(ValueError, match='signal 0 has 10 samples'):
        L(4, 16).trainCorpus(np.zeros((3, 40)), 50, lengths=[10, 40, 40])
    with pytest.raises(ValueError):
        L(0, 16).trainCorpus(good, 50)
    with pytest.raises(ValueError):
        L(4, 16).trainCorpus(good, 0)
    with pytest.raises(NotImplementedError):
        L(4, 256).trainCorpus([rs.randn(600)], 50)                            # W > MAX_WINDOW_SIZE
    with pytest.raises(NotImplementedError):
        L(4, 1).trainCorpus(good, 50)                                         # W * F = 1
    with pytest.raises(ValueError):
        L(4, 16).trainCorpus(good[0], 50)                                     # an array corpus is [B,T(,F)]
    with pytest.raises(ValueError):
        L(4, 16).trainCorpus([], 50)
    with pytest.raises(ValueError):
        L(4, 16).trainCorpus([good[0], rs.randn(300, 2)], 50)                 # one F
    with pytest.raises(ValueError):
        L(4, 16).trainCorpus([good[0], good[1].astype(np.float32)], 50)       # one dtype
    with pytest.raises(ValueError):
        L(4, 16).trainCorpus([q.astype(np.int64) for q in good], 50)
    with pytest.raises(ValueError):
        L(4, 16).trainCorpus(good, 50, lengths=[500, 300])                    # lengths= goes with a padded array
    with pytest.raises(ValueError):
        L(4, 16).trainCorpus(np.zeros((2, 100)), 50, lengths=[100, 101])
    big = [np.broadcast_to(np.zeros((1, 4), dtype=np.float32), (2 ** 28, 4))] * 2 + [np.zeros((40, 4), dtype=np.float32)]
    with pytest.raises(NotImplementedError, match='2\\^31 - 1 elements'):
        L(4, 16).trainCorpus(big, 50)                                         # sum T_b * F = 2^31 + 160 (views: nothing that large is allocated)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:3], state[1:3]))    # nothing drawn
    with pytest.raises(_DeviceTouched):
        L(4, 16).trainCorpus(good, 50)
    with pytest.raises(_DeviceTouched):
        L(4, 16).trainCorpus(np.zeros((2, 100)), 50, lengths=[100, 33])


def test_new_entry_points_are_exported():
    assert 'hsckmeans_set_corpus' in kmeans.EXPORTS and 'hsckmeans_set_plan' in kmeans.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hsckmeans.h')).read()
    for name, value in (('WIDE_CHUNK_WINDOWS', kmeans.WIDE_CHUNK_WINDOWS), ('WIDE_RING_ROWS', kmeans.WIDE_RING_ROWS),
                        ('WIDE_MAX_K', kmeans.WIDE_MAX_K), ('WIDE_FROM_WINDOWS', kmeans.WIDE_FROM_WINDOWS)):
        import re
        m = re.search(r'HSCKMEANS_%s = (\d+)' % name, header)
        assert m and int(m.group(1)) == value, name
