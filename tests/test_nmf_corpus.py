"""ConvolutionalNMFLearner.trainCorpus (ONE NMF dictionary from many signals) on the CPU: the float64
restatement against the reference's goldens (tests/golden/nmf_corpus.npz: the reference's _train_nmf on the concatenation
with the straddling coefficient rows at zero), the restatement of one signal against the single-signal restatement, the
draw order and dtypes, the argument errors and the input forms.  The GPU tests are in tests/test_gpu_nmf_corpus.py."""
import os

import numpy as np
import pytest

from hsc_amd import _native, nmf
from hsc_amd.learning import ConvolutionalDictionaryLearner
from hsc_amd.nmf import ConvolutionalNMFLearner
from tests import nmf_corpus_restatement as crst
from tests import nmf_learn_restatement as lrst
from tests.test_nmf_learn import _err, _gpu_visible

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nmf_corpus.npz')


def split(stack, lengths):
    """The signals (or per-signal coefficient arrays) of a stack."""
    ends = np.cumsum(lengths)
    return [stack[e - n:e] for e, n in zip(ends, lengths)]


def load_cases():
    g = np.load(GOLDEN)
    out = []
    for name in g['names']:
        name = str(name)
        c = {k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(name + '/')}
        c['name'] = name
        c['init'] = str(c['init'])
        c['tol_rs'] = None if np.isnan(c['tol_rs']) else float(c['tol_rs'])
        c['tol_snr'] = None if np.isnan(c['tol_snr']) else float(c['tol_snr'])
        for k in ('K', 'W', 'max_iterations', 'iterations', 'stop'):
            c[k] = int(c[k])
        c['signals'] = split(c['x'], c['lengths'])
        c['A0s'] = split(c['A0'], c['lengths'])
        out.append(c)
    return out


CASES = load_cases()
IDS = [c['name'] for c in CASES]


def ref64(c):
    return c['D64'] if 'D64' in c else c['D']


def stop_kw(c):
    return dict(nbMaxIterations=c['max_iterations'], toleranceResidualScale=c['tol_rs'], toleranceSnr=c['tol_snr'])


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_restatement_matches_reference_float64(c):
    D, iters, stop, snr, _, sig_snr, _ = crst.learn_corpus([x.astype(np.float64) for x in c['signals']],
                                                           c['D_init'].astype(np.float64),
                                                           [a.astype(np.float64) for a in c['A0s']],
                                                           c['max_iterations'], c['tol_rs'], c['tol_snr'])
    ref = ref64(c)
    assert _err(D.reshape(ref.shape), ref) <= 1e-11
    assert iters == c['iterations']
    assert stop == c['stop']
    assert len(sig_snr) == len(c['signals'])
    if 'D64' not in c:
        assert abs(snr - float(c['snr'])) <= 1e-5          # (the reference's record prints six decimals)


def test_fixtures_cover_the_issue_matrix():
    assert any(3 <= len(c['lengths']) <= 5 and c['x'].ndim == 1 and len(set(c['lengths'].tolist())) > 1 for c in CASES)
    assert any(3 <= len(c['lengths']) <= 5 and c['x'].ndim == 2 and c['x'].shape[1] == 3 for c in CASES)
    assert any(c['W'] in c['lengths'].tolist() for c in CASES)
    assert {c['stop'] for c in CASES} == {1, 2, 3}
    for c in CASES:
        if c['stop'] == 3:
            assert c['margin'] >= 1e-3
        elif c['stop'] == 2:
            assert c['margin'] >= 1e-4
        if c['x'].dtype == np.float32:
            assert 'D64' in c and c['D64'].dtype == np.float64
    assert any(c['x'].dtype == np.float32 and c['D'].dtype == np.float32 for c in CASES)
    assert any(c['x'].dtype == np.float32 and c['init'] == 'noise' and c['D'].dtype == np.float64 for c in CASES)
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize('K,W,F,T,iters,tol', [(3, 4, 1, 17, 4, None), (5, 7, 2, 130, 3, None), (4, 5, 3, 20, 6, 3.0)])
def test_restatement_of_one_signal_is_the_single_signal_restatement(K, W, F, T, iters, tol):
    rs = np.random.RandomState(K * 100 + W)
    x = rs.uniform(0.5, 1.5, (T, F))
    D0 = rs.uniform(0.5, 1.5, (K, W, F))
    A0 = rs.uniform(1.0, 2.0, (T, K))
    for dtype in (np.float64, np.float32):
        one = lrst.learn(x, D0, A0, iters, None, tol, dtype=dtype)
        cor = crst.learn_corpus([x], D0, [A0], iters, None, tol, dtype=dtype)
        assert np.array_equal(one[0], cor[0]) and one[0].dtype == cor[0].dtype
        assert one[1:5] == cor[1:5]
        assert cor[5][0] == one[3] and cor[6][0] == one[4]


def test_restatement_is_the_single_signal_restatement_on_the_zeroed_concatenation():
    """The identity the goldens rest on, in the restatements: the corpus sums are the single-signal learner's sums on the
    concatenation once the straddling rows start at zero (they differ only by the order of the additions)."""
    K, W, F, lengths = 5, 7, 2, [130, 7, 260, 40]
    rs = np.random.RandomState(5)
    sigs = [rs.uniform(0.5, 1.5, (T, F)) for T in lengths]
    D0 = rs.uniform(0.5, 1.5, (K, W, F))
    A0s = [rs.uniform(1.0, 2.0, (T, K)) for T in lengths]
    cat = []
    for a in A0s:
        a = a.copy()
        a[a.shape[0] - W + 1:] = 0.0
        cat.append(a)
    one = lrst.learn(np.concatenate(sigs), D0, np.concatenate(cat), 3)
    cor = crst.learn_corpus(sigs, D0, A0s, 3)
    assert _err(one[0], cor[0]) <= 1e-13
    assert one[1:3] == cor[1:3] and abs(one[3] - cor[3]) <= 1e-10 and abs(one[4] - cor[4]) <= 1e-12


# ------------------------------------------------------------------------------------------------ the Python layer
def _capture(monkeypatch):
    captured = {}

    def fake(device, dt, x, lengths, D0, a0, energy, params):
        captured.update(dt=dt, x=x, lengths=lengths, D0=D0, a0=a0, energy=energy, max_iterations=params.max_iterations,
                        calls=captured.get('calls', 0) + 1)
        st = nmf.NMFStats(np.ones(1, np.int32), np.ones(1, np.int32), np.zeros(1), np.zeros(1), np.zeros(5))
        st.signal_snr, st.signal_residual_scale = np.zeros(len(lengths)), np.zeros(len(lengths))
        return D0.copy(), st
    monkeypatch.setattr(nmf, '_call_learn_corpus', fake)
    return captured


def _ragged(dtype, F, lengths=(40, 9, 23)):
    rs = np.random.RandomState(1)
    return [rs.random_sample((T,) if F == 1 else (T, F)).astype(dtype) for T in lengths]


@pytest.mark.parametrize('init', ['random_samples', 'noise'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('F', [1, 3])
def test_draw_order_and_dtypes(monkeypatch, init, dtype, F):
    """trainCorpus draws the dictionary first (corpus_windows / uniform over the stack), then the coefficients signal by
    signal, from the global generator or from `rng`; computes in _compute_dtype(data, D_init); hands over the stack, the
    rows 0 .. L_b-1 of every signal's coefficients and the signals' energies; returns D in D_init's dtype."""
    from hsc_amd.kmeans import corpus_windows
    from hsc_amd.utils import normalize
    captured = _capture(monkeypatch)
    K, W = 5, 4
    sigs = _ragged(dtype, F)
    lengths = [q.shape[0] for q in sigs]
    np.random.seed(17)
    learner = ConvolutionalNMFLearner(K, W)
    D = learner.trainCorpus(sigs, initMethod=init, nbMaxIterations=None)
    np.random.seed(17)
    stack = np.concatenate(sigs).reshape((-1, F))
    if init == 'noise':
        d0 = normalize(np.random.uniform(low=np.min(stack), high=np.max(stack), size=(K, W, F)))
    else:
        ib, it = corpus_windows(sigs, K, W)
        off = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        d0 = normalize(np.stack([stack[off[b] + t:off[b] + t + W] for b, t in zip(ib, it)]))
    a0 = [np.random.random((T, K)).astype(dtype) + 2.0 for T in lengths]
    dt = np.float64 if (dtype == np.float64 or init == 'noise') else np.float32
    assert captured['dt'] == dt and captured['max_iterations'] == 1
    assert captured['x'].dtype == dt and captured['D0'].dtype == dt and captured['a0'].dtype == dt
    assert captured['lengths'].dtype == np.int64 and captured['lengths'].tolist() == lengths
    assert captured['x'].shape == (sum(lengths), F) and np.array_equal(captured['x'], stack.astype(dt))
    assert captured['D0'].shape == (K, W, F) and np.array_equal(captured['D0'], d0.astype(dt))
    assert captured['a0'].shape == (sum(T - W + 1 for T in lengths), K)
    assert np.array_equal(captured['a0'], np.concatenate([a[:T - W + 1] for a, T in zip(a0, lengths)]).astype(dt))
    assert np.array_equal(captured['energy'], [np.sum(np.square(q)) for q in split(captured['x'], lengths)])
    assert captured['energy'].dtype == np.float64
    assert D.dtype == d0.dtype and D.shape == ((K, W) if F == 1 else (K, W, F))
    assert learner.lastStats.signal_snr.shape == (len(sigs),) and learner.lastStats.snr.shape == (1,)
    # the same draws from a seeded RandomState given as rng
    first = {k: captured[k].copy() for k in ('D0', 'a0')}
    ConvolutionalNMFLearner(K, W, rng=np.random.RandomState(17)).trainCorpus(sigs, initMethod=init, nbMaxIterations=2)
    assert np.array_equal(captured['D0'], first['D0']) and np.array_equal(captured['a0'], first['a0'])
    assert captured['max_iterations'] == 2
    # explicit initial values: no draw at all
    state = np.random.get_state()[1].copy()
    ConvolutionalNMFLearner(K, W).trainCorpus(sigs, initialDictionary=d0, initialCoefficients=a0, nbMaxIterations=3)
    assert np.array_equal(np.random.get_state()[1], state)
    assert np.array_equal(captured['D0'], first['D0']) and np.array_equal(captured['a0'], first['a0'])


@pytest.mark.parametrize('init', ['random_samples', 'noise'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('F', [1, 3])
def test_one_signal_draws_are_trains(monkeypatch, init, dtype, F):
    """For one signal the draws are the reference's (train's): _init_D on the signal, then random((T, K)) + 2.0."""
    captured = _capture(monkeypatch)
    K, W, T = 5, 4, 40
    x = _ragged(dtype, F, (T,))[0]
    np.random.seed(23)
    D = ConvolutionalNMFLearner(K, W).trainCorpus([x], initMethod=init, nbMaxIterations=2)
    np.random.seed(23)
    d0 = ConvolutionalDictionaryLearner(K, W, algorithm='nmf')._init_D(x, init)
    a0 = np.random.random((T, K)).astype(dtype) + 2.0
    dt = captured['dt']
    assert np.array_equal(captured['D0'].reshape(d0.shape), d0.astype(dt))
    assert np.array_equal(captured['a0'], a0[:T - W + 1].astype(dt))
    assert D.dtype == d0.dtype and D.shape == d0.shape
    # ... and what trainBatch hands to hscnmf_learn for that signal
    seen = {}

    def fake_learn(device, dt, x, D0, a0, energy, params):
        seen.update(x=x, D0=D0, a0=a0, energy=energy)
        return D0.copy(), nmf.NMFStats(np.ones(1, np.int32), np.ones(1, np.int32), np.zeros(1), np.zeros(1), np.zeros(5))
    monkeypatch.setattr(nmf, '_call_learn', fake_learn)
    np.random.seed(23)
    ConvolutionalNMFLearner(K, W).train(x, initMethod=init, nbMaxIterations=2)
    assert np.array_equal(seen['x'][0], captured['x']) and np.array_equal(seen['D0'][0], captured['D0'])
    assert np.array_equal(seen['a0'][0][:T - W + 1], captured['a0']) and np.array_equal(seen['energy'], captured['energy'])


def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(nmf, '_context', no_device)
    monkeypatch.setattr(nmf, 'load_library', no_device)
    monkeypatch.setattr(nmf, '_call_learn_corpus', no_device)


def _sig(*lengths, **kw):
    return [np.random.RandomState(T).random_sample((T,) + kw.get('tail', ())).astype(kw.get('dtype', np.float64)) for T in lengths]


BAD = [
    ('w_below_2', 1, dict(sequences=_sig(30, 40), initMethod='noise'), 'filter width'),
    ('shorter_than_w', 8, dict(sequences=_sig(30, 7, 40), initMethod='noise'), 'signal 1'),
    ('as_long_as_w_random_samples', 8, dict(sequences=_sig(30, 8), initMethod='random_samples'), 'longer than the filter'),
    ('mixed_dtypes', 4, dict(sequences=_sig(30) + _sig(31, dtype=np.float32)), 'one dtype'),
    ('mixed_f', 4, dict(sequences=_sig(30, tail=(2,)) + _sig(31, tail=(3,))), 'same F'),
    ('mixed_ndim', 4, dict(sequences=_sig(30) + _sig(31, tail=(1,))), 'same F'),
    ('empty_list', 4, dict(sequences=[]), 'at least one signal'),
    ('empty_array', 4, dict(sequences=np.zeros((0, 30))), 'at least one signal'),
    ('lengths_with_list', 4, dict(sequences=_sig(30, 40), lengths=[30, 40]), 'lengths='),
    ('lengths_too_long', 4, dict(sequences=np.zeros((2, 30)), lengths=[30, 31]), 'padded length'),
    ('lengths_count', 4, dict(sequences=np.zeros((2, 30)), lengths=[30]), 'entries'),
    ('one_dimension', 4, dict(sequences=np.zeros((30,))), 'dimensions'),
    ('init_method', 4, dict(sequences=_sig(30, 40), initMethod='zeros'), 'Unsupported initialization method'),
    ('dictionary_shape', 4, dict(sequences=_sig(30, 40), initialDictionary=np.ones((4, 5))), 'initial dictionary'),
    ('coefficients_count', 4, dict(sequences=_sig(30, 40), initialCoefficients=[np.ones((30, 4))]), 'initial coefficient arrays'),
    ('coefficients_shape', 4, dict(sequences=_sig(30, 40), initialCoefficients=[np.ones((30, 4)), np.ones((39, 4))]),
     'initial coefficients of signal 1'),
]


@pytest.mark.parametrize('name,W,kw,needle', BAD, ids=[b[0] for b in BAD])
def test_argument_errors_raise_before_any_device_call(monkeypatch, name, W, kw, needle):
    _no_device(monkeypatch)
    with pytest.raises(Exception) as ei:
        ConvolutionalNMFLearner(4, W).trainCorpus(nbMaxIterations=2, **kw)
    assert not isinstance(ei.value, AssertionError), ei.value
    assert needle in str(ei.value), str(ei.value)
    assert 'k-means' not in str(ei.value)


def test_noise_accepts_a_signal_as_long_as_the_filter(monkeypatch):
    captured = _capture(monkeypatch)
    D = ConvolutionalNMFLearner(4, 8).trainCorpus(_sig(30, 8), initMethod='noise', nbMaxIterations=2)
    assert D.shape == (4, 8) and captured['a0'].shape == (23 + 1, 4) and captured['calls'] == 1


@pytest.mark.parametrize('F', [1, 2])
def test_input_forms_prepare_the_same_stack(monkeypatch, F):
    """[B,T] array = list of its rows; padded + lengths with NaN padding = the list of the signals."""
    captured = _capture(monkeypatch)
    K, W = 3, 4
    sigs = _ragged(np.float64, F)
    lengths = [q.shape[0] for q in sigs]
    padded = np.full((len(sigs), max(lengths) + 5) + sigs[0].shape[1:], np.nan)
    for b, q in enumerate(sigs):
        padded[b, :q.shape[0]] = q
    got = []
    for kw in (dict(sequences=sigs), dict(sequences=tuple(sigs)), dict(sequences=padded, lengths=lengths),
               dict(sequences=padded, lengths=np.array(lengths, dtype=np.int32))):
        np.random.seed(3)
        ConvolutionalNMFLearner(K, W).trainCorpus(initMethod='random_samples', nbMaxIterations=2, **kw)
        got.append({k: captured[k].copy() for k in ('x', 'lengths', 'D0', 'a0', 'energy')})
        assert np.all(np.isfinite(captured['x'])) and np.all(np.isfinite(captured['D0']))
    for g in got[1:]:
        for k in g:
            assert np.array_equal(g[k], got[0][k]), k
    same = np.stack([q[:lengths[1]] for q in sigs])            # [B,T(,F)]: every row a signal
    np.random.seed(3)
    ConvolutionalNMFLearner(K, W).trainCorpus(same, nbMaxIterations=2)
    a = {k: captured[k].copy() for k in ('x', 'lengths', 'D0', 'a0')}
    np.random.seed(3)
    ConvolutionalNMFLearner(K, W).trainCorpus(list(same), nbMaxIterations=2)
    for k in a:
        assert np.array_equal(a[k], captured[k]), k


def test_entry_point_is_exported_and_typed():
    assert 'hscnmf_learn_corpus' in nmf.EXPORTS
    lib = nmf.load_library()
    assert len(lib.hscnmf_learn_corpus.argtypes) == 20


def test_algorithm_nmf_is_still_not_routed():
    with pytest.raises(NotImplementedError):
        ConvolutionalDictionaryLearner(4, 8, algorithm='nmf').train(np.random.random(64))


def test_no_cpu_path():
    if _gpu_visible():
        pytest.skip('a GPU is visible: the no-GPU error path cannot be exercised here')
    with pytest.raises(_native.HscmpError):
        ConvolutionalNMFLearner(4, 8).trainCorpus(_sig(64, 30), nbMaxIterations=2)
    with pytest.raises(_native.HscmpError):
        ConvolutionalNMFLearner(4, 8).trainCorpus(np.random.random((2, 64, 3)), initMethod='noise', nbMaxIterations=2)
