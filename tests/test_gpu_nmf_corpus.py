"""ConvolutionalNMFLearner.trainCorpus on the GPU (hscnmf_learn_corpus): against the reference's
goldens (tests/golden/nmf_corpus.npz), against `train` for a corpus of one signal (bit for bit), against the float64
restatement at the tile edges of the ragged geometry, and against itself (input forms, determinism, the corpus stop rule,
the memory budget)."""
import re

import numpy as np
import pytest

from hsc_amd import _native
from hsc_amd.nmf import ConvolutionalNMFLearner
from tests import nmf_corpus_restatement as crst
from tests.test_gpu_nmf_limits import _close
from tests.test_nmf_corpus import CASES, stop_kw
from tests.test_nmf_learn import STOP_NAMES, _batch_inputs, _err

pytestmark = pytest.mark.gpu

F64 = [c for c in CASES if c['x'].dtype == np.float64]
F32 = [c for c in CASES if c['x'].dtype == np.float32 and c['D'].dtype == np.float32]
MIXED = [c for c in CASES if c['x'].dtype == np.float32 and c['D'].dtype == np.float64]


def _gpu_train(c):
    learner = ConvolutionalNMFLearner(c['K'], c['W'])
    D = learner.trainCorpus(c['signals'], initialDictionary=c['D_init'], initialCoefficients=c['A0s'], **stop_kw(c))
    st = learner.lastStats
    assert int(st.iterations[0]) == c['iterations']
    assert st.stop_reasons() == [STOP_NAMES[c['stop']]]
    assert st.signal_snr.shape == (len(c['signals']),) and st.signal_residual_scale.shape == (len(c['signals']),)
    assert st.residual_scale[0] == np.max(st.signal_residual_scale)
    return D


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize('c', F64, ids=[c['name'] for c in F64])
def test_float64_matches_reference(c):
    D = _gpu_train(c)
    assert D.shape == c['D'].shape and D.dtype == np.float64
    print('err', _err(D, c['D']))
    assert _err(D, c['D']) <= 1e-10, _err(D, c['D'])


@pytest.mark.parametrize('c', F32, ids=[c['name'] for c in F32])
def test_float32_within_reference_spread(c):
    D = _gpu_train(c)
    assert D.shape == c['D'].shape and D.dtype == np.float32
    spread = _err(c['D'], c['D64'])
    err = _err(D, c['D64'])
    print('err', err, 'spread', spread)
    assert err <= 4.0 * spread + 1e-6, (c['name'], err, spread)


@pytest.mark.parametrize('c', MIXED, ids=[c['name'] for c in MIXED])
def test_mixed_dtype_runs_in_float64(c):
    """float32 data with a float64 'noise' dictionary: the learner runs in float64, within 1e-10 of the reference's
    float64 run on the same values (the rule of test_nmf_learn.test_gpu_mixed_dtype_runs_in_float64)."""
    D = _gpu_train(c)
    assert D.shape == c['D'].shape and D.dtype == np.float64
    print('err', _err(D, c['D64']))
    assert _err(D, c['D64']) <= 1e-10, _err(D, c['D64'])


# ------------------------------------------------------------------------------------------------ one signal = train
@pytest.mark.parametrize('init', ['random_samples', 'noise'])
@pytest.mark.parametrize('F', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_corpus_of_one_signal_is_train_bit_for_bit(dtype, F, init):
    T, K, W = 300, 6, 6
    x = np.random.RandomState(F).random_sample((T,) if F == 1 else (T, F)).astype(dtype)
    one, cor = ConvolutionalNMFLearner(K, W), ConvolutionalNMFLearner(K, W)
    np.random.seed(29)
    D1 = one.train(x, initMethod=init, nbMaxIterations=4)
    np.random.seed(29)
    Dc = cor.trainCorpus([x], initMethod=init, nbMaxIterations=4)
    s1, sc = one.lastStats, cor.lastStats
    assert Dc.dtype == D1.dtype and Dc.shape == D1.shape and np.array_equal(Dc, D1)
    assert int(sc.iterations[0]) == int(s1.iterations[0]) == 4 and int(sc.stop[0]) == int(s1.stop[0])
    assert sc.snr[0] == s1.snr[0] and sc.residual_scale[0] == s1.residual_scale[0]
    assert sc.signal_snr[0] == s1.snr[0] and sc.signal_residual_scale[0] == s1.residual_scale[0]


# ------------------------------------------------------------------------------------------------ tile edges
# (K, W, F, lengths): row tiles of 128 coefficient rows, sample tiles of 128 samples
EDGES = [
    (7, 5, 3, [5, 132, 133, 260, 37]),      # L = 1, 128, 129, 256, 33: every offset off the 128-row grid
    (7, 5, 3, [133]),
    (7, 5, 3, [5]),
    (33, 33, 1, [160, 33, 300]),            # two K blocks in f32, three in f64; W*F across column blocks; L = 128, 1, 268
    (33, 33, 1, [300]),
    (9, 129, 1, [300, 129, 260]),           # the halo as wide as the tile; L = 172, 1, 132
    (9, 129, 1, [300]),
]


def _edge_inputs(K, W, F, lengths):
    rs = np.random.RandomState(K * 1000 + W * 10 + F)
    sigs = [rs.uniform(0.5, 1.5, (T, F)) for T in lengths]
    D = rs.uniform(0.5, 1.5, (K, W, F))
    D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
    A0s = [rs.uniform(1.0, 2.0, (T, K)) for T in lengths]
    return sigs, D, A0s


_edge_refs = {}


def _edge_ref(K, W, F, lengths, dtype, arithmetic):
    """The restatement in `arithmetic` on the inputs rounded to the run's dtype, computed once per shape."""
    key = (K, W, F, tuple(lengths), np.dtype(dtype).name, np.dtype(arithmetic).name)
    if key not in _edge_refs:
        sigs, D, A0s = _edge_inputs(K, W, F, lengths)
        sigs, D, A0s = [q.astype(dtype) for q in sigs], D.astype(dtype), [a.astype(dtype) for a in A0s]
        _edge_refs[key] = crst.learn_corpus(sigs, D, A0s, 2, dtype=arithmetic)
    return _edge_refs[key]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('K,W,F,lengths', EDGES, ids=['K%d-W%d-F%d-%s' % (e[0], e[1], e[2], '_'.join(map(str, e[3]))) for e in EDGES])
def test_ragged_tile_edges_match_restatement(dtype, K, W, F, lengths):
    """float64: 1e-10 relative; float32: 4x the spread of the float32 restatement + 1e-6 of the largest value (the rule of
    tests/test_gpu_nmf_limits.py)."""
    sigs, D0, A0s = _edge_inputs(K, W, F, lengths)
    sigs, D0, A0s = [q.astype(dtype) for q in sigs], D0.astype(dtype), [a.astype(dtype) for a in A0s]
    learner = ConvolutionalNMFLearner(K, W)
    D = learner.trainCorpus(sigs, nbMaxIterations=2, initialDictionary=D0, initialCoefficients=A0s)
    r64 = _edge_ref(K, W, F, lengths, dtype, np.float64)
    r32 = _edge_ref(K, W, F, lengths, dtype, np.float32) if dtype == np.float32 else None
    assert D.dtype == dtype and D.shape == (K, W, F)
    print('err', _err(D, r64[0]), 'spread', None if r32 is None else _err(r32[0], r64[0]))
    _close(D, r64[0], None if r32 is None else r32[0], 'D')
    st = learner.lastStats
    assert int(st.iterations[0]) == 2 and st.stop_reasons() == ['max_iterations']
    if dtype == np.float64:
        assert abs(st.snr[0] - r64[3]) <= 1e-9 and np.max(np.abs(st.signal_snr - r64[5])) <= 1e-9
        assert abs(st.residual_scale[0] - r64[4]) <= 1e-10 * r64[4]


# ------------------------------------------------------------------------------------------------ against itself
def _planted(dtype=np.float64, lengths=(300, 250, 180, 300, 97, 211)):
    """Planted signals whose residual shrinks (test_nmf_learn._batch_inputs), cut to different lengths."""
    X, D0, A0 = _batch_inputs(dtype)
    return [X[b, :T] for b, T in enumerate(lengths)], D0[0], [A0[b, :T] for b, T in enumerate(lengths)]


@pytest.mark.parametrize('F', [1, 2])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_input_forms_give_the_same_bits(dtype, F):
    """A [B,T] (F = 1) or [B,T,F] (F = 2) array, the list of its signals, and the padded array with `lengths` against the
    list of the cut signals."""
    X, D0, A0 = _batch_inputs(dtype, B=3, T=200)
    D0 = D0[0]
    if F == 1:
        X = np.ascontiguousarray(X[:, :, 0])                                         # [B,T]: 1-D signals, D [K,W]
        D0 = D0[:, :, 0] / np.sqrt(np.sum(np.square(D0[:, :, 0]), axis=1, keepdims=True))
    assert X.ndim == (2 if F == 1 else 3) and X.shape[2:] == ((2,) if F == 2 else ())
    learner = ConvolutionalNMFLearner(6, 6)
    kw = dict(nbMaxIterations=3, initialDictionary=D0)
    Da = learner.trainCorpus(X, initialCoefficients=list(A0), **kw)                  # the array
    Dl = learner.trainCorpus(list(X), initialCoefficients=list(A0), **kw)            # a list
    assert Da.shape == D0.shape and np.array_equal(Da, Dl)
    lengths = [200, 77, 131]
    padded = X.copy()
    for b, T in enumerate(lengths):
        padded[b, T:] = np.nan
    cut = [X[b, :T] for b, T in enumerate(lengths)]
    a0 = [A0[b, :T] for b, T in enumerate(lengths)]
    Dp = learner.trainCorpus(padded, lengths=lengths, initialCoefficients=a0, **kw)
    snr_p = learner.lastStats.snr[0]
    Dc = learner.trainCorpus(cut, initialCoefficients=a0, **kw)
    assert np.all(np.isfinite(Dp)) and np.array_equal(Dp, Dc) and snr_p == learner.lastStats.snr[0]
    assert not np.array_equal(Dp, Da)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_two_identical_calls_give_the_same_bits(dtype):
    sigs, D0, A0s = _planted(dtype)
    out = []
    for _ in range(2):
        learner = ConvolutionalNMFLearner(6, 6)
        D = learner.trainCorpus(sigs, nbMaxIterations=3, initialDictionary=D0, initialCoefficients=A0s)
        st = learner.lastStats
        out.append((D, st.snr.copy(), st.residual_scale.copy(), st.signal_snr.copy(), st.signal_residual_scale.copy()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_corpus_stop_rule():
    """The SNR tolerance is met by the corpus SNR, 10 log10(sum energy / sum r^2), not by a signal's: a tolerance half
    way between the corpus SNR of two consecutive iterations stops at the later one."""
    sigs, D0, A0s = _planted()
    learner = ConvolutionalNMFLearner(6, 6)
    kw = dict(initialDictionary=D0, initialCoefficients=A0s)
    S, sig = [], []
    for i in range(1, 7):
        learner.trainCorpus(sigs, nbMaxIterations=i, **kw)
        S.append(float(learner.lastStats.snr[0]))
        sig.append(learner.lastStats.signal_snr.copy())
    print('corpus SNR', S)
    # iteration i + 1 is the first at which the corpus reaches tol, and some signal of its own reaches it earlier: a
    # decision per signal would be seen to differ
    ok = [i for i in range(2, 6) if S[i] > max(S[:i]) + 1e-3
          and any(np.any(s >= 0.5 * (max(S[:i]) + S[i])) for s in sig[:i])]
    if not ok:
        pytest.fail('the planted corpus of _planted() no longer has an iteration at which a signal is ahead of the corpus: '
                    'corpus SNR %s, signal SNR %s' % (S, sig))
    i = ok[0]
    tol = 0.5 * (max(S[:i]) + S[i])
    D = learner.trainCorpus(sigs, nbMaxIterations=9, toleranceSnr=tol, **kw)
    st = learner.lastStats
    assert int(st.iterations[0]) == i + 1 and st.stop_reasons() == ['snr']
    assert st.signal_snr.shape == (len(sigs),)
    r = crst.learn_corpus(sigs, D0, A0s, 9, None, tol)
    assert (r[1], r[2]) == (i + 1, 3)
    assert abs(st.snr[0] - r[3]) <= 1e-9 and st.snr[0] == S[i]
    assert np.max(np.abs(st.signal_snr - r[5])) <= 1e-9
    _close(D, r[0], None, 'D')
    # the residual scale rule, on max_b max|r_b|: a tolerance just above the first iteration's value stops there
    learner.trainCorpus(sigs, nbMaxIterations=1, **kw)
    rs1 = float(learner.lastStats.residual_scale[0])
    assert rs1 == np.max(learner.lastStats.signal_residual_scale)
    learner.trainCorpus(sigs, nbMaxIterations=9, toleranceResidualScale=rs1 * (1.0 + 1e-6), **kw)
    assert int(learner.lastStats.iterations[0]) == 1 and learner.lastStats.stop_reasons() == ['residual_scale']


def corpus_bytes(lengths, K, W, F, itemsize):
    """The device bytes of a hscnmf_learn_corpus call, restated from learn_corpus_t: every buffer rounded up to 256."""
    Ts = np.asarray(lengths, dtype=np.int64)
    Ls = Ts - W + 1
    rows, arows, B = int(Ts.sum()), int(Ls.sum()), len(lengths)
    nrt, nst = int(np.sum((Ls + 127) // 128)), int(np.sum((Ts + 127) // 128))
    ld = W * F + 1
    sizes = [arows * K * itemsize] * 2 + [rows * F * itemsize] * 2 + [K * W * F * itemsize, nrt * K * ld * itemsize,
                                                                      B * K * ld * itemsize, nst * 2 * 8, B * 5 * 8, B * 40,
                                                                      (nrt + nst) * 8, 3 * 4 + 2 * 8]
    return sum((max(v, 256) + 255) // 256 * 256 for v in sizes)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_memory_budget(dtype):
    sigs, D0, A0s = _planted(dtype)
    kw = dict(nbMaxIterations=2, initialDictionary=D0, initialCoefficients=A0s)
    fresh = ConvolutionalNMFLearner(6, 6).trainCorpus(sigs, **kw)
    need = corpus_bytes([q.shape[0] for q in sigs], 6, 6, sigs[0].shape[1], np.dtype(dtype).itemsize)
    for budget in (1, need - 1):
        with pytest.raises(_native.HscmpError) as ei:
            ConvolutionalNMFLearner(6, 6, memoryBudget=budget).trainCorpus(sigs, **kw)
        assert ei.value.code == _native.ERR_ALLOC, str(ei.value)
        assert re.search(r'needs %d bytes' % need, str(ei.value)) and re.search(r'budget is %d bytes' % budget, str(ei.value))
    # the same context afterwards: an ordinary call, and one whose budget is just enough
    assert np.array_equal(ConvolutionalNMFLearner(6, 6).trainCorpus(sigs, **kw), fresh)
    assert np.array_equal(ConvolutionalNMFLearner(6, 6, memoryBudget=need).trainCorpus(sigs, **kw), fresh)


def test_grid_limit_is_unsupported_before_any_allocation():
    """B * ceil(K (W F + 1) / 256) workgroups of nmf_dsum_kernel lie on a 1-D grid, which HIP launches only below 2^32
    threads: 2^24 - 1 workgroups of 256.  1009 signals at K = 65535, W = 64 need 1009 * 16640 > 2^24 - 1: answered with
    HSCNMF_ERR_UNSUPPORTED before the byte count (a budget of 1 byte would otherwise answer HSCNMF_ERR_ALLOC) and before
    any buffer is read (the zeros below are never touched)."""
    from hsc_amd import nmf
    B, K, W = 1009, 65535, 64
    assert B * -(-(K * (W + 1)) // 256) > 2 ** 24 - 1 >= (B - 1) * -(-(K * (W + 1)) // 256)
    x = np.zeros((B * W, 1), dtype=np.float32)
    lengths = np.full((B,), W, dtype=np.int64)
    D0 = np.zeros((K, W, 1), dtype=np.float32)
    a0 = np.zeros((B, K), dtype=np.float32)
    params = nmf._params(1, None, None, 1)
    with pytest.raises(_native.HscmpError) as ei:
        nmf._call_learn_corpus(0, np.dtype(np.float32), x, lengths, D0, a0, np.zeros((B,)), params)
    assert ei.value.code == _native.ERR_UNSUPPORTED, str(ei.value)
    assert '%d' % (2 ** 24 - 1) in str(ei.value)
