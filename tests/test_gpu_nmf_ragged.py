"""ConvolutionalNMF.computeCoefficientsRaggedBatch on the GPU (hscnmf_compute_ragged): against the
reference's goldens (tests/golden/nmf.npz, under the checks of tests/test_nmf.py), bit for bit against the uniform coder
signal by signal (tile edges, signals that stop at different iterations), and against itself (chunking, permutation,
determinism, input forms)."""
import numpy as np
import pytest

from hsc_amd import nmf
from hsc_amd.nmf import ConvolutionalNMF
from tests.test_gpu_nmf_corpus import EDGES, _edge_inputs
from tests.test_nmf import CASES, IDS, STOP_NAMES, _rel

pytestmark = pytest.mark.gpu


def stop_kw(c):
    return dict(nbMaxIterations=c['max_iterations'], toleranceResidualScale=c['tol_rs'], toleranceSnr=c['tol_snr'])


def check_golden(c, coef, resid, st, b):
    """Signal b of a ragged call against the case's golden: the checks of tests/test_nmf.py (test_gpu_float64_matches_reference,
    test_gpu_float32_within_reference_spread), unchanged."""
    assert coef.shape == c['coef'].shape and resid.shape == c['resid'].shape
    if c['x'].dtype == np.float64:
        assert coef.dtype == np.float64
        print(c['name'], 'coef', _rel(coef, c['coef']), 'resid', _rel(resid, c['resid']))
        assert _rel(coef, c['coef']) <= 1e-10
        assert _rel(resid, c['resid']) <= 1e-10
    else:
        assert coef.dtype == np.float32 and resid.dtype == np.float32
        for got, r32, r64 in ((coef, c['coef'], c['coef64']), (resid, c['resid'], c['resid64'])):
            spread = np.max(np.abs(r32.astype(np.float64) - r64))
            err = np.max(np.abs(got.astype(np.float64) - r64))
            print(c['name'], 'err', err, 'spread', spread)
            assert err <= 4.0 * spread + 1e-6 * np.max(np.abs(r64)), (c['name'], err, spread)
    assert int(st.iterations[b]) == int(c['iterations'])
    assert st.stop_reasons()[b] == STOP_NAMES[int(c['stop'])]


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_golden_as_a_corpus_of_one_signal(c):
    cnmf = ConvolutionalNMF()
    np.random.seed(int(c['seed']))
    coef, resid, st = cnmf.computeCoefficientsRaggedBatch([c['x']], c['D'], **stop_kw(c))
    assert len(coef) == len(resid) == 1 and st.iterations.shape == (1,)
    check_golden(c, coef[0], resid[0], st, 0)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_golden_between_two_unrelated_signals(c):
    """The case as signal 1 of three, its golden initial coefficients handed in; signals 0 and 2 are random, of other lengths."""
    x, D = c['x'], c['D']
    T, K, W = x.shape[0], D.shape[0], D.shape[1]
    np.random.seed(int(c['seed']))
    a1 = np.random.random((T, K)).astype(x.dtype) + 2.0                 # the reference's draw (hsc/modeling.py:684)
    rs = np.random.RandomState(int(c['seed']) + 7)
    sigs, a0s = [], []
    for Tb in (T + 37, max(W, T // 2 + 1)):
        sigs.append(rs.random_sample((Tb,) + x.shape[1:]).astype(x.dtype))
        a0s.append((rs.random_sample((Tb, K)) + 2.0).astype(x.dtype))
    coef, resid, st = ConvolutionalNMF().computeCoefficientsRaggedBatch([sigs[0], x, sigs[1]], D, initialCoefficients=[a0s[0], a1, a0s[1]],
                                                                        **stop_kw(c))
    assert [q.shape[0] for q in coef] == [T + 37, T, max(W, T // 2 + 1)]
    check_golden(c, coef[1], resid[1], st, 1)


def test_goldens_cover_the_tolerance_stops():
    names = {c['name']: int(c['stop']) for c in CASES}
    assert names['f64_snr'] == names['f64_f7_snr'] == names['f32_snr'] == 3 and names['f64_rs'] == names['f32_rs'] == 2


# ------------------------------------------------------------------------------------------------ against the uniform coder
def assert_same_as_per_signal(sigs, D, A0s, got, **kw):
    """Every signal of the ragged result `got`, bit for bit, against computeCoefficientsBatch on that signal alone.
    Returns the per-signal iteration counts."""
    coef, resid, st = got
    one = ConvolutionalNMF()
    its = []
    for b, (x, a) in enumerate(zip(sigs, A0s)):
        c1, r1, s1 = one.computeCoefficientsBatch(x[np.newaxis], D, initialCoefficients=a[np.newaxis], **kw)
        assert coef[b].dtype == c1.dtype and coef[b].shape == c1[0].shape and resid[b].shape == r1[0].shape
        assert np.array_equal(coef[b], c1[0]), ('coefficients', b)
        assert np.array_equal(resid[b], r1[0]), ('residual', b)
        assert int(st.iterations[b]) == int(s1.iterations[0]) and int(st.stop[b]) == int(s1.stop[0]), ('stop', b)
        assert st.snr[b] == s1.snr[0] and st.residual_scale[b] == s1.residual_scale[0], ('statistics', b)
        its.append(int(s1.iterations[0]))
    return its


# the tile-edge corpora of tests/test_gpu_nmf_corpus.py, and K = 8: the 16-byte loads of A (K a multiple of 8), with
# L = 295, 1, 124, 128 and 129 beside one another
SHAPES = EDGES + [(8, 6, 2, [300, 6, 129, 133, 134])]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('K,W,F,lengths', SHAPES, ids=['K%d-W%d-F%d-%s' % (e[0], e[1], e[2], '_'.join(map(str, e[3]))) for e in SHAPES])
def test_tile_edges_bit_for_bit(dtype, K, W, F, lengths):
    sigs, D, A0s = _edge_inputs(K, W, F, lengths)
    sigs, D, A0s = [q.astype(dtype) for q in sigs], D.astype(dtype), [a.astype(dtype) for a in A0s]
    kw = dict(nbMaxIterations=3)                                        # odd W: the result lies in the second buffer
    got = ConvolutionalNMF().computeCoefficientsRaggedBatch(sigs, D, initialCoefficients=A0s, **kw)
    off = (W - 1) // 2
    for c, T in zip(got[0], lengths):                                   # the centred layout: zero outside the L rows
        assert c.shape == (T, K) and not np.any(c[:off]) and not np.any(c[off + T - W + 1:]) and np.all(c[off:off + T - W + 1] > 0)
    assert assert_same_as_per_signal(sigs, D, A0s, got, **kw) == [3] * len(lengths)
    assert got[2].stop_reasons() == ['max_iterations'] * len(lengths)


# ------------------------------------------------------------------------------------------------ different stops
PLANTED = dict(seed=1, lengths=[300, 130, 260, 77, 200, 150, 410, 97], K=6, W=7, F=2, tolerance=13.45, iterations=12)


def planted_corpus(dtype, seed=PLANTED['seed'], lengths=PLANTED['lengths'], K=PLANTED['K'], W=PLANTED['W'], F=PLANTED['F']):
    """make_inputs(..., planted=True) of tools/make_golden_nmf.py for every signal of a corpus under one D: a little
    positive noise plus T // W atoms of D at random places, on which the SNR grows from one iteration to the next."""
    rs = np.random.RandomState(seed)
    D = rs.random_sample((K, W, F))
    D = D / np.sqrt(np.sum(np.square(D.reshape(K, -1)), axis=1)).reshape((K, 1, 1))
    sigs, A0s = [], []
    for T in lengths:
        x = 0.01 * rs.random_sample((T, F))
        for t in rs.randint(0, T - W + 1, size=max(2, T // W)):
            x[t:t + W] += (1.0 + rs.random_sample()) * D[rs.randint(K)]
        sigs.append(x.astype(dtype))
        A0s.append((rs.random_sample((T, K)) + 2.0).astype(dtype))
    return sigs, D.astype(dtype), A0s


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_signals_that_stop_at_different_iterations(dtype):
    """One SNR tolerance over planted signals, odd W: the signals stop after 4 to 12 iterations (the seed is chosen so), so
    their coefficients lie in either buffer of the pair ((n W) & 1) and stopped signals sit beside running ones."""
    sigs, D, A0s = planted_corpus(dtype)
    kw = dict(nbMaxIterations=PLANTED['iterations'], toleranceSnr=PLANTED['tolerance'])
    got = ConvolutionalNMF().computeCoefficientsRaggedBatch(sigs, D, initialCoefficients=A0s, **kw)
    its = assert_same_as_per_signal(sigs, D, A0s, got, **kw)
    print('iterations', its)
    assert len(set(its)) >= 3 and {n % 2 for n in its} == {0, 1} and max(its) == PLANTED['iterations'], its
    reasons = got[2].stop_reasons()
    assert 'max_iterations' in reasons and 'snr' in reasons
    assert all(r == ('max_iterations' if n == PLANTED['iterations'] else 'snr') for r, n in zip(reasons, its))
    assert got[2].timing_ms[4] == max(its) and got[2].timing_ms[3] == 1


# ------------------------------------------------------------------------------------------------ against itself
def _same(a, b):
    for p, q in zip(a[0], b[0]):
        assert np.array_equal(p, q)
    for p, q in zip(a[1], b[1]):
        assert np.array_equal(p, q)
    for k in ('iterations', 'stop', 'snr', 'residual_scale'):
        assert np.array_equal(getattr(a[2], k), getattr(b[2], k)), k


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_chunking_does_not_change_a_byte(dtype):
    """memoryBudget values from ragged_plan that give 1, 2 and B chunks (and one in between): identical results, and
    timing_ms[3] counts the chunks."""
    sigs, D, A0s = planted_corpus(dtype)
    lengths, B = [q.shape[0] for q in sigs], len(sigs)
    K, W, F = D.shape
    kw = dict(nbMaxIterations=PLANTED['iterations'], toleranceSnr=PLANTED['tolerance'], initialCoefficients=A0s)
    _, whole = nmf.ragged_plan(dtype, lengths, F, K, W, 1 << 40)
    budgets = {}
    for m in range(1, B):                                               # the bytes of the first m signals as the budget
        budget = nmf.ragged_plan(dtype, lengths[:m], F, K, W, 1 << 40)[1]
        budgets.setdefault(len(nmf.ragged_plan(dtype, lengths, F, K, W, budget)[0]) - 1, budget)
    budgets[1], budgets[B] = whole, 1
    assert 2 in budgets and len(budgets) >= 4, budgets
    ref = ConvolutionalNMF().computeCoefficientsRaggedBatch(sigs, D, **kw)
    assert ref[2].timing_ms[3] == 1
    for chunks, budget in sorted(budgets.items()):
        first, _ = nmf.ragged_plan(dtype, lengths, F, K, W, budget)
        assert len(first) - 1 == chunks
        got = ConvolutionalNMF(memoryBudget=budget).computeCoefficientsRaggedBatch(sigs, D, **kw)
        _same(got, ref)
        assert got[2].timing_ms[3] == chunks, (chunks, budget, got[2].timing_ms)
        # timing_ms[4] sums the iterations each chunk ran: the most any of its signals needed
        assert got[2].timing_ms[4] == sum(int(np.max(ref[2].iterations[a:b])) for a, b in zip(first[:-1], first[1:]))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_permutation_determinism_and_input_forms(dtype):
    sigs, D, A0s = planted_corpus(dtype)
    B = len(sigs)
    kw = dict(nbMaxIterations=PLANTED['iterations'], toleranceSnr=PLANTED['tolerance'])
    cnmf = ConvolutionalNMF()
    ref = cnmf.computeCoefficientsRaggedBatch(sigs, D, initialCoefficients=A0s, **kw)
    _same(cnmf.computeCoefficientsRaggedBatch(sigs, D, initialCoefficients=A0s, **kw), ref)        # two runs
    perm = np.random.RandomState(3).permutation(B)
    assert not np.array_equal(perm, np.arange(B))
    got = cnmf.computeCoefficientsRaggedBatch([sigs[i] for i in perm], D, initialCoefficients=[A0s[i] for i in perm], **kw)
    for j, i in enumerate(perm):
        assert np.array_equal(got[0][j], ref[0][i]) and np.array_equal(got[1][j], ref[1][i])
        for k in ('iterations', 'stop', 'snr', 'residual_scale'):
            assert getattr(got[2], k)[j] == getattr(ref[2], k)[i]
    # the padded array with NaN padding and `lengths`
    lengths = [q.shape[0] for q in sigs]
    padded = np.full((B, max(lengths) + 3, D.shape[2]), np.nan, dtype=dtype)
    for b, q in enumerate(sigs):
        padded[b, :q.shape[0]] = q
    got = cnmf.computeCoefficientsRaggedBatch(padded, D, initialCoefficients=A0s, lengths=lengths, **kw)
    assert all(np.all(np.isfinite(r)) for r in got[1])
    _same(got, ref)
    # a [B,T,F] array is the list of its rows, and the batch call on it (one length): the same bits
    X = np.stack([q[:lengths[3]] for q in sigs if q.shape[0] >= lengths[3]])
    A = np.stack([a[:lengths[3]] for a, q in zip(A0s, sigs) if q.shape[0] >= lengths[3]])
    got = cnmf.computeCoefficientsRaggedBatch(X, D, initialCoefficients=list(A), **kw)
    cb, rb, sb = cnmf.computeCoefficientsBatch(X, D, initialCoefficients=A, **kw)
    assert np.array_equal(np.stack(got[0]), cb) and np.array_equal(np.stack(got[1]), rb)
    assert np.array_equal(got[2].iterations, sb.iterations) and np.array_equal(got[2].snr, sb.snr)


def test_global_draws_equal_a_loop_of_compute_coefficients():
    sigs, D, _ = planted_corpus(np.float64, lengths=[90, 200, 33])
    sigs, D = [q[:, 0].copy() for q in sigs], D[:, :, 0].copy()          # 1-D signals, D [K,W]: squeezed residuals
    np.random.seed(11)
    coef, resid, _ = ConvolutionalNMF().computeCoefficientsRaggedBatch(sigs, D, nbMaxIterations=3)
    np.random.seed(11)
    for b, q in enumerate(sigs):
        c1, r1 = ConvolutionalNMF().computeCoefficients(q, D, nbMaxIterations=3)
        assert r1.shape == q.shape and np.array_equal(c1, coef[b]) and np.array_equal(r1, resid[b])
