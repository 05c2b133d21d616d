"""B independent K-SVD sweeps in one launch (hscksvd_update_batch) and ConvolutionalKSVDLearner.trainBatch on top of it and
of the dictionary-per-signal encode.

update_batch: problem b equals ksvd.update on problem b bit for bit -- D, coefficient values and stats -- in both branches, for
problems that are dense in occurrences, have an atom without occurrence, an atom with one occurrence, or no stored entry at
all; and, as the three entry points share one driver, every problem also equals the float64 restatement
(tests/ksvd_restatement.py) within ksvd.update's tolerances, problems of very different entry counts included.  trainBatch: learner b equals train on sequences[b] with the same seed, bit for bit, every learner stops on its own, and
a shared generator draws the initial dictionaries in batch order."""
import numpy as np
import pytest
import scipy.sparse

pytestmark = pytest.mark.gpu

K, W, T = 4, 6, 60


def _coefficients(rng, counts):
    """[T,K] CSC with counts[k] entries in column k at random rows."""
    rows, cols, vals = [], [], []
    for k, n in enumerate(counts):
        r = np.sort(rng.choice(T, size=n, replace=False))
        rows.extend(r); cols.extend([k] * n); vals.extend(rng.randn(n))
    return scipy.sparse.csc_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))),
                                   shape=(T, K))


def _problems(F, seed=0):
    rng = np.random.RandomState(seed)
    Ds = rng.randn(4, K, W, F) if F > 1 else rng.randn(4, K, W)
    Ds /= np.sqrt(np.sum(Ds.reshape((4, K, -1)) ** 2, axis=2)).reshape((4, K) + (1,) * (Ds.ndim - 2))
    Cs = [_coefficients(rng, [25, 30, 20, 28]),        # dense in occurrences: the patches overlap everywhere
          _coefficients(rng, [9, 0, 7, 11]),           # atom 1 has no occurrence
          _coefficients(rng, [8, 6, 1, 10]),           # atom 2 has one occurrence
          scipy.sparse.csc_matrix((T, K))]             # no stored entry at all
    return Ds, Cs


def _same_update(single, batch_D, batch_C, batch_stats, what):
    D1, C1, st1, _ = single
    assert np.array_equal(D1, batch_D), what + ': D'
    assert np.array_equal(C1.indptr, batch_C.indptr) and np.array_equal(C1.indices, batch_C.indices), what + ': structure'
    assert np.array_equal(C1.data, batch_C.data), what + ': coefficient values'
    assert np.array_equal(st1, batch_stats), what + ': stats'


@pytest.mark.parametrize('F,usePCA', [(1, False), (2, False), (1, True)], ids=['F1_svd', 'F2_svd', 'F1_pca'])
def test_update_batch_equals_update(F, usePCA):
    from hsc_amd import ksvd
    Ds, Cs = _problems(F)
    Ds0, Cs0 = Ds.copy(), [c.copy() for c in Cs]
    newD, newC, stats, timing = ksvd.update_batch(Ds, Cs, usePCA=usePCA)
    assert newD.shape == Ds.shape and newD.dtype == np.float64 and stats.shape == (4, K, 4) and timing.shape == (3,)
    assert np.array_equal(Ds, Ds0) and all((a != b).nnz == 0 for a, b in zip(Cs, Cs0)), 'an input was modified'
    for b in range(4):
        _same_update(ksvd.update(Ds[b], Cs[b], usePCA=usePCA), newD[b], newC[b], stats[b], 'problem %d' % b)
    assert stats[1, 1, 0] == 0 and np.array_equal(newD[1, 1], Ds[1, 1])          # no occurrence: the atom is kept
    assert stats[2, 2, 0] == 1 and stats[2, 2, 3] == 0                           # one occurrence: no eigensolver
    assert np.array_equal(newD[3], Ds[3]) and not stats[3].any()                 # no entry: the dictionary is kept
    assert not np.array_equal(newD[0], Ds[0])
    # B = 1, and a batch in another order (a problem's result does not depend on its neighbours)
    oneD, oneC, one_stats, _ = ksvd.update_batch(Ds[:1], Cs[:1], usePCA=usePCA)
    _same_update(ksvd.update(Ds[0], Cs[0], usePCA=usePCA), oneD[0], oneC[0], one_stats[0], 'B = 1')
    order = [3, 0, 2, 1]
    pD, pC, p_stats, _ = ksvd.update_batch(Ds[order], [Cs[i] for i in order], usePCA=usePCA)
    for i, b in enumerate(order):
        assert np.array_equal(pD[i], newD[b]) and np.array_equal(pC[i].data, newC[b].data) and np.array_equal(p_stats[i], stats[b])
    # a list of dictionaries
    lD, _, _, _ = ksvd.update_batch([Ds[0], Ds[1]], Cs[:2], usePCA=usePCA)
    assert np.array_equal(lD, newD[:2])


@pytest.mark.parametrize('F,usePCA', [(1, False), (2, False), (1, True)], ids=['F1_svd', 'F2_svd', 'F1_pca'])
def test_update_batch_matches_restatement(F, usePCA):
    """Every problem of the batch against the float64 restatement, at ksvd.update's tolerances: an anchor outside the library,
    which test_update_batch_equals_update (one driver behind both sides) is not."""
    from hsc_amd import ksvd
    from tests.test_gpu_ksvd_limits import compare_with_restatement
    Ds, Cs = _problems(F)
    newD, newC, stats, _ = ksvd.update_batch(Ds, Cs, usePCA=usePCA)
    for b in range(4):
        st_ref = compare_with_restatement((newD[b], newC[b], stats[b]), Ds[b], Cs[b], usePCA)
        assert np.any(st_ref[:, 3] == 1) == (b < 3)                              # (eigenvectors were taken)


@pytest.mark.parametrize('usePCA', [False, True], ids=['svd', 'pca'])
def test_update_batch_uneven_problems_match_restatement(usePCA):
    """Problems of 103, 0 and 1 stored entries, the empty one in the middle, in both orders: an entry offset or a patch offset
    that is wrong puts a problem's entries or patches into a neighbour's."""
    from hsc_amd import ksvd
    from tests.test_gpu_ksvd_limits import compare_with_restatement
    rng = np.random.RandomState(5)
    Ds = rng.randn(3, K, W)
    Ds /= np.sqrt(np.sum(Ds ** 2, axis=2, keepdims=True))
    Cs = [_coefficients(rng, [25, 30, 20, 28]), scipy.sparse.csc_matrix((T, K)), _coefficients(rng, [0, 1, 0, 0])]
    assert [c.nnz for c in Cs] == [103, 0, 1]
    for order in ([0, 1, 2], [2, 1, 0]):
        newD, newC, stats, _ = ksvd.update_batch(Ds[order], [Cs[b] for b in order], usePCA=usePCA)
        for i, b in enumerate(order):
            compare_with_restatement((newD[i], newC[i], stats[i]), Ds[b], Cs[b], usePCA)
        assert [int(np.sum(stats[i, :, 0])) for i in range(3)] == [Cs[b].nnz for b in order]
        assert np.array_equal(newD[1], Ds[1]) and not np.array_equal(newD[order.index(0)], Ds[0])


def test_update_batch_all_empty():
    from hsc_amd import ksvd
    Ds, _ = _problems(1)
    newD, newC, stats, _ = ksvd.update_batch(Ds[:2], [scipy.sparse.csc_matrix((T, K))] * 2)
    assert np.array_equal(newD, Ds[:2]) and not stats.any() and all(c.nnz == 0 for c in newC)


def test_update_batch_library_refusals():
    """The limits and messages of hscksvd_update, through the C entry point."""
    from hsc_amd import _native, ksvd
    ctx = ksvd._context(0)
    p = _native._ptr
    D = np.zeros((1, 2, 33, 2)); off = np.zeros(2, dtype=np.int64); ip = np.zeros((1, 3), dtype=np.int32)
    with pytest.raises(_native.HscmpError, match='hscksvd_update_batch: W \\* F = 66 exceeds the limit of 64') as ei:
        ctx.call('update_batch', 1, 100, 2, 33, 2, p(D), p(off), p(ip), None, None, 0, None, None)
    assert ei.value.code == -5
    with pytest.raises(_native.HscmpError, match='hscksvd_update_batch: the PCA branch needs F = 1 \\(got F = 2\\)') as ei:
        ctx.call('update_batch', 1, 100, 2, 8, 2, p(D), p(off), p(ip), None, None, 1, None, None)
    assert ei.value.code == -5
    ip[0, 2] = 3                                       # indptr and entry_offsets disagree
    with pytest.raises(_native.HscmpError, match='problem 0: indptr\\[K\\] = 3') as ei:
        ctx.call('update_batch', 1, 100, 2, 8, 1, p(D), p(off), p(ip), None, None, 0, None, None)
    assert ei.value.code == -1
    # the same three inputs through hscksvd_update and hscksvd_update_corpus: the same texts under their own names, no problem
    # named; they have no entry_offsets to disagree with, so the third is three entries without indices or data
    rows = np.array([0, 100], dtype=np.int32)
    for fn, lead, plan in (('update', (100,), ()), ('update_corpus', (1, p(rows)), (0,))):
        refused = []
        for W, F, pca in ((33, 2, 0), (8, 2, 1), (8, 1, 0)):
            with pytest.raises(_native.HscmpError) as ei:
                ctx.call(fn, *lead, 2, W, F, p(D), p(ip), None, None, pca, *plan, None, None)
            assert 'problem' not in str(ei.value)
            refused.append((ei.value.code, str(ei.value).split(': ', 1)[1]))     # ('<fn> failed (<rc>): <the library's text>')
        assert refused == [(-5, 'hscksvd_%s: W * F = 66 exceeds the limit of 64' % fn),
                           (-5, 'hscksvd_%s: the PCA branch needs F = 1 (got F = 2)' % fn),
                           (-1, 'hscksvd_%s: indices or data is NULL' % fn)]
    # and a refusal of the per-problem checks, which only the batch prefixes
    ip[0, 0] = 5
    with pytest.raises(_native.HscmpError, match='hscksvd_update_batch: problem 0: indptr\\[0\\] = 5, expected 0'):
        ctx.call('update_batch', 1, 100, 2, 8, 1, p(D), p(off), p(ip), None, None, 0, None, None)
    with pytest.raises(_native.HscmpError, match='hscksvd_update: indptr\\[0\\] = 5, expected 0'):
        ctx.call('update', 100, 2, 8, 1, p(D), p(ip), None, None, 0, None, None)
    with pytest.raises(_native.HscmpError, match='hscksvd_update_corpus: indptr\\[0\\] = 5, expected 0'):
        ctx.call('update_corpus', 1, p(rows), 2, 8, 1, p(D), p(ip), None, None, 0, 0, None, None)


# ---- trainBatch ------------------------------------------------------------------------------------------------------
TK, TW, TT, TB = 4, 8, 400, 3


def _signals(seed=4):
    rng = np.random.RandomState(seed)
    x = np.zeros((TB, TT))
    for b in range(TB):
        atoms = rng.randn(TK, TW)
        for _ in range(30):
            t = rng.randint(0, TT - TW)
            x[b, t:t + TW] += rng.randn() * atoms[rng.randint(TK)]
        x[b] += 0.01 * rng.randn(TT)
    # learner 2: an exact multiple of learner 0's signal, so small that every coefficient falls below minCoefficients: its
    # first encode stores nothing, its sweep keeps the dictionary, alpha is exactly 0 and it stops after its first iteration
    # (alpha > tolerance fails at the default tolerance 0.0) -- alone: the others run their four iterations
    x[2] = x[0] * 2.0 ** -80
    return x


def _same_stats(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for i, (u, v) in enumerate(zip(a, b)):
        assert u['alpha'] == v['alpha'] and u['nnz'] == v['nnz'], (what, i, u['alpha'], v['alpha'], u['nnz'], v['nnz'])
        assert np.array_equal(u['n_k'], v['n_k']) and np.array_equal(u['eigenvalues'], v['eigenvalues']), (what, i)


@pytest.fixture(scope='module')
def single_runs():
    """train on every signal with its own seeded generator, both methods: computed once, shared, left unchanged."""
    from hsc_amd.ksvd import ConvolutionalKSVDLearner
    x = _signals()
    runs = {}
    for method in ('cmp', 'locomp'):
        for b in range(TB):
            learner = ConvolutionalKSVDLearner(TK, TW, rng=np.random.RandomState(100 + b))
            D = learner.train(x[b], method=method, maxIterations=4, nbNonzeroCoefs=12)
            runs[method, b] = (D, learner.lastStats)
    return x, runs


@pytest.mark.parametrize('method', ['cmp', 'locomp'])
def test_train_batch_equals_train(single_runs, method):
    from hsc_amd.ksvd import ConvolutionalKSVDLearner
    x, runs = single_runs
    learner = ConvolutionalKSVDLearner(TK, TW)
    D, stats = learner.trainBatch(x, method=method, maxIterations=4, nbNonzeroCoefs=12,
                                  rngs=[np.random.RandomState(100 + b) for b in range(TB)])
    assert D.shape == (TB, TK, TW) and D.dtype == np.float64 and stats is learner.lastStats
    assert [len(s) for s in stats] == [4, 4, 1], 'learner 2 stops alone after its first iteration'
    assert stats[2][0]['alpha'] == 0.0 and stats[2][0]['nnz'] == 0
    for b in range(TB):
        D1, st1 = runs[method, b]
        assert np.array_equal(D[b], D1), 'learner %d' % b
        _same_stats(stats[b], st1, 'learner %d' % b)
        assert all(s['variant'].endswith('_multi') for s in stats[b])


def test_train_batch_shared_generator_draws_in_batch_order(single_runs):
    from hsc_amd.ksvd import ConvolutionalKSVDLearner
    from hsc_amd.learning import ConvolutionalDictionaryLearner
    x, _ = single_runs
    shared = np.random.RandomState(7)
    init = ConvolutionalDictionaryLearner(TK, TW, rng=shared)
    D0 = np.stack([np.asarray(init._init_D(x[b], initMethod='noise'), dtype=np.float64) for b in range(TB)])
    # maxIterations = 0: the initial dictionaries come back as drawn
    D, stats = ConvolutionalKSVDLearner(TK, TW).trainBatch(x, maxIterations=0, rngs=np.random.RandomState(7))
    assert np.array_equal(D, D0) and stats == [[], [], []]
    # the learner's own generator when rngs is None
    D, _ = ConvolutionalKSVDLearner(TK, TW, rng=np.random.RandomState(7)).trainBatch(x, maxIterations=0)
    assert np.array_equal(D, D0)
    # ... and one iteration from them is update_batch of the multi-dictionary encode
    from hsc_amd import ksvd
    from hsc_amd.modeling import LoCOMP
    D1, _ = ConvolutionalKSVDLearner(TK, TW).trainBatch(x, maxIterations=1, nbNonzeroCoefs=12, rngs=np.random.RandomState(7))
    res = LoCOMP().computeCoefficientsMultiBatch(x, D0, nbNonzeroCoefs=12, toleranceSnr=40.0)
    assert np.array_equal(D1, ksvd.update_batch(D0, res.coefficients)[0])
