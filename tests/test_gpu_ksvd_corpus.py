"""The corpus form of the K-SVD learner on the GPU: hsc_amd.ksvd.update_corpus against hscksvd_update at the contract's
two anchors (bit for bit), against the restatement where signal ends matter, against itself (plans, runs), and
ConvolutionalKSVDLearner.trainCorpus against `train` and against the restatement's corpus learner."""
import numpy as np
import pytest
import scipy.sparse

from hsc_amd import _native
from hsc_amd import ksvd
from hsc_amd.ksvd import ConvolutionalKSVDLearner
from tests import ksvd_corpus_restatement as crst
from tests import test_ksvd as single
from tests import test_ksvd_corpus as cpu

pytestmark = pytest.mark.gpu

PLANS = ('one', 'wide')


def _same_update(a, b):
    """(D, matrix or list, stats, ...) of two device updates: D, values and every stat (the Jacobi sweep count too)."""
    return cpu.same_bits(a, b)


# ------------------------------------------------------------------------------------------------ the two anchors
@pytest.mark.parametrize('plan', PLANS)
@pytest.mark.parametrize('name,shape,pca', single.UPDATE_INPUTS, ids=[u[0] for u in single.UPDATE_INPUTS])
def test_one_signal_equals_update(name, shape, pca, plan):
    D, A = single._random_input(*shape)
    ref = ksvd.update(D, A, usePCA=pca)
    out = ksvd.update_corpus(D, [A], usePCA=pca, plan=plan)
    assert len(out[1]) == 1 and out[1][0].shape == A.shape
    assert _same_update(out, ref)
    assert np.any(ref[2][:, 3] > 0)                              # (eigenvectors were taken)


def _large_ragged_lengths():
    return [int(t) for t in np.random.RandomState(9).randint(2000, 8000, 24)]


# (name, lengths, K, W, F, nnz per signal, seed, usePCA); every signal longer than W
INTERIOR = [
    ('uniform', [400, 400, 400], 8, 16, 1, 60, 1, False),
    ('ragged_pca', [400, 250, 17, 333], 8, 16, 1, 50, 2, True),
    ('ragged_odd_w_f2', [300, 8, 120, 300, 64], 6, 7, 2, 40, 3, False),
    ('uniform_large', [4096] * 16, 64, 32, 1, 400, 4, False),
    ('ragged_large', _large_ragged_lengths(), 64, 32, 1, 300, 5, False),
]


@pytest.mark.parametrize('plan', PLANS)
@pytest.mark.parametrize('name,lengths,K,W,F,nnz,seed,pca', INTERIOR, ids=[s[0] for s in INTERIOR])
def test_interior_corpus_equals_update_on_the_stack(name, lengths, K, W, F, nnz, seed, pca, plan):
    D, A = cpu.random_corpus(lengths, K, W, F, nnz, seed, where='interior')
    assert crst.interior_only(A, W)
    ref = ksvd.update(D, cpu.plain_stack(A), usePCA=pca)
    out = ksvd.update_corpus(D, A, usePCA=pca, plan=plan)
    assert [c.shape for c in out[1]] == [c.shape for c in A]
    assert _same_update(out, ref)


# ------------------------------------------------------------------------------------------------ the restatement
def _ends_corpus(lengths, K, W, F, nnz, seed):
    """Entries at and across the signal ends; atom 2 never occurs, and signal 1 holds no occurrence of atom 3."""
    D, A = cpu.random_corpus(lengths, K, W, F, nnz, seed, where='ends')
    for b in range(len(A)):
        M = A[b].tolil()
        M[:, 2] = 0.0
        if b == 1:
            M[:, 3] = 0.0
        A[b] = scipy.sparse.csc_matrix(M)
    return D, A


ENDS = [
    ('svd', [120, 90, 150, 33], 6, 16, 1, 60, 6, False),
    ('pca', [200, 64, 17, 180], 6, 16, 1, 80, 7, True),
    ('odd_w_f2', [150, 9, 80, 150], 6, 7, 2, 60, 8, False),
    ('wide_atoms', [700] * 12, 8, 32, 2, 300, 9, False),
]


@pytest.mark.parametrize('plan', PLANS)
@pytest.mark.parametrize('name,lengths,K,W,F,nnz,seed,pca', ENDS, ids=[s[0] for s in ENDS])
def test_corpus_matches_restatement(name, lengths, K, W, F, nnz, seed, pca, plan):
    D, A = _ends_corpus(lengths, K, W, F, nnz, seed)
    assert not crst.interior_only(A, W) and A[1][:, 3].nnz == 0
    D_ref, A_ref, st_ref = crst.sweep(D, A, pca)
    assert st_ref[2, 0] == 0 and st_ref[3, 0] > 0
    D_gpu, A_gpu, st_gpu, _ = ksvd.update_corpus(D, A, usePCA=pca, plan=plan)
    print('%s/%s: |D - D_ref| = %.3e' % (name, plan, np.max(np.abs(D_gpu - D_ref))))
    assert np.array_equal(st_gpu[:, 0], st_ref[:, 0])
    assert np.array_equal(D_gpu[2], np.asarray(D, np.float64)[2])            # an atom that never occurs is kept
    # D within 1e-10, with the restatement's signs
    assert np.max(np.abs(D_gpu - D_ref)) <= 1e-10
    scale = max(np.max(np.abs(c.data)) for c in A_ref if c.nnz)
    for g, r in zip(A_gpu, A_ref):
        r = scipy.sparse.csc_matrix(r)
        r.sort_indices()
        assert g.shape == r.shape and np.array_equal(g.indices, r.indices) and np.array_equal(g.indptr, r.indptr)
        if r.nnz:
            assert np.max(np.abs(g.data - r.data)) <= 1e-12 * scale
    occ = st_ref[:, 3] == 1
    assert np.allclose(st_gpu[occ, 1], st_ref[occ, 1], rtol=1e-10, atol=1e-12 * np.max(st_ref[:, 1]))
    # it is not the plain stack's update
    D_stack = ksvd.update(D, cpu.plain_stack(A), usePCA=pca)[0]
    assert np.max(np.abs(D_gpu - D_stack)) > 1e-6


def test_inputs_are_not_modified():
    D, A = _ends_corpus([120, 90, 150], 6, 16, 1, 60, 6)
    D0, A0 = D.copy(), [c.copy() for c in A]
    ksvd.update_corpus(D, A)
    assert np.array_equal(D, D0)
    assert all(np.array_equal(a.data, b.data) and np.array_equal(a.indices, b.indices) for a, b in zip(A, A0))


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize('pca', [False, True], ids=['svd', 'pca'])
def test_plans_and_runs_bit_identical(pca):
    D, A = cpu.random_corpus([4096] * 16, 8, 16, 1, 420, 10, where='ends')
    runs = {plan: [ksvd.update_corpus(D, A, usePCA=pca, plan=plan) for _ in range(2)] for plan in PLANS + ('auto',)}
    st = runs['one'][0][2]
    assert sum(c.nnz for c in A) > 4096 and np.max(st[:, 0]) > 512
    assert np.max(st[:, 0]) >= ksvd.WIDE_FROM_OCCURRENCES          # 'auto' is the wide plan here
    for plan in runs:
        assert _same_update(runs[plan][0], runs[plan][1]), plan
        assert _same_update(runs[plan][0], runs['one'][0]), plan
    # below the threshold 'auto' is the one-workgroup plan; the same bits again
    D, A = cpu.random_corpus([300] * 4, 8, 16, 1, 60, 11, where='ends')
    outs = [ksvd.update_corpus(D, A, usePCA=pca, plan=plan) for plan in PLANS + ('auto',)]
    assert np.max(outs[0][2][:, 0]) < ksvd.WIDE_FROM_OCCURRENCES
    assert _same_update(outs[0], outs[1]) and _same_update(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ trainCorpus
def _golden(name):
    return single.CASES[single.IDS.index(name)]


def _f2_case():
    return next(c for c in single.CMP_CASES if c['x'].ndim == 2)


@pytest.mark.parametrize('c', [_golden('odd_w'), _golden('dense'), _f2_case()], ids=['odd_w', 'dense', 'f2'])
def test_train_corpus_of_one_signal_equals_train_cmp(c):
    kw = single._kw(c)
    np.random.seed(c['seed'])
    learner = ConvolutionalKSVDLearner(c['K'], c['W'])
    D = learner.train(c['x'], **kw)
    # (the list form is a ragged batch, which the engine encodes for single-feature signals only: DESIGN section 15)
    for corpus in (c['x'][np.newaxis], [c['x']])[:2 if c['x'].ndim == 1 else 1]:
        np.random.seed(c['seed'])
        corp = ConvolutionalKSVDLearner(c['K'], c['W'])
        assert np.array_equal(corp.trainCorpus(corpus, **kw), D)
        assert [s['alpha'] for s in corp.lastStats] == [s['alpha'] for s in learner.lastStats]
    D_rng = ConvolutionalKSVDLearner(c['K'], c['W'], rng=np.random.RandomState(c['seed'])).trainCorpus(c['x'][np.newaxis], **kw)
    assert np.array_equal(D_rng, D)


def test_train_corpus_of_one_signal_equals_train_locomp():
    c = _golden('script_locomp')
    kw = dict(method='locomp', maxIterations=2, nbNonzeroCoefs=c['nbNonzeroCoefs'], toleranceSnr=c['toleranceSnr'])
    np.random.seed(c['seed'])
    D = ConvolutionalKSVDLearner(c['K'], c['W']).train(c['x'], **kw)
    np.random.seed(c['seed'])
    assert np.array_equal(ConvolutionalKSVDLearner(c['K'], c['W']).trainCorpus(c['x'][np.newaxis], **kw), D)
    with pytest.raises(NotImplementedError, match='ragged'):
        ConvolutionalKSVDLearner(c['K'], c['W']).trainCorpus([c['x']], **kw)


@pytest.mark.parametrize('case', cpu.LEARN_CASES, ids=cpu.LEARN_IDS)
def test_train_corpus_matches_restatement(case):
    name, lengths, K, W, nnz, iterations, sseed, dseed = case
    xs, (hist, alphas, stats, codes) = cpu.restate_learn(case)
    tol = cpu.learn_tol(stats)
    kw = dict(method='cmp', maxIterations=iterations, nbNonzeroCoefs=nnz, toleranceSnr=40.0)
    ragged = len(set(lengths)) > 1
    np.random.seed(dseed)
    learner = ConvolutionalKSVDLearner(K, W)
    D = learner.trainCorpus(xs if ragged else np.stack(xs), **kw)
    err = single._err_up_to_sign(D, hist[-1])
    print('%s: error up to sign %.3e, tolerance %.3e (gap %.3e)' % (name, err, tol, cpu.learn_gap(stats)))
    assert D.dtype == np.float64 and D.shape == (K, W)
    assert err <= tol
    st = learner.lastStats
    assert len(st) == iterations
    assert np.allclose([s['alpha'] for s in st], alphas, rtol=1e-9)
    for s, r, c in zip(st, stats, codes):
        assert np.array_equal(s['n_k'], r[:, 0].astype(np.int64))
        assert s['nnz'] == sum(m.nnz for m in c) and s['plan'] == 1
        assert s['variant'].endswith('_ragged') == ragged
    if ragged:
        # the padded array with lengths=: the same bits as the list
        padded = np.zeros((len(xs), max(lengths)))
        for b, x in enumerate(xs):
            padded[b, :len(x)] = x
        np.random.seed(dseed)
        assert np.array_equal(ConvolutionalKSVDLearner(K, W).trainCorpus(padded, lengths=lengths, **kw), D)
    else:
        # a list of signals of one length is a ragged batch too: the same bits
        np.random.seed(dseed)
        assert np.array_equal(ConvolutionalKSVDLearner(K, W).trainCorpus(xs, **kw), D)


# ------------------------------------------------------------------------------------------------ failures
def _raw_call(B, offsets, K, W, F, indptr, indices, data, pca=0, plan=0):
    """hscksvd_update_corpus through the context's checked call; returns the HscmpError (None: the call succeeded)."""
    p = _native._ptr
    off = None if offsets is None else np.asarray(offsets, dtype=np.int32)
    D = np.ones((K, max(W, 1), max(F, 1)))
    ip, ix, dv = np.asarray(indptr, np.int32), np.asarray(indices, np.int32), np.asarray(data, np.float64)
    try:
        ksvd._context(0).call('update_corpus', B, p(off), K, W, F, p(D), p(ip), p(ix), p(dv), pca, plan, None, None)
    except _native.HscmpError as e:
        return e
    return None


def test_failures_name_their_cause_and_leave_the_context_usable():
    ok = dict(K=2, W=4, F=1, indptr=[0, 1, 2], indices=[3, 12], data=[1.0, 2.0])
    bad = [
        (dict(ok, B=0, offsets=[0, 10]), -1, 'bad shape B = 0'),
        (dict(ok, B=2, offsets=None), -1, 'row_offsets is NULL'),
        (dict(ok, B=2, offsets=[1, 10, 20]), -1, 'row_offsets[0] = 1'),
        (dict(ok, B=2, offsets=[0, 10, 5]), -1, 'row_offsets decreases at signal 1'),
        (dict(ok, B=2, offsets=[0, 10, 10]), -1, 'signal 1 is empty'),
        (dict(ok, B=2, offsets=[0, 6, 12]), -1, 'row 12 of entry 1 is outside [0, 12)'),
        (dict(ok, B=2, offsets=[0, 10, 20], indptr=[0, 2, 2], indices=[12, 3]), -1, 'rows of column 0 are not strictly ascending'),
        (dict(ok, B=2, offsets=[0, 10, 20], indptr=[0, 2, 2], indices=[3, 3]), -1, 'rows of column 0 are not strictly ascending'),
        (dict(ok, B=2, offsets=[0, 100, 200], W=65), -5, 'W * F = 65 exceeds the limit of 64'),
        (dict(ok, B=2, offsets=[0, 100, 200], W=33, F=2), -5, 'W * F = 66 exceeds the limit of 64'),
        (dict(ok, B=2, offsets=[0, 10, 20], F=2, pca=1), -5, 'the PCA branch needs F = 1'),
        (dict(ok, B=2, offsets=[0, 10, 20], plan=3), -5, 'unknown plan 3'),
        (dict(ok, B=2, offsets=[0, 10, 20], plan=-1), -5, 'unknown plan -1'),
    ]
    for kw, code, text in bad:
        e = _raw_call(**kw)
        assert e is not None and e.code == code, (kw, e)
        assert 'hscksvd_update_corpus: ' in str(e) and text in str(e), (text, str(e))
        assert _raw_call(B=2, offsets=[0, 10, 20], **ok) is None             # the context still works
    # a stack of 2^31 rows or more cannot be expressed in the int32 offsets: refused before the device
    huge = scipy.sparse.csc_matrix((2 ** 30, 2))
    with pytest.raises(NotImplementedError, match='2\\^31'):
        ksvd.update_corpus(np.ones((2, 4)), [huge, huge])
    D, A = cpu.random_corpus([300] * 4, 8, 16, 1, 60, 11, where='ends')
    assert _same_update(ksvd.update_corpus(D, A, plan='one'), ksvd.update_corpus(D, A, plan='wide'))
