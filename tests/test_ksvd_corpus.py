"""The corpus form of the K-SVD learner (hsc_amd.ksvd.update_corpus / ConvolutionalKSVDLearner.trainCorpus), CPU side:
the restatement of hscksvd_update_corpus against the restatement of hscksvd_update at the contract's two anchors
(B = 1; interior-only corpora against the plain stack), the argument checks that must come before any device call, and
the conditions the GPU comparisons of tests/test_gpu_ksvd_corpus.py rely on for their seeds."""
import os

import numpy as np
import pytest
import scipy.sparse

from hsc_amd import _native
from hsc_amd import ksvd
from hsc_amd.learning import ConvolutionalDictionaryLearner
from hsc_amd.ksvd import ConvolutionalKSVDLearner
from tests import ksvd_restatement as rst
from tests import ksvd_corpus_restatement as crst

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ inputs
def random_corpus(lengths, K, W, F, nnz, seed, where='any'):
    """Random unit atoms and, per signal, up to `nnz` random coefficients (a few stored zeros among them).
    where: 'any' (every row, the signal ends included), 'interior' (every atom span inside its signal) or 'ends' (as
    'any', plus entries on the first and the last row of every signal)."""
    rs = np.random.RandomState(seed)
    D = rs.randn(K, W, F)
    D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
    lead = (W - 1) // 2
    out = []
    for T in lengths:
        lo, hi = (lead, T - W + lead + 1) if where == 'interior' else (0, T)
        t = rs.randint(lo, hi, nnz)
        k = rs.randint(0, K, nnz)
        if where == 'ends':
            t = np.concatenate([t, [0, 0, T - 1, T - 1]])
            k = np.concatenate([k, [0, 1, K - 1, K - 2]])
        key = np.unique(t.astype(np.int64) * K + k)
        t, k = key // K, key % K
        c = rs.randn(len(key))
        c[rs.rand(len(key)) < 0.02] = 0.0                     # stored zeros: never occurrences, never terms
        out.append(scipy.sparse.csc_matrix((c, (t, k)), shape=(T, K)))
    return (D[:, :, 0] if F == 1 else D), out


def plain_stack(coefficients):
    return scipy.sparse.vstack(coefficients, format='csc')


# (name, lengths, K, W, F, nnz per signal, seed, usePCA): SVD and PCA, F = 1 and 2, odd and even W, a signal of length W
ANCHOR_SHAPES = [
    ('svd_even_w', [400, 400, 400], 8, 16, 1, 60, 1, False),
    ('pca_even_w', [400, 250, 16, 333], 8, 16, 1, 50, 2, True),
    ('svd_odd_w_f2', [300, 7, 120, 300, 64], 6, 7, 2, 40, 3, False),
    ('svd_w8', [8, 200, 8, 150], 8, 8, 1, 40, 4, False),
    ('pca_odd_w', [90, 15, 200], 5, 15, 1, 60, 5, True),
]
ANCHOR_IDS = [s[0] for s in ANCHOR_SHAPES]


def same_bits(a, b):
    """(D, matrix or list of matrices, stats) of two sweeps: D, structure, values and stats bit for bit."""
    Da, Aa, sa = a[:3]
    Db, Ab, sb = b[:3]
    Aa = plain_stack(Aa) if isinstance(Aa, list) else scipy.sparse.csc_matrix(Aa)
    Ab = plain_stack(Ab) if isinstance(Ab, list) else scipy.sparse.csc_matrix(Ab)
    for M in (Aa, Ab):
        M.sort_indices()
    return (np.array_equal(Da, Db) and np.array_equal(Aa.indptr, Ab.indptr) and np.array_equal(Aa.indices, Ab.indices)
            and np.array_equal(Aa.data, Ab.data) and np.array_equal(sa, sb))


# ------------------------------------------------------------------------------------------------ restatement anchors
@pytest.mark.parametrize('name,lengths,K,W,F,nnz,seed,pca', ANCHOR_SHAPES, ids=ANCHOR_IDS)
def test_restatement_one_signal_is_the_plain_sweep(name, lengths, K, W, F, nnz, seed, pca):
    """B = 1: bit for bit ksvd_restatement.sweep, entries at the signal's ends included."""
    for T in sorted(set(lengths)):
        D, A = random_corpus([T], K, W, F, nnz, seed, where='ends')
        assert same_bits(crst.sweep(D, A, pca), rst.sweep(D, A[0], pca)), (name, T)


@pytest.mark.parametrize('name,lengths,K,W,F,nnz,seed,pca', ANCHOR_SHAPES, ids=ANCHOR_IDS)
def test_restatement_interior_corpus_is_the_plain_stack(name, lengths, K, W, F, nnz, seed, pca):
    """Every span inside its signal: bit for bit ksvd_restatement.sweep on the stack, T = sum T_b."""
    D, A = random_corpus(lengths, K, W, F, nnz, seed, where='interior')
    assert crst.interior_only(A, W)
    assert same_bits(crst.sweep(D, A, pca), rst.sweep(D, plain_stack(A), pca)), name


def test_restatement_entries_at_the_ends_differ_from_the_stack():
    """Entries whose spans cross a seam: the stack lets them reach into the neighbouring signal, the corpus does not."""
    D, A = random_corpus([120, 90, 150], 6, 16, 1, 40, 6, where='ends')
    assert not crst.interior_only(A, 16)
    Dc, Ac, sc = crst.sweep(D, A)
    Ds, As, ss = rst.sweep(D, plain_stack(A))
    assert np.array_equal(sc[:, 0], ss[:, 0])                    # the same occurrences ...
    assert np.max(np.abs(Dc - Ds)) > 1e-3                        # ... another dictionary
    assert np.max(np.abs(plain_stack(Ac).data - scipy.sparse.csc_matrix(As).data)) > 1e-3


def test_restatement_patch_sees_its_own_signal_only():
    """Two signals, one occurrence each side of the seam: by hand.  Atom 0 sits on the last row of signal 0, atom 1 on
    the first row of signal 1.  In the stack they overlap; in the corpus neither sees the other, both patches are zero
    and the zero-Gram rule (u = e_0, coefficient 0) applies to both."""
    W, T = 8, 20
    D = np.eye(2, W) + 0.5 * np.eye(2, W, 1)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    A0 = scipy.sparse.csc_matrix(([2.0], ([T - 1], [0])), shape=(T, 2))
    A1 = scipy.sparse.csc_matrix(([3.0], ([0], [1])), shape=(T, 2))
    Dc, Ac, sc = crst.sweep(D, [A0, A1])
    assert np.array_equal(sc[:, 3], [3, 3]) and np.array_equal(Dc, np.eye(2, W)[[0, 0]])
    assert Ac[0].data.tolist() == [0.0] and Ac[1].data.tolist() == [0.0]
    _, _, ss = rst.sweep(D, plain_stack([A0, A1]))
    assert np.array_equal(ss[:, 3], [2, 2])                      # the stack: each patch holds the other atom


# ------------------------------------------------------------------------------------------------ argument checks
class _DeviceTouched(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise _DeviceTouched()
    monkeypatch.setattr(ksvd, 'load_library', touched)
    monkeypatch.setattr(ksvd, '_context', touched)
    monkeypatch.setattr(_native, 'default_engine', touched)
    monkeypatch.setattr(_native, 'engine_for', touched)


def test_train_corpus_argument_checks_raise_before_any_device_call(no_device):
    rs = np.random.RandomState(0)
    x = rs.randn(3, 500)
    ragged = [rs.randn(500), rs.randn(300), rs.randn(64)]
    # W * F > 64 in any signal
    with pytest.raises(NotImplementedError, match='64'):
        ConvolutionalKSVDLearner(4, 65).trainCorpus(x, method='cmp')
    with pytest.raises(NotImplementedError, match='64'):
        ConvolutionalKSVDLearner(4, 33).trainCorpus(np.zeros((3, 500, 2)), method='cmp')
    # a signal not longer than W
    with pytest.raises(AssertionError):
        ConvolutionalKSVDLearner(4, 16).trainCorpus(x[:, :16], method='cmp')
    with pytest.raises(AssertionError):
        ConvolutionalKSVDLearner(4, 16).trainCorpus(ragged[:2] + [rs.randn(16)], method='cmp')
    with pytest.raises(AssertionError):
        ConvolutionalKSVDLearner(4, 16).trainCorpus(np.zeros((2, 500)), method='cmp', lengths=[500, 16])
    # usePCA with F > 1
    with pytest.raises(ValueError):
        ConvolutionalKSVDLearner(4, 16).trainCorpus(np.zeros((3, 500, 2)), method='cmp', usePCA=True)
    # ragged input needs method='cmp'
    with pytest.raises(NotImplementedError, match='ragged'):
        ConvolutionalKSVDLearner(4, 16).trainCorpus(ragged, method='locomp')
    with pytest.raises(NotImplementedError, match='ragged'):
        ConvolutionalKSVDLearner(4, 16).trainCorpus(x, method='locomp', lengths=[500, 400, 300])
    # MPTK and unknown methods
    for m in ('mptk-mp', 'mptk-cmp'):
        with pytest.raises(NotImplementedError, match='MPTK'):
            ConvolutionalKSVDLearner(4, 16).trainCorpus(x, method=m)
    with pytest.raises(Exception, match='Unsupported sparse coding method'):
        ConvolutionalKSVDLearner(4, 16).trainCorpus(x, method='omp')
    # valid arguments reach the device
    for data, kw in ((x, dict(method='cmp')), (x, dict(method='locomp')), (ragged, dict(method='cmp')),
                     (x, dict(method='cmp', lengths=[500, 400, 17]))):
        with pytest.raises(_DeviceTouched):
            ConvolutionalKSVDLearner(4, 16).trainCorpus(data, **kw)


def test_update_corpus_argument_checks_raise_before_any_device_call(no_device):
    A = [scipy.sparse.csc_matrix(np.eye(500, 4)), scipy.sparse.csc_matrix(np.eye(300, 4))]
    with pytest.raises(NotImplementedError, match='64'):
        ksvd.update_corpus(np.ones((4, 65)), A)
    with pytest.raises(NotImplementedError, match='64'):
        ksvd.update_corpus(np.ones((4, 33, 2)), A)
    with pytest.raises(AssertionError):
        ksvd.update_corpus(np.ones((4, 16)), A + [scipy.sparse.csc_matrix(np.eye(16, 4))])
    with pytest.raises(ValueError):
        ksvd.update_corpus(np.ones((4, 16, 2)), A, usePCA=True)
    # mismatched K
    with pytest.raises(AssertionError):
        ksvd.update_corpus(np.ones((4, 16)), A + [scipy.sparse.csc_matrix(np.eye(300, 5))])
    with pytest.raises(ValueError, match='plan'):
        ksvd.update_corpus(np.ones((4, 16)), A, plan='fastest')
    with pytest.raises(ValueError):
        ksvd.update_corpus(np.ones((4, 16)), [])
    with pytest.raises(_DeviceTouched):
        ksvd.update_corpus(np.ones((4, 16)), A)


def test_anchor_shapes_cover_the_issue_matrix():
    assert {s[7] for s in ANCHOR_SHAPES} == {False, True} and {s[4] for s in ANCHOR_SHAPES} == {1, 2}
    assert {s[3] % 2 for s in ANCHOR_SHAPES} == {0, 1}
    assert sum(s[3] in s[1] for s in ANCHOR_SHAPES) >= 3          # signals of length exactly W
    assert any(len(set(s[1])) == 1 for s in ANCHOR_SHAPES) and any(len(set(s[1])) > 1 for s in ANCHOR_SHAPES)


def test_python_mirrors_the_header():
    assert 'hscksvd_update_corpus' in ksvd.EXPORTS
    text = open(os.path.join(ROOT, 'include', 'hscksvd.h')).read()
    assert 'HSCKSVD_WIDE_FROM_OCCURRENCES = %d ' % ksvd.WIDE_FROM_OCCURRENCES in text


# ------------------------------------------------------------------------------------------------ seeds of the GPU comparisons
def learn_corpus(lengths, W, seed):
    """The signals of a learn case: planted float64 signals that share 4 random unit atoms, T_b / 25 of them per
    signal at random positions, one more cut off by each end of the signal, plus white noise."""
    rs = np.random.RandomState(seed)
    atoms = rs.randn(4, W)
    atoms /= np.linalg.norm(atoms, axis=1, keepdims=True)
    xs = []
    for T in lengths:
        x = 0.01 * rs.randn(T)
        nb = max(1, T // 25)
        starts = np.concatenate([rs.randint(0, T - W + 1, nb), [-(W // 3), T - W + W // 3]])
        for t, k, a in zip(starts, rs.randint(0, 4, nb + 2), rs.randn(nb + 2)):
            lo, hi = max(t, 0), min(t + W, T)
            x[lo:hi] += ((2.0 + abs(a)) * np.sign(a) * atoms[k])[lo - t:hi - t]
        xs.append(x)
    return xs


# (name, lengths, K, W, nbNonzeroCoefs, iterations, seed of the signals, seed of the draw)
LEARN_CASES = [
    ('uniform', [300] * 6, 6, 12, 12, 3, 11, 21),
    ('ragged', [300, 220, 64, 180, 257, 300], 6, 12, 12, 3, 12, 22),
]
LEARN_IDS = [c[0] for c in LEARN_CASES]


def draw(K, W, xs, seed):
    """What trainCorpus draws: _init_D(..., 'noise') with low / high over the whole corpus."""
    np.random.seed(seed)
    return ConvolutionalDictionaryLearner(K, W, algorithm='ksvd')._init_D(np.concatenate(xs), initMethod='noise')


def restate_learn(case):
    name, lengths, K, W, nnz, iterations, sseed, dseed = case
    xs = learn_corpus(lengths, W, sseed)
    return xs, crst.learn(xs, draw(K, W, xs, dseed), nbNonzeroCoefs=nnz, toleranceSnr=40.0, maxIterations=iterations)


def learn_gap(stats):
    """The smallest relative gap of the top two eigenvalues over every atom an eigenvector was taken for."""
    gap = 1.0
    for st in stats:
        ev = st[st[:, 3] == 1]
        if len(ev):
            gap = min(gap, float(np.min((ev[:, 1] - ev[:, 2]) / ev[:, 1])))
    return gap


def learn_tol(stats):
    return max(1e-10, 64.0 * EPS / learn_gap(stats))


@pytest.mark.parametrize('case', LEARN_CASES, ids=LEARN_IDS)
def test_learn_seeds_meet_the_conditions_of_the_gpu_comparison(case):
    K, W = case[2], case[3]
    xs, (hist, alphas, stats, codes) = restate_learn(case)
    assert len(hist) == case[5]
    # no exact tie ("Degenerate seeds"): no two atoms that both occur once, at the same place, and so
    # no two atoms refitted to the same patch up to sign
    for coefficients, st, D in zip(codes, stats, hist):
        A, _ = crst.stack(coefficients)
        once = [int(A.indices[A.indptr[k]]) for k in range(K) if st[k, 0] == 1]
        assert len(once) == len(set(once))
        flat = D.reshape(K, -1)
        for i in range(K):
            for j in range(i + 1, K):
                assert min(np.max(np.abs(flat[i] - flat[j])), np.max(np.abs(flat[i] + flat[j]))) > 1e-6
    # the eigenvalue gaps keep the tolerance of the comparison at or below 1e-8
    assert learn_tol(stats) <= 1e-8
    # the corpus matters: some entry's span crosses an end of its signal
    assert not all(crst.interior_only(c, W) for c in codes)
