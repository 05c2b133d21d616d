"""hsckmeans_set_corpus_sparse and sparse corpora in ConvolutionalKMeansLearner.trainCorpus on the GPU (DESIGN.md section
19), bit for bit against the dense path: the window stack gathered on the device against hsckmeans_set_corpus of the
densified stack at the raw step outputs, trainCorpus on CSR signals against trainCorpus on their dense form, a corpus
beyond the dense element limit against a dense stand-in of its windows, the refusals of the entry point, and one
context reused across the three kinds of data."""
import numpy as np
import pytest
import scipy.sparse

from hsc_amd import _native
from hsc_amd import kmeans
from hsc_amd.kmeans import ConvolutionalKMeansLearner, PLAN_AUTO, PLAN_LISTS, PLAN_WIDE, WIDE_CHUNK_WINDOWS

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    """The shared context of device 0, handed back on the automatic plan."""
    c = kmeans._context(0)
    try:
        yield c
    finally:
        c.set_plan(PLAN_AUTO)


def _csr_arrays(m):
    return m.indptr.astype(np.int64), np.ascontiguousarray(m.indices.astype(np.int32)), np.ascontiguousarray(m.data)


def _mode(dtype):
    return np.array([1 if dtype == np.float32 else 2], dtype=np.int32)


def _dictionary(K, W, F, dtype, seed):
    D = np.random.RandomState(seed).standard_normal((1, K, W, F))
    D /= np.sqrt(np.sum(D ** 2, axis=(2, 3), keepdims=True))
    return D.astype(dtype).astype(np.float64)


def _assert_steps_equal(got, exp):
    for name, a, b in zip(('t', 'k', 'count', 'nonzero', 'sums'), got[:5], exp[:5]):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a, b, equal_nan=True), name


# ------------------------------------------------------------------------------------------------ 1. gather against dense
def _gather_problem(W, F, dtype, seed):
    """Three signals of different lengths as one dense stack [rows,F], about 15 % of its cells set, with a stretch of
    3W + 2 empty rows in the second signal and (F > 1) a row that holds several entries next to it.  Returns
    (dense, row_offsets, the special starts by name, the row with several entries)."""
    rs = np.random.RandomState(seed)
    L2 = 2 * W
    lens = np.array([L2 + 1, 60 + 9 * W, 23 + 4 * W], dtype=np.int64)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dense = rs.standard_normal((int(ro[-1]), F)) * (rs.rand(int(ro[-1]), F) < 0.15)
    gap = int(ro[1]) + 11                                                  # rows gap .. gap + 3W + 2 hold nothing
    dense[gap:gap + 3 * W + 2] = 0.0
    multi = gap + 3 * W + 2 + W                                            # inside the overlapping pair below
    dense[multi, :min(F, 3)] = rs.standard_normal(min(F, 3)) + 3.0
    special = dict(first_row=int(ro[1]), last_row=int(ro[3]) - L2, empty=gap + 1,
                   overlap_a=multi - W, overlap_b=multi - W + max(1, W // 2))
    return np.ascontiguousarray(dense.astype(dtype)), ro, special, multi


def _check_window_kinds(dense, ro, starts, W, F, kinds, multi):
    """The host's own account of what the windows cover (asserted, so that a change of the generator cannot hollow the case)."""
    L2 = 2 * W
    if 'first_row' in kinds:
        assert np.any(np.isin(starts, ro[:-1]))                            # a window starting at a signal's row 0
    if 'last_row' in kinds:
        assert np.any(np.isin(starts + L2, ro[1:]))                        # a window ending at a signal's last row
    if 'overlap' in kinds:
        s = np.sort(starts)
        assert np.any((np.diff(s) > 0) & (np.diff(s) < L2))                # two windows that overlap without being equal
    if 'empty' in kinds:
        assert any(not dense[s:s + L2].any() for s in starts)              # no entry at all: the norm is 0 and divides by 1
    if 'multi' in kinds and F > 1:                                         # (F = 1: a row holds one entry at the most)
        assert np.count_nonzero(dense[multi]) > 1 and np.any((starts <= multi) & (multi < starts + L2))


@pytest.mark.parametrize('N', [1, 65, WIDE_CHUNK_WINDOWS + 1])
@pytest.mark.parametrize('W,F', [(2, 1), (15, 3), (8, 17), (1, 257)], ids=lambda v: str(v))
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('plan', [PLAN_LISTS, PLAN_WIDE], ids=['lists', 'wide'])
def test_gathered_window_stack_equals_dense_corpus(plan, dtype, W, F, N, ctx):
    """N = 1 cannot hold all the kinds of window at once: it runs once per kind, each with its one window."""
    dense, ro, special, multi = _gather_problem(W, F, dtype, 100 * W + F)
    indptr, indices, data = _csr_arrays(scipy.sparse.csr_matrix(dense))
    K = 5
    D = _dictionary(K, W, F, dtype, 7)
    if N == 1:
        runs = [(np.array([special[name]], dtype=np.int64), kinds) for name, kinds in (
            ('first_row', ('first_row',)), ('last_row', ('last_row',)), ('empty', ('empty',)), ('overlap_a', ('multi',)))]
    else:
        rs = np.random.RandomState(N)
        sig = rs.randint(0, 3, N)
        rnd = ro[sig] + (rs.rand(N) * (np.diff(ro)[sig] - 2 * W + 1)).astype(np.int64)
        starts = np.concatenate([np.array(list(special.values()), dtype=np.int64), rnd[len(special):]])
        runs = [(starts[rs.permutation(N)], ('first_row', 'last_row', 'overlap', 'empty', 'multi'))]
    ctx.set_plan(plan)
    for starts, kinds in runs:
        starts = np.ascontiguousarray(starts)
        _check_window_kinds(dense, ro, starts, W, F, kinds, multi)
        ctx.set_corpus_sparse(indptr, indices, data, F, ro, starts, W)
        got = ctx.step(D, _mode(dtype))
        ctx.set_corpus(dense, ro, starts, W)
        exp = ctx.step(D, _mode(dtype))
        _assert_steps_equal(got, exp)
        assert got[2].sum() == len(starts) and got[4].dtype == dtype
        if 'empty' in kinds:
            empties = [n for n, s in enumerate(starts) if not dense[s:s + 2 * W].any()]
            assert all(got[0][0, n] == 0 and got[1][0, n] == 0 for n in empties)     # all scores equal: (0, 0)


# ------------------------------------------------------------------------------------------------ 2. trainCorpus
# the generator seed per initMethod, picked on the numpy twin of the library so that resetMethod='random_samples' resets
TRAIN_SEEDS = {'random_samples': 3, 'noise': 72}


def train_signals(dtype, init):
    """Three sparse signals of 200 to 400 rows, F = 4, about 3 % of the cells set.  Under initMethod='noise' the entries
    are positive, as the coefficients of a non-negative level are: the 'noise' bounds are then [the implicit 0, the
    largest entry], all atoms start positive and one of them loses its members, so a reset happens there too."""
    rs = np.random.RandomState(21)
    dense = [rs.standard_normal((T, 4)) * (rs.rand(T, 4) < 0.03) for T in (400, 200, 310)]
    return [scipy.sparse.csr_matrix((np.abs(x) if init == 'noise' else x).astype(dtype)) for x in dense]


def train_both(dtype, init, reset):
    signals = train_signals(dtype, init)
    seed = TRAIN_SEEDS[init]
    kw = dict(nbRandomWindows=300, maxIterations=3, tolerance=0.0, initMethod=init, resetMethod=reset, nbAveragedPatches=3)
    a = ConvolutionalKMeansLearner(5, 6, rng=np.random.RandomState(seed))
    Da = a.trainCorpus(signals, **kw)
    b = ConvolutionalKMeansLearner(5, 6, rng=np.random.RandomState(seed))
    Db = b.trainCorpus([m.toarray() for m in signals], **kw)
    return a, Da, b, Db


@pytest.mark.parametrize('reset', kmeans.RESET_METHODS)
@pytest.mark.parametrize('init', kmeans.INIT_METHODS)
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_train_corpus_sparse_equals_dense(dtype, init, reset):
    a, Da, b, Db = train_both(dtype, init, reset)
    assert Da.dtype == Db.dtype and Da.shape == Db.shape == (5, 6, 4) and np.array_equal(Da, Db)
    assert len(a.lastStats) == len(b.lastStats) == 3
    for s, r in zip(a.lastStats, b.lastStats):
        assert np.array_equal(s['assignment'][0], r['assignment'][0]) and np.array_equal(s['assignment'][1], r['assignment'][1])
        assert s['nbResets'] == r['nbResets'] and np.array_equal(s['counts'], r['counts']) and s['alpha'] == r['alpha']
    assert np.array_equal(a.lastWindows[0], b.lastWindows[0]) and np.array_equal(a.lastWindows[1], b.lastWindows[1])
    if reset == 'random_samples':
        if init == 'noise':
            assert a.lastStats and min(m.data.min() for m in train_signals(dtype, init)) > 0.0     # the lower bound is the implicit 0
        # a reset patch was cut from the sparse rows
        assert sum(s['nbResets'] for s in a.lastStats) > 0


# ------------------------------------------------------------------------------------------------ 3. beyond the dense limit
def test_corpus_beyond_the_dense_element_limit(ctx):
    """Two signals of 2^22 rows, F = 257: 2^23 * 257 elements dense (refused: tests/test_kmeans_corpus.py), a few
    thousand entries each.  The windows sit on rows that hold entries, at both signals' ends and on empty rows; their
    dense stand-in is N signals of 2W + 1 rows: window n's rows and one neighbouring row."""
    T, F, W, N, K = 2 ** 22, 257, 2, 64, 6
    L2 = 2 * W
    rs = np.random.RandomState(5)
    mats = []
    for b in range(2):
        nnz = 3000
        rows = np.sort(rs.randint(0, T // 4096, nnz) * 4096 + rs.randint(0, 6, nnz))     # clusters of six rows
        rows[:8] = [0, 0, 1, 3, T - 4, T - 2, T - 1, T - 1]
        rows.sort()
        m = scipy.sparse.coo_matrix((rs.standard_normal(nnz), (rows, rs.randint(0, F, nnz))), shape=(T, F)).tocsr()
        m.sum_duplicates()
        mats.append(m)
    assert (2 * T) * F > kmeans.MAX_STACK_ELEMENTS and all(2000 < m.nnz <= 3000 for m in mats)
    learner = ConvolutionalKMeansLearner(K, W, rng=np.random.RandomState(1))
    D = learner.trainCorpus(mats, N, maxIterations=2)                     # the call runs
    assert D.shape == (K, W, F) and D.dtype == np.float64 and np.all(np.isfinite(D)) and len(learner.lastStats) == 2

    stack = kmeans.SparseStack(mats)
    ro = stack.row_offsets
    indptr, indices, data = stack.csr()
    occupied = np.flatnonzero(np.diff(indptr) > 0)
    starts = np.concatenate([[0, T - L2, T, 2 * T - L2, 2 * T - L2 - 1, 12345, T + 54321],
                             occupied[rs.randint(0, len(occupied), N - 7)] - rs.randint(0, L2, N - 7)]).astype(np.int64)
    starts = np.clip(starts, 0, 2 * T - L2)
    cross = (starts < T) & (starts + L2 > T)
    starts[cross] = T - L2
    assert len(starts) == N and int(np.max(starts)) * F > 2 ** 31         # a dense index past 2^31
    Dk = _dictionary(K, W, F, np.float64, 3)
    ctx.set_corpus_sparse(indptr, indices, data, F, ro, np.ascontiguousarray(starts), W)
    got = ctx.step(Dk, _mode(np.float64))
    # the stand-in: signal n = rows start - 1 .. start + 2W of the corpus (start .. start + 2W + 1 at a signal's row 0)
    standin = np.zeros((N * (L2 + 1), F))
    s_starts = np.zeros((N,), dtype=np.int64)
    for n, s in enumerate(starts):
        before = 0 if s in (0, T) else 1
        standin[n * (L2 + 1):(n + 1) * (L2 + 1)] = stack[int(s) - before:int(s) - before + L2 + 1]
        s_starts[n] = n * (L2 + 1) + before
    ctx.set_corpus(standin, np.arange(N + 1, dtype=np.int64) * (L2 + 1), s_starts, W)
    exp = ctx.step(Dk, _mode(np.float64))
    _assert_steps_equal(got, exp)
    assert np.count_nonzero(got[4]) > 0 and np.count_nonzero(got[2]) > 1


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_set_corpus_sparse_refusals(ctx):
    W, F = 4, 3
    dense = np.zeros((40 + 17 + 60, F), dtype=np.float32)
    dense[[3, 3, 50, 116], [0, 2, 1, 2]] = [1.0, 2.0, 3.0, 4.0]
    ro = np.array([0, 40, 57, 117], dtype=np.int64)
    indptr, indices, data = _csr_arrays(scipy.sparse.csr_matrix(dense))
    ok = np.array([0, 40, 57, 117 - 8], dtype=np.int64)
    D = _dictionary(3, W, F, np.float32, 2)

    def works():
        ctx.set_corpus_sparse(indptr, indices, data, F, ro, ok, W)
        got = ctx.step(D, _mode(np.float32))
        ctx.set_corpus(dense, ro, ok, W)
        _assert_steps_equal(got, ctx.step(D, _mode(np.float32)))

    def refused(match, code, indptr_=indptr, indices_=indices, starts=ok, ro_=ro, N_W=None):
        with pytest.raises(_native.HscmpError, match=match) as e:
            ctx.set_corpus_sparse(indptr_, indices_, data, F, ro_, starts, W if N_W is None else N_W)
        assert e.value.code == code
        works()                                                            # the context works on the next valid call

    works()
    bad = indptr.copy()
    bad[51] = bad[50] - 1                                                  # row 50 ends before it begins
    refused(r'indptr descends at row 50', -1, indptr_=bad)
    bad = indptr.copy()
    bad[0] = 1
    refused(r'indptr\[0\] = 1, must be 0', -1, indptr_=bad)
    bad = indices.copy()
    bad[2] = F                                                             # the entry of row 50
    refused(r'column 3 of row 50 is outside \[0, 3\)', -1, indices_=bad)
    bad = indices.copy()
    bad[0], bad[1] = 2, 0                                                  # row 3: columns 2, 0
    refused(r'the columns of row 3 do not ascend \(0 after 2\)', -1, indices_=bad)
    bad[0], bad[1] = 2, 2                                                  # a column twice
    refused(r'the columns of row 3 do not ascend \(2 after 2\)', -1, indices_=bad)
    refused(r'window 1 \(rows 36 \.\. 44\) crosses the end of signal 0 at row 40', -1, starts=np.array([0, 36], dtype=np.int64))
    refused(r'start 117 of window 0 is outside the stack of 117 rows', -1, starts=np.array([117], dtype=np.int64))
    refused(r'signal 1 has 8 samples', -1, ro_=np.array([0, 49, 57, 117], dtype=np.int64))
    refused(r'row_offsets descend at signal 1', -1, ro_=np.array([0, 60, 40, 117], dtype=np.int64))
    # a window stack beyond 2^31 - 1 elements (the starts are only read as far as they are checked: a broadcast view)
    many = (2 ** 31) // (2 * W * F) + 1
    with pytest.raises(_native.HscmpError, match=r'the window stack of \d+ x 3 elements exceeds 2\^31 - 1') as e:
        ctx.set_corpus_sparse(indptr, indices, data, F, ro, np.broadcast_to(np.zeros((1,), dtype=np.int64), (many,)), W)
    assert e.value.code == -5
    works()


# ------------------------------------------------------------------------------------------------ 5. one context reused
def test_context_reused_across_plain_sparse_and_dense_corpus():
    rs = np.random.RandomState(8)
    W, F = 5, 3
    x = np.ascontiguousarray((rs.standard_normal((2, 90, F)) * (rs.rand(2, 90, F) < 0.3)).astype(np.float32))
    sx = rs.randint(0, 90 - 2 * W, (2, 40)).astype(np.int64)
    Dx = np.concatenate([_dictionary(4, W, F, np.float32, 1), _dictionary(4, W, F, np.float32, 2)])
    mx = np.array([1, 1], dtype=np.int32)
    sp = np.ascontiguousarray((rs.standard_normal((150, F)) * (rs.rand(150, F) < 0.1)))
    ro_s = np.array([0, 70, 150], dtype=np.int64)
    ss = np.concatenate([rs.randint(0, 70 - 2 * W + 1, 30), 70 + rs.randint(0, 80 - 2 * W + 1, 30)]).astype(np.int64)
    csr = _csr_arrays(scipy.sparse.csr_matrix(sp))
    Ds = _dictionary(6, W, F, np.float64, 3)
    dn = np.ascontiguousarray(rs.standard_normal((120, F)).astype(np.float32))
    ro_d = np.array([0, 50, 120], dtype=np.int64)
    sd = np.concatenate([rs.randint(0, 50 - 2 * W + 1, 25), 50 + rs.randint(0, 70 - 2 * W + 1, 25)]).astype(np.int64)
    Dd = _dictionary(3, W, F, np.float32, 4)

    def plain(c):
        c.set_data(x, sx, W)
        return c.step(Dx, mx)

    def sparse(c):
        c.set_corpus_sparse(csr[0], csr[1], csr[2], F, ro_s, ss, W)
        return c.step(Ds, _mode(np.float64))

    def corpus(c):
        c.set_corpus(dn, ro_d, sd, W)
        return c.step(Dd, _mode(np.float32))

    fresh = []
    for run in (plain, sparse, corpus):
        c = kmeans._Context(0)
        fresh.append(run(c))
        del c
    # the sparse corpus against its dense form, on a context of its own
    c = kmeans._Context(0)
    c.set_corpus(sp, ro_s, ss, W)
    _assert_steps_equal(fresh[1], c.step(Ds, _mode(np.float64)))
    del c
    one = kmeans._Context(0)
    for run, exp in list(zip((plain, sparse, corpus), fresh)) + [(sparse, fresh[1]), (plain, fresh[0])]:
        _assert_steps_equal(run(one), exp)
