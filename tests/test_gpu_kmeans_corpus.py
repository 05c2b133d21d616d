"""ConvolutionalKMeansLearner.trainCorpus and the wide centroid plan of libhsckmeans.so on the GPU,
bit for bit: the reference's corpus goldens under every plan, a corpus of one signal against train, plan 1 = plan 2 =
auto = a rerun on the raw step outputs at the boundaries of the wide plan (chunks of the partition, batches of the LDS
ring, tiles of 256 elements), the step against the numpy twin on a ragged stack, the refusals of hsckmeans_set_corpus
and hsckmeans_set_plan, and one context reused across corpus and plain data."""
import numpy as np
import pytest

from hsc_amd import _native
from hsc_amd import kmeans
from hsc_amd.kmeans import ConvolutionalKMeansLearner, PLAN_AUTO, PLAN_LISTS, PLAN_WIDE, WIDE_CHUNK_WINDOWS, WIDE_RING_ROWS
from tests import kmeans_corpus_restatement as crst
from tests.test_kmeans_corpus import CASES, check_case, train_case

pytestmark = pytest.mark.gpu
PLANS = [PLAN_LISTS, PLAN_WIDE, PLAN_AUTO]
CHUNK, RING = WIDE_CHUNK_WINDOWS, WIDE_RING_ROWS


@pytest.fixture
def ctx():
    """The shared context of device 0, handed back on the automatic plan."""
    c = kmeans._context(0)
    try:
        yield c
    finally:
        c.set_plan(PLAN_AUTO)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 1. the goldens
@pytest.mark.parametrize('plan', PLANS, ids=['lists', 'wide', 'auto'])
@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_train_corpus_matches_golden(c, plan, ctx):
    ctx.set_plan(plan)
    D, learner = train_case(c)
    check_case(c, D, learner)


# ------------------------------------------------------------------------------------------------ 2. B = 1 is train
def _signal(T, F, dtype, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((T,) if F is None else (T, F)) * (rs.rand(T, *([] if F is None else [1])) < 0.05)
    return x.astype(dtype)


@pytest.mark.parametrize('reset', kmeans.RESET_METHODS)
@pytest.mark.parametrize('init', kmeans.INIT_METHODS)
@pytest.mark.parametrize('F', [None, 3], ids=['T', 'TF'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_one_signal_corpus_equals_train(dtype, F, init, reset):
    x = _signal(2000, F, dtype, 11)
    kw = dict(nbRandomWindows=300, maxIterations=5, tolerance=0.0, initMethod=init, resetMethod=reset, nbAveragedPatches=3)
    np.random.seed(4)
    one = ConvolutionalKMeansLearner(6, 8)
    ref = one.train(x, **kw)
    for form in (x[np.newaxis], [x]):
        np.random.seed(4)
        learner = ConvolutionalKMeansLearner(6, 8)
        D = learner.trainCorpus(form, **kw)
        assert _same(D, ref)
        assert [s['nbResets'] for s in learner.lastStats] == [s['nbResets'] for s in one.lastStats]
        assert not learner.lastWindows[0].any()


# ------------------------------------------------------------------------------------------------ 3. plans and reruns
def _steps_agree(ctx, setter, D, mode, live=None):
    """The raw step outputs under plan 1, plan 2, auto and a rerun of plan 2, on the rows of the learners in `live`."""
    outs = []
    for plan in (PLAN_LISTS, PLAN_WIDE, PLAN_AUTO, PLAN_WIDE):
        setter()
        ctx.set_plan(plan)
        outs.append(ctx.step(D, mode)[:5])
    live = range(D.shape[0]) if live is None else live
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.dtype == b.dtype
            for l in live:
                assert np.array_equal(a[l], b[l], equal_nan=True)
    return outs[0]


def _random_problem(N, K, W, F, dtype, seed, B=1, T=700):
    """Sparse bursts on a little noise, so that the members' normalised rows differ and a sum in another order
    would round differently; the head of every signal is zero (windows assigned to (0, 0))."""
    rs = np.random.RandomState(seed)
    T = max(T, 6 * W)
    x = 1e-3 * rs.standard_normal((B, T, F))
    x += rs.standard_normal((B, T, F)) * (rs.rand(B, T, 1) < 0.1)
    x[:, :3 * W] = 0.0
    D = rs.standard_normal((B, K, W, F))
    D /= np.sqrt(np.sum(D ** 2, axis=(2, 3), keepdims=True))
    starts = rs.randint(0, T - 2 * W, (B, N)).astype(np.int64)
    mode = np.full((B,), 1 if dtype == np.float32 else 2, dtype=np.int32)
    return np.ascontiguousarray(x.astype(dtype)), starts, D.astype(dtype).astype(np.float64), mode


@pytest.mark.parametrize('N', [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7])
def test_plans_agree_across_window_counts(N, ctx):
    x, starts, D, mode = _random_problem(N, 5, 15, 1, np.float32, N)
    t, k, count, nonzero, sums = _steps_agree(ctx, lambda: ctx.set_data(x, starts, 15), D, mode)
    assert count.sum() == N and sums.dtype == np.float32
    assert np.array_equal(count[0], np.bincount(k[0], minlength=5))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('W,F', [(2, 1), (15, 1), (16, 4), (64, 4), (1, 257), (33, 16)], ids=lambda v: str(v))
def test_plans_agree_across_tile_widths(W, F, dtype, ctx):
    """Q = W * F in {2, 15, 64, 256, 257, 528}: less than a tile, one full tile, a tile of one element, three tiles."""
    x, starts, D, mode = _random_problem(2 * CHUNK + 5, 5, W, F, dtype, W * F)
    t, k, count, nonzero, sums = _steps_agree(ctx, lambda: ctx.set_data(x, starts, W), D, mode)
    assert count.sum() == 2 * CHUNK + 5 and np.count_nonzero(count) > 1


@pytest.mark.parametrize('K', [1, 5, 70])
def test_plans_agree_across_centroid_counts(K, ctx):
    x, starts, D, mode = _random_problem(CHUNK + 100, K, 8, 2, np.float64, K)
    t, k, count, nonzero, sums = _steps_agree(ctx, lambda: ctx.set_data(x, starts, 8), D, mode)
    assert count.sum() == CHUNK + 100 and (K == 1 or np.count_nonzero(count) > 1)


def _rows_per_batch(tw):
    """Members a workgroup of wide_sum_kernel stages per half of its ring, for a tile of tw elements (their rows lie at
    a pitch of tw rounded up to a power of two)."""
    return (RING * 256) // (1 << (tw - 1).bit_length())


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('W,F', [(16, 16), (15, 1)], ids=['Q256', 'Q15'])
def test_plans_agree_across_member_counts(W, F, dtype, ctx):
    """K = 3: all-zero windows go to centroid 0, windows around a planted copy of atom 2 to centroid 2 (no other atom
    correlates as strongly anywhere in them), centroid 1 stays empty (count 0).  Centroid 2's member count walks the
    batches of the ring: 1, one short of a batch, a batch, one more, two batches and one."""
    rb = _rows_per_batch(min(256, W * F))
    assert rb == RING or W * F < 256
    rs = np.random.RandomState(W)
    D = rs.standard_normal((3, W, F))
    D /= np.sqrt(np.sum(D ** 2, axis=(1, 2), keepdims=True))
    sites = 9
    T = sites * 3 * W + 4 * W
    x = np.zeros((T, F))
    where = []
    for i in range(sites):                                                # atom 2, scaled, under 1 % noise, W apart from the next
        at = 3 * W + i * 3 * W
        x[at:at + W] = rs.uniform(0.5, 2.0) * D[2] * (1.0 + 1e-2 * rs.standard_normal((W, F)))
        where.append(at)
    x = np.ascontiguousarray(x.astype(dtype)[np.newaxis])
    mode = np.array([1 if dtype == np.float32 else 2], dtype=np.int32)
    for m in (1, rb - 1, rb, rb + 1, 2 * rb + 1):
        planted = np.array([where[i % sites] - (i * 7) % (W + 1) for i in range(m)], dtype=np.int64)     # the atom at every t
        starts = np.concatenate([np.zeros(37, dtype=np.int64), planted, np.zeros(5, dtype=np.int64)])
        starts = starts[rs.permutation(len(starts))][np.newaxis]
        t, k, count, nonzero, sums = _steps_agree(ctx, lambda: ctx.set_data(x, starts, W), D[np.newaxis].astype(dtype).astype(np.float64), mode)
        assert count[0].tolist() == [42, 0, m], m
        assert not sums[0, 1].any() and not sums[0, 0].any() and sums[0, 2].any()


def test_every_window_in_one_centroid(ctx):
    """An all-zero stack assigns every window to (0, 0): one list of N members, over several chunks and batches."""
    N = 2 * CHUNK + 3
    lens = np.array([100, 33, 400], dtype=np.int64)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = np.zeros((int(ro[-1]), 2), dtype=np.float32)
    starts = np.random.RandomState(0).randint(0, 400 - 32, N).astype(np.int64) + ro[2]
    D = np.random.RandomState(1).standard_normal((1, 4, 16, 2)).astype(np.float32).astype(np.float64)
    t, k, count, nonzero, sums = _steps_agree(ctx, lambda: ctx.set_corpus(x, ro, starts, 16), D, np.array([1], dtype=np.int32))
    assert not t.any() and not k.any() and count[0].tolist() == [N, 0, 0, 0] and nonzero[0].tolist() == [1, 0, 0, 0]
    assert not sums.any()


def _ragged_stack(dtype, F, lens, seed):
    rs = np.random.RandomState(seed)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = rs.standard_normal((int(ro[-1]), F)) * (rs.rand(int(ro[-1]), 1) < 0.2)
    return np.ascontiguousarray(x.astype(dtype)), ro


def _ragged_starts(ro, W, N, rs):
    """Window starts over the stack, the last admissible row of every signal (the window ends at the signal's end) first."""
    lens = np.diff(ro)
    sig = rs.randint(0, len(lens), N)
    local = (rs.rand(N) * (lens[sig] - 2 * W + 1)).astype(np.int64)
    local[:len(lens)] = lens - 2 * W
    sig[:len(lens)] = np.arange(len(lens))
    return (ro[sig] + local).astype(np.int64)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_plans_agree_on_corpus_and_batch_data(dtype, ctx):
    W, F, K = 9, 3, 6
    x, ro = _ragged_stack(dtype, F, [2 * W + 1, 500, 64, 2 * W + 1, 301], 5)
    rs = np.random.RandomState(6)
    starts = _ragged_starts(ro, W, CHUNK + 9, rs)
    D = rs.standard_normal((1, K, W, F)).astype(dtype).astype(np.float64)
    mode = np.array([1 if dtype == np.float32 else 2], dtype=np.int32)
    _steps_agree(ctx, lambda: ctx.set_corpus(x, ro, starts, W), D, mode)
    # plain data, three learners, the middle one skipped
    xb, sb, Db, mb = _random_problem(CHUNK + 9, K, W, F, dtype, 8, B=3)
    mb[1] = kmeans.SKIP
    _steps_agree(ctx, lambda: ctx.set_data(xb, sb, W), Db, mb, live=(0, 2))


# ------------------------------------------------------------------------------------------------ 4. the twin
@pytest.mark.parametrize('plan', [PLAN_LISTS, PLAN_WIDE], ids=['lists', 'wide'])
@pytest.mark.parametrize('W,F,dtype', [(8, 1, np.float32), (9, 3, np.float64)], ids=['f32', 'f64'])
def test_step_matches_twin_on_ragged_stack(W, F, dtype, plan, ctx):
    x, ro = _ragged_stack(dtype, F, [2 * W + 1, 300, 2 * W + 2, 150], 3)
    rs = np.random.RandomState(4)
    starts = _ragged_starts(ro, W, 300, rs)
    assert np.all(np.isin(ro[1:] - 2 * W, starts))                       # windows ending exactly at every signal's end
    D = rs.standard_normal((1, 7, W, F))
    D = (D / np.sqrt(np.sum(D ** 2, axis=(2, 3), keepdims=True))).astype(dtype).astype(np.float64)
    mode = np.array([1 if dtype == np.float32 else 2], dtype=np.int32)
    ctx.set_plan(plan)
    ctx.set_corpus(x, ro, starts, W)
    got = ctx.step(D, mode)[:5]
    twin = crst.FakeCorpusContext()
    twin.set_corpus(x, ro, starts, W)
    exp = twin.step(D, mode)[:5]
    for a, b in zip(got, exp):
        assert _same(a, b)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_set_corpus_and_set_plan_refusals(ctx):
    W = 8
    x, ro = _ragged_stack(np.float32, 1, [40, 17, 60], 1)
    ok = np.array([0, 40, 57, 57 + 60 - 16], dtype=np.int64)

    def refused(match, code, ro_=ro, starts=ok, x_=x):
        with pytest.raises(_native.HscmpError, match=match) as e:
            ctx.set_corpus(x_, ro_, starts, W)
        assert e.value.code == code

    refused(r'window 1 \(rows 30 \.\. 46\) crosses the end of signal 0 at row 40', -1, starts=np.array([0, 30], dtype=np.int64))
    refused(r'window 0 .* crosses the end of signal 2', -1, starts=np.array([57 + 60 - 15], dtype=np.int64))
    refused(r'start -1 of window 2 is outside', -1, starts=np.array([0, 0, -1], dtype=np.int64))
    refused(r'row_offsets descend at signal 1', -1, ro_=np.array([0, 60, 40, 117], dtype=np.int64))
    refused(r'signal 1 has 16 samples', -1, ro_=np.array([0, 40, 56, 117], dtype=np.int64))
    with pytest.raises(_native.HscmpError, match=r'plan = 3 is not') as e:
        ctx.set_plan(3)
    assert e.value.code == -1
    # the context still works
    ctx.set_corpus(x, ro, ok, W)
    D = np.random.RandomState(2).standard_normal((1, 3, W, 1)).astype(np.float32).astype(np.float64)
    t, k, count, nonzero, sums = ctx.step(D, np.array([1], dtype=np.int32))[:5]
    assert count.sum() == 4
    ctx.set_plan(PLAN_WIDE)
    with pytest.raises(_native.HscmpError, match='the wide plan takes K <= %d' % kmeans.WIDE_MAX_K) as e:
        ctx.step(np.zeros((1, kmeans.WIDE_MAX_K + 1, W, 1)), np.array([1], dtype=np.int32))
    assert e.value.code == -5
    assert ctx.step(D, np.array([1], dtype=np.int32))[2].sum() == 4


# ------------------------------------------------------------------------------------------------ 6. one context reused
def test_context_reused_across_corpus_and_plain_data(monkeypatch):
    signals = [_signal(T, 2, np.float64, 20 + T) for T in (400, 90, 700)]
    x = _signal(900, None, np.float32, 30)
    kw = dict(nbRandomWindows=250, maxIterations=4, resetMethod='random_samples')

    def corpus():
        return ConvolutionalKMeansLearner(6, 12, rng=np.random.RandomState(1)).trainCorpus(signals, **kw)

    def plain():
        return ConvolutionalKMeansLearner(5, 16, rng=np.random.RandomState(2)).train(x, **kw)

    fresh = []
    for run in (corpus, plain):
        monkeypatch.setattr(kmeans, '_contexts', {})
        fresh.append(run())
    monkeypatch.setattr(kmeans, '_contexts', {})
    assert _same(corpus(), fresh[0])
    assert _same(plain(), fresh[1])
    assert _same(corpus(), fresh[0])
    assert len(kmeans._contexts) == 1
