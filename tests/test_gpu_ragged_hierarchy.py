"""Ragged batches through the whole hierarchy on the GPU: computeCoefficientsRaggedBatch,
computeCoefficientsFromLevelRaggedBatch and MultilevelDictionaryLearner.trainRaggedCorpus.

Two dictionaries of three levels: one learnt by the uniform MultilevelDictionaryLearner, as in
tests/test_gpu_from_level_batch.py, and one from MultilevelDictionaryGenerator, as in tests/test_hierarchical.py -- decomposition
dictionaries, so the chain runs on row lists: the scatter writes them, prepare_from_slots walks them, dictlist_init and the
dictlist loops read them, kept lists are cleared lazily between chunks.  The generator does not terminate for the scales
[8, 12, 20] of the learnt case (no decomposition of a 12-sample pattern into 8-sample ones); the generated case uses [8, 16, 36].
Per signal, the matrices of all levels, the residual and the event records must equal, bit for bit, the hierarchical
host logic driven by the CPU oracle as its level coder on the signal alone, and the uniform computeCoefficientsBatch of the
signal alone.  The lengths include the widest filter Wmax, 3 Wmax - 3 and the stride."""
import numpy as np
import pytest
import scipy.sparse

import hsc_amd.synth as synth
from hsc_amd.dataset import (MultilevelDictionary, MultilevelDictionaryGenerator, SignalGenerator, convertSparseMatricesToEvents,
                             scalesToWindowSizes)
from hsc_amd.modeling import (HierarchicalConvolutionalMatchingPursuit, HierarchicalConvolutionalSparseCoder,
                              MultilevelDictionaryLearner)

pytestmark = pytest.mark.gpu

COUNTS, SCALES = [4, 3, 3], [8, 12, 20]
KMEANS = dict(nbRandomWindows=200, maxIterations=3, tolerance=0.0, resetMethod='random_samples')
ENCODE = dict(toleranceSnr=10, nbBlocks=4, singletonWeight=0.95)
GENERATED_SCALES = [8, 16, 36]             # (see the module docstring)
B = 5


def _lengths(scales):
    wmax = int(max(scalesToWindowSizes(np.asarray(scales))))
    return [512, wmax, 3 * wmax - 3, 333, 200]


LENGTHS = _lengths(SCALES)


class _OracleLevelCoder(object):
    """Stand-in level coder: same encode() contract, computed by the CPU oracle (the arrangement of tests/test_hierarchical.py)."""

    def __init__(self, D):
        self.D = D

    def encode(self, X, **kw):
        from oracle import hsc_oracle as orc
        coefficients, residual, _ = orc.cmp_encode(np.asarray(X), self.D, **kw)
        return coefficients, residual


def _planted(lengths, ids=None, seed=2, dtype=np.float64):
    D = synth.make_dictionary(4, 8, seed=seed, dtype=dtype)
    ids = range(len(lengths)) if ids is None else ids
    return [synth.make_signal(D, int(n), i, kind='planted', nb_atoms=max(1, int(n) // 12), seed=seed, dtype=dtype) for i, n in zip(ids, lengths)]


# Signal numbers of LENGTHS: the signals of Wmax and 3 Wmax - 3 samples trade places.  At Wmax = 9 samples (W = 8 at level 0:
# multi-bounce reflection) signal 1 under nbBlocks=4 sends the reference's own pursuit round in circles -- the CPU oracle takes
# 7028 selections and ends with nothing --, which says nothing about ragged batches; signal 2 converges and reaches every level.
SIGNAL_IDS = [0, 2, 1, 3, 4]


def _learnt():
    """(signals, dictionary learnt by the uniform learner as in tests/test_gpu_from_level_batch.py)"""
    D = synth.make_dictionary(4, 8, seed=2, dtype=np.float64)
    corpus = synth.make_batch(D, 512, 0, 3, kind='planted', nb_atoms=512 // 12, seed=2, dtype=np.float64)
    learner = MultilevelDictionaryLearner(COUNTS, SCALES, method='cmp', rng=np.random.RandomState(6))
    mld = learner.trainCorpus(corpus, resume=False, **dict(KMEANS, **ENCODE))
    return _planted(LENGTHS, SIGNAL_IDS), mld


def _generated():
    """(signals, decomposition dictionary with its singleton bases)"""
    rs = np.random.RandomState(503)
    mld = MultilevelDictionaryGenerator(rs).generate(scales=GENERATED_SCALES, counts=COUNTS, decompositionSize=2, multilevelDecomposition=False,
                                                     maxNbPatternsConsecutiveRejected=30)
    gen = SignalGenerator(mld, [0.02 / (l + 1) for l in range(3)], rng=rs)
    xs = []
    for n in _lengths(GENERATED_SCALES):
        # (rendered at the longest length and cut: the generator places whole patterns)
        x = gen.generateSignalFromEvents(gen.generateEvents(512), nbSamples=512)[:n]
        xs.append((x + 0.01 * rs.standard_normal(x.shape)).astype(np.float32))
    return xs, mld.withSingletonBases()


@pytest.fixture(scope='module')
def cases():
    """name -> (name, signals, dictionary, coder, cache of ragged runs, cache of per-signal references), built on first use"""
    made = {}

    def get(name):
        if name not in made:
            xs, mld = _learnt() if name == 'learnt' else _generated()
            assert mld.getNbLevels() == 3 and [len(x) for x in xs] == _lengths(SCALES if name == 'learnt' else GENERATED_SCALES)
            made[name] = (name, xs, mld, HierarchicalConvolutionalMatchingPursuit(method='cmp'), {}, {})
        return made[name]
    yield get
    for c in made.values():
        c[3].close()


@pytest.fixture(params=['learnt', 'generated'])
def case(request, cases):
    return cases(request.param)


def _ragged(case, **kw):
    name, xs, mld, hcmp, cache, _ = case
    key = tuple(sorted((k, str(v)) for k, v in kw.items()))
    if key not in cache:
        cache[key] = hcmp.computeCoefficientsRaggedBatch(xs, mld, returnEvents=True, **dict(ENCODE, **kw))
    return cache[key]


def _oracle_reference(case, b, distributed, nbBlocks=4):
    """Signal b alone through the hierarchical host logic with the CPU oracle as its level coder: computed once, shared."""
    name, xs, mld, _, _, refs = case
    key = (b, distributed, str(nbBlocks))
    if key not in refs:
        ref = HierarchicalConvolutionalMatchingPursuit(method='cmp')
        ref._level_coder = lambda D: _OracleLevelCoder(D)
        coefs, residual = ref.computeCoefficients(xs[b], mld, returnDistributed=distributed, **dict(ENCODE, nbBlocks=nbBlocks))
        refs[key] = (coefs, np.asarray(residual, dtype=np.float64), convertSparseMatricesToEvents(coefs))
    return refs[key]


def _same_levels(got, exp, what=''):
    assert len(got) == len(exp), what
    for l, (a, e) in enumerate(zip(got, exp)):
        a, e = scipy.sparse.csc_matrix(a), scipy.sparse.csc_matrix(e)
        a.sort_indices(); e.sort_indices()
        assert a.shape == e.shape, (what, l, a.shape, e.shape)
        assert np.array_equal(a.indptr, e.indptr) and np.array_equal(a.indices, e.indices), (what, l)
        assert a.data.astype(np.float64).tobytes() == e.data.astype(np.float64).tobytes(), (what, l)


def _same_run(got, exp):
    """Two ragged runs byte for byte: matrices, residuals, events."""
    for b in range(B):
        _same_levels(got[0][b], exp[0][b], b)
        assert np.asarray(got[1][b]).tobytes() == np.asarray(exp[1][b]).tobytes(), b
        assert got[3][b].dtype == exp[3][b].dtype and got[3][b].tobytes() == exp[3][b].tobytes(), b


@pytest.mark.parametrize('distributed', [True, False], ids=['distributed', 'last_level'])
@pytest.mark.parametrize('nbBlocks', [4, 'auto'])
def test_ragged_equals_oracle_and_uniform_per_signal(case, distributed, nbBlocks):
    name, xs, mld, hcmp, _, _ = case
    coefs, residuals, timings, events = _ragged(case, returnDistributed=distributed, nbBlocks=nbBlocks)
    assert len(coefs) == len(residuals) == len(events) == B
    assert all(t['variant'].endswith('_ragged') for t in timings), [t['variant'] for t in timings]
    # levels >= 1 take the level kernels; the decomposition dictionaries the dictlist pair, on row lists
    assert all(t['variant'].startswith(('sparse_init+', 'dictlist_init+')) for t in timings[1:]), [t['variant'] for t in timings]
    if name == 'generated':
        assert all(t['variant'].startswith('dictlist_init+dictlist_loop') for t in timings[1:]), [t['variant'] for t in timings]
    if not distributed and nbBlocks == 4:
        # every signal, the one of exactly Wmax samples included, reaches the last level with something to encode
        assert all(c[2].nnz > 0 for c in coefs), [c[2].nnz for c in coefs]
    for b, x in enumerate(xs):
        n = len(x)
        assert [c.shape for c in coefs[b]] == [(n, mld.getRawDictionary(l).shape[0]) for l in range(3)]
        assert residuals[b].shape == (n,) and residuals[b].dtype == np.float64
        # the CPU oracle under the hierarchical host logic, on the signal alone
        ocoefs, ores, oev = _oracle_reference(case, b, distributed, nbBlocks)
        _same_levels(coefs[b], ocoefs, ('oracle', b))
        assert residuals[b].tobytes() == ores.tobytes(), b
        assert np.array_equal(events[b], oev), b
        # the uniform entry on the signal alone
        one = hcmp.computeCoefficientsBatch(x[np.newaxis], mld, returnDistributed=distributed, returnEvents=True, **dict(ENCODE, nbBlocks=nbBlocks))
        _same_levels(coefs[b], one[0][0], ('uniform', b))
        assert residuals[b].tobytes() == one[1][0].tobytes(), b
        assert events[b].dtype == one[3][0].dtype and events[b].tobytes() == one[3][0].tobytes(), b


def test_host_epilogue_energy_chunks_and_padded_form(case):
    name, xs, mld, hcmp, _, _ = case
    exp = _ragged(case)
    _same_run(hcmp.computeCoefficientsRaggedBatch(xs, mld, returnEvents=True, epilogue='host', **ENCODE), exp)
    # the energies, summed on the device: what a lone signal's uniform encode gives
    energy = hcmp.computeCoefficientsRaggedBatch(xs, mld, residuals='energy', **ENCODE)[1]
    assert energy.shape == (B,) and energy.dtype == np.float64
    for b, x in enumerate(xs):
        one = hcmp.computeCoefficientsBatch(x[np.newaxis], mld, residuals='energy', **ENCODE)[1]
        assert energy[b:b + 1].tobytes() == one.tobytes(), b
    # a memory budget that forces chunks of two signals (per signal: the formula of _LevelPipeline.chunk_size)
    lengths = [len(x) for x in xs]
    stride = max(lengths)
    per_signal = sum(1.05 * stride * mld.getRawDictionary(l).shape[2] * 8 + 160 * stride + 80.0 * 4096 for l in (1, 2))
    got = hcmp.computeCoefficientsRaggedBatch(xs, mld, returnEvents=True, memoryBudget=int(2.5 * per_signal), **ENCODE)
    assert got[2][1]['chunks'] == got[2][2]['chunks'] == 3
    _same_run(got, exp)
    # the padded form with lengths=.  (The host repacks it, zero padded, before the upload: this checks the repacking and
    # that the caller's padding is ignored; that the device never reads dead rows is tests/test_gpu_ragged_levels.py's.)
    x = np.full((B, stride), np.nan, dtype=xs[0].dtype)
    for b, s in enumerate(xs):
        x[b, :len(s)] = s
    _same_run(hcmp.computeCoefficientsRaggedBatch(x, mld, returnEvents=True, lengths=lengths, **ENCODE), exp)
    _same_run(HierarchicalConvolutionalSparseCoder(mld, hcmp).encodeRaggedBatch(xs, returnEvents=True, **ENCODE), exp)


def _first_levels(mld, n):
    if n == 1:
        return mld.upToLevel(0)
    return MultilevelDictionary.fromRawDictionaries(mld.dictionaries[:n], np.asarray(mld.scales)[:n], hasSingletonBases=True)


def test_level_by_level_equals_uninterrupted(cases):
    """(the learnt dictionary: its first levels are rebuilt from the same raw dictionaries, see _first_levels)"""
    case = cases('learnt')
    name, xs, mld, hcmp, _, _ = case
    exp = _ragged(case)
    c0 = hcmp.computeCoefficientsRaggedBatch(xs, mld.upToLevel(0), returnDistributed=False, **ENCODE)[0]
    c1, second, tm = hcmp.computeCoefficientsFromLevelRaggedBatch(xs, c0, _first_levels(mld, 2), returnDistributed=False, **ENCODE)
    assert second is None and tm[0]['variant'] == 'loaded' and tm[1]['variant'].endswith('_ragged')
    assert all(len(c) == 2 and c[1].shape == (len(x), 7) for c, x in zip(c1, xs))
    for given, loaded in ((c0, [True, False, False]), (c1, [True, True, False])):
        for kw in (dict(), dict(epilogue='host'), dict(memoryBudget=1)):
            got = hcmp.computeCoefficientsFromLevelRaggedBatch(xs, given, mld, residuals='samples', returnEvents=True, **dict(ENCODE, **kw))
            _same_run(got, exp)
            assert [t['variant'] == 'loaded' for t in got[2]] == loaded
            assert all(t['variant'].endswith('_ragged') for t, ld in zip(got[2], loaded) if not ld)
    coder = HierarchicalConvolutionalSparseCoder(mld, hcmp)
    _same_run(coder.encodeFromLevelRaggedBatch(xs, c1, residuals='samples', returnEvents=True, **ENCODE), exp)
    energy = hcmp.computeCoefficientsFromLevelRaggedBatch(xs, c1, mld, residuals='energy', **ENCODE)[1]
    assert energy.tobytes() == hcmp.computeCoefficientsRaggedBatch(xs, mld, residuals='energy', **ENCODE)[1].tobytes()


def test_load_level_ragged_refuses_a_dead_row_and_keeps_the_batch():
    from hsc_amd import _native
    K, T = 5, 40
    lens = np.array([40, 17, 25], dtype=np.int32)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(np.random.RandomState(0).standard_normal((K, 4, 1)))
        good = [scipy.sparse.random(int(n), K, density=0.2, format='csc', random_state=np.random.RandomState(b)) for b, n in enumerate(lens)]
        good[1] = scipy.sparse.csc_matrix(([1.5, -2.0], ([16, 3], [0, 4])), shape=(17, K))         # the last live row is fine
        eng.load_level_ragged(None, T, lens, good)
        st, sk, sa = eng.fetch_slots()
        stats = eng.fetch_stats()
        assert list(stats[:, _native.STAT_SLOTS]) == [m.nnz for m in good] and (stats[:, _native.STAT_STOP] == _native.STOP_LOADED).all()
        # row 17 of a signal of 17 rows: refused, naming signal, entry, row and T_b; the batch stays
        offsets = np.array([0, 1, 3, 3], dtype=np.int64)
        rows = np.array([5, 3, 17], dtype=np.int32); cols = np.array([0, 1, 2], dtype=np.int32); data = np.array([1.0, 2.0, 3.0])
        rc = eng._lib.hscmp_load_level_ragged(eng._h, None, 3, T, lens.ctypes.data, offsets.ctypes.data, rows.ctypes.data, cols.ctypes.data,
                                              data.ctypes.data)
        assert rc == _native.ERR_INVALID
        msg = eng._lib.hscmp_last_error(eng._h).decode()
        assert 'signal 1' in msg and 'entry 1' in msg and 'row 17' in msg and 'T_b=17' in msg, msg
        st2, sk2, sa2 = eng.fetch_slots()
        assert np.array_equal(st, st2) and np.array_equal(sk, sk2) and np.array_equal(sa, sa2)
        assert np.array_equal(stats, eng.fetch_stats())
        # a length outside [1, T]
        bad = np.array([40, 41, 25], dtype=np.int32)
        rc = eng._lib.hscmp_load_level_ragged(eng._h, None, 3, T, bad.ctypes.data, offsets.ctypes.data, rows.ctypes.data, cols.ctypes.data,
                                              data.ctypes.data)
        assert rc == _native.ERR_INVALID and 'signal 1' in eng._lib.hscmp_last_error(eng._h).decode()
        assert np.array_equal(stats, eng.fetch_stats())
    finally:
        eng.close()


def test_chain_refuses_a_signal_shorter_than_the_level_filter():
    """hscmp_encode_batch_from_level with a ragged previous level: HSCMP_ERR_INVALID naming signal and W when T_b < W of this level."""
    from hsc_amd import _native
    rs = np.random.RandomState(1)
    lens = np.array([40, 6, 25], dtype=np.int32)
    prev, lvl = _native.Engine(0), _native.Engine(0)
    try:
        prev.set_dictionary(rs.standard_normal((5, 4, 1)))
        lvl.set_dictionary(rs.standard_normal((3, 9, 5)), dtype=np.float64)
        prev.load_level_ragged(None, 40, lens, [scipy.sparse.random(int(n), 5, density=0.2, format='csc', random_state=rs) for n in lens])
        params = _native.make_params(None, None, 10.0, 1, 1e-16, float(np.finfo(np.float64).eps), 256, 0)
        with pytest.raises(_native.HscmpError) as e:
            lvl.encode_batch_from_level(prev, 0, 3, 1e-16, params)
        assert e.value.code == _native.ERR_INVALID and 'signal 1' in str(e.value) and 'W=9' in str(e.value)
        lvl.encode_batch_from_level(prev, 2, 1, 1e-16, params)             # (signal 2 alone is long enough)
        assert lvl.last_variant().endswith('_ragged')
    finally:
        prev.close(); lvl.close()


def _train(corpus, ragged, resume):
    learner = MultilevelDictionaryLearner(COUNTS, SCALES, method='cmp', rng=np.random.RandomState(6))
    fn = learner.trainRaggedCorpus if ragged else learner.trainCorpus
    mld = fn(corpus, resume=resume, **dict(KMEANS, **ENCODE))
    return mld, learner


def test_train_ragged_corpus():
    xs = _planted([512, 300, 411, 96])
    a, la = _train(xs, True, True)
    b, lb = _train(xs, True, False)
    assert a.getNbLevels() == 3
    for da, db in zip(la.lastDictionaries, lb.lastDictionaries):
        assert da.shape == db.shape and da.tobytes() == db.tobytes()
    assert la.lastStats[1]['input_shape'] == [(len(x), 4) for x in xs] and la.lastStats[0]['input_shape'] == [x.shape for x in xs]
    assert la.lastStats[1]['encode_timings'][0]['variant'] == 'loaded' and la.lastStats[1]['encode_timings'][1]['variant'].endswith('_ragged')
    assert lb.lastStats[1]['encode_timings'][0]['variant'].endswith('_ragged')
    # equal lengths: the uniform learner's dictionaries under the same seed
    same = _planted([256] * 4)
    c, lc = _train(same, True, True)
    d, ld = _train(np.stack(same), False, True)
    for dc, dd in zip(lc.lastDictionaries, ld.lastDictionaries):
        assert dc.shape == dd.shape and dc.tobytes() == dd.tobytes()
