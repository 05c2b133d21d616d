"""A toleranceSnr per signal and level through the hierarchical batch encodes: computeCoefficientsBatch,
computeCoefficientsRaggedBatch, their from-level forms and MultilevelDictionaryLearner.trainCorpus with a table [B, nbLevels].

The cases are the two three-level dictionaries of tests/test_gpu_ragged_hierarchy.py with their five signals; the uniform batch is
those signals cut or padded to 256 samples.  What defines the result: signal b comes out, byte for byte in the matrices of all
levels, the residual and the events, as the same method returns it alone with toleranceSnr=list(S[b]) -- and, for the generated
dictionary, as the hierarchical host logic returns it with the CPU oracle as its level coder.  That the table S can tell a
signal's targets from its neighbours' is tests/test_rules_hierarchy_census.py's.

One GPU test runs every row -- those below and the engine-level ones of tests/test_gpu_from_level_rules.py -- and names each row
that fails: a row takes milliseconds (the whole test about three seconds), and the suite's item count grows by one, not by 26
(as tests/test_gpu_rules.py groups its rows)."""
import numpy as np
import pytest

from hsc_amd.dataset import convertSparseMatricesToEvents
from hsc_amd.modeling import HierarchicalConvolutionalSparseCoder, MultilevelDictionaryLearner
from tests.rules_hierarchy_util import S, SINGLETON_WEIGHT, oracle_hcmp
from tests.test_gpu_ragged_hierarchy import COUNTS, KMEANS, SCALES, _first_levels, _same_levels, cases  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

B, T_UNIFORM = 5, 256
TABLE = np.array(S, dtype=np.float64)
_ALONE = {}


def _uniform(xs):
    """The five signals cut or padded (with zeros) to one length."""
    x = np.zeros((len(xs), T_UNIFORM), dtype=xs[0].dtype)
    for b, s in enumerate(xs):
        n = min(len(s), T_UNIFORM)
        x[b, :n] = s[:n]
    return x


def _run(hcmp, form, signals, mld, table, **kw):
    """(levels per signal, residual per signal, events per signal, timings) of one batch call; form: 'uniform' or 'ragged'."""
    kw = dict(dict(nbBlocks=4, singletonWeight=SINGLETON_WEIGHT, returnEvents=True), **kw)
    fn = hcmp.computeCoefficientsBatch if form == 'uniform' else hcmp.computeCoefficientsRaggedBatch
    coefs, second, timings, events = fn(signals, mld, toleranceSnr=table, **kw)
    return coefs, [second[b] for b in range(len(coefs))], events, timings


def _signals(case, form):
    xs = case[1]
    return _uniform(xs) if form == 'uniform' else xs


def _alone(case, form, b, **kw):
    """Signal b through the same method alone with its row as the one-per-level list: computed once per key."""
    name, xs, mld, hcmp = case[:4]
    key = (name, form, b) + tuple(sorted((k, str(v)) for k, v in kw.items()))
    if key not in _ALONE:
        sig = _signals(case, form)
        one = sig[b:b + 1] if form == 'uniform' else [sig[b]]
        coefs, res, events, _ = _run(hcmp, form, one, mld, list(S[b]), **kw)
        _ALONE[key] = (coefs[0], res[0], events[0])
    return _ALONE[key]


def _oracle(case, form, b, distributed, nbBlocks):
    name, xs, mld = case[:3]
    key = (name, form, b, 'oracle', distributed, str(nbBlocks))
    if key not in _ALONE:
        x = _signals(case, form)[b]
        coefs, residual = oracle_hcmp().computeCoefficients(x, mld, toleranceSnr=list(S[b]), nbBlocks=nbBlocks, singletonWeight=SINGLETON_WEIGHT,
                                                            returnDistributed=distributed)
        _ALONE[key] = (coefs, np.asarray(residual, dtype=np.float64), convertSparseMatricesToEvents(coefs))
    return _ALONE[key]


def _same_signal(got, exp, what):
    _same_levels(got[0], exp[0], what)
    assert np.asarray(got[1]).dtype == np.asarray(exp[1]).dtype and np.asarray(got[1]).tobytes() == np.asarray(exp[1]).tobytes(), what
    assert got[2].dtype == exp[2].dtype and got[2].tobytes() == exp[2].tobytes(), what


def _same_batch(got, exp, what=''):
    for b in range(B):
        _same_signal((got[0][b], got[1][b], got[2][b]), (exp[0][b], exp[1][b], exp[2][b]), (what, b))


def _differing_signals(got, exp):
    out = []
    for b in range(B):
        try:
            _same_signal((got[0][b], got[1][b], got[2][b]), (exp[0][b], exp[1][b], exp[2][b]), b)
        except AssertionError:
            out.append(b)
    return out


def _every_signal_equals_its_own_encode(case, distributed, nbBlocks):
    name, xs, mld, hcmp = case[:4]
    kw = dict(returnDistributed=distributed, nbBlocks=nbBlocks)
    for form in ('uniform', 'ragged'):
        sig = _signals(case, form)
        coefs, res, events, timings = _run(hcmp, form, sig, mld, TABLE, **kw)
        assert len(coefs) == len(res) == len(events) == B
        assert all(t['variant'].endswith('_rules') for t in timings), [t['variant'] for t in timings]
        for b in range(B):
            n = len(sig[b])
            assert [c.shape for c in coefs[b]] == [(n, mld.getRawDictionary(l).shape[0]) for l in range(3)]
            assert res[b].shape == (n,) and res[b].dtype == np.float64
            _same_signal((coefs[b], res[b], events[b]), _alone(case, form, b, **kw), (form, 'alone', b))
            if name == 'generated':
                _same_signal((coefs[b], res[b], events[b]), _oracle(case, form, b, distributed, nbBlocks), (form, 'oracle', b))


def _equal_rows_are_the_per_level_call_and_one_row_for_all_is_another_result(case):
    name, xs, mld, hcmp = case[:4]
    for form in ('uniform', 'ragged'):
        sig = _signals(case, form)
        table = _run(hcmp, form, sig, mld, TABLE)
        # five equal rows: exactly what the one-per-level list gives
        per_level = _run(hcmp, form, sig, mld, list(S[2]))
        assert not any(t['variant'].endswith('_rules') for t in per_level[3])
        equal_rows = _run(hcmp, form, sig, mld, np.tile(TABLE[2], (B, 1)))
        assert all(t['variant'].endswith('_rules') for t in equal_rows[3])
        _same_batch(equal_rows, per_level, form)
        # row 0 for everybody is not the table's result
        row0 = _run(hcmp, form, sig, mld, list(S[0]))
        _same_signal((row0[0][0], row0[1][0], row0[2][0]), (table[0][0], table[1][0], table[2][0]), (form, 0))
        differing = _differing_signals(row0, table)
        assert len(differing) >= 3, (form, differing)


def _host_epilogue_energy_chunks_and_device_input(case):
    import torch
    from hsc_amd.modeling import _compute_dtype
    name, xs, mld, hcmp = case[:4]
    for form in ('uniform', 'ragged'):
        sig = _signals(case, form)
        exp = _run(hcmp, form, sig, mld, TABLE)
        _same_batch(_run(hcmp, form, sig, mld, TABLE, epilogue='host'), exp, (form, 'host'))
        # the energies, summed on the device: each signal's own encode's
        fn = hcmp.computeCoefficientsBatch if form == 'uniform' else hcmp.computeCoefficientsRaggedBatch
        kw = dict(nbBlocks=4, singletonWeight=SINGLETON_WEIGHT, residuals='energy')
        energy = fn(sig, mld, toleranceSnr=TABLE, **kw)[1]
        assert energy.shape == (B,) and energy.dtype == np.float64
        for b in range(B):
            one = fn(sig[b:b + 1] if form == 'uniform' else [sig[b]], mld, toleranceSnr=list(S[b]), **kw)[1]
            assert energy[b:b + 1].tobytes() == one.tobytes(), (form, b)
        # a memory budget that forces chunks of two, two and one signals (per signal: the formula of _LevelPipeline.chunk_size):
        # the levels >= 1 get their slice of the table
        stride = max(len(s) for s in sig)
        per_signal = sum(1.05 * stride * mld.getRawDictionary(l).shape[2] * 8 + 160 * stride + 80.0 * 4096 for l in (1, 2))
        got = _run(hcmp, form, sig, mld, TABLE, memoryBudget=int(2.5 * per_signal))
        assert got[3][1]['chunks'] == got[3][2]['chunks'] == 3
        _same_batch(got, exp, (form, 'chunks'))
        coder = HierarchicalConvolutionalSparseCoder(mld, hcmp)
        enc = coder.encodeBatch if form == 'uniform' else coder.encodeRaggedBatch
        c, r, _, e = enc(sig, toleranceSnr=TABLE, nbBlocks=4, singletonWeight=SINGLETON_WEIGHT, returnEvents=True)
        _same_batch((c, [r[b] for b in range(B)], e), exp, (form, 'coder'))
    # the signals already in GPU memory (the uniform method has deviceInput)
    x = _uniform(xs)
    x = np.ascontiguousarray(x, dtype=_compute_dtype(x.dtype, mld.getRawDictionary(0).dtype))
    xd = torch.from_numpy(x).cuda()
    got = _run(hcmp, 'uniform', np.zeros_like(x), mld, TABLE, deviceInput=xd.data_ptr())
    assert all(t['variant'].endswith('_rules') for t in got[3])
    _same_batch(got, _run(hcmp, 'uniform', x, mld, TABLE), 'deviceInput')


def _from_a_level_with_the_table(cases):
    """(the learnt dictionary: its first levels are rebuilt from the same raw dictionaries, tests/test_gpu_ragged_hierarchy.py)"""
    case = cases('learnt')
    name, xs, mld, hcmp = case[:4]
    kw = dict(nbBlocks=4, singletonWeight=SINGLETON_WEIGHT)
    for form in ('uniform', 'ragged'):
        sig = _signals(case, form)
        full = hcmp.computeCoefficientsBatch if form == 'uniform' else hcmp.computeCoefficientsRaggedBatch
        resume = hcmp.computeCoefficientsFromLevelBatch if form == 'uniform' else hcmp.computeCoefficientsFromLevelRaggedBatch
        exp = _run(hcmp, form, sig, mld, TABLE)
        c0 = full(sig, mld.upToLevel(0), toleranceSnr=TABLE[:, :1], returnDistributed=False, **kw)[0]
        c1, second, tm = resume(sig, c0, _first_levels(mld, 2), toleranceSnr=TABLE[:, :2], returnDistributed=False, **kw)
        assert second is None and tm[0]['variant'] == 'loaded' and tm[1]['variant'].endswith('_rules')
        for given, loaded in ((c0, [True, False, False]), (c1, [True, True, False])):
            L = sum(loaded)
            table = TABLE.copy()
            table[:, :L] = np.nan                  # the columns below fromLevel are not read
            for more in (dict(), dict(epilogue='host'), dict(memoryBudget=1)):
                c, r, t, e = resume(sig, given, mld, toleranceSnr=table, residuals='samples', returnEvents=True, **dict(kw, **more))
                _same_batch((c, [r[b] for b in range(B)], e), exp, (form, L, more))
                assert [x['variant'] == 'loaded' for x in t] == loaded
                assert all(x['variant'].endswith('_rules') for x, ld in zip(t, loaded) if not ld)
        coder = HierarchicalConvolutionalSparseCoder(mld, hcmp)
        enc = coder.encodeFromLevelBatch if form == 'uniform' else coder.encodeFromLevelRaggedBatch
        c, r, _, e = enc(sig, c1, toleranceSnr=TABLE, residuals='samples', returnEvents=True, **kw)
        _same_batch((c, [r[b] for b in range(B)], e), exp, (form, 'coder'))


def _train_corpus_with_a_table():
    """trainCorpus with a target per signal and level: resume=True and resume=False learn the same dictionaries bit for bit, and
    the hand-off encodes are rules batches."""
    import hsc_amd.synth as synth
    D = synth.make_dictionary(4, 8, seed=2, dtype=np.float64)
    corpus = synth.make_batch(D, 512, 0, 3, kind='planted', nb_atoms=512 // 12, seed=2, dtype=np.float64)
    table = TABLE[:3, :2]
    learners = []
    for resume in (True, False):
        learner = MultilevelDictionaryLearner(COUNTS, SCALES, method='cmp', rng=np.random.RandomState(6))
        mld = learner.trainCorpus(corpus, resume=resume, toleranceSnr=table, nbBlocks=4, singletonWeight=SINGLETON_WEIGHT, **KMEANS)
        assert mld.getNbLevels() == 3
        learners.append(learner)
    la, lb = learners
    for da, db in zip(la.lastDictionaries, lb.lastDictionaries):
        assert da.shape == db.shape and da.tobytes() == db.tobytes()
    assert la.lastStats[1]['encode_timings'][0]['variant'] == 'loaded' and la.lastStats[1]['encode_timings'][1]['variant'].endswith('_rules')
    assert all(t['variant'].endswith('_rules') for t in lb.lastStats[1]['encode_timings'])
    assert la.lastStats[0]['encode_timings'][0]['variant'].endswith('_rules')


def _rows(cases):
    """(name, check) of every row: the hierarchy rows of this module, then the engine-level rows."""
    from tests.test_gpu_from_level_rules import ROWS as engine_rows
    rows = []
    for name in ('learnt', 'generated'):
        for nbBlocks in (4, 'auto', 1):
            for distributed in (True, False):
                rows.append(('every_signal_equals_its_own_encode[%s-%s-%s]' % (name, nbBlocks, 'distributed' if distributed else 'last_level'),
                             lambda n=name, d=distributed, nb=nbBlocks: _every_signal_equals_its_own_encode(cases(n), d, nb)))
        rows.append(('equal_rows_and_one_row_for_all[%s]' % name,
                     lambda n=name: _equal_rows_are_the_per_level_call_and_one_row_for_all_is_another_result(cases(n))))
        rows.append(('host_epilogue_energy_chunks_and_device_input[%s]' % name, lambda n=name: _host_epilogue_energy_chunks_and_device_input(cases(n))))
    rows.append(('from_a_level_with_the_table', lambda: _from_a_level_with_the_table(cases)))
    rows.append(('train_corpus_with_a_table', _train_corpus_with_a_table))
    return rows + [('from_level_rules: ' + name, check) for name, check in engine_rows]


def test_snr_table_through_the_hierarchy_and_the_chain(cases):  # noqa: F811
    """Every row of this module and of tests/test_gpu_from_level_rules.py; every failing row is named at the end."""
    rows = _rows(cases)
    assert len(rows) == 26
    failed = []
    for name, check in rows:
        try:
            check()
        except AssertionError as e:
            failed.append('%s: %s' % (name, (str(e).splitlines() or [repr(e)])[0]))
    assert not failed, '%d of %d rows failed:\n%s' % (len(failed), len(rows), '\n'.join(failed))
