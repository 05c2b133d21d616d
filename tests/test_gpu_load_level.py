"""hscmp_load_level at the ABI (include/hscmp.h): coefficient matrices the caller holds go back to the device as a context's
results.  A level chained from the loaded context equals, byte for byte, the level chained from the context that computed
those coefficients -- although the loaded slots are in column-major order, not in first-selection order.  float64; the
shapes are those of tests/test_gpu_multilevel.py."""
import numpy as np
import pytest
import scipy.sparse

import hsc_amd.synth as synth

pytestmark = pytest.mark.gpu

B, T, K0, W0 = 3, 512, 4, 8
K1, W1 = 3, 5
PARAMS = [dict(toleranceSnr=10, nbBlocks=4), dict(nbNonzeroCoefs=30)]


def _params(**kw):
    from hsc_amd import _native
    kw.setdefault('maxEvents', 4096)
    return _native.make_params(eps=float(np.finfo(np.float64).eps), **kw)


def _level1_dictionary(F=K0, K=K1, W=W1, seed=4):
    """F singleton atoms, then K atoms of three non-zeros; singletons down-weighted as the hierarchical encoder does."""
    rs = np.random.RandomState(seed)
    D = np.zeros((K, W, F))
    for k in range(K):
        for _ in range(3):
            D[k, rs.randint(0, W), rs.randint(0, F)] = rs.uniform(0.5, 1.5) * rs.choice([-1.0, 1.0])
    S = np.zeros((F, W, F))
    S[np.arange(F), (W - 1) // 2, np.arange(F)] = 1.0
    D = np.concatenate((S, D), axis=0)
    D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
    w = np.ones(F + K)
    w[:F] = 0.95
    return D, w


def _corpus(T=T, nb=None):
    D = synth.make_dictionary(K0, W0, seed=2, dtype=np.float64)
    x = synth.make_batch(D, T, 0, B, kind='planted', nb_atoms=nb or max(8, T // 12), seed=2, dtype=np.float64)
    return D, np.ascontiguousarray(x.reshape((B, T, 1)))


def _matrices(eng, T=T):
    """The engine's coefficient slots as canonical CSC matrices (what a caller of the encoder holds)."""
    from hsc_amd import _native
    st, sk, sa = eng.fetch_slots()
    n = eng.fetch_stats()[:, _native.STAT_SLOTS]
    out = []
    for b in range(st.shape[0]):
        m = scipy.sparse.coo_matrix((sa[b, :n[b]], (st[b, :n[b]], sk[b, :n[b]])), shape=(T, eng.K)).tocsc()
        m.eliminate_zeros()
        out.append(m)
    return out


def _slots(eng):
    from hsc_amd import _native
    st, sk, sa = eng.fetch_slots()
    n = eng.fetch_stats()[:, _native.STAT_SLOTS]
    return [(st[b, :n[b]].copy(), sk[b, :n[b]].copy(), sa[b, :n[b]].copy()) for b in range(st.shape[0])]


def _snapshot(eng):
    """Everything an encode leaves: counters, slots, events, residual."""
    from hsc_amd import _native
    stats = eng.fetch_stats().copy()
    t, k, c = eng.fetch_events()
    n = stats[:, _native.STAT_EVENTS]
    events = [(t[b, :n[b]].copy(), k[b, :n[b]].copy(), c[b, :n[b]].copy()) for b in range(stats.shape[0])]
    return stats, _slots(eng), events, eng.fetch_residual().copy()


def _same(a, b, signals=None):
    """Byte for byte (array_equal on the raw bytes: -0.0 and NaN payloads included)."""
    idx = range(a[0].shape[0]) if signals is None else signals
    for i in idx:
        assert a[0][i].tobytes() == b[0][i].tobytes(), ('stats', i, a[0][i], b[0][i])
        for u, v in zip(a[1][i] + a[2][i], b[1][i] + b[2][i]):
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), i
        assert a[3][i].tobytes() == b[3][i].tobytes(), ('residual', i)


@pytest.fixture(scope='module')
def level0():
    """(e0, its matrices, e0b loaded with them, the level-1 dictionary and weights): computed once, left unchanged."""
    from hsc_amd import _native
    D0, x = _corpus()
    e0, e0b = _native.Engine(0), _native.Engine(0)
    e0.set_dictionary(D0)
    e0.encode_batch(x, _params(toleranceSnr=10, nbBlocks=4))
    mats = _matrices(e0)
    e0b.set_dictionary(D0)
    e0b.load_level(None, T, mats)
    D1, w1 = _level1_dictionary()
    yield e0, mats, e0b, D1, w1, x
    e0.close(); e0b.close()


def test_loaded_context_holds_the_matrices_in_column_major_order(level0):
    from hsc_amd import _native
    e0, mats, e0b, _, _, _ = level0
    stats = e0b.fetch_stats()
    assert e0b._batch == (B, T, max(m.nnz for m in mats))
    exp = np.zeros((B, _native.STAT_COUNT), dtype=np.int32)
    exp[:, _native.STAT_SLOTS] = [m.nnz for m in mats]
    exp[:, _native.STAT_STOP] = _native.STOP_LOADED
    assert np.array_equal(stats, exp) and all(m.nnz > 20 for m in mats)
    st, sk, sa = e0b.fetch_slots()
    for b, m in enumerate(mats):
        n = m.nnz
        assert np.array_equal(st[b, :n], m.indices) and np.array_equal(sk[b, :n], np.repeat(np.arange(K0), np.diff(m.indptr)))
        assert sa[b, :n].tobytes() == m.data.tobytes()
        assert not st[b, n:].any() and not sk[b, n:].any() and not sa[b, n:].any()      # zero behind the last entry
        # ... a different order from the encode's own (first selection), the same set
        t0, k0, a0 = _slots(e0)[b]
        keep = a0 != 0.0
        assert not np.array_equal(t0[keep], st[b, :n])
        o = np.lexsort((t0[keep], k0[keep]))
        assert np.array_equal(t0[keep][o], st[b, :n]) and np.array_equal(k0[keep][o], sk[b, :n]) and a0[keep][o].tobytes() == sa[b, :n].tobytes()
    assert e0b.last_variant() == 'loaded'


@pytest.mark.parametrize('first,count', [(0, 3), (1, 2)])
@pytest.mark.parametrize('params', PARAMS, ids=['snr10_blocks4', 'nnz30'])
def test_chain_from_loaded_equals_chain_from_encoded(level0, first, count, params):
    from hsc_amd import _native
    e0, _, e0b, D1, w1, _ = level0
    e1, e1b = _native.Engine(0), _native.Engine(0)
    try:
        for e, prev in ((e1, e0), (e1b, e0b)):
            e.set_dictionary(D1, w1)
            e.encode_batch_from_level(prev, first, count, 1e-16, _params(**params))
        a, b = _snapshot(e1), _snapshot(e1b)
        assert a[0].shape[0] == count and (a[0][:, _native.STAT_ITERATIONS] > 0).all()
        _same(a, b)
        assert e1.last_variant() == e1b.last_variant()
    finally:
        e1.close(); e1b.close()


def test_emptied_signal_equals_the_all_zero_dense_input(level0):
    from hsc_amd import _native
    e0, mats, _, D1, w1, _ = level0
    p = dict(toleranceSnr=10, nbBlocks=4)
    es = [_native.Engine(0) for _ in range(4)]
    e1, eload, e1b, ez = es
    try:
        e1.set_dictionary(D1, w1)
        e1.encode_batch_from_level(e0, 0, B, 1e-16, _params(**p))
        eload.set_dictionary(synth.make_dictionary(K0, W0, seed=2, dtype=np.float64))
        eload.load_level(None, T, [mats[0], scipy.sparse.csc_matrix((T, K0)), mats[2]])
        assert eload.fetch_stats()[:, _native.STAT_SLOTS].tolist() == [mats[0].nnz, 0, mats[2].nnz]
        e1b.set_dictionary(D1, w1)
        e1b.encode_batch_from_level(eload, 0, B, 1e-16, _params(**p))
        ez.set_dictionary(D1, w1)
        ez.encode_batch(np.zeros((1, T, K0)), _params(**p))
        a, b, z = _snapshot(e1), _snapshot(e1b), _snapshot(ez)
        _same(a, b, signals=[0, 2])
        assert b[0][1].tobytes() == z[0][0].tobytes() and b[0][1][_native.STAT_ITERATIONS] == 0
        assert len(b[1][1][0]) == 0 and len(b[2][1][0]) == 0 and len(z[2][0][0]) == 0
        assert b[3][1].tobytes() == z[3][0].tobytes() and not b[3][1].any()
    finally:
        for e in es:
            e.close()


def test_long_list_takes_the_sorted_prepare_kernel(level0, monkeypatch):
    """The chain's energy kernel for long lists (prepare_from_slots_sorted_kernel) is chosen by the longest list against
    HSCMP_SORTED_PREPARE_MIN: lowered to 16, every list here is longer, so the sorted kernel runs; with
    HSCMP_NO_SORTED_PREPARE the unsorted one.  Both from the loaded context, both equal to the chain from the encoded one."""
    from hsc_amd import _native
    e0, mats, e0b, D1, w1, _ = level0
    assert min(m.nnz for m in mats) > 16
    p = dict(toleranceSnr=10, nbBlocks=4)
    snaps = {}
    for name, env, prev in (('sorted_loaded', ('HSCMP_SORTED_PREPARE_MIN', '16'), e0b), ('unsorted_loaded', ('HSCMP_NO_SORTED_PREPARE', '1'), e0b),
                            ('sorted_encoded', ('HSCMP_SORTED_PREPARE_MIN', '16'), e0)):
        monkeypatch.setenv(*env)
        e1 = _native.Engine(0)
        try:
            e1.set_dictionary(D1, w1)
            e1.encode_batch_from_level(prev, 0, B, 1e-16, _params(**p))
            snaps[name] = _snapshot(e1)
        finally:
            e1.close()
            monkeypatch.delenv(env[0])
    _same(snaps['sorted_loaded'], snaps['unsorted_loaded'])
    _same(snaps['sorted_loaded'], snaps['sorted_encoded'])


def _bad(mats, b, edit):
    """(offsets, rows, cols, data) of `mats` with edit(rows, cols, data, lo) applied to signal b's range."""
    from hsc_amd import _native
    offsets, rows, cols, data, _ = _native.pack_level(mats, T, K0)
    edit(rows, cols, data, int(offsets[b]))
    return offsets, rows, cols, data


def _raw_load(eng, offsets, rows, cols, data):
    from hsc_amd import _native
    p = _native._ptr
    return eng._lib.hscmp_load_level(eng._h, None, len(offsets) - 1, T, p(offsets), p(rows), p(cols), p(data))


def _set(name, i, v):
    def edit(rows, cols, data, lo):
        dict(rows=rows, cols=cols, data=data)[name][lo + i] = v
    return edit


def _equal_pair(rows, cols, data, lo):
    rows[lo + 6], cols[lo + 6] = rows[lo + 5], cols[lo + 5]


@pytest.mark.parametrize('case,b,edit,entry,why', [
    ('row_T', 1, _set('rows', 3, T), 3, r'row outside \[0, T\)'),
    ('col_K', 2, _set('cols', 0, K0), 0, r'column outside \[0, K\)'),
    ('zero', 0, _set('data', 7, 0.0), 7, 'value zero or not finite'),
    ('nan', 1, _set('data', 0, float('nan')), 0, 'value zero or not finite'),
    ('equal_pair', 2, _equal_pair, 6, r'\(column, row\) not above the entry before it'),
])
def test_rejections_name_the_signal_and_leave_the_batch(level0, case, b, edit, entry, why):
    import re
    from hsc_amd import _native
    e0, mats, _, _, _, _ = level0
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(synth.make_dictionary(K0, W0, seed=2, dtype=np.float64))
        eng.load_level(None, T, mats[::-1])                     # a batch to keep
        before = (eng.fetch_stats().copy(), _slots(eng))
        assert _raw_load(eng, *_bad(mats, b, edit)) == _native.ERR_INVALID
        msg = eng._lib.hscmp_last_error(eng._h).decode()
        assert re.match(r'hscmp_load_level: signal %d, entry %d \(.*\): %s$' % (b, entry, why), msg), msg
        after = (eng.fetch_stats(), _slots(eng))
        assert np.array_equal(before[0], after[0])
        for u, v in zip(before[1], after[1]):
            assert all(p.tobytes() == q.tobytes() for p, q in zip(u, v))
        # ... and the same holds for a batch that was encoded, which a chain can still read
        if case == 'row_T':
            snap = _slots(e0)
            assert _raw_load(e0, *_bad(mats, b, edit)) == _native.ERR_INVALID
            for u, v in zip(snap, _slots(e0)):
                assert all(p.tobytes() == q.tobytes() for p, q in zip(u, v))
            assert e0.fetch_residual().shape == (B, T, 1)
    finally:
        eng.close()


def test_host_argument_checks(level0):
    from hsc_amd import _native
    _, mats, _, _, _, _ = level0
    eng = _native.Engine(0)
    try:
        offsets, rows, cols, data, _ = _native.pack_level(mats, T, K0)
        assert _raw_load(eng, offsets, rows, cols, data) == _native.ERR_STATE          # no dictionary
        eng.set_dictionary(synth.make_dictionary(K0, W0, seed=2, dtype=np.float64))
        bad = offsets.copy(); bad[2] = bad[1] - 1
        assert _raw_load(eng, bad, rows, cols, data) == _native.ERR_INVALID
        assert 'signal 1: offsets decrease' in eng._lib.hscmp_last_error(eng._h).decode()
        bad = offsets.copy(); bad[0] = 1
        assert _raw_load(eng, bad, rows, cols, data) == _native.ERR_INVALID
        assert eng._lib.hscmp_fetch_stats(eng._h, None) == _native.ERR_STATE           # still no batch
    finally:
        eng.close()


def test_loaded_context_refuses_what_only_an_encode_leaves(level0):
    from hsc_amd import _native
    _, _, e0b, _, _, _ = level0
    for call, args in ((e0b.continue_rounds, (0,)), (e0b.grow_events, (1 << 14,)), (e0b.fetch_residual, ()), (e0b.fetch_events, ()),
                       (e0b.stop_signal, (0,)), (e0b.device_view, ()), (e0b.fetch_energies, ())):
        with pytest.raises(_native.HscmpError, match='the batch was loaded') as info:
            call(*args)
        assert info.value.code == _native.ERR_STATE
    assert e0b.fetch_stats()[0, _native.STAT_STOP] == _native.STOP_LOADED           # ... and is still there


def test_loaded_signals_serve_the_epilogue_as_level0_but_not_as_last(level0):
    """With x the loaded context is the epilogue's level0: the residual equals the one from the context that encoded x."""
    from hsc_amd import _native
    e0, mats, _, D1, w1, x = level0
    D0 = synth.make_dictionary(K0, W0, seed=2, dtype=np.float64)
    ex, e1, e1b = _native.Engine(0), _native.Engine(0), _native.Engine(0)
    try:
        ex.set_dictionary(D0)
        ex.load_level(x, T, mats)
        out = []
        for e, prev in ((e1, e0), (e1b, ex)):
            e.set_dictionary(D1, w1)
            e.encode_batch_from_level(prev, 0, B, 1e-16, _params(toleranceSnr=10, nbBlocks=4))
            counts = e.fetch_stats()[:, _native.STAT_SLOTS]
            rep1 = np.random.RandomState(8).standard_normal((K0 + K1, W0 + W1 - 1, 1))     # (any patterns: both runs get the same)
            out.append(e.hierarchy_epilogue(prev, 0, [(0, 0, None), (0, K0 + K1, rep1)], 1e-16, counts))
        for u, v in zip(out[0], out[1]):
            assert u.tobytes() == v.tobytes()
        with pytest.raises(_native.HscmpError, match='the batch was loaded') as info:
            ex.hierarchy_epilogue(ex, 0, [(0, K0, D0[:, :, np.newaxis])], 1e-16, [m.nnz for m in mats])
        assert info.value.code == _native.ERR_STATE
    finally:
        for e in (ex, e1, e1b):
            e.close()


def test_allocation_failure_leaves_no_batch_and_a_usable_engine(level0, monkeypatch):
    """HSCMP_ALLOC_FAIL_AT = n fails the n-th device allocation of the call (tests/test_gpu_alloc_failure.py): swept until
    load_level first succeeds.  Behind every failure the engine holds no batch, and it encodes afterwards."""
    from hsc_amd import _native
    _, mats, _, _, _, x = level0
    D0 = synth.make_dictionary(K0, W0, seed=2, dtype=np.float64)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D0)
        failures = 0
        for n in range(1, 16):
            eng.encode_batch(x[:1], _params(nbNonzeroCoefs=4, maxEvents=8))           # a batch the failed call must not leave half alive
            monkeypatch.setenv('HSCMP_ALLOC_FAIL_AT', str(n))
            try:
                eng.load_level(x, T, mats)
                rc = 0
            except _native.HscmpError as ex:
                rc = ex.code
            monkeypatch.delenv('HSCMP_ALLOC_FAIL_AT')
            if rc == 0:
                break
            failures += 1
            assert rc == _native.ERR_ALLOC
            for probe in (eng._lib.hscmp_fetch_stats(eng._h, None), eng._lib.hscmp_continue(eng._h, 0)):
                assert probe == _native.ERR_STATE
            assert 'no batch encoded' in eng._lib.hscmp_last_error(eng._h).decode()
        # (the staging, and what the one-signal encode's buffers are too small for)
        assert rc == 0 and failures >= 2
        assert eng.fetch_stats()[:, _native.STAT_SLOTS].tolist() == [m.nnz for m in mats]
        eng.encode_batch(x, _params(toleranceSnr=10, nbBlocks=4))
        assert (eng.fetch_stats()[:, _native.STAT_ITERATIONS] > 0).all()
    finally:
        eng.close()
