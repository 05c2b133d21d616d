"""What a failed device allocation leaves behind (include/hscmp.h, "What a failed call leaves behind").

HSCMP_ALLOC_FAIL_AT=n makes the n-th device allocation of an entry-point call answer hipErrorOutOfMemory without calling
HIP.  Every case sweeps n = 1, 2, ... until the call first succeeds, and behind every failure probes the context IN THIS
ORDER: first hscmp_get_device_view (host only: it queues nothing whatever the state), and only when that answered as it
must, the calls that would queue kernels on a half-updated context if a state check were missing."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOB = 'HSCMP_ALLOC_FAIL_AT'
ERR_STATE = -4          # include/hscmp.h
F32, F64 = np.float32, np.float64


def _code(call, *args, **kw):
    """0, or the hscmp_status the call failed with."""
    from hsc_amd import _native
    try:
        call(*args, **kw)
    except _native.HscmpError as ex:
        assert ex.code != 0
        return ex.code
    return 0


def _raw_encode(eng, x, params):
    """hscmp_encode_batch past the Python layer's own bookkeeping (it has no dictionary shape after a failed set_dictionary)."""
    from hsc_amd import _native
    x3 = np.ascontiguousarray(x)
    return eng._lib.hscmp_encode_batch(eng._h, _native._ptr(x3), x3.shape[0], x3.shape[1], ctypes.byref(params))


def _sweep(monkeypatch, call, after_failure):
    """call() with the knob at 1, 2, ...: HSCMP_ERR_ALLOC and after_failure() every time until the first success."""
    from hsc_amd import _native
    for n in range(1, 64):
        monkeypatch.setenv(KNOB, str(n))
        rc = _code(call)
        monkeypatch.delenv(KNOB)
        if rc == 0:
            assert n > 1, 'the first allocation of the call did not fail'
            return n
        assert rc == _native.ERR_ALLOC, 'n=%d: status %d' % (n, rc)
        after_failure()
    raise AssertionError('the call did not succeed before n = 64')


def _no_batch(eng):
    """The probe order of the module docstring: the host-only call first."""
    assert _code(eng.device_view) == ERR_STATE
    assert _code(eng.continue_rounds, 2) == ERR_STATE


def _snapshot(eng):
    from hsc_amd import _native
    st = eng.fetch_stats().copy()
    t, k, c = eng.fetch_events()
    n = st[:, _native.STAT_EVENTS]
    ev = [(t[b, :n[b]].copy(), k[b, :n[b]].copy(), c[b, :n[b]].copy()) for b in range(st.shape[0])]
    return st, ev, eng.fetch_residual().copy()


def _assert_same(a, b):
    assert np.array_equal(a[0], b[0])
    for u, v in zip(a[1], b[1]):
        assert all(np.array_equal(p, q) for p, q in zip(u, v))
    assert np.array_equal(a[2], b[2])


def _resume_until_stopped(eng):
    from hsc_amd import _native
    for _ in range(10000):
        if not (eng.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_RUNNING).any():
            return
        eng.continue_rounds(2)
    raise AssertionError('the resumed launches did not finish')


def _dense(dtype, K=32, W=32, T=2048, B=3, seed=5):
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed, dtype=dtype)
    x = np.stack([synth.make_signal(D, T, i, kind='planted', nb_atoms=40, seed=seed, dtype=dtype) for i in range(B)])
    return x[:, :, np.newaxis], D


def _sparse_level(T=600, F=24, K=12, W=8, B=3, seed=7):
    """A level >= 1 shaped float64 problem: F singletons plus K atoms of three non-zeros, a sparse [B, T, F] input."""
    rs = np.random.RandomState(seed)
    D = np.zeros((K, W, F))
    for k in range(K):
        for _ in range(3):
            D[k, rs.randint(0, W), rs.randint(0, F)] = rs.uniform(0.5, 1.5) * rs.choice([-1.0, 1.0])
    S = np.zeros((F, W, F))
    S[np.arange(F), (W - 1) // 2, np.arange(F)] = 1.0
    D = np.concatenate((S, D), axis=0)
    D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
    x = np.zeros((B, T, F))
    for b in range(B):
        for _ in range(int(0.03 * T)):
            k, t = rs.randint(0, D.shape[0]), rs.randint(0, T - W)
            x[b, t:t + W] += rs.uniform(0.5, 2.0) * rs.choice([-1.0, 1.0]) * D[k]
    return x, D


def _params(dtype, **kw):
    from hsc_amd import _native
    kw.setdefault('maxEvents', 512)
    return _native.make_params(eps=float(np.finfo(dtype).eps), **kw)


def _level1_dictionary(F=16, K=20, W=8):
    rs = np.random.RandomState(2)
    D1 = np.zeros((K, W, F))
    for k in range(K):
        for _ in range(3):
            D1[k, rs.randint(0, W), rs.randint(0, F)] = rs.uniform(0.5, 1.5)
    return D1 / np.sqrt(np.sum(np.square(D1), axis=(1, 2), keepdims=True))


def _two_levels(count=3, level1_events=512):
    """Level 0 (float32, 16 atoms) encoded, level 1 (sparse float64) chained from its first `count` signals."""
    from hsc_amd import _native
    x, D0 = _dense(F32, K=16, W=16, T=1500, B=3)
    e0, e1 = _native.Engine(0), _native.Engine(0)
    e0.set_dictionary(D0)
    e0.encode_batch(x, _params(F32, nbNonzeroCoefs=80))
    e1.set_dictionary(_level1_dictionary())
    e1.encode_batch_from_level(e0, 0, count, 1e-16, _params(F64, nbNonzeroCoefs=30, maxEvents=level1_events))
    return e0, e1


@pytest.mark.parametrize('case', ['f32_weights', 'f64_sparse_lists'])
def test_set_dictionary(case, monkeypatch):
    from hsc_amd import _native
    if case == 'f32_weights':
        x, D = _dense(F32)
        _, D2 = _dense(F32, seed=6)
        w2 = np.linspace(0.5, 1.5, D2.shape[0]).astype(F32)
        p = _params(F32, nbNonzeroCoefs=60)
    else:
        x, D = _sparse_level()
        _, D2 = _sparse_level(seed=8)
        w2 = None
        p = _params(F64, nbNonzeroCoefs=40)
    eng, fresh = _native.Engine(0), _native.Engine(0)
    try:
        eng.set_dictionary(D)
        eng.encode_batch(x, p)

        def after_failure():
            assert _code(eng.device_view) == ERR_STATE
            assert _raw_encode(eng, x, p) == ERR_STATE
            assert b'no dictionary set' in eng._lib.hscmp_last_error(eng._h)

        _sweep(monkeypatch, lambda: eng.set_dictionary(D2, w2), after_failure)
        eng.set_dictionary(D, None)
        eng.set_dictionary(D2, w2)
        eng.encode_batch(x, p)
        fresh.set_dictionary(D2, w2)
        fresh.encode_batch(x, p)
        assert eng.last_variant() == fresh.last_variant()
        _assert_same(_snapshot(eng), _snapshot(fresh))
    finally:
        eng.close(); fresh.close()


@pytest.mark.parametrize('ragged', [False, True])
def test_encode_batch(ragged, monkeypatch):
    from hsc_amd import _native
    small, D = _dense(F32, T=1024, B=2)
    x, _ = _dense(F32, T=3000, B=4)
    lengths = np.array([3000, 1700, 2048, 999], dtype=np.int32)
    p = _params(F32, nbNonzeroCoefs=60, maxEvents=1024)
    eng, fresh = _native.Engine(0), _native.Engine(0)
    try:
        encode = (lambda e: e.encode_batch_ragged(x, lengths, p)) if ragged else (lambda e: e.encode_batch(x, p))
        eng.set_dictionary(D)
        eng.encode_batch(small, _params(F32, nbNonzeroCoefs=60))
        _sweep(monkeypatch, lambda: encode(eng), lambda: _no_batch(eng))
        fresh.set_dictionary(D)
        encode(fresh)
        assert eng.last_variant() == fresh.last_variant()
        _assert_same(_snapshot(eng), _snapshot(fresh))
        # steady state: the same shape again allocates nothing, so the first allocation is never asked for
        monkeypatch.setenv(KNOB, '1')
        encode(eng)
        monkeypatch.delenv(KNOB)
        _assert_same(_snapshot(eng), _snapshot(fresh))
    finally:
        eng.close(); fresh.close()


def test_encode_batch_from_level(monkeypatch):
    from hsc_amd import _native
    e0, e1 = _two_levels(count=1, level1_events=256)
    f0, f1 = _two_levels()
    try:
        before = _snapshot(e0)
        p = _params(F64, nbNonzeroCoefs=30)

        def after_failure():
            _no_batch(e1)
            _assert_same(_snapshot(e0), before)

        _sweep(monkeypatch, lambda: e1.encode_batch_from_level(e0, 0, 3, 1e-16, p), after_failure)
        assert e1.last_variant() == f1.last_variant()
        _assert_same(_snapshot(e1), _snapshot(f1))
        monkeypatch.setenv(KNOB, '1')           # steady state: a repeated chained level allocates nothing
        e1.encode_batch_from_level(e0, 0, 3, 1e-16, p)
        monkeypatch.delenv(KNOB)
        _assert_same(_snapshot(e1), _snapshot(f1))
        _assert_same(_snapshot(e0), before)
    finally:
        for e in (e0, e1, f0, f1):
            e.close()


def test_grow_events(monkeypatch):
    from hsc_amd import _native
    x, D = _dense(F32)
    p = _params(F32, nbNonzeroCoefs=60, maxEvents=16)         # every signal stops on capacity
    eng, ref = _native.Engine(0), _native.Engine(0)
    try:
        for e in (eng, ref):
            e.set_dictionary(D)
            e.encode_batch(x, p)
        assert (ref.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_CAPACITY).all()
        ref.grow_events(256)
        _resume_until_stopped(ref)
        before = _snapshot(eng)

        def after_failure():
            assert _code(eng.device_view) == 0          # the old batch is still there
            _assert_same(_snapshot(eng), before)

        _sweep(monkeypatch, lambda: eng.grow_events(256), after_failure)
        _resume_until_stopped(eng)
        _assert_same(_snapshot(eng), _snapshot(ref))
    finally:
        eng.close(); ref.close()


def test_table_open(monkeypatch):
    from hsc_amd import _native
    x, D = _dense(F32, T=512, B=1)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D)

        def after_failure():
            assert _code(eng.table_read) == ERR_STATE
            assert b'no table open' in eng._lib.hscmp_last_error(eng._h)

        eng._table_T = 512
        _sweep(monkeypatch, lambda: eng.table_open(x[0]), after_failure)
        table, _ = eng.table_read()
        assert np.array_equal(table, eng.convolve1d(x[0], True))
    finally:
        eng.close()


def _epilogue(e0, e1):
    from hsc_amd import _native
    rep = np.random.RandomState(3).standard_normal((e1.K, 23, 1))
    counts = e1.fetch_stats()[:, _native.STAT_SLOTS]
    out = e1.hierarchy_epilogue(e0, 0, [(0, 0, None), (0, e1.K, rep)], 1e-16, counts)
    total = int(out[2][-1])
    return [out[0], out[1], out[2], out[3][:total], out[4][:total], out[5][:total], out[6]]


def test_hierarchy_epilogue(monkeypatch):
    e0, e1 = _two_levels()
    f0, f1 = _two_levels()
    try:
        ref = _epilogue(f0, f1)
        before0, before1 = _snapshot(e0), _snapshot(e1)
        got = []

        def after_failure():
            assert _code(e0.device_view) == 0 and _code(e1.device_view) == 0
            _assert_same(_snapshot(e0), before0)
            _assert_same(_snapshot(e1), before1)

        _sweep(monkeypatch, lambda: got.append(_epilogue(e0, e1)), after_failure)
        got.append(_epilogue(e0, e1))
        monkeypatch.setenv(KNOB, '1')           # steady state: a repeated epilogue allocates nothing
        got.append(_epilogue(e0, e1))
        monkeypatch.delenv(KNOB)
        assert len(got) == 3
        for out in got:
            assert all(np.array_equal(a, b) for a, b in zip(out, ref))
    finally:
        for e in (e0, e1, f0, f1):
            e.close()
