"""Kernel choice of the batch encode (csrc/hscmp_api.hip: plan_encode), one small encode per path.

Each row pins the exact variant string the encode reports, and checks that a launch limited to two rounds, resumed by
hscmp_continue until every signal has stopped, leaves the same events, stats and residual as one launch, bit for bit:
the resumed launches must run the loop the encode chose."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dense_f1(dtype, K=32, W=32, T=2048, B=3, seed=5):
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed, dtype=dtype)
    x = np.stack([synth.make_signal(D, T, i, kind='planted', nb_atoms=40, seed=seed, dtype=dtype) for i in range(B)])
    return x[:, :, np.newaxis], D


def _level(dtype=np.float64, sparse=True, T=600, F=24, K=12, W=8, B=3, seed=7):
    """A level >= 1 shaped problem: sparse [B, T, F] input; a dictionary of F singletons plus K atoms of three non-zeros
    (sparse), or of dense random atoms (dense)."""
    rs = np.random.RandomState(seed)
    if sparse:
        D = np.zeros((K, W, F))
        for k in range(K):
            for _ in range(3):
                D[k, rs.randint(0, W), rs.randint(0, F)] = rs.uniform(0.5, 1.5) * rs.choice([-1.0, 1.0])
        S = np.zeros((F, W, F))
        S[np.arange(F), (W - 1) // 2, np.arange(F)] = 1.0
        D = np.concatenate((S, D), axis=0)
    else:
        D = rs.standard_normal((K, W, F))
    D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
    x = np.zeros((B, T, F))
    for b in range(B):
        for _ in range(int(0.03 * T)):
            k, t = rs.randint(0, D.shape[0]), rs.randint(0, T - W)
            x[b, t:t + W] += rs.uniform(0.5, 2.0) * rs.choice([-1.0, 1.0]) * D[k]
    return x.astype(dtype), D.astype(dtype)


F32, F64 = np.float32, np.float64

# name: (problem, method, env, params, expected variant)
ROWS = {
    'f32_default': (lambda: _dense_f1(F32), 0, {}, dict(nbNonzeroCoefs=60), 'mfma_init+mfma_loop_f32_bound'),
    'f32_exact_init': (lambda: _dense_f1(F32), 0, {'HSCMP_EXACT_INIT': '1'}, dict(nbNonzeroCoefs=60), 'mfma_init+mfma_loop_f32'),
    'f32_four_signals': (lambda: _dense_f1(F32, T=256, B=600), 0, {}, dict(nbNonzeroCoefs=12), 'mfma_init+mfma_loop_f32_bound_x4'),
    'f32_quad_forced': (lambda: _dense_f1(F32), 0, {'HSCMP_MFMA_QUAD': '1', 'HSCMP_EXACT_INIT': '1'}, dict(nbNonzeroCoefs=60),
                        'mfma_init+mfma_loop_f32_x4'),
    'f32_blocked_rp': (lambda: _dense_f1(F32), 0, {'HSCMP_RP': '1'}, dict(toleranceSnr=20.0, nbBlocks=6), 'mfma_init+mfma_loop_f32_rp'),
    'f32_blocked_no_rp': (lambda: _dense_f1(F32), 0, {'HSCMP_RP': '0'}, dict(toleranceSnr=20.0, nbBlocks=6), 'mfma_init+mfma_loop_f32'),
    'f32_force_generic': (lambda: _dense_f1(F32), 0, {'HSCMP_FORCE_GENERIC': '1'}, dict(nbNonzeroCoefs=60), 'generic_init+generic_loop_f32'),
    'f32_short_signal': (lambda: _dense_f1(F32, T=80), 0, {}, dict(nbNonzeroCoefs=10), 'generic_init+generic_loop_f32'),
    'f64_default': (lambda: _dense_f1(F64), 0, {}, dict(nbNonzeroCoefs=60), 'mfma_init+mfma_loop_f64'),
    'level_sparse': (lambda: _level(), 0, {}, dict(nbNonzeroCoefs=40), 'dictlist_init+dictlist_loop_f64'),
    'level_sparse_rp': (lambda: _level(), 0, {'HSCMP_RP': '1'}, dict(toleranceSnr=25.0, nbBlocks=4), 'dictlist_init+dictlist_loop_f64_rp'),
    'level_sparse_unpacked': (lambda: _level(), 0, {'HSCMP_SPARSE_PACKED': '0'}, dict(nbNonzeroCoefs=40), 'dictlist_init+dictlist_loop_f64'),
    'level_sparse_packed': (lambda: _level(), 0, {'HSCMP_SPARSE_PACKED': '1'}, dict(nbNonzeroCoefs=40), 'dictlist_init+dictlist_loop_f64'),
    'level_sparse_f32': (lambda: _level(F32), 0, {}, dict(nbNonzeroCoefs=40), 'dictlist_init+dictlist_loop_f32'),
    'level_dense': (lambda: _level(sparse=False), 0, {}, dict(nbNonzeroCoefs=30), 'sparse_init+generic_loop_f64'),
    'level_dense_gathered': (lambda: _level(sparse=False), 0, {'HSCMP_FORCE_GATHERED': '1'}, dict(nbNonzeroCoefs=30),
                             'sparse_init+gathered_loop_f64'),
    'locomp_f32': (lambda: _dense_f1(F32), 1, {}, dict(toleranceSnr=15.0, nbBlocks=3), 'own_init+locomp_mfma_loop_f32'),
    'locomp_f32_pack1': (lambda: _dense_f1(F32), 1, {'HSCMP_LOCOMP_PACK': '1'}, dict(toleranceSnr=15.0, nbBlocks=3), 'own_init+locomp_mfma_loop_f32'),
    'locomp_f32_pack2': (lambda: _dense_f1(F32), 1, {'HSCMP_LOCOMP_PACK': '2'}, dict(toleranceSnr=15.0, nbBlocks=3), 'own_init+locomp_mfma_loop_f32'),
    'locomp_f32_pack4': (lambda: _dense_f1(F32), 1, {'HSCMP_LOCOMP_PACK': '4'}, dict(toleranceSnr=15.0, nbBlocks=3), 'own_init+locomp_mfma_loop_f32'),
    'locomp_f32_no_mfma': (lambda: _dense_f1(F32), 1, {'HSCMP_LOCOMP_NO_MFMA': '1'}, dict(toleranceSnr=15.0, nbBlocks=3),
                           'generic_init+locomp_loop_f32'),
    'locomp_f64': (lambda: _dense_f1(F64), 1, {}, dict(toleranceSnr=15.0, nbBlocks=3), 'generic_init+locomp_loop_f64'),
    'locomp_level_sparse': (lambda: _level(), 1, {}, dict(toleranceSnr=25.0, nbBlocks=4), 'dictlist_init+locomp_dictlist_loop_f64'),
    # One encode on each side of each dictionary-image limit of mfma_supported (64 KiB float32, 128 KiB float64): the last shape
    # whose image fits, and one atom more (a ninth / seventeenth group).  The variants are those the commit before the shared
    # launch helper reported for these rows.
    'f32_image_at_limit_w64': (lambda: _dense_f1(F32, K=256, W=64, T=512), 0, {}, dict(nbNonzeroCoefs=10), 'mfma_init+mfma_loop_f32_bound'),
    'f32_image_past_limit_w64': (lambda: _dense_f1(F32, K=257, W=64, T=512), 0, {}, dict(nbNonzeroCoefs=10), 'generic_init+generic_loop_f32'),
    'f32_image_at_limit_w32': (lambda: _dense_f1(F32, K=512, W=32, T=512), 0, {}, dict(nbNonzeroCoefs=10), 'mfma_init+mfma_loop_f32_bound'),
    'f32_image_past_limit_w32': (lambda: _dense_f1(F32, K=513, W=32, T=512), 0, {}, dict(nbNonzeroCoefs=10), 'generic_init+generic_loop_f32'),
    'f64_image_at_limit_w64': (lambda: _dense_f1(F64, K=256, W=64, T=512), 0, {}, dict(nbNonzeroCoefs=10), 'mfma_init+mfma_loop_f64'),
    'f64_image_past_limit_w64': (lambda: _dense_f1(F64, K=257, W=64, T=512), 0, {}, dict(nbNonzeroCoefs=10), 'generic_init+generic_loop_f64'),
}


def _snapshot(eng):
    st = eng.fetch_stats().copy()
    t, k, c = eng.fetch_events()
    from hsc_amd import _native
    n = st[:, _native.STAT_EVENTS]
    ev = [(t[b, :n[b]].copy(), k[b, :n[b]].copy(), c[b, :n[b]].copy()) for b in range(st.shape[0])]
    return st, ev, eng.fetch_residual().copy()


def _resume_until_stopped(eng):
    from hsc_amd import _native
    for _ in range(10000):
        if not (eng.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_RUNNING).any():
            return
        eng.continue_rounds(2)
    raise AssertionError('the resumed launches did not finish')


def _assert_same(a, b):
    assert np.array_equal(a[0], b[0])
    for u, v in zip(a[1], b[1]):
        assert all(np.array_equal(p, q) for p, q in zip(u, v))
    assert np.array_equal(a[2], b[2])


@pytest.mark.parametrize('name', sorted(ROWS))
def test_encode_path(name, monkeypatch):
    from hsc_amd import _native
    problem, method, env, kw, expected = ROWS[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    x, D = problem()
    eps = float(np.finfo(x.dtype).eps)
    eng = _native.Engine(0)
    try:
        eng.set_method(method)
        eng.set_dictionary(D)
        eng.encode_batch(x, _native.make_params(eps=eps, maxEvents=2048, **kw))
        assert eng.last_variant() == expected
        one = _snapshot(eng)
        eng.encode_batch(x, _native.make_params(eps=eps, maxEvents=2048, maxRounds=2, **kw))
        assert eng.last_variant() == expected
        _resume_until_stopped(eng)
        _assert_same(_snapshot(eng), one)
    finally:
        eng.close()


def test_level_chained_encode(monkeypatch):
    """encode_batch_from_level: the scatter and the loop make one decision about the per-row feature lists."""
    from hsc_amd import _native
    x, D0 = _dense_f1(F32, K=16, W=16, T=1500, B=3)
    e0 = _native.Engine(0)
    e1 = _native.Engine(0)
    try:
        e0.set_dictionary(D0)
        e0.encode_batch(x, _native.make_params(nbNonzeroCoefs=80, eps=float(np.finfo(F32).eps), maxEvents=512))
        rs = np.random.RandomState(2)
        D1 = np.zeros((20, 8, 16))
        for k in range(20):
            for _ in range(3):
                D1[k, rs.randint(0, 8), rs.randint(0, 16)] = rs.uniform(0.5, 1.5)
        D1 /= np.sqrt(np.sum(np.square(D1), axis=(1, 2), keepdims=True))
        e1.set_dictionary(D1)
        eps = float(np.finfo(F64).eps)
        e1.encode_batch_from_level(e0, 0, 3, 1e-16, _native.make_params(nbNonzeroCoefs=30, eps=eps, maxEvents=512))
        assert e1.last_variant() == 'dictlist_init+dictlist_loop_f64'
        one = _snapshot(e1)
        e1.encode_batch_from_level(e0, 0, 3, 1e-16, _native.make_params(nbNonzeroCoefs=30, eps=eps, maxEvents=512, maxRounds=2))
        assert e1.last_variant() == 'dictlist_init+dictlist_loop_f64'
        _resume_until_stopped(e1)
        _assert_same(_snapshot(e1), one)
    finally:
        e0.close(); e1.close()


@pytest.mark.parametrize('name', ['f32_blocked_rp', 'f32_default', 'level_sparse', 'level_sparse_packed', 'level_sparse_rp',
                                  'locomp_level_sparse'])
def test_resume_keeps_the_encode_knobs(name, monkeypatch):
    """hscmp_continue resumes with the knobs the encode read: knobs changed after the encode change neither the loop nor
    its arguments."""
    from hsc_amd import _native
    problem, method, env, kw, expected = ROWS[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    x, D = problem()
    eps = float(np.finfo(x.dtype).eps)
    eng = _native.Engine(0)
    try:
        eng.set_method(method)
        eng.set_dictionary(D)
        eng.encode_batch(x, _native.make_params(eps=eps, maxEvents=2048, **kw))
        one = _snapshot(eng)
        eng.encode_batch(x, _native.make_params(eps=eps, maxEvents=2048, maxRounds=2, **kw))
        monkeypatch.setenv('HSCMP_NO_PAIRING', '1')
        monkeypatch.setenv('HSCMP_NO_ROWBITS', '1')
        monkeypatch.setenv('HSCMP_RP', '1' if env.get('HSCMP_RP') == '0' else '0')
        _resume_until_stopped(eng)
        assert eng.last_variant() == expected
        _assert_same(_snapshot(eng), one)
    finally:
        eng.close()
