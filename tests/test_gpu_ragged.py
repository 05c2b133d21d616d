"""Ragged batches (hscmp_encode_batch_ragged): signals of different lengths in one call.

Every dense level-0 row of tests/test_gpu_dispatch.py runs as a ragged batch.  Each signal must give, bit for bit, what the
same engine gives it alone and what the CPU oracle gives it: events, stats, CSC of shape (T_b, K), residual and energies.
The lengths include 3W-2 (the shortest the matrix-core path takes), lengths off the multiples of 64 and of the block size,
and the longest length T; the generic rows also W and 3W-3."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _signals(dtype, lengths, K=32, W=32, seed=5, weights=False):
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed, dtype=dtype)
    xs = []
    for i, n in enumerate(lengths):
        nb = max(1, min(40, n // 48))
        xs.append(synth.make_signal(D, int(n), i, kind='planted', nb_atoms=nb, seed=seed, dtype=dtype))
    w = None
    if weights:
        w = np.ones(K, dtype=dtype)
        w[::3] = dtype(0.5)              # (the singleton weights of a level dictionary: some atoms count less)
    return xs, D, w


def _padded(xs, fill=0.0):
    T = max(len(x) for x in xs)
    x = np.full((len(xs), T, 1), fill, dtype=xs[0].dtype)
    for b, s in enumerate(xs):
        x[b, :len(s), 0] = s
    return x, np.array([len(s) for s in xs], dtype=np.int32)


W32 = 32
MF_LENGTHS = [3 * W32 - 2, 1000, 2048, 1537, 700, 2001]          # 3W-2, off 64 / off the block size, T = 2048
GEN_LENGTHS = [W32, 3 * W32 - 3, 80, 1000, 300, 3 * W32 - 2]     # + W and 3W-3

# name: (dtype, lengths, env, params, expected variant without the _ragged suffix, weights)
ROWS = {
    'f32_default': (F32, MF_LENGTHS, {}, dict(nbNonzeroCoefs=60), 'mfma_init+mfma_loop_f32_bound', False),
    'f32_exact_init': (F32, MF_LENGTHS, {'HSCMP_EXACT_INIT': '1'}, dict(nbNonzeroCoefs=60), 'mfma_init+mfma_loop_f32', False),
    'f32_quad_forced': (F32, MF_LENGTHS, {'HSCMP_MFMA_QUAD': '1', 'HSCMP_EXACT_INIT': '1'}, dict(nbNonzeroCoefs=60),
                        'mfma_init+mfma_loop_f32_x4', False),
    'f32_blocked_rp': (F32, MF_LENGTHS, {'HSCMP_RP': '1'}, dict(toleranceSnr=20.0, nbBlocks=6), 'mfma_init+mfma_loop_f32_rp', False),
    'f32_blocked_rp_auto': (F32, MF_LENGTHS, {'HSCMP_RP': '1'}, dict(toleranceSnr=20.0, nbBlocks='auto'), 'mfma_init+mfma_loop_f32_rp', False),
    'f32_blocked_no_rp': (F32, MF_LENGTHS, {'HSCMP_RP': '0'}, dict(toleranceSnr=20.0, nbBlocks=6), 'mfma_init+mfma_loop_f32', False),
    'f32_blocked_no_rp_auto': (F32, MF_LENGTHS, {'HSCMP_RP': '0'}, dict(toleranceSnr=20.0, nbBlocks='auto'), 'mfma_init+mfma_loop_f32', False),
    'f32_force_generic': (F32, GEN_LENGTHS, {'HSCMP_FORCE_GENERIC': '1'}, dict(nbNonzeroCoefs=60), 'generic_init+generic_loop_f32', False),
    'f32_force_generic_blocked': (F32, GEN_LENGTHS, {'HSCMP_FORCE_GENERIC': '1'}, dict(toleranceSnr=20.0, nbBlocks=3),
                                  'generic_init+generic_loop_f32', False),
    'f32_short_signal': (F32, GEN_LENGTHS, {}, dict(nbNonzeroCoefs=10), 'generic_init+generic_loop_f32', False),
    'f64_default': (F64, MF_LENGTHS, {}, dict(nbNonzeroCoefs=60), 'mfma_init+mfma_loop_f64', False),
    'f64_generic': (F64, GEN_LENGTHS, {}, dict(nbNonzeroCoefs=30), 'generic_init+generic_loop_f64', False),
    # (weighted rows: the variant the uniform entry picks for the padded batch -- whether the bound pass takes a weighted
    #  dictionary depends on its error model; every signal here is at least 3W-2 long, so the plan is the same)
    'f32_weights': (F32, MF_LENGTHS, {'HSCMP_EXACT_INIT': '1'}, dict(nbNonzeroCoefs=60), None, True),
    'f32_weights_default': (F32, MF_LENGTHS, {}, dict(nbNonzeroCoefs=60), None, True),
    'f64_weights': (F64, MF_LENGTHS, {}, dict(nbNonzeroCoefs=60), None, True),
}


def _signal_results(eng, b, Tb):
    from hsc_amd import _native
    st = eng.fetch_stats()[b].copy()
    t, k, c = eng.fetch_events()
    n = int(st[_native.STAT_EVENTS])
    sl_t, sl_k, sl_a = eng.fetch_slots()
    ns = int(st[_native.STAT_SLOTS])
    return dict(stats=st, t=t[b, :n].copy(), k=k[b, :n].copy(), c=c[b, :n].copy(), slots=(sl_t[b, :ns].copy(), sl_k[b, :ns].copy(), sl_a[b, :ns].copy()),
                residual=eng.fetch_residual()[b, :Tb].copy(), energies=eng.fetch_energies()[b].copy())


def _all_results(eng, lengths):
    from hsc_amd import _native
    st = eng.fetch_stats().copy()
    t, k, c = eng.fetch_events()
    sl_t, sl_k, sl_a = eng.fetch_slots()
    r = eng.fetch_residual()
    e = eng.fetch_energies()
    out = []
    for b, Tb in enumerate(lengths):
        n, ns = int(st[b, _native.STAT_EVENTS]), int(st[b, _native.STAT_SLOTS])
        out.append(dict(stats=st[b].copy(), t=t[b, :n].copy(), k=k[b, :n].copy(), c=c[b, :n].copy(),
                        slots=(sl_t[b, :ns].copy(), sl_k[b, :ns].copy(), sl_a[b, :ns].copy()),
                        residual=r[b, :int(Tb)].copy(), energies=e[b].copy()))
    return out, r


def _same(a, b):
    assert np.array_equal(a['stats'], b['stats']), (a['stats'], b['stats'])
    for key in ('t', 'k', 'c', 'residual', 'energies'):
        assert np.array_equal(a[key], b[key]), key
    for u, v in zip(a['slots'], b['slots']):
        assert np.array_equal(u, v)


def _csc(res, Tb, K):
    from hsc_amd.modeling import _slots_to_csc
    return _slots_to_csc(*res['slots'], len(res['slots'][0]), (Tb, K), 1e-16)


def _check_against_oracle(res, x_b, D, w, kw, K):
    from oracle import hsc_oracle as orc
    from hsc_amd import _native
    okw = dict(kw)
    coef, r_ref, info = orc.cmp_encode(x_b, D, weights=w, **okw)
    assert np.array_equal(res['t'], info['t']) and np.array_equal(res['k'], info['k']), 'positions / atoms differ from the oracle'
    assert np.array_equal(res['c'], info['c']), 'coefficients differ from the oracle'
    assert np.array_equal(res['residual'][:, 0], r_ref), 'residual differs from the oracle'
    st = res['stats']
    assert st[_native.STAT_NNZ] == info['nnz'] and st[_native.STAT_DUPLICATES] == info['duplicates']
    assert st[_native.STAT_ROUNDS] == info['rounds'] and st[_native.STAT_ITERATIONS] == info['iterations']
    assert _native.STOP_NAMES.get(int(st[_native.STAT_STOP])) == info['stop']
    mine = _csc(res, len(x_b), K)
    assert mine.shape == coef.shape == (len(x_b), K)
    assert (mine != coef).nnz == 0


@pytest.mark.parametrize('name', sorted(ROWS))
def test_ragged_row(name, monkeypatch):
    from hsc_amd import _native
    dtype, lengths, env, kw, expected, weighted = ROWS[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    xs, D, w = _signals(dtype, lengths, weights=weighted)
    x, lens = _padded(xs)
    eps = float(np.finfo(dtype).eps)
    K = D.shape[0]
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        if expected is None:
            eng.encode_batch(x, _native.make_params(eps=eps, maxEvents=2048, **kw))
            expected = eng.last_variant()
            assert expected.startswith('mfma_init')
        eng.encode_batch_ragged(x, lens, _native.make_params(eps=eps, maxEvents=2048, **kw))
        assert eng.last_variant() == expected + '_ragged'
        got, raw = _all_results(eng, lens)
        for b, Tb in enumerate(lens):
            assert not raw[b, Tb:].any(), 'the residual above the signal length is not zero'
        for b, s in enumerate(xs):
            eng.encode_batch(s.reshape((1, -1, 1)), _native.make_params(eps=eps, maxEvents=2048, **kw))
            _same(got[b], _signal_results(eng, 0, len(s)))
            _check_against_oracle(got[b], s, D, w, kw, K)
    finally:
        eng.close()


def test_ragged_four_signals(monkeypatch):
    """600 signals: the natural four-signal loop (x4) with the bound re-correlation, lengths from 3W-2 to T."""
    from hsc_amd import _native
    rs = np.random.RandomState(11)
    lengths = list(rs.randint(3 * W32 - 2, 257, size=600))
    lengths[0], lengths[1], lengths[2] = 3 * W32 - 2, 256, 129
    xs, D, _ = _signals(F32, lengths)
    x, lens = _padded(xs)
    eps = float(np.finfo(F32).eps)
    kw = dict(nbNonzeroCoefs=12)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D)
        eng.encode_batch_ragged(x, lens, _native.make_params(eps=eps, maxEvents=512, **kw))
        assert eng.last_variant() == 'mfma_init+mfma_loop_f32_bound_x4_ragged'
        got, _ = _all_results(eng, lens)
        for b in list(range(0, 600, 37)) + [1, 2, 599]:
            eng.encode_batch(xs[b].reshape((1, -1, 1)), _native.make_params(eps=eps, maxEvents=512, **kw))
            _same(got[b], _signal_results(eng, 0, len(xs[b])))
        for b, s in enumerate(xs):
            _check_against_oracle(got[b], s, D, None, kw, D.shape[0])
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['f32_default', 'f32_blocked_rp', 'f32_force_generic', 'f64_default'])
def test_nan_padding_and_device_entry(name, monkeypatch):
    """Rows above a signal's length are never read: NaN there changes nothing.  The device-pointer entry equals the host one."""
    import torch
    from hsc_amd import _native
    dtype, lengths, env, kw, expected, weighted = ROWS[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    xs, D, w = _signals(dtype, lengths, weights=weighted)
    x0, lens = _padded(xs)
    xn, _ = _padded(xs, fill=np.nan)
    eps = float(np.finfo(dtype).eps)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        params = _native.make_params(eps=eps, maxEvents=2048, **kw)
        eng.encode_batch_ragged(x0, lens, params)
        ref, raw0 = _all_results(eng, lens)
        eng.encode_batch_ragged(xn, lens, params)
        got, raw = _all_results(eng, lens)
        assert np.array_equal(raw, raw0)
        for b, Tb in enumerate(lens):
            assert not raw[b, Tb:].any()
            _same(got[b], ref[b])
        xd = torch.from_numpy(xn).to('cuda:0')
        torch.cuda.synchronize()
        eng.encode_batch_ragged_device(xd.data_ptr(), xd.shape[0], xd.shape[1], lens, params)
        eng.synchronize()
        assert eng.last_variant() == expected + '_ragged'
        dev, _ = _all_results(eng, lens)
        for b in range(len(lens)):
            _same(dev[b], ref[b])
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['f32_default', 'f32_quad_forced', 'f32_blocked_rp', 'f32_blocked_no_rp', 'f32_force_generic', 'f64_default'])
def test_equal_lengths_match_uniform(name, monkeypatch):
    """Equal lengths through the ragged entry: the uniform entry's results bit for bit."""
    from hsc_amd import _native
    dtype, _, env, kw, expected, weighted = ROWS[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    xs, D, w = _signals(dtype, [2048] * 3, weights=weighted)
    x, lens = _padded(xs)
    eps = float(np.finfo(dtype).eps)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        params = _native.make_params(eps=eps, maxEvents=2048, **kw)
        eng.encode_batch(x, params)
        uni_variant = eng.last_variant()
        uni, _ = _all_results(eng, lens)
        eng.encode_batch_ragged(x, lens, params)
        assert eng.last_variant() == uni_variant + '_ragged'
        rag, _ = _all_results(eng, lens)
        for a, b in zip(rag, uni):
            _same(a, b)
        eng.encode_batch(x, params)                      # a plain encode clears the lengths
        assert eng.last_variant() == uni_variant
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['f32_default', 'f32_blocked_rp', 'f32_blocked_no_rp', 'f32_force_generic', 'f64_default'])
def test_resume_matches_one_launch(name, monkeypatch):
    """max_rounds = 2 and hscmp_continue until every signal stopped: one launch's results."""
    from hsc_amd import _native
    dtype, lengths, env, kw, expected, weighted = ROWS[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    xs, D, w = _signals(dtype, lengths, weights=weighted)
    x, lens = _padded(xs)
    eps = float(np.finfo(dtype).eps)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        eng.encode_batch_ragged(x, lens, _native.make_params(eps=eps, maxEvents=2048, **kw))
        one, raw1 = _all_results(eng, lens)
        eng.encode_batch_ragged(x, lens, _native.make_params(eps=eps, maxEvents=2048, maxRounds=2, **kw))
        for _ in range(10000):
            if not (eng.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_RUNNING).any():
                break
            eng.continue_rounds(2)
        assert eng.last_variant() == expected + '_ragged'
        two, raw2 = _all_results(eng, lens)
        assert np.array_equal(raw1, raw2)
        for a, b in zip(two, one):
            _same(a, b)
    finally:
        eng.close()


def _reference_signal(cmp_single, s, D, **kw):
    coef, residual = cmp_single.computeCoefficients(s, D, **kw)
    return coef, residual, cmp_single.lastResult


def test_modeling_list_capacity_regrowth_and_callback():
    """computeCoefficientsBatch on a list of signals: a small maxEvents that forces the STOP_CAPACITY regrowth, and a stopCondition
    that stops some signals early -- per signal what computeCoefficients gives it alone."""
    from hsc_amd.modeling import ConvolutionalMatchingPursuit, ConvolutionalSparseCoder
    xs, D, _ = _signals(F32, MF_LENGTHS)
    cmp = ConvolutionalMatchingPursuit()
    res = cmp.computeCoefficientsBatch(xs, D, nbNonzeroCoefs=60, maxEvents=8)
    assert res.variant.endswith('_ragged')
    assert list(res.lengths) == [len(s) for s in xs]
    single = ConvolutionalMatchingPursuit()
    for b, s in enumerate(xs):
        coef, residual, one = _reference_signal(single, s, D, nbNonzeroCoefs=60)
        assert res.coefficients[b].shape == (len(s), D.shape[0])
        assert (res.coefficients[b] != coef).nnz == 0
        assert res.residuals[b].shape == residual.shape and np.array_equal(res.residuals[b], residual)
        assert all(np.array_equal(u, v) for u, v in zip(res.events[b], one.events[0]))
        assert np.array_equal(res.stats[b], one.stats[0]) and np.array_equal(res.energies[b], one.energies[0])

    seen = {}

    def stop(seq, residual, coefficients):
        # stops the signals whose length is odd once they hold 20 coefficients
        seen.setdefault(seq.shape[0], set()).add((residual.shape, coefficients.shape))
        return seq.shape[0] % 2 == 1 and coefficients.nnz >= 20

    res = ConvolutionalSparseCoder(D, cmp).encodeBatch(xs, nbNonzeroCoefs=60, stopCondition=stop)
    for b, s in enumerate(xs):
        assert seen[len(s)] == {((len(s), 1), (len(s), D.shape[0]))}
        coef, residual, one = _reference_signal(single, s, D, nbNonzeroCoefs=60, stopCondition=stop)
        assert (res.coefficients[b] != coef).nnz == 0
        assert np.array_equal(res.residuals[b], residual)
        assert all(np.array_equal(u, v) for u, v in zip(res.events[b], one.events[0]))
        assert np.array_equal(res.stats[b], one.stats[0])
    stops = res.stop_reasons()
    assert 'callback' in stops and any(r != 'callback' for r in stops)

    # the padded form with lengths= gives the same
    x, lens = _padded(xs, fill=np.nan)
    res2 = cmp.computeCoefficientsBatch(x[:, :, 0], D, nbNonzeroCoefs=60, lengths=lens)
    res1 = cmp.computeCoefficientsBatch(xs, D, nbNonzeroCoefs=60)
    for b in range(len(xs)):
        assert np.array_equal(res2.residuals[b], res1.residuals[b])
        assert all(np.array_equal(u, v) for u, v in zip(res2.events[b], res1.events[b]))


def test_ragged_rejections_on_the_device():
    """Ragged input the engine has no kernels for fails with HSCMP_ERR_UNSUPPORTED / INVALID, naming the reason."""
    from hsc_amd import _native
    xs, D, _ = _signals(F32, [200, 300])
    x, lens = _padded(xs)
    eps = float(np.finfo(F32).eps)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D)
        params = _native.make_params(eps=eps, maxEvents=256, nbNonzeroCoefs=10)
        eng.set_method(_native.METHOD_LOCOMP)
        with pytest.raises(_native.HscmpError) as e:
            eng.encode_batch_ragged(x, lens, params)
        assert e.value.code == -5
        eng.set_method(_native.METHOD_CMP)
        with pytest.raises(_native.HscmpError) as e:
            eng.encode_batch_ragged(x, np.array([200, 301], dtype=np.int32), params)
        assert e.value.code == -1 and 'signal 1' in str(e.value)
        with pytest.raises(_native.HscmpError) as e:
            eng.encode_batch_ragged(x, np.array([31, 300], dtype=np.int32), params)
        assert e.value.code == -1 and 'signal 0' in str(e.value)
    finally:
        eng.close()
