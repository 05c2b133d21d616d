"""A batch encoded with a dictionary per signal (hscmp_set_dictionaries / hscmp_encode_batch_multi).

Signal b of the batch must come out, bit for bit, as an engine holding dictionary dict_of[b] alone (set_dictionary with that
dictionary and its weights) encodes signal b alone: events, coefficient slots, stats, residual and both energies -- for CMP
whatever kernels that single encode picks (and the CPU oracle agrees), for LoCOMP against the dense LoCOMP loop (the single
encode runs with HSCMP_LOCOMP_NO_MFMA / HSCMP_NO_DICT_LISTS so that it takes that policy too).  Shapes: K = 5, W = 8 and 7, F = 1
and 3, T = 96 and T = 2W, B = 5, G = 3 with dict_of = [2, 0, 2, 1, 2] (not monotone, one dictionary three times), a dictionary
nobody uses, G = 1 and G = B."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DICT_OF = [2, 0, 2, 1, 2]
LOCOMP_SINGLE_ENV = {'HSCMP_LOCOMP_NO_MFMA': '1', 'HSCMP_NO_DICT_LISTS': '1'}


def _problem(dtype, K, W, F, T, B, G, seed, weighted):
    """G unit-norm dictionaries, B signals each planted from a dictionary of the set plus noise, weights [G,K] or None."""
    rng = np.random.RandomState(seed)
    Ds = rng.randn(G, K, W, F)
    Ds /= np.sqrt(np.sum(Ds ** 2, axis=(2, 3), keepdims=True))
    x = 0.02 * rng.randn(B, T, F)
    for b in range(B):
        g = rng.randint(G)
        for _ in range(max(2, T // 16)):
            k, t = rng.randint(K), rng.randint(0, T - W + 1)
            x[b, t:t + W] += rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0]) * Ds[g, k]
    w = None
    if weighted:
        w = rng.uniform(0.25, 1.0, size=(G, K))
    return Ds.astype(dtype), x.astype(dtype), None if w is None else w.astype(dtype)


def _results(eng, B):
    from hsc_amd import _native
    st = eng.fetch_stats().copy()
    t, k, c = eng.fetch_events()
    sl_t, sl_k, sl_a = eng.fetch_slots()
    r = eng.fetch_residual()
    e = eng.fetch_energies()
    out = []
    for b in range(B):
        n, ns = int(st[b, _native.STAT_EVENTS]), int(st[b, _native.STAT_SLOTS])
        out.append(dict(stats=st[b].copy(), t=t[b, :n].copy(), k=k[b, :n].copy(), c=c[b, :n].copy(),
                        slots=(sl_t[b, :ns].copy(), sl_k[b, :ns].copy(), sl_a[b, :ns].copy()),
                        residual=r[b].copy(), energies=e[b].copy()))
    return out


def _same(a, b, what=''):
    assert np.array_equal(a['stats'], b['stats']), (what, a['stats'], b['stats'])
    for key in ('t', 'k', 'c', 'residual', 'energies'):
        assert np.array_equal(a[key], b[key]), (what, key)
    for u, v in zip(a['slots'], b['slots']):
        assert np.array_equal(u, v), (what, 'slots')


def _params(dtype, **kw):
    from hsc_amd import _native
    kw.setdefault('maxEvents', 512)
    return _native.make_params(eps=float(np.finfo(dtype).eps), **kw)


def _encode_multi(eng, Ds, w, x, dict_of, method, params):
    from hsc_amd import _native
    eng.set_dictionaries(Ds, w)
    eng.set_method(method)
    try:
        eng.encode_batch_multi(x, dict_of, params)
    finally:
        eng.set_method(_native.METHOD_CMP)
    return _results(eng, x.shape[0])


def _encode_singles(eng, Ds, w, x, dict_of, method, params, monkeypatch):
    """Signal b alone on a plain dictionary: a batch of one."""
    from hsc_amd import _native
    out = []
    with monkeypatch.context() as m:
        if method == _native.METHOD_LOCOMP:
            for key, val in LOCOMP_SINGLE_ENV.items():
                m.setenv(key, val)
        for b, g in enumerate(dict_of):
            eng.set_dictionary(Ds[g], None if w is None else w[g])
            eng.set_method(method)
            try:
                eng.encode_batch(x[b:b + 1], params)
            finally:
                eng.set_method(_native.METHOD_CMP)
            if method == _native.METHOD_LOCOMP:
                assert 'locomp_loop' in eng.last_variant(), eng.last_variant()      # the dense LoCOMP policy
            out.append(_results(eng, 1)[0])
    return out


def _check_oracle(res, x_b, D, w, kw):
    from oracle import hsc_oracle as orc
    from hsc_amd import _native
    coef, r_ref, info = orc.cmp_encode(x_b, D, weights=w, maxEvents=512, **kw)            # x_b [T,F], D [K,W,F]
    assert np.array_equal(res['t'], info['t']) and np.array_equal(res['k'], info['k']), 'positions / atoms differ from the oracle'
    assert np.array_equal(res['c'], info['c']), 'coefficients differ from the oracle'
    assert np.array_equal(res['residual'], r_ref), 'residual differs from the oracle'
    st = res['stats']
    assert st[_native.STAT_NNZ] == info['nnz'] and st[_native.STAT_ROUNDS] == info['rounds']
    assert _native.STOP_NAMES.get(int(st[_native.STAT_STOP])) == info['stop']


@pytest.fixture(scope='module')
def engines():
    from hsc_amd import _native
    multi, single = _native.Engine(0), _native.Engine(0)
    yield multi, single
    multi.close()
    single.close()


SHAPES = {'W8_F1': (8, 1, 96), 'W7_F1': (7, 1, 96), 'W8_F3': (8, 3, 96), 'W7_F3': (7, 3, 96), 'W8_F1_short': (8, 1, 16)}


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_multi_equals_single(engines, dtype, monkeypatch):
    """Every shape x method x nbBlocks x weights of one dtype (60 small encodes of five signals; the failing combination is named
    in the assertion): one test per dtype keeps the suite's test count down, the cases are all here."""
    for shape in sorted(SHAPES):
        for method in ('cmp', 'locomp'):
            for nbBlocks in (1, 3, 'auto'):
                for weighted in (False, True):
                    _multi_equals_single(engines, shape, dtype, method, nbBlocks, weighted, monkeypatch)


def _multi_equals_single(engines, shape, dtype, method, nbBlocks, weighted, monkeypatch):
    from hsc_amd import _native
    case = '%s %s %s nbBlocks=%r %s' % (shape, np.dtype(dtype).name, method, nbBlocks, 'weights' if weighted else 'plain')
    W, F, T = SHAPES[shape]
    if nbBlocks == 3 and T == 16:
        nbBlocks = 2                                  # (T = 2W: blocks of 8 samples, the smallest even block)
    K, B, G = 5, 5, 3
    Ds, x, w = _problem(dtype, K, W, F, T, B, G, seed=11 + W + F, weighted=weighted)
    kw = dict(nbNonzeroCoefs=12, nbBlocks=nbBlocks) if nbBlocks == 1 else dict(toleranceSnr=15.0, nbBlocks=nbBlocks)
    meth = _native.METHOD_LOCOMP if method == 'locomp' else _native.METHOD_CMP
    multi, single = engines
    got = _encode_multi(multi, Ds, w, x, DICT_OF, meth, _params(dtype, **kw))
    variant = multi.last_variant()
    assert variant.endswith('_multi'), (case, variant)
    assert variant == 'generic_init+%s_loop_%s_multi' % ('locomp' if method == 'locomp' else 'generic', 'f32' if dtype == F32 else 'f64'), case
    want = _encode_singles(single, Ds, w, x, DICT_OF, meth, _params(dtype, **kw), monkeypatch)
    for b in range(B):
        assert got[b]['stats'][_native.STAT_EVENTS] > 0, case
        _same(got[b], want[b], '%s signal %d' % (case, b))
        if method == 'cmp':
            g = DICT_OF[b]
            _check_oracle(got[b], x[b], Ds[g], None if w is None else w[g], kw)


def test_set_sizes(engines, monkeypatch):
    """G = 1, G = B, and a set with dictionaries (1 and 2) that no signal uses."""
    from hsc_amd import _native
    multi, single = engines
    for G, dict_of in [(1, [0, 0, 0, 0, 0]), (5, [0, 1, 2, 3, 4]), (4, [3, 0, 3, 0, 3])]:
        Ds, x, w = _problem(F64, 5, 8, 1, 96, 5, G, seed=3, weighted=True)
        p = _params(F64, nbNonzeroCoefs=10)
        got = _encode_multi(multi, Ds, w, x, dict_of, _native.METHOD_CMP, p)
        want = _encode_singles(single, Ds, w, x, dict_of, _native.METHOD_CMP, p, monkeypatch)
        for b in range(5):
            _same(got[b], want[b], 'G = %d signal %d' % (G, b))


def test_all_ones_weights_beside_weighted(engines, monkeypatch):
    """One weight set all ones beside a weighted one: the set is weighted, the weighted dictionary's signals select by their
    weights (and differ from the unweighted selection), the all-ones dictionary's as without weights."""
    from hsc_amd import _native
    Ds, x, _ = _problem(F32, 5, 8, 1, 96, 5, 3, seed=21, weighted=False)
    w = np.ones((3, 5), dtype=F32)
    w[2] = [1.0, 0.05, 1.0, 0.05, 0.05]
    multi, single = engines
    p = _params(F32, nbNonzeroCoefs=10)
    got = _encode_multi(multi, Ds, w, x, DICT_OF, _native.METHOD_CMP, p)
    want = _encode_singles(single, Ds, w, x, DICT_OF, _native.METHOD_CMP, p, monkeypatch)
    plain = _encode_singles(single, Ds, None, x, DICT_OF, _native.METHOD_CMP, p, monkeypatch)
    for b in range(5):
        _same(got[b], want[b], 'signal %d' % b)
    assert any(not np.array_equal(got[b]['k'], plain[b]['k']) for b in (0, 2, 4)), 'the weights of dictionary 2 changed no selection'
    for b in (1, 3):
        _same(got[b], plain[b], 'all-ones signal %d' % b)
    # every set all ones: the unweighted instances
    got1 = _encode_multi(multi, Ds, np.ones((3, 5), dtype=F32), x, DICT_OF, _native.METHOD_CMP, p)
    for b in range(5):
        _same(got1[b], plain[b], 'signal %d' % b)


@pytest.mark.parametrize('method', ['cmp', 'locomp'])
def test_continue_one_round_at_a_time(engines, method):
    """hscmp_continue with max_rounds = 1 stepped to the end equals the uninterrupted run."""
    from hsc_amd import _native
    meth = _native.METHOD_LOCOMP if method == 'locomp' else _native.METHOD_CMP
    Ds, x, w = _problem(F64, 5, 8, 3, 96, 5, 3, seed=5, weighted=True)
    multi, _ = engines
    kw = dict(toleranceSnr=15.0, nbBlocks=3)
    whole = _encode_multi(multi, Ds, w, x, DICT_OF, meth, _params(F64, **kw))
    _encode_multi(multi, Ds, w, x, DICT_OF, meth, _params(F64, maxRounds=1, **kw))
    for _ in range(400):
        if not np.any(multi.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_RUNNING):
            break
        multi.continue_rounds(1)
    else:
        raise AssertionError('the stepped encode did not end')
    assert multi.last_variant().endswith('_multi')
    stepped = _results(multi, 5)
    for b in range(5):
        _same(stepped[b], whole[b], 'signal %d' % b)


def test_grow_events_after_capacity(engines):
    from hsc_amd import _native
    Ds, x, w = _problem(F32, 5, 7, 1, 96, 5, 3, seed=6, weighted=False)
    multi, _ = engines
    whole = _encode_multi(multi, Ds, w, x, DICT_OF, _native.METHOD_CMP, _params(F32, nbNonzeroCoefs=20, maxEvents=128))
    _encode_multi(multi, Ds, w, x, DICT_OF, _native.METHOD_CMP, _params(F32, nbNonzeroCoefs=20, maxEvents=6))
    assert np.all(multi.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_CAPACITY)
    multi.grow_events(128)
    multi.continue_rounds(0)
    grown = _results(multi, 5)
    for b in range(5):
        _same(grown[b], whole[b], 'signal %d' % b)


def test_stop_signal(engines):
    from hsc_amd import _native
    Ds, x, w = _problem(F32, 5, 8, 1, 96, 5, 3, seed=7, weighted=False)
    multi, _ = engines
    _encode_multi(multi, Ds, w, x, DICT_OF, _native.METHOD_CMP, _params(F32, nbNonzeroCoefs=20, maxRounds=1))
    multi.stop_signal(1)
    multi.continue_rounds(0)
    st = multi.fetch_stats()
    assert st[1, _native.STAT_STOP] == 6 and st[1, _native.STAT_EVENTS] == 1          # STOP_CALLBACK, after its first round
    assert np.all(st[[0, 2, 3, 4], _native.STAT_STOP] == 2)                              # the others ran to nbNonzeroCoefs


def test_refusals(engines):
    """Every refusal has its code and names its reason; the set survives them."""
    from hsc_amd import _native
    Ds, x, w = _problem(F64, 5, 8, 1, 96, 5, 3, seed=8, weighted=False)
    multi, single = engines
    p = _params(F64, nbNonzeroCoefs=5)
    multi.set_dictionaries(Ds, None)
    K = 5
    sparse = [__import__('scipy.sparse').sparse.csc_matrix((96, K))] * 5
    calls = {
        'hscmp_encode_batch': lambda: multi.encode_batch(x, p),
        'hscmp_encode_batch_device': lambda: multi.encode_batch_device(0x1000, 5, 96, p),
        'hscmp_encode_batch_ragged': lambda: multi.encode_batch_ragged(x, [96, 90, 80, 70, 60], p),
        'hscmp_encode_batch_ragged_device': lambda: multi.encode_batch_ragged_device(0x1000, 5, 96, [96, 90, 80, 70, 60], p),
        'hscmp_load_level': lambda: multi.load_level(None, 96, sparse),
        'hscmp_load_level_ragged': lambda: multi.load_level_ragged(None, 96, [96] * 5, sparse),
        'hscmp_table_open': lambda: multi.table_open(x[0]),
        'hscmp_assign_windows': lambda: multi.assign_windows(x[:, :20]),
        'hscmp_convolve1d': lambda: multi.convolve1d(x[0], True),
    }
    for name, call in sorted(calls.items()):
        with pytest.raises(_native.HscmpError) as ei:
            call()
        assert ei.value.code == _native.ERR_STATE, name
        assert name in str(ei.value) and 'holds a set of 3 dictionaries' in str(ei.value) and 'hscmp_encode_batch_multi' in str(ei.value), str(ei.value)
    # from-level and the epilogue, with the set on either side
    single.set_dictionary(Ds[0])
    single.encode_batch(x, p)
    multi.encode_batch_multi(x, DICT_OF, p)
    for name, call in (('hscmp_encode_batch_from_level', lambda: multi.encode_batch_from_level(single, 0, 5, None, p)),
                       ('hscmp_encode_batch_from_level', lambda: single.encode_batch_from_level(multi, 0, 5, None, p)),
                       ('hscmp_hierarchy_epilogue', lambda: multi.hierarchy_epilogue(single, 0, [], None, np.zeros(5, np.int64))),
                       ('hscmp_hierarchy_epilogue', lambda: single.hierarchy_epilogue(multi, 0, [], None, np.zeros(5, np.int64)))):
        with pytest.raises(_native.HscmpError) as ei:
            call()
        assert ei.value.code == _native.ERR_STATE, name
        assert name in str(ei.value) and 'set of' in str(ei.value) and 'dictionaries' in str(ei.value), str(ei.value)
    # the set is still there, and so is its batch
    assert multi.fetch_stats().shape == (5, 8)
    multi.encode_batch_multi(x, DICT_OF, p)
    # dict_of out of range: HSCMP_ERR_INVALID naming the signal, nothing queued
    for bad, b in (([2, 0, 3, 1, 2], 2), ([2, 0, 2, 1, -1], 4)):
        with pytest.raises(_native.HscmpError) as ei:
            multi.encode_batch_multi(x, bad, p)
        assert ei.value.code == _native.ERR_INVALID
        assert 'signal %d asks for dictionary %d outside [0, G=3)' % (b, bad[b]) in str(ei.value)
    # a plain dictionary: hscmp_encode_batch_multi answers HSCMP_ERR_STATE
    with pytest.raises(_native.HscmpError) as ei:
        single.encode_batch_multi(x, DICT_OF, p)
    assert ei.value.code == _native.ERR_STATE and 'holds one dictionary' in str(ei.value)
    # ... and set_dictionary on the engine of the set puts a plain dictionary back
    multi.set_dictionary(Ds[1])
    multi.encode_batch(x, p)
    assert not multi.last_variant().endswith('_multi')


def test_random_sweep(engines, monkeypatch):
    """About 40 seeded random small shapes against the single-dictionary encode; W <= T always (no draw is refused)."""
    from hsc_amd import _native
    rng = np.random.RandomState(2024)
    multi, single = engines
    for case in range(40):
        K, F, B, G = rng.randint(1, 9), rng.randint(1, 4), rng.randint(1, 7), rng.randint(1, 5)
        W = rng.randint(1, 13)
        T = rng.randint(max(W, 2), 161)
        dtype = [F32, F64][rng.randint(2)]
        method = [_native.METHOD_CMP, _native.METHOD_LOCOMP][rng.randint(2)]
        weighted = bool(rng.randint(2))
        blocks = [1, 1, 2, 3, 'auto'][rng.randint(5)]
        if blocks != 1 and blocks != 'auto' and T // blocks < 2:
            blocks = 1
        Ds, x, w = _problem(dtype, K, W, F, T, B, G, seed=1000 + case, weighted=weighted)
        dict_of = rng.randint(0, G, size=B)
        kw = dict(nbNonzeroCoefs=int(rng.randint(1, 15)), nbBlocks=blocks) if rng.randint(2) else dict(toleranceSnr=12.0, nbBlocks=blocks)
        what = 'case %d: K=%d W=%d F=%d T=%d B=%d G=%d %s method=%d %r' % (case, K, W, F, T, B, G, np.dtype(dtype).name, method, kw)
        p = _params(dtype, **kw)
        got = _encode_multi(multi, Ds, w, x, dict_of, method, p)
        want = _encode_singles(single, Ds, w, x, dict_of, method, p, monkeypatch)
        for b in range(B):
            _same(got[b], want[b], '%s signal %d' % (what, b))


def test_python_surface(monkeypatch):
    """computeCoefficientsMultiBatch (CMP and LoCOMP) against computeCoefficients signal by signal."""
    from hsc_amd.modeling import ConvolutionalMatchingPursuit, LoCOMP
    Ds, x, w = _problem(F64, 5, 8, 1, 96, 5, 3, seed=9, weighted=True)
    for coder_type in (ConvolutionalMatchingPursuit, LoCOMP):
        res = coder_type().computeCoefficientsMultiBatch(x[:, :, 0], Ds[:, :, :, 0], DICT_OF, nbNonzeroCoefs=10, weights=w)
        assert res.variant.endswith('_multi') and res.residuals.shape == (5, 96)
        for b, g in enumerate(DICT_OF):
            coef, residual = coder_type().computeCoefficients(x[b, :, 0], Ds[g, :, :, 0], nbNonzeroCoefs=10, weights=w[g])
            assert (res.coefficients[b] != coef).nnz == 0 and np.array_equal(res.residuals[b], residual)
    # dictionaryOf=None: signal b takes dictionary b; a list of dictionaries
    res = ConvolutionalMatchingPursuit().computeCoefficientsMultiBatch(x[:3], [Ds[0], Ds[1], Ds[2]], nbNonzeroCoefs=6)
    for b in range(3):
        coef, residual = ConvolutionalMatchingPursuit().computeCoefficients(x[b], Ds[b], nbNonzeroCoefs=6)
        assert (res.coefficients[b] != coef).nnz == 0 and np.array_equal(res.residuals[b], residual)


def test_locomp_group_stop_goes_to_the_host_loop_with_its_own_dictionary(monkeypatch):
    """HSCMP_LOCOMP_GROUP_CAP=3: the device loop gives up every signal whose groups exceed two neighbours (stop reason 'group');
    computeCoefficientsMultiBatch takes such a signal again through the host loop with ITS OWN dictionary and weights, and books
    it as computeCoefficientsBatch does."""
    from hsc_amd import _native
    from hsc_amd.modeling import LoCOMP
    Ds, x, w = _problem(F64, 5, 8, 1, 96, 5, 3, seed=13, weighted=True)
    monkeypatch.setenv('HSCMP_LOCOMP_GROUP_CAP', '3')
    res = LoCOMP().computeCoefficientsMultiBatch(x[:, :, 0], Ds[:, :, :, 0], DICT_OF, nbNonzeroCoefs=30, weights=w)
    host = np.where(res.stats[:, _native.STAT_STOP] == _native.STOP_HOST)[0]
    assert host.size > 0, 'no signal reached the group capacity: %r' % res.stop_reasons()
    for b in host:
        g = DICT_OF[b]
        coef, residual = LoCOMP()._computeCoefficientsHost(x[b, :, 0], Ds[g, :, :, 0], nbNonzeroCoefs=30, weights=w[g])
        assert (res.coefficients[b] != coef).nnz == 0 and np.array_equal(res.residuals[b], residual)
        assert res.stats[b, _native.STAT_NNZ] == coef.nnz and len(res.events[b][0]) == 0
        assert res.energies[b, 1] == float(np.sum(np.square(residual)))
