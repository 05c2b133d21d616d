"""Ragged batches through the level kernels: multi-feature signals of different lengths in one call.

Level-shaped problems as tests/test_gpu_sparse.py builds them (sparse [T_b, F] inputs, composite atoms plus unit singletons)
run through Engine.encode_batch_ragged on every sparse plan: sparse / dictlist initial correlation with the generic, gathered
and dictlist loops in their plain, packed and round-parallel forms.  Per signal and bit for bit, the events, stats, slots,
residual[:T_b], energies and the (T_b, K) CSC must equal the CPU oracle on the signal alone and the same engine's uniform
single-signal encode.  The lengths are W, 3W-3, 3W-2, a multiple of neither 2W-1 nor 32, an odd length, and the stride T."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64

VARIANTS = {'paired': {}, 'atom_lists': {'HSCMP_NO_PAIRING': '1'},
            'gathered': {'HSCMP_NO_DICT_LISTS': '1', 'HSCMP_FORCE_GATHERED': '1'},
            'dense_dictionary': {'HSCMP_NO_DICT_LISTS': '1'},
            'paired_row_scan': {'HSCMP_NO_ROW_LISTS': '1'},
            'paired_no_rowbits': {'HSCMP_NO_ROW_LISTS': '1', 'HSCMP_NO_ROWBITS': '1'},
            'packed': {'HSCMP_SPARSE_PACKED': '1'}}


def _level_dictionary(seed, F, K, W, dtype, nnz_atom=3):
    """K composite atoms of nnz_atom events each behind F unit singleton atoms at the centre tap (hsc/dataset.py:826-860)."""
    rs = np.random.RandomState(seed)
    D = np.zeros((K, W, F), dtype=dtype)
    for k in range(K):
        for _ in range(nnz_atom):
            D[k, rs.randint(0, W), rs.randint(0, F)] = rs.uniform(0.5, 1.5) * rs.choice([-1.0, 1.0])
        D[k] /= np.sqrt(np.sum(np.square(D[k])))
    S = np.zeros((F, W, F), dtype=dtype)
    S[np.arange(F), (W - 1) // 2, np.arange(F)] = 1.0
    return np.concatenate((S, D), axis=0)


def _level_input(seed, T, D, density=0.02):
    """Sparse [T, F] input: planted composite events + stray singles, clipped at the signal's ends."""
    rs = np.random.RandomState(seed)
    W, F = D.shape[1], D.shape[2]
    dtype = D.dtype.type
    x = np.zeros((T, F), dtype=dtype)
    for _ in range(max(1, int(density * T))):
        k = rs.randint(0, D.shape[0]); t = rs.randint(0, T); c = rs.uniform(0.5, 2.0) * rs.choice([-1.0, 1.0])
        s, e = max(0, t - (W - 1) // 2), min(T, t - (W - 1) // 2 + W)
        x[s:e] += (c * D[k][s - (t - (W - 1) // 2):e - (t - (W - 1) // 2)]).astype(dtype)
    return x


W8 = 8
LENGTHS = [W8, 3 * W8 - 3, 3 * W8 - 2, 100, 333, 512]
LENGTHS_F32 = [16, 45, 46, 300]                                 # W = 16: W, 3W-3, 3W-2, the stride


def _problem(kind):
    """(signals, D): one dictionary, per-signal inputs."""
    if kind == 'f32':
        D = _level_dictionary(4, 16, 8, 16, F32)
        return [_level_input(400 + b, n, D) for b, n in enumerate(LENGTHS_F32)], D
    D = _level_dictionary(1, 24, 12, W8, F64)
    if kind == 'dense':         # dense inputs: the window / pair lists overflow and the fallback chains run
        return [np.random.RandomState(100 + b).standard_normal((n, 24)) for b, n in enumerate(LENGTHS)], D
    return [_level_input(100 + b, n, D) for b, n in enumerate(LENGTHS)], D


def _weights(D):
    F = D.shape[2]
    w = np.ones(D.shape[0], dtype=D.dtype)
    w[:F] = 0.9                                         # singletonWeight, modeling.py:1469-1476
    w[F] = 0.0                                          # a muted atom: its score is 0 whatever its coefficient
    return w


L0 = dict(nbNonzeroCoefs=60)
BLOCKED = dict(toleranceSnr=25.0, nbBlocks=4)

# name: (problem, env, params, weighted)
ROWS = {}
for _name, _env in VARIANTS.items():
    ROWS[_name + '_l0'] = ('f64', _env, L0, False)
    ROWS[_name + '_blocked'] = ('f64', _env, BLOCKED, False)
ROWS.update({
    'blocked_no_rp': ('f64', {'HSCMP_RP': '0'}, BLOCKED, False),
    'blocked_rp': ('f64', {'HSCMP_RP': '1'}, BLOCKED, False),
    'auto_blocks': ('f64', {}, dict(toleranceSnr=25.0, nbBlocks='auto'), False),
    'auto_blocks_rp': ('f64', {'HSCMP_RP': '1'}, dict(toleranceSnr=25.0, nbBlocks='auto'), False),
    'f32_blocked': ('f32', {}, dict(toleranceSnr=20.0, nbBlocks=3), False),
    'weighted_l0': ('f64', {}, L0, True),
    'weighted_blocked_rp': ('f64', {'HSCMP_RP': '1'}, BLOCKED, True),
    'dense_inputs': ('dense', {}, dict(nbNonzeroCoefs=25), False),
    'dense_inputs_blocked': ('dense', {}, dict(toleranceSnr=3.0, nbBlocks=2), False),
})

_ORACLE = {}


def _oracle(kind, kw, weighted, b):
    """The CPU oracle on signal b alone: computed once per (problem, parameters, weights), shared by the rows."""
    from oracle import hsc_oracle as orc
    key = (kind, tuple(sorted(kw.items())), weighted, b)
    if key not in _ORACLE:
        xs, D = _problem(kind)
        _ORACLE[key] = orc.cmp_encode(xs[b], D, weights=_weights(D) if weighted else None, **kw)
    return _ORACLE[key]


def _padded(xs, fill=0.0):
    T = max(len(x) for x in xs)
    x = np.full((len(xs), T, xs[0].shape[1]), fill, dtype=xs[0].dtype)
    for b, s in enumerate(xs):
        x[b, :len(s)] = s
    return x, np.array([len(s) for s in xs], dtype=np.int32)


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
    return out, r.copy()


def _same(a, b):
    assert np.array_equal(a['stats'], b['stats']), (a['stats'], b['stats'])
    for key in ('t', 'k', 'c', 'residual', 'energies'):
        assert np.array_equal(a[key], b[key]), key
    for u, v in zip(a['slots'], b['slots']):
        assert np.array_equal(u, v)


def _check_against_oracle(res, ref, Tb, K):
    from hsc_amd import _native
    from hsc_amd.modeling import _slots_to_csc
    coef, r_ref, info = ref
    assert len(info['t']) > 0
    assert np.array_equal(res['t'], info['t']) and np.array_equal(res['k'], info['k']), 'positions / atoms differ from the oracle'
    assert np.array_equal(res['c'], info['c']), 'coefficients differ from the oracle'
    assert np.array_equal(res['residual'], r_ref.reshape(res['residual'].shape)), 'residual differs from the oracle'
    st = res['stats']
    assert st[_native.STAT_NNZ] == info['nnz'] and st[_native.STAT_DUPLICATES] == info['duplicates']
    assert st[_native.STAT_ROUNDS] == info['rounds'] and st[_native.STAT_ITERATIONS] == info['iterations']
    assert _native.STOP_NAMES.get(int(st[_native.STAT_STOP])) == info['stop']
    mine = _slots_to_csc(*res['slots'], len(res['slots'][0]), (Tb, K), 1e-16)
    assert mine.shape == coef.shape == (Tb, K)
    assert (mine != coef).nnz == 0


def _setup(name, monkeypatch):
    kind, env, kw, weighted = ROWS[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    xs, D = _problem(kind)
    return kind, kw, weighted, xs, D, (_weights(D) if weighted else None), float(np.finfo(D.dtype).eps)


@pytest.mark.parametrize('name', sorted(ROWS))
def test_ragged_level_row(name, monkeypatch):
    from hsc_amd import _native
    kind, kw, weighted, xs, D, w, eps = _setup(name, monkeypatch)
    x, lens = _padded(xs)
    K = D.shape[0]
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        params = _native.make_params(eps=eps, maxEvents=2048, **kw)
        eng.encode_batch(x, params)
        uniform = eng.last_variant()
        assert uniform.startswith(('sparse_init', 'dictlist_init')), uniform
        eng.encode_batch_ragged(x, lens, params)
        assert eng.last_variant() == uniform + '_ragged'
        got, raw = _all_results(eng, lens)
        for b, Tb in enumerate(lens):
            assert not raw[b, Tb:].any(), 'the residual above the signal length is not zero'
        for b, s in enumerate(xs):
            eng.encode_batch(s[np.newaxis], params)
            one, _ = _all_results(eng, [len(s)])
            _same(got[b], one[0])
            _check_against_oracle(got[b], _oracle(kind, kw, weighted, b), len(s), K)
    finally:
        eng.close()


def test_variants_cover_every_level_plan(monkeypatch):
    """The rows above run the ragged form of the plans a variant name tells apart: both initial correlations, the three loops, plain
    and rp.  The packed build of the loop (HSCMP_SPARSE_PACKED=1, the 'packed_*' rows) has no suffix of its own in hscmp_last_variant,
    so its rows prove its results, not -- by name -- that SparseRecorr<R, true, true> is the instantiation that ran."""
    from hsc_amd import _native
    seen = set()
    for name in ('paired_l0', 'gathered_l0', 'dense_dictionary_l0', 'blocked_rp', 'packed_l0'):
        with monkeypatch.context() as m:
            kind, kw, weighted, xs, D, w, eps = _setup(name, m)
            x, lens = _padded(xs)
            eng = _native.Engine(0)
            try:
                eng.set_dictionary(D, w)
                eng.encode_batch_ragged(x, lens, _native.make_params(eps=eps, maxEvents=2048, **kw))
                seen.add(eng.last_variant())
            finally:
                eng.close()
    assert {'dictlist_init+dictlist_loop_f64_ragged', 'sparse_init+gathered_loop_f64_ragged', 'sparse_init+generic_loop_f64_ragged',
            'dictlist_init+dictlist_loop_f64_rp_ragged'} <= seen, seen


NAN_ROWS = ['paired_l0', 'paired_row_scan_l0', 'paired_no_rowbits_blocked', 'gathered_l0', 'dense_dictionary_l0', 'blocked_rp', 'f32_blocked']


@pytest.mark.parametrize('name', NAN_ROWS)
def test_nan_padding_changes_nothing(name, monkeypatch):
    """Rows above a signal's length are never read (row-list build, row-flag scan, prepare): NaN there changes nothing."""
    from hsc_amd import _native
    kind, kw, weighted, xs, D, w, eps = _setup(name, monkeypatch)
    x0, lens = _padded(xs)
    xn, _ = _padded(xs, fill=np.nan)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        params = _native.make_params(eps=eps, maxEvents=2048, **kw)
        eng.encode_batch_ragged(x0, lens, params)
        ref, raw0 = _all_results(eng, lens)
        eng.encode_batch_ragged(xn, lens, params)
        got, raw = _all_results(eng, lens)
        assert np.array_equal(raw, raw0)
        for b in range(len(lens)):
            _same(got[b], ref[b])
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['paired_l0', 'packed_blocked', 'gathered_blocked', 'dense_dictionary_l0', 'blocked_rp', 'f32_blocked'])
def test_equal_lengths_match_uniform(name, monkeypatch):
    """All lengths equal to T through the ragged entry: the uniform entry's bits."""
    from hsc_amd import _native
    kind, kw, weighted, xs, D, w, eps = _setup(name, monkeypatch)
    T = 200
    xs = [_level_input(900 + b, T, D) for b in range(3)]
    x, lens = _padded(xs)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        params = _native.make_params(eps=eps, maxEvents=2048, **kw)
        eng.encode_batch(x, params)
        uni_variant = eng.last_variant()
        uni, raw_u = _all_results(eng, lens)
        eng.encode_batch_ragged(x, lens, params)
        assert eng.last_variant() == uni_variant + '_ragged'
        rag, raw_r = _all_results(eng, lens)
        assert np.array_equal(raw_u, raw_r)
        for a, b in zip(rag, uni):
            _same(a, b)
        eng.encode_batch(x, params)                      # a plain encode clears the lengths
        assert eng.last_variant() == uni_variant
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['paired_blocked', 'paired_row_scan_blocked', 'gathered_blocked', 'blocked_rp', 'paired_l0'])
def test_resume_matches_one_launch(name, monkeypatch):
    """maxRounds = 2 and hscmp_continue until every signal stopped: the uninterrupted run's results (the row flags and row lists
    of a ragged batch carry over between launches with the batch's stride)."""
    from hsc_amd import _native
    kind, kw, weighted, xs, D, w, eps = _setup(name, monkeypatch)
    x, lens = _padded(xs)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        eng.encode_batch_ragged(x, lens, _native.make_params(eps=eps, maxEvents=2048, **kw))
        variant = eng.last_variant()
        one, raw1 = _all_results(eng, lens)
        eng.encode_batch_ragged(x, lens, _native.make_params(eps=eps, maxEvents=2048, maxRounds=2, **kw))
        for _ in range(10000):
            if not (eng.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_RUNNING).any():
                break
            eng.continue_rounds(2)
        assert eng.last_variant() == variant
        two, raw2 = _all_results(eng, lens)
        assert np.array_equal(raw1, raw2)
        for a, b in zip(two, one):
            _same(a, b)
    finally:
        eng.close()


@pytest.mark.parametrize('kw', [L0, BLOCKED], ids=['l0', 'blocked'])
def test_modeling_list_form_and_capacity_regrowth(kw):
    """ConvolutionalMatchingPursuit.computeCoefficientsBatch on a list of [T_b, F] signals, with a maxEvents of 8 that forces the
    STOP_CAPACITY regrowth: per signal what computeCoefficients gives it alone; the padded form with lengths= gives the same."""
    from hsc_amd.modeling import ConvolutionalMatchingPursuit
    D = _level_dictionary(1, 24, 12, W8, F64)
    xs = [_level_input(700 + b, n, D, density=0.1) for b, n in enumerate(LENGTHS)]     # (51 planted events in the longest signal)
    cmp = ConvolutionalMatchingPursuit()
    res = cmp.computeCoefficientsBatch(xs, D, maxEvents=8, **kw)
    assert res.variant.endswith('_ragged')
    assert list(res.lengths) == [len(s) for s in xs]
    assert max(len(ev[0]) for ev in res.events) > 8
    single = ConvolutionalMatchingPursuit()
    for b, s in enumerate(xs):
        coef, residual = single.computeCoefficients(s, D, **kw)
        one = single.lastResult
        assert res.coefficients[b].shape == (len(s), D.shape[0])
        assert (res.coefficients[b] != coef).nnz == 0
        assert res.residuals[b].shape == residual.shape and np.array_equal(res.residuals[b], residual)
        assert all(np.array_equal(u, v) for u, v in zip(res.events[b], one.events[0]))
        assert np.array_equal(res.stats[b], one.stats[0]) and np.array_equal(res.energies[b], one.energies[0])
    x, lens = _padded(xs, fill=np.nan)
    res2 = cmp.computeCoefficientsBatch(x, D, lengths=lens, **kw)
    for b in range(len(xs)):
        assert np.array_equal(res2.residuals[b], res.residuals[b])
        assert all(np.array_equal(u, v) for u, v in zip(res2.events[b], res.events[b]))
