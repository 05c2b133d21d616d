"""The bound pass of the initial correlation, one bf16 product per tap: csrc/hscmp_bound.h, DESIGN.md section 11.

1. Validity: the bound pass alone (HSCMP_INIT_ONLY=1) against the exact pass alone (HSCMP_EXACT_INIT=1): ub[t] >= score[t]
   at every bound position, exact positions equal bit for bit.  Seven input families, two of them built to line the
   rounding errors of the single product up; median and maximum of ub / exact - 1 are printed, not asserted.
2. Identity: whole encodes against HSCMP_EXACT_INIT=1, bit for bit: events, slots, stats, energies, residuals.  The same
   families, and a near-tie input on which the one-product bounds of many positions outrank the best exact score, so
   that the first selection refines more rows than a RefineList holds and takes the commit path.
3. Chunks outside the model (a non-finite or tiny sample) hold exact scores, in batches where one, every or no chunk is one.

Mutation tried against this file (a scratch build, run once): with kBoundEps1 halved, test_bound_is_valid fails on the
`tight` family at all three shapes, with and without weights, and on `magnitudes` at W = 16; the other 77 validity cases
of the one-product pass still pass, so the `tight` family is what holds the constant."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _env(object):
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(D, w):
    from hsc_amd import _native
    eng = _native.Engine(0)
    eng.set_dictionary(D, weights=w)
    return eng


def _under_midpoint(rs, shape, tight):
    """Magnitudes just under a bf16 rounding midpoint.  The family as stated: m (1 + 2^-8 - 2^-22) 2^e for a random 8-bit
    significand m in 128..255 (just under the midpoint at m = 128; larger m lie past theirs and round up).  tight: m = 128
    everywhere and one exponent, the largest relative rounding error a bf16 has, so that the tile's error comes within
    2 % of the slack when a window is a multiple of an atom (tests/test_bound_one_product.py works the figure out)."""
    if tight:
        return np.full(shape, 128.0 * (1.0 + 2.0 ** -8 - 2.0 ** -22) * 2.0 ** -10, dtype=np.float32)
    m = rs.randint(128, 256, size=shape).astype(np.float64)
    return (m * (1.0 + 2.0 ** -8 - 2.0 ** -22) * np.exp2(rs.randint(-12, -8, size=shape))).astype(np.float32)


def _family(kind, B, T, K, W, seed):
    """(x [B,T] float32, D [K,W] float32) for one input family."""
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed)
    rs = np.random.RandomState(seed)
    if kind == 'planted':
        x = np.stack([synth.make_signal(D, T, b, kind='planted', nb_atoms=max(4, T // 100), noise=0.05, seed=seed) for b in range(B)])
    elif kind == 'noise':
        x = rs.standard_normal((B, T))
    elif kind == 'magnitudes':          # 2^-50 .. 2^50 inside one chunk
        x = rs.standard_normal((B, T)) * np.exp2(rs.randint(-50, 51, size=(B, T)))
    elif kind == 'zero_const':          # all-zero and constant stretches
        x = np.zeros((B, T))
        x[:, T // 3: 2 * T // 3] = 1.5
        x[1::2, :T // 4] = -0.25
    elif kind == 'repeated':            # one atom repeated: many tied scores
        x = np.zeros((B, T))
        for p in range(W, T - W, 3 * W):
            x[:, p: p + W] += D[1 % K]
    elif kind in ('adversarial', 'tight'):
        # every dictionary entry and every sample of a planted window just under a rounding midpoint, the sample's sign
        # that of the atom's tap: both factors of every product round towards zero and every dropped term is positive
        tight = kind == 'tight'
        D = _under_midpoint(rs, (K, W), tight) * rs.choice(np.float32([-1.0, 1.0]), size=(K, W))
        x = np.zeros((B, T), dtype=np.float32)
        for b in range(B):
            for i, p in enumerate(range(W, T - 2 * W, 2 * W)):
                k = (i + b) % K
                x[b, p: p + W] = np.float32(4.0) * D[k] if tight else _under_midpoint(rs, W, False) * np.sign(D[k])
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(D, dtype=np.float32)


def _weights(K, shape, weights):
    return (0.5 + np.random.RandomState(shape).random_sample(K)).astype(np.float32) if weights else None


def _init_state(eng, x, exact, L0=8):
    from hsc_amd import _native
    with _env(HSCMP_INIT_ONLY='1', HSCMP_EXACT_INIT='1' if exact else None):
        eng.encode_batch(x[:, :, None], _native.make_params(nbNonzeroCoefs=L0, eps=1e-30, maxEvents=4 * L0))
    v = eng.device_view()
    B, T = x.shape
    bc = eng.copy_from_device(v.best_c, (B, T), np.float32)
    bk = eng.copy_from_device(v.best_k, (B, T), np.int32)
    return bc, bk, eng.last_variant()


def _encode_all(eng, x, params, exact, quad=None, rounds=None, scramble=None):
    """One whole encode (or one resumed in rounds, the caller's buffer overwritten in between) and everything it leaves."""
    from hsc_amd import _native
    with _env(HSCMP_EXACT_INIT='1' if exact else None, HSCMP_MFMA_QUAD=quad, HSCMP_INIT_ONLY=None):
        if rounds is None:
            eng.encode_batch(x[:, :, None], params)
        else:
            xd = np.array(x)
            eng.encode_batch(xd[:, :, None], params)
            for _ in range(2000):
                if scramble is not None:
                    xd[:] = scramble
                if np.all(eng.fetch_stats()[:, _native.STAT_STOP] != _native.STOP_RUNNING):
                    break
                eng.continue_rounds(rounds)
        variant = eng.last_variant()
    t, k, c = eng.fetch_events()
    return dict(t=t, k=k, c=c, stats=eng.fetch_stats(), slots=eng.fetch_slots(), energies=eng.fetch_energies(),
                residual=eng.fetch_residual(), variant=variant)


def _same(a, b):
    for key in ('stats', 'energies', 'residual'):
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
    assert np.array_equal(a['t'], b['t']) and np.array_equal(a['k'], b['k'])
    assert np.array_equal(a['c'].view(np.int32), b['c'].view(np.int32))
    for u, v in zip(a['slots'], b['slots']):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


def _check_valid(ub, uk, ex, ek, label=None):
    assert np.all(ek >= 0)
    bound = uk == -1
    assert np.array_equal(ub[~bound].view(np.int32), ex[~bound].view(np.int32)) and np.array_equal(uk[~bound], ek[~bound])
    assert np.all(ub[bound] >= ex[bound])
    if label and bound.any():
        rel = ub[bound].astype(np.float64) / np.maximum(ex[bound].astype(np.float64), 1e-30) - 1.0
        print('%s: ub/exact - 1 median %.3g max %.3g' % (label, np.median(rel), rel.max()))
    return bound


FAMILIES = ['planted', 'noise', 'magnitudes', 'zero_const', 'repeated', 'adversarial', 'tight']
SHAPES = [(2, 4500, 40, 64), (2, 4500, 33, 31), (2, 3000, 20, 16)]     # SB = 4, 2, 1; K not a multiple of 32; T across a chunk and its halo
PRODUCTS = [None]       # one product per tap is the only pass there is; the parameter stays, and with it the ids of the cases

_exact_cache = {}


def _init_case(kind, shape, weights):
    """The inputs of a validity case and its exact init state, computed once; nothing changes them afterwards."""
    B, T, K, W = SHAPES[shape]
    key = (kind, shape, weights)
    if key not in _exact_cache:
        x, D = _family(kind, B, T, K, W, 11 + shape)
        w = _weights(K, shape, weights)
        _exact_cache[key] = (x, D, w, _init_state(_engine(D, w), x, True))
    return _exact_cache[key]


@pytest.mark.parametrize('products', PRODUCTS)
@pytest.mark.parametrize('kind', FAMILIES)
@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_bound_is_valid(kind, shape, weights, products):
    x, D, w, (ex, ek, var_e) = _init_case(kind, shape, weights)
    ub, uk, var_b = _init_state(_engine(D, w), x, False)
    assert var_b == 'bound_init' and var_e == 'mfma_init'
    bound = _check_valid(ub, uk, ex, ek, '%s W=%d weights=%d products=%s' % (kind, SHAPES[shape][3], weights, products or '1'))
    if kind not in ('zero_const',):
        assert bound.any()


@pytest.mark.parametrize('kind', FAMILIES)
@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_encode_identity(kind, shape, weights):
    """The bound pass against the exact reference, both on one engine: the slot arrays are compared whole, and what lies
    behind a signal's last slot is whatever the engine's buffer held before."""
    from hsc_amd import _native
    B, T, K, W = SHAPES[shape]
    x, D = _family(kind, B, T, K, W, 31 + shape)
    eng = _engine(D, _weights(K, shape, weights))
    params = _native.make_params(nbNonzeroCoefs=40, eps=1e-30, maxEvents=4096)
    ref = _encode_all(eng, x, params, True)
    assert '_bound' not in ref['variant']
    a = _encode_all(eng, x, params, False)
    assert a['variant'].startswith('mfma_init+mfma_loop_f32_bound'), a['variant']
    _same(a, ref)


# ---- near ties: more winning bounds in front of the exact winner than a RefineList holds ------------------------------
def _near_tie(B, T, K, W, seed):
    """One atom planted at 12 positions 3W apart with amplitudes 1 + 5e-4 j (the steps far below the one-product slack
    of 2^-7), on a background of noise a hundred times smaller than a step."""
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed)
    rs = np.random.RandomState(seed)
    x = 5e-6 * rs.standard_normal((B, T))
    pos = [W + 3 * W * j for j in range(12)]
    assert pos[-1] + W <= T
    for j, p in enumerate(pos):
        x[:, p: p + W] += (1.0 + 5e-4 * j) * D[3 % K]
    return np.ascontiguousarray(x, dtype=np.float32), D


def _assert_many_winning_bounds(eng, x):
    ub, uk, _ = _init_state(eng, x, False)
    ex, ek, _ = _init_state(eng, x, True)
    _check_valid(ub, uk, ex, ek)
    above = ((uk == -1) & (ub > ex.max(axis=1, keepdims=True))).sum(axis=1)
    print('bounds above the largest exact score, per signal: min %d max %d' % (above.min(), above.max()))
    assert np.all(above >= 6)


@pytest.mark.parametrize('quad', ['0', '1'])
def test_near_tie_identity(quad):
    from hsc_amd import _native
    x, D = _near_tie(4, 6000, 64, 64, 5)
    eng = _engine(D, None)
    _assert_many_winning_bounds(eng, x)
    params = _native.make_params(nbNonzeroCoefs=30, eps=1e-30, maxEvents=1024)
    ref = _encode_all(eng, x, params, True, quad=quad)
    _same(_encode_all(eng, x, params, False, quad=quad), ref)
    rparams = _native.make_params(nbNonzeroCoefs=30, eps=1e-30, maxEvents=1024, maxRounds=5)
    _same(_encode_all(eng, x, rparams, False, quad=quad, rounds=5, scramble=np.float32(123.0)), ref)


@pytest.mark.parametrize('quad', ['0', '1'])
def test_near_tie_identity_four_signals(quad):
    """600 signals: more than two per CU, the batch size of the four-signal build.  (12 positions 3W apart span 2240
    samples at W = 64, so the signals are 2304 long, not 2000.)"""
    from hsc_amd import _native
    x, D = _near_tie(600, 2304, 64, 64, 6)
    eng = _engine(D, None)
    _assert_many_winning_bounds(eng, x)
    params = _native.make_params(nbNonzeroCoefs=20, eps=1e-30, maxEvents=1024)
    ref = _encode_all(eng, x, params, True, quad=quad)
    a = _encode_all(eng, x, params, False, quad=quad)
    assert a['variant'] == ('mfma_init+mfma_loop_f32_bound_x4' if quad == '1' else 'mfma_init+mfma_loop_f32_bound'), a['variant']
    _same(a, ref)
    rparams = _native.make_params(nbNonzeroCoefs=20, eps=1e-30, maxEvents=1024, maxRounds=5)
    _same(_encode_all(eng, x, rparams, False, quad=quad, rounds=5, scramble=np.float32(123.0)), ref)


# ---- chunks outside the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('products', PRODUCTS)
def test_out_of_model_chunks(products):
    """One inf, one 1e-30 and one NaN in different chunks (with the halo: a chunk stages 32 samples before its first position
    and 64 + 32 after its last): those chunks hold exact scores, the others valid bounds, and encodes are identical."""
    from hsc_amd import _native
    x, D = _family('noise', 3, 6000, 64, 64, 3)
    x[0, 100] = np.inf
    x[1, 4100] = 1e-30
    x[2, 2500] = np.nan
    eng = _engine(D, None)
    ub, uk, _ = _init_state(eng, x, False)
    ex, ek, _ = _init_state(eng, x, True)
    assert np.all(uk[0, :2048] >= 0) and np.all(uk[0, 2048:] == -1)
    assert np.all(uk[1, 2048:] >= 0) and np.all(uk[1, :2048] == -1)          # (sample 4100 is in the halo of chunk 1 too)
    assert np.all(uk[2, 2048:4096] >= 0) and np.all(uk[2, :2048] == -1) and np.all(uk[2, 4096:] == -1)
    same = uk >= 0
    assert np.array_equal(ub[same].view(np.int32), ex[same].view(np.int32)) and np.array_equal(uk[same], ek[same])
    assert np.all(ub[~same] >= ex[~same])
    params = _native.make_params(nbNonzeroCoefs=30, eps=1e-30, maxEvents=4096)
    _same(_encode_all(eng, x, params, False), _encode_all(eng, x, params, True))


@pytest.mark.parametrize('products', PRODUCTS)
@pytest.mark.parametrize('every', [True, False])
def test_every_chunk_or_none_out_of_model(every, products):
    from hsc_amd import _native
    x, D = _family('noise', 3, 6000, 64, 64, 4)
    if every:
        x[:, 1000::2048] = 1e-30
    eng = _engine(D, None)
    ub, uk, _ = _init_state(eng, x, False)
    ex, ek, _ = _init_state(eng, x, True)
    if every:
        assert np.array_equal(ub.view(np.int32), ex.view(np.int32)) and np.array_equal(uk, ek)
    else:
        assert np.all(uk == -1) and np.all(ub >= ex)
    params = _native.make_params(nbNonzeroCoefs=30, eps=1e-30, maxEvents=4096)
    _same(_encode_all(eng, x, params, False), _encode_all(eng, x, params, True))
