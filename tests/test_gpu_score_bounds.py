"""The bound pass of the initial correlation (csrc/hscmp_bound.h) on the GPU.

1. Validity: the bound pass alone against the exact pass alone (HSCMP_INIT_ONLY=1, with and without
   HSCMP_EXACT_INIT=1): ub[t] >= score[t] at every position, exact positions (best_k != -1) equal.
2. Identity: whole encodes with the bound pass against HSCMP_EXACT_INIT=1 give the same events, slots,
   stats, energies and residuals, bit for bit -- one signal per workgroup and the four-signal build,
   resumed encodes whose caller input is overwritten between rounds, non-finite inputs."""
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
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32), D


def _init_state(eng, x, exact, L0):
    from hsc_amd import _native
    with _env(HSCMP_INIT_ONLY='1', HSCMP_EXACT_INIT='1' if exact else None):
        eng.encode_batch(x[:, :, None], _native.make_params(nbNonzeroCoefs=L0, eps=1e-30, maxEvents=4 * L0))
    v = eng.device_view()
    B, T = x.shape
    bc = eng.copy_from_device(v.best_c, (B, T), np.float32)
    bk = eng.copy_from_device(v.best_k, (B, T), np.int32)
    return bc, bk, eng.last_variant()


FAMILIES = ['planted', 'noise', 'magnitudes', 'zero_const', 'repeated']
SHAPES = [(3, 5000, 256, 64), (2, 4500, 100, 63), (2, 2048, 40, 32), (3, 7000, 33, 31), (2, 3000, 20, 16)]


@pytest.mark.parametrize('kind', FAMILIES)
@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_bound_is_valid(kind, shape, weights):
    B, T, K, W = SHAPES[shape]
    x, D = _family(kind, B, T, K, W, 11 + shape)
    w = (0.5 + np.random.RandomState(shape).random_sample(K)).astype(np.float32) if weights else None
    eng = _engine(D, w)
    ub, uk, var_b = _init_state(eng, x, False, 8)
    ex, ek, var_e = _init_state(eng, x, True, 8)
    assert var_b == 'bound_init' and var_e == 'mfma_init'
    assert np.all(ek >= 0)
    bound = uk == -1
    assert np.all(ub[~bound] == ex[~bound]) and np.all(uk[~bound] == ek[~bound])
    assert np.all(ub[bound] >= ex[bound])
    if bound.any() and kind in ('planted', 'noise'):
        rel = ub[bound].astype(np.float64) / np.maximum(ex[bound].astype(np.float64), 1e-30) - 1.0
        print('%s W=%d: ub/exact - 1 median %.3g max %.3g' % (kind, W, np.median(rel), rel.max()))


def test_out_of_model_chunks_are_exact():
    """A chunk with a non-finite or out-of-range sample runs the exact tile: its positions hold exact scores."""
    x, D = _family('noise', 2, 6000, 64, 64, 3)
    x[0, 100] = np.inf
    x[1, 4100] = 1e-30
    eng = _engine(D, None)
    ub, uk, _ = _init_state(eng, x, False, 8)
    ex, ek, _ = _init_state(eng, x, True, 8)
    assert np.all(uk[0, :2048] >= 0) and np.all(uk[1, 4096:] >= 0)
    same = uk >= 0
    assert np.array_equal(ub[same].view(np.int32), ex[same].view(np.int32)) and np.array_equal(uk[same], ek[same])
    assert np.all(ub[~same] >= ex[~same])


def _encode_all(eng, x, params, exact, quad=None, rounds=None, scramble=None):
    from hsc_amd import _native
    with _env(HSCMP_EXACT_INIT='1' if exact else None, HSCMP_MFMA_QUAD=quad):
        if rounds is None:
            eng.encode_batch(x[:, :, None], params)
        else:
            xd = np.array(x)
            eng.encode_batch(xd[:, :, None], params)
            for _ in range(2000):
                if scramble is not None:
                    xd[:] = scramble                     # the caller's buffer changes between rounds
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


@pytest.mark.parametrize('kind', FAMILIES)
@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_encode_identity(kind, shape, weights):
    from hsc_amd import _native
    B, T, K, W = SHAPES[shape]
    x, D = _family(kind, B, T, K, W, 31 + shape)
    w = (0.5 + np.random.RandomState(shape).random_sample(K)).astype(np.float32) if weights else None
    eng = _engine(D, w)
    params = _native.make_params(nbNonzeroCoefs=40, eps=1e-30, maxEvents=4096)
    a = _encode_all(eng, x, params, False)
    b = _encode_all(eng, x, params, True)
    assert a['variant'].startswith('mfma_init+mfma_loop_f32_bound'), a['variant']
    assert '_bound' not in b['variant']
    _same(a, b)


@pytest.mark.parametrize('kind', ['planted', 'noise', 'repeated'])
def test_encode_identity_four_signals(kind):
    """GS = 4 (four signals per workgroup) needs more signals than two per CU: 600 short signals."""
    from hsc_amd import _native
    x, D = _family(kind, 600, 2000, 64, 64, 5)
    eng = _engine(D, None)
    params = _native.make_params(nbNonzeroCoefs=30, eps=1e-30, maxEvents=1024)
    a = _encode_all(eng, x, params, False, quad='1')
    b = _encode_all(eng, x, params, True, quad='1')
    c = _encode_all(eng, x, params, False, quad='0')
    assert a['variant'] == 'mfma_init+mfma_loop_f32_bound_x4', a['variant']
    _same(a, b)
    _same(a, c)


@pytest.mark.parametrize('kind', ['planted', 'noise'])
def test_resumed_encode_identity(kind):
    from hsc_amd import _native
    x, D = _family(kind, 4, 6000, 96, 64, 7)
    eng = _engine(D, None)
    params = _native.make_params(toleranceSnr=20.0, eps=1e-30, maxEvents=4096, maxRounds=7)
    a = _encode_all(eng, x, params, False, rounds=5, scramble=np.float32(123.0))
    b = _encode_all(eng, x, params, True, rounds=5)
    full = _encode_all(eng, x, _native.make_params(toleranceSnr=20.0, eps=1e-30, maxEvents=4096), True)
    _same(a, b)
    _same(a, full)


def test_non_finite_inputs_identity():
    from hsc_amd import _native
    x, D = _family('planted', 3, 5000, 64, 64, 9)
    x[0, 2500] = np.nan
    x[1, 10] = np.inf
    x[2, 4000:4100] = 3e38
    eng = _engine(D, None)
    params = _native.make_params(nbNonzeroCoefs=30, eps=1e-30, maxEvents=4096)
    a = _encode_all(eng, x, params, False)
    b = _encode_all(eng, x, params, True)
    _same(a, b)


def test_config2_batch_identity():
    """One full config-2 batch (1024 x 65536, 256 x 64, L0 = 256), bound pass against the exact pass."""
    from hsc_amd import _native
    import hsc_amd.synth as synth
    D = synth.make_dictionary(256, 64, seed=2)
    x = np.stack([synth.make_signal(D, 65536, b, kind='planted', nb_atoms=256, seed=2) for b in range(1024)]).astype(np.float32)
    eng = _engine(D, None)
    params = _native.make_params(nbNonzeroCoefs=256, eps=1e-30, maxEvents=1024)
    a = _encode_all(eng, x, params, False)
    b = _encode_all(eng, x, params, True)
    _same(a, b)
