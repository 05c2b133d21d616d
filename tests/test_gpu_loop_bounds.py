"""The bound re-correlation of the four-signal loop (MfmaRecorr with BOUND) on the GPU.

The loop writes upper bounds (best_k == -1) for the rows it re-correlates and refines a row only when it wins a
selection.  HSCMP_MFMA_QUAD=1 forces the four-signal loop, the only one with the bound form.

1. Validity: after a limited-round encode the state holds, where best_k >= 0, exactly the HSCMP_EXACT_INIT=1 state, and
   elsewhere at least as much; the loop did write bounds (HSCMP_EXACT_RECORR=1 leaves none in re-correlated rows).
2. Identity: whole encodes against HSCMP_EXACT_INIT=1 (both passes exact) and HSCMP_EXACT_RECORR=1 (exact loop behind
   the bound pass), bit for bit: input families with and without weights, K not a multiple of 32, odd and even W, atoms
   at both signal ends (the stale row T-1 with even W), samples outside the model inside planted atoms' windows,
   resumed encodes with the caller's buffer scrambled, one full config-2 batch."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = {'bound': {}, 'exact': {'HSCMP_EXACT_INIT': '1'}, 'exact_recorr': {'HSCMP_EXACT_RECORR': '1'}}


class _env(object):
    def __init__(self, kv):
        self.kv = dict(kv)

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


def _weights(K, on, seed):
    return (0.5 + np.random.RandomState(seed).random_sample(K)).astype(np.float32) if on else None


def _family(kind, B, T, K, W, seed):
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed)
    rs = np.random.RandomState(seed)
    if kind == 'planted':
        x = np.stack([synth.make_signal(D, T, b, kind='planted', nb_atoms=max(4, T // 100), noise=0.05, seed=seed) for b in range(B)])
    elif kind == 'noise':
        x = rs.standard_normal((B, T))
    elif kind == 'repeated':            # one atom repeated: many tied scores
        x = np.zeros((B, T))
        for p in range(W, T - W, 3 * W):
            x[:, p: p + W] += D[1 % K]
    elif kind == 'ends':                # strong atoms at both ends, p = T-1-W among them (the stale row with even W)
        x = 0.01 * rs.standard_normal((B, T))
        for b in range(B):
            for j, p in enumerate([0, 1, W // 2, T - 1, T - 2, T - 1 - W, T - 1 - W + b % 3, T - 1 - W // 2, 2 * W]):
                s, e, es, ee = synth.centered_span(T, W, p)
                x[b, s:e] += (4.0 + j + b) * D[(j + b) % K][es:ee]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32), D


def _encode(eng, x, params, mode, rounds=None, scramble=None):
    from hsc_amd import _native
    with _env(dict(MODES[mode], HSCMP_MFMA_QUAD='1')):
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


def _identity(x, D, w, params, **kw):
    eng = _engine(D, w)
    a = _encode(eng, x, params, 'bound', **kw)
    b = _encode(eng, x, params, 'exact', **kw)
    c = _encode(eng, x, params, 'exact_recorr', **kw)
    assert a['variant'] == 'mfma_init+mfma_loop_f32_bound_x4', a['variant']
    assert c['variant'] == a['variant']
    assert '_bound' not in b['variant']
    _same(a, b)
    _same(a, c)


SHAPES = [(8, 5000, 256, 64), (8, 4500, 100, 63), (6, 3000, 40, 32), (6, 7000, 33, 31), (6, 3000, 20, 16), (5, 2500, 50, 57)]


def _state(eng, x, params, mode):
    _encode(eng, x, params, mode)
    v = eng.device_view()
    B, T = x.shape
    return eng.copy_from_device(v.best_c, (B, T), np.float32), eng.copy_from_device(v.best_k, (B, T), np.int32)


@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('kind', ['planted', 'noise'])
def test_loop_bounds_are_valid(shape, kind):
    from hsc_amd import _native
    B, T, K, W = SHAPES[shape]
    x, D = _family(kind, B, T, K, W, 21 + shape)
    eng = _engine(D, _weights(K, shape % 2 == 1, shape))
    params = _native.make_params(nbNonzeroCoefs=200, eps=1e-30, maxEvents=4096, maxRounds=25)
    ub, uk = _state(eng, x, params, 'bound')
    t, _, _ = eng.fetch_events()
    nev = eng.fetch_stats()[:, _native.STAT_EVENTS]
    ex, ek = _state(eng, x, params, 'exact')
    rb, rk = _state(eng, x, params, 'exact_recorr')
    assert np.all(ek >= 0)
    same = uk >= 0
    assert np.array_equal(ub[same].view(np.int32), ex[same].view(np.int32)) and np.array_equal(uk[same], ek[same])
    assert np.all(ub[~same] >= ex[~same])
    # the rows the loop re-correlated: bounds with the bound loop, exact scores behind HSCMP_EXACT_RECORR=1
    rows = np.zeros_like(same)
    for b in range(B):
        for p in t[b, :nev[b]]:
            rows[b, max(0, p - (W - 1)): p + W] = True
    assert np.all(rk[rows] >= 0)
    assert np.count_nonzero(uk[rows] == -1) > rows.sum() // 2


@pytest.mark.parametrize('kind', ['planted', 'noise', 'repeated', 'ends'])
@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_encode_identity(kind, shape, weights):
    from hsc_amd import _native
    B, T, K, W = SHAPES[shape]
    x, D = _family(kind, B, T, K, W, 41 + shape)
    params = _native.make_params(nbNonzeroCoefs=60, eps=1e-30, maxEvents=4096)
    _identity(x, D, _weights(K, weights, shape), params)


@pytest.mark.parametrize('value', [np.inf, -np.inf, np.nan, 1e-30, 3e38, 2.0 ** 61])
def test_out_of_model_samples_in_atom_windows(value):
    """Samples outside the model inside the windows of planted atoms: those tiles run the exact float32 tile."""
    from hsc_amd import _native
    import hsc_amd.synth as synth
    B, T, K, W = 6, 4000, 64, 64
    D = synth.make_dictionary(K, W, seed=3)
    x = np.stack([synth.make_signal(D, T, b, kind='planted', nb_atoms=30, noise=0.01, seed=3, return_events=False) for b in range(B)])
    for b in range(B):
        p = 500 + 400 * b
        s, e, es, ee = synth.centered_span(T, W, p)
        x[b, s:e] += 6.0 * D[b][es:ee]
        x[b, p + 20 + b] = value                    # inside the re-correlated rows' windows of the atom at p
    x = np.ascontiguousarray(x, dtype=np.float32)
    params = _native.make_params(nbNonzeroCoefs=40, eps=1e-30, maxEvents=4096)
    _identity(x, D, None, params)


@pytest.mark.parametrize('kind', ['planted', 'ends'])
def test_resumed_encode_identity(kind):
    from hsc_amd import _native
    x, D = _family(kind, 8, 6000, 96, 64, 7)
    params = _native.make_params(toleranceSnr=20.0, eps=1e-30, maxEvents=4096, maxRounds=7)
    eng = _engine(D, None)
    a = _encode(eng, x, params, 'bound', rounds=5, scramble=np.float32(123.0))
    b = _encode(eng, x, params, 'exact', rounds=5)
    c = _encode(eng, x, params, 'exact_recorr', rounds=3, scramble=np.float32(-7.0))
    full = _encode(eng, x, _native.make_params(toleranceSnr=20.0, eps=1e-30, maxEvents=4096), 'bound')
    _same(a, b)
    _same(a, c)
    _same(a, full)


def test_config2_batch_identity():
    """One full config-2 batch (1024 x 65536, 256 x 64, L0 = 256): the bound loop against both exact forms."""
    from hsc_amd import _native
    import hsc_amd.synth as synth
    D = synth.make_dictionary(256, 64, seed=2)
    x = np.stack([synth.make_signal(D, 65536, b, kind='planted', nb_atoms=256, seed=2) for b in range(1024)]).astype(np.float32)
    params = _native.make_params(nbNonzeroCoefs=256, eps=1e-30, maxEvents=1024)
    _identity(x, D, None, params)
