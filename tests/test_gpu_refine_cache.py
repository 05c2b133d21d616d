"""The bound loop's cache of committed refines (MfmaRecorr::cache_commit): whole encodes, bit for bit,
against HSCMP_EXACT_INIT=1 (both passes exact) and HSCMP_EXACT_RECORR=1 (exact loop behind the bound pass) -- events, slots,
stats, energies, residual.  HSCMP_MFMA_QUAD=1 forces the four-signal loop, the only one with the bound form.  No case
carries a tolerance, and the tests assert identity only.

A selection refines the bound that leads; a refined position that does not win is committed to memory with its exact score,
and its (k, c) go to the signal's cache (64 entries).  The selection it wins later takes them from there.  The inputs are
built so that winners come from the cache:

(a) atoms planted far apart with amplitudes 1 % apart (the step the one-product slack of 2^-7 just about covers) and
    0.3 % apart (several steps inside the slack): every selection refines the next candidates, and its winner is an
    older refine;
(b) two overlapping planted atoms, q and q + d, and a third far away, their exact scores 0.3 % apart: the first selection
    refines all three and commits q and q + d, the second takes q from the cache and applies it within W - 1 of the cached
    q + d, whose entry must be dropped -- the overlap changes that row's (k, c).  d = 1, W/2, W - 1 (the last re-correlated
    row) and W (the first row outside: the entry stays);
(c) noise, T = 6000: the first selections refine more positions than the cache holds (the ring overwrites live entries,
    whose winners then resolve from window and hint);
(d) atoms at both signal ends (the `ends` family: the stale row T-1 with even W);
(e) a resumed encode, maxRounds = 3, the caller's buffer scrambled between the rounds: every launch starts with an empty
    cache."""
import numpy as np
import pytest

from test_gpu_loop_bounds import _encode, _engine, _family, _identity, _same, _weights

pytestmark = pytest.mark.gpu

SHAPES = [(6, 5000, 256, 64), (6, 3000, 40, 32), (5, 2500, 50, 57)]


def _plant(x, b, D, k, p, amp):
    import hsc_amd.synth as synth
    s, e, es, ee = synth.centered_span(x.shape[1], D.shape[1], p)
    x[b, s:e] += amp * D[k].astype(np.float64)[es:ee]


def _steps(B, T, K, W, step, seed, w=None):
    """One atom per position, 4W apart, scores 2 (1 + step)^j (the weight divided out of the amplitude) in an order that
    differs from signal to signal."""
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed)
    rs = np.random.RandomState(seed)
    x = 1e-5 * rs.standard_normal((B, T))
    pos = np.arange(2 * W, T - 2 * W, 4 * W)
    for b in range(B):
        order = rs.permutation(len(pos))
        for j, i in enumerate(order):
            k = (3 * i + b) % K
            _plant(x, b, D, k, pos[i], 2.0 * (1.0 + step) ** j / (1.0 if w is None else float(w[k])))
    return np.ascontiguousarray(x, dtype=np.float32), D


def _overlapping(B, T, K, W, seed, w=None):
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed)
    Dd = D.astype(np.float64)
    rs = np.random.RandomState(seed)
    x = 1e-5 * rs.standard_normal((B, T))
    gaps = [1, W // 2, W - 1, W]
    for b in range(B):
        for j in range(3):                                      # three groups per signal, the scores of a group 0.3 % apart
            d = gaps[(b + j) % len(gaps)]
            q = 3 * W + j * (T // 3)
            k1, k2, kz = (5 + 7 * b + j) % K, (11 + 3 * b + 2 * j) % K, (23 + b + 5 * j) % K
            # exact chains of k1 at q and of k2 at q + d as functions of the two amplitudes: a 2 x 2 system
            g12 = float(np.dot(Dd[k1][d:], Dd[k2][:W - d])) if d < W else 0.0
            n1, n2 = float(np.dot(Dd[k1], Dd[k1])), float(np.dot(Dd[k2], Dd[k2]))
            top = 3.0 + j                                       # (scores: the chain times the atom's weight)
            w1, w2, wz = (1.0, 1.0, 1.0) if w is None else (float(w[k1]), float(w[k2]), float(w[kz]))
            a1, a2 = np.linalg.solve(np.array([[n1, g12], [g12, n2]]), np.array([top / w1, 0.997 * top / w2]))
            _plant(x, b, D, k1, q, a1)
            _plant(x, b, D, k2, q + d, a2)
            _plant(x, b, D, kz, q + 6 * W, 1.003 * top / (wz * float(np.dot(Dd[kz], Dd[kz]))))
    return np.ascontiguousarray(x, dtype=np.float32), D


def _params(L0=60, **kw):
    from hsc_amd import _native
    return _native.make_params(nbNonzeroCoefs=L0, eps=1e-30, maxEvents=4096, **kw)


@pytest.mark.parametrize('step', [1e-2, 3e-3])
@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_winners_are_older_refines(shape, weights, step):
    B, T, K, W = SHAPES[shape]
    w = _weights(K, weights, shape)
    x, D = _steps(B, T, K, W, step, 70 + shape, w)
    _identity(x, D, w, _params(40))


@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_atom_beside_a_cached_position(shape, weights):
    B, T, K, W = SHAPES[shape]
    w = _weights(K, weights, shape)
    x, D = _overlapping(B, T, K, W, 80 + shape, w)
    _identity(x, D, w, _params(40))


@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_more_live_entries_than_the_cache_holds(shape, weights):
    B, _, K, W = SHAPES[shape]
    x, D = _family('noise', B, 6000, K, W, 90 + shape)
    _identity(x, D, _weights(K, weights, shape), _params(120))


@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_both_signal_ends(shape, weights):
    B, T, K, W = SHAPES[shape]
    x, D = _family('ends', B, T, K, W, 100 + shape)
    _identity(x, D, _weights(K, weights, shape), _params(60))


@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_resumed_encode_starts_cold(shape, weights):
    B, T, K, W = SHAPES[shape]
    w = _weights(K, weights, shape)
    x, D = _steps(B, T, K, W, 3e-3, 110 + shape, w)
    eng = _engine(D, w)
    a = _encode(eng, x, _params(40, maxRounds=3), 'bound', rounds=3, scramble=np.float32(123.0))
    b = _encode(eng, x, _params(40, maxRounds=3), 'exact', rounds=3)
    c = _encode(eng, x, _params(40, maxRounds=3), 'exact_recorr', rounds=3, scramble=np.float32(-7.0))
    full = _encode(eng, x, _params(40), 'bound')
    assert full['variant'] == 'mfma_init+mfma_loop_f32_bound_x4', full['variant']
    _same(a, b)
    _same(a, c)
    _same(a, full)
