"""The bound loop's refine, shared by the signal's four waves (MfmaRecorr::refine with BOUND).

Wave q of a signal computes the pinned chains of the atoms 64 q + lane + 256 j, the four waves exchange one record each
(largest score, lowest atom attaining it, its coefficient) and merge them alike; the atom body then takes (k, c) from
that record instead of resolving them again.  Whole encodes, bit for bit, against HSCMP_EXACT_INIT=1 (both passes
exact, every wave for itself), with HSCMP_MFMA_QUAD=1 (the four-signal loop, the only one with the bound form).  Every
case asserts that the bound loop ran.  No case carries a tolerance.

* K around the waves' shares (idle waves and lanes in the merge), W = 64 and 31, with and without weights;
* one atom at two indices in different waves' shares: the tie goes to the lower index;
* more refines in one selection than the list holds (the full-list path together with the alternating slots);
* a resumed encode, stopped and restarted every few selections;
* a coefficient threshold that ends the encode on a null coefficient (the handed-over c meets the null test);
* one full-length batch."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUND_X4 = 'mfma_init+mfma_loop_f32_bound_x4'


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


def _engine(D, w=None):
    from hsc_amd import _native
    eng = _native.Engine(0)
    eng.set_dictionary(D, weights=w)
    return eng


def _weights(K, on, seed):
    return (0.5 + np.random.RandomState(seed).random_sample(K)).astype(np.float32) if on else None


def _planted(D, B, T, nb_atoms, seed, noise=0.05):
    import hsc_amd.synth as synth
    return np.ascontiguousarray(np.stack([synth.make_signal(D, T, b, kind='planted', nb_atoms=nb_atoms, noise=noise, seed=seed)
                                          for b in range(B)]), dtype=np.float32)


def _encode(eng, x, params, exact, rounds=None):
    from hsc_amd import _native
    with _env({'HSCMP_MFMA_QUAD': '1', 'HSCMP_EXACT_INIT': '1' if exact else None, 'HSCMP_EXACT_RECORR': None, 'HSCMP_INIT_ONLY': None}):
        eng.encode_batch(x[:, :, None], params)
        if rounds is not None:
            for _ in range(4000):
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
    a = _encode(eng, x, params, False, **kw)
    b = _encode(eng, x, params, True, **kw)
    assert a['variant'] == BOUND_X4, a['variant']
    assert '_bound' not in b['variant'], b['variant']
    _same(a, b)
    return a


def _init_state(eng, x, exact):
    """best_c / best_k behind the initial correlation alone"""
    from hsc_amd import _native
    with _env({'HSCMP_MFMA_QUAD': '1', 'HSCMP_INIT_ONLY': '1', 'HSCMP_EXACT_INIT': '1' if exact else None}):
        eng.encode_batch(x[:, :, None], _native.make_params(nbNonzeroCoefs=8, eps=1e-30, maxEvents=64))
    v = eng.device_view()
    B, T = x.shape
    return eng.copy_from_device(v.best_c, (B, T), np.float32), eng.copy_from_device(v.best_k, (B, T), np.int32)


# K: one wave's share and less (31, 64), one atom into the second wave (65), two shares less one (127), three full shares
# (192), all but one atom (255), one chain per lane (256).  Six signals: one full workgroup and a ragged one.
@pytest.mark.parametrize('weights', [False, True])
@pytest.mark.parametrize('W', [64, 31])
@pytest.mark.parametrize('K', [31, 64, 65, 127, 192, 255, 256])
def test_wave_shares(K, W, weights):
    from hsc_amd import _native
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=100 + K)
    x = _planted(D, 6, 3000, 40, seed=K + W)
    params = _native.make_params(nbNonzeroCoefs=60, eps=1e-30, maxEvents=4096)
    _identity(x, D, _weights(K, weights, K), params)


@pytest.mark.parametrize('copies', [(5, 70), (70, 130), (63, 64, 255), (1, 129, 193)])
def test_tie_between_waves_goes_to_the_lower_atom(copies):
    """The same atom at indices that fall into different waves' shares, planted strongly: every wave that holds a copy reports
    the same score, and the merge keeps the lowest index."""
    from hsc_amd import _native
    import hsc_amd.synth as synth
    K, W, B, T = 256, 64, 5, 4000
    D = synth.make_dictionary(K, W, seed=9)
    for kk in copies[1:]:
        D[kk] = D[copies[0]]
    rs = np.random.RandomState(3)
    x = 0.01 * rs.standard_normal((B, T))
    planted = [200 + 333 * j for j in range(10)]
    for b in range(B):
        for j, p in enumerate(planted):
            s, e, es, ee = synth.centered_span(T, W, p)
            x[b, s:e] += (5.0 + 0.25 * j + b) * D[copies[0]].astype(np.float64)[es:ee]
    x = np.ascontiguousarray(x, dtype=np.float32)
    a = _identity(x, D, None, _native.make_params(nbNonzeroCoefs=30, eps=1e-30, maxEvents=4096))
    nev = a['stats'][:, _native.STAT_EVENTS]
    for b in range(B):
        t, k = a['t'][b, :nev[b]], a['k'][b, :nev[b]]
        first = {p: k[np.nonzero(t == p)[0][0]] for p in planted}      # every planted position is selected
        assert all(v == copies[0] for v in first.values()), first
        assert not np.any(np.isin(k, copies[1:]))


def test_more_refines_than_the_list_holds():
    """Eight copies of one atom at equal amplitude, far apart, nothing else: the eight positions hold the same bound and the
    same exact score, so the first selection refines all eight before its winner is exact -- a fifth refine commits the
    full list behind two barriers and the exchange goes through both slot sets several times within one selection."""
    from hsc_amd import _native
    import hsc_amd.synth as synth
    K, W, B, T = 256, 64, 5, 4000
    D = synth.make_dictionary(K, W, seed=5)
    x = np.zeros((B, T))
    for b in range(B):
        for j in range(8):
            s, e, es, ee = synth.centered_span(T, W, 300 + 450 * j + 7 * b)
            x[b, s:e] += (3.0 + b) * D[17 + 50 * b].astype(np.float64)[es:ee]
    x = np.ascontiguousarray(x, dtype=np.float32)
    eng = _engine(D)
    ub, uk = _init_state(eng, x, False)
    ex, ek = _init_state(eng, x, True)
    assert np.all(ek >= 0)
    for b in range(B):
        above = np.count_nonzero((uk[b] == -1) & (ub[b] > ex[b].max()))
        print('signal %d: %d positions hold a bound above the largest exact score' % (b, above))
        assert above > 4, above
    _identity(x, D, None, _native.make_params(nbNonzeroCoefs=24, eps=1e-30, maxEvents=4096))


@pytest.mark.parametrize('rounds', [1, 3])
def test_resumed_every_few_selections(rounds):
    from hsc_amd import _native
    import hsc_amd.synth as synth
    D = synth.make_dictionary(200, 64, seed=12)
    x = _planted(D, 7, 5000, 50, seed=12)
    params = _native.make_params(nbNonzeroCoefs=45, eps=1e-30, maxEvents=4096, maxRounds=rounds)
    a = _identity(x, D, None, params, rounds=rounds)
    full = _encode(_engine(D), x, _native.make_params(nbNonzeroCoefs=45, eps=1e-30, maxEvents=4096), False)
    assert full['variant'] == BOUND_X4
    _same(a, full)


@pytest.mark.parametrize('weights', [False, True])
def test_ends_on_a_null_coefficient(weights):
    """A coefficient threshold above the noise: the planted atoms go, then a selection's coefficient -- handed over by the
    refine -- fails the null test and the encode stops as 'empty'."""
    from hsc_amd import _native
    import hsc_amd.synth as synth
    K, W = 192, 64
    D = synth.make_dictionary(K, W, seed=8)
    x = _planted(D, 6, 4000, 12, seed=8, noise=0.01)
    params = _native.make_params(minCoefficients=0.2, eps=1e-30, maxEvents=4096)
    a = _identity(x, D, _weights(K, weights, 4), params)
    stop = a['stats'][:, _native.STAT_STOP]
    assert np.all(stop == 5), stop                         # 'empty' (STOP_NAMES)
    assert np.all(a['stats'][:, _native.STAT_EVENTS] > 0)


def test_full_length_batch():
    """T = 65536, 8 signals, 256 selections: about 2 000 exchanges per workgroup, four signals out of step."""
    from hsc_amd import _native
    import hsc_amd.synth as synth
    D = synth.make_dictionary(256, 64, seed=2)
    x = np.ascontiguousarray(synth.make_batch(D, 65536, 0, 8, kind='planted', nb_atoms=256, seed=2), dtype=np.float32)
    a = _identity(x, D, None, _native.make_params(nbNonzeroCoefs=256, eps=1e-30, maxEvents=1024))
    assert np.all(a['stats'][:, _native.STAT_EVENTS] >= 256)
