"""The four-signal loop's tile with one bf16 product per tap (MfmaRecorr with BOUND, bound_tile<SB, HAS_W>; csrc/hscmp_bound.h,
DESIGN.md section 11): a bound written by the LOOP whose slack is nearly used up.

The `tight` dictionary of tests/test_gpu_bound_products.py (every magnitude just under a bf16 rounding midpoint, m = 128: the
largest relative rounding error a bf16 has) with one atom replaced by a trigger whose taps are zero over its second half.
Each signal holds a large multiple of the trigger at p and 4 D[k] as the whole window of row t = p + W/2.  The trigger is the
first selection; its support overlaps the window of row t only where its taps are zero, so the subtraction leaves the tight
window's samples bit for bit, and the tile of the atom at p re-correlates row t: the hi.hi sum of a window that is a multiple
of an atom, both factors of every product rounded towards zero, an error within 2 % of the slack kBoundEps1 ||xh_win|| cmax
(tests/test_bound_one_product.py works the figure out).  After ONE selection (maxRounds = 1) row t must hold a bound
(best_k == -1) that is at least the exact score of the HSCMP_EXACT_INIT=1 state.  HSCMP_MFMA_QUAD=1 forces the four-signal
loop, the only one with the bound form.  No case carries a tolerance.

The construction selects the trigger first at all three shapes, with and without weights (asserted: the first event is the
trigger at p); with weights the trigger's own weight is the largest of the range the helper draws from, 1.5, so that no tight
atom outranks it through its weight alone.

Mutation tried against this file (a scratch build, run once): with kBoundEps1 halved all six cases fail on `ub >= exact`, at
W = 64, 32 and 16, with and without weights (W = 64 without weights: the loop wrote 4.0159 where the exact score is 4.0313).
On the real constant the printed ub/exact - 1 at the tight rows is 1.4e-4 without weights and 1.4e-4 .. 1.5e-2 with them
(cmax is the largest ||d_k|| |w_k| of the dictionary, not the planted atom's).  All three shapes select the trigger first."""
import numpy as np
import pytest

from test_gpu_bound_products import _under_midpoint
from test_gpu_loop_bounds import _encode, _engine, _weights

pytestmark = pytest.mark.gpu

SHAPES = [(4, 2000, 64, 64), (4, 1500, 40, 32), (4, 1200, 20, 16)]      # SB = 4, 2, 1; K not a multiple of 32
TRIGGER = 5
AMPLITUDE = 64.0


def _case(B, T, K, W, weights, seed):
    import hsc_amd.synth as synth
    rs = np.random.RandomState(seed)
    D = _under_midpoint(rs, (K, W), True) * rs.choice(np.float32([-1.0, 1.0]), size=(K, W))
    D[TRIGGER, W // 2:] = 0.0
    D = np.ascontiguousarray(D, dtype=np.float32)
    w = _weights(K, weights, seed)
    if w is not None:
        w[TRIGGER] = 1.5
    x = np.zeros((B, T), dtype=np.float32)
    ps, ts, ks = [], [], []
    for b in range(B):
        p = 300 + 211 * b
        t = p + W // 2
        k = (7 + 3 * b) % K
        assert k != TRIGGER
        ws = t - (W - 1) // 2                                   # first sample of row t's window
        x[b, ws: ws + W] = np.float32(4.0) * D[k]
        s, e, es, ee = synth.centered_span(T, W, p)
        assert e - s == W and np.all(D[TRIGGER][np.arange(es, ee)[np.arange(s, e) >= ws]] == 0.0)
        x[b, s:e] += np.float32(AMPLITUDE) * D[TRIGGER][es:ee]   # (zero taps where the two overlap: the sum is exact)
        assert np.array_equal(x[b, ws: ws + W], np.float32(4.0) * D[k])
        ps.append(p); ts.append(t); ks.append(k)
    return x, D, w, np.array(ps), np.array(ts), np.array(ks)


def _state_after_one(eng, x, params, mode):
    out = _encode(eng, x, params, mode)
    v = eng.device_view()
    B, T = x.shape
    return out, eng.copy_from_device(v.best_c, (B, T), np.float32), eng.copy_from_device(v.best_k, (B, T), np.int32)


@pytest.mark.parametrize('weights', [False, True])
@pytest.mark.parametrize('shape', range(len(SHAPES)))
def test_loop_bound_nearly_attained(shape, weights):
    from hsc_amd import _native
    B, T, K, W = SHAPES[shape]
    x, D, w, ps, ts, ks = _case(B, T, K, W, weights, 60 + shape)
    eng = _engine(D, w)
    params = _native.make_params(nbNonzeroCoefs=8, eps=1e-30, maxEvents=64, maxRounds=1)
    a, ub, uk = _state_after_one(eng, x, params, 'bound')
    e, ex, ek = _state_after_one(eng, x, params, 'exact')
    assert a['variant'] == 'mfma_init+mfma_loop_f32_bound_x4', a['variant']
    assert '_bound' not in e['variant']
    for out in (a, e):                                          # one selection each: the trigger at p
        assert np.all(out['stats'][:, _native.STAT_EVENTS] == 1)
        assert np.array_equal(out['t'][:, 0], ps) and np.all(out['k'][:, 0] == TRIGGER)
    assert np.array_equal(a['residual'].view(np.int32), e['residual'].view(np.int32))
    rows = np.arange(B)
    ws = ts - (W - 1) // 2
    for b in range(B):                                          # the tight window came through the subtraction bit for bit
        assert np.array_equal(a['residual'][b].reshape(-1)[ws[b]: ws[b] + W], np.float32(4.0) * D[ks[b]])
    assert np.all(ek[rows, ts] >= 0)
    rel = ub[rows, ts].astype(np.float64) / ex[rows, ts].astype(np.float64) - 1.0
    print('W=%d weights=%d: loop-written ub/exact - 1 at the tight rows: %s' % (W, weights, rel))
    assert np.all(uk[rows, ts] == -1), uk[rows, ts]
    assert np.all(ub[rows, ts] >= ex[rows, ts]), (ub[rows, ts], ex[rows, ts])
