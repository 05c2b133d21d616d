"""libhscnmf (ConvolutionalNMF and ConvolutionalNMFLearner) at the edges of its launch plans, against the float64
restatements: K across the MFMA k-groups of 8 and the learner's nmf_dpart_kernel K blocks (RB = 32 f32 / 16 f64), W*F
across the column blocks (CB = 32 f32 / 16 f64) and the LDS slabs, halos of W-1 rows wider than the 128-row tile,
L = T-W+1 around multiples of 128, and the largest W and F that lds_plan accepts, with the first ones it refuses.

Positive data, dictionaries and initial coefficients (|recon| stays far from 0), explicit initial values, 1 to 3
iterations.  float64 runs match the restatement to 1e-10 relative; a float32 run stays within 4x the round-off spread
of the restatement in numpy float32 arithmetic, plus 1e-6 of the largest value.  The LDS limits are restated from the
launch code and checked on the CPU; the GPU tests run the last accepted shapes and expect the first refused ones to
fail with HSCNMF_ERR_UNSUPPORTED."""
import numpy as np
import pytest

from hsc_amd import _native
from tests import nmf_learn_restatement as lrst
from tests import nmf_restatement as rst

# ---- the LDS limits, restated from hscnmf.hip (lds_plan, and learn_t's lds_part / lds_upd) ----------------------------
ROWS = 128                  # kRows: A rows / reconstructed samples per workgroup
THREADS = 256               # kThreads
LDS_BYTES = 64 * 1024       # kLdsBytes
TILE = {4: (32, 32), 8: (16, 16)}   # itemsize -> (RB, CB): v_mfma_f32_32x32x2f32 / v_mfma_f64_16x16x4f64 blocks


def coder_fits(W, F, itemsize):
    """lds_plan: the reconstruction tile [ROWS][F], then a slab of column blocks of the P rows, PR = ROWS + W - 1 rounded
    up to RB, CB columns each.  One column block must fit beside the tile, and the slab (at least one block) must hold
    the residual kernel's 2 * THREADS doubles of reduction scratch."""
    RB, CB = TILE[itemsize]
    PR = (ROWS + W - 1 + RB - 1) // RB * RB
    rec, col = ROWS * F * itemsize, PR * CB * itemsize
    if rec + col > LDS_BYTES:
        return False
    ncb = (W * F + CB - 1) // CB
    slab = max(1, min(ncb, (LDS_BYTES - rec) // col))
    return rec + max(col * slab, 2 * THREADS * 8) <= LDS_BYTES


def learner_fits(W, F, itemsize):
    """The coder's plan, and the learner's own kernels: nmf_dpart_kernel stages the R samples of a row tile and its halo,
    (ROWS + W - 1) * F values; nmf_dupdate_kernel holds THREADS sums of squares and the W * F + 1 sums of an atom."""
    return (coder_fits(W, F, itemsize) and (ROWS + W - 1) * F * itemsize <= LDS_BYTES
            and (THREADS + W * F + 1) * itemsize <= LDS_BYTES)


def first_unsupported_W(fits, itemsize, F=1):
    W = 2
    while fits(W, F, itemsize):
        W += 1
    return W


def first_unsupported_F(fits, itemsize, W=2):
    F = 1
    while fits(W, F, itemsize):
        F += 1
    return F


# ---- shapes: (K, W, F, T, iterations); L = T - W + 1 coefficient rows, ceil(L/128) row tiles, ceil(T/128) sample tiles
COMMON = [
    (1, 2, 1, 100, 3),      # K = 1: one k of the masked (K % 8) path; L = 99 < 128; three iterations
    (7, 2, 3, 130, 2),      # K = 7 masked; L = 129: the second row tile holds one row
    (8, 5, 1, 130, 2),      # K = 8: one full k-group; L = 126: one row tile but two sample tiles (the 2nd has no rows)
    (9, 33, 1, 160, 2),     # K = 9: a second, masked k-group; L = 128 exactly; W*F = 33: 2 column blocks f32, 3 f64
    (31, 33, 3, 288, 1),    # K = 31: one dpart K block f32, two f64; W*F = 99; L = 256
    (32, 127, 1, 382, 1),   # K = 32: 4 full k-groups, one full dpart K block f32 (2 f64); W = 127: 126 halo rows; L = 256
    (33, 128, 1, 384, 1),   # K = 33: two dpart K blocks f32 (3 f64), the last of one atom; W = 128: PR = 256; L = 257
    (48, 129, 1, 300, 1),   # W = 129: a halo of 128 rows, as wide as the tile; K = 48: 2 K blocks f32, 3 f64
    (64, 200, 1, 456, 1),   # W = 200: the halo wider than the tile; K = 64: 2 K blocks f32, 4 f64; L = 257
    (16, 2, 16, 257, 2),    # F = 16; W*F = 32: one full column block f32, two f64; L = 256
    (8, 3, 40, 200, 2),     # F = 40: a 20 KB (f32) / 40 KB (f64) reconstruction tile, one column block per slab in f64
    (33, 33, 16, 300, 1),   # W*F = 528: 17 column blocks f32, 33 f64, in slabs of 2; K = 33
    (7, 129, 3, 260, 1),    # W > 128 and F = 3: W*F = 387, one column block per slab pass; L = 132
    (9, 200, 2, 330, 1),    # W = 200, F = 2: 13 / 25 single-block passes; L = 131: 2 row tiles, 3 sample tiles
    (1, 128, 1, 128, 2),    # T = W: L = 1, a single coefficient row
    (64, 9, 4, 520, 1),     # L = 512 = 4 * 128: four full row tiles, a fifth sample tile; K = 64 with F = 4
]


def _limit_rows(fits, itemsize):
    Wmax, Fmax = first_unsupported_W(fits, itemsize) - 1, first_unsupported_F(fits, itemsize) - 1
    return [(3, Wmax, 1, Wmax + 129, 1),     # the largest W at F = 1: L = 130
            (5, 2, Fmax, 140, 2)]            # the largest F at W = 2: lds_plan's LDS full (or nearly)


def _rows(fits):
    out = []
    for dtype in (np.float64, np.float32):
        for r in COMMON + _limit_rows(fits, np.dtype(dtype).itemsize):
            out.append(pytest.param(dtype, *r, id='%s-K%d-W%d-F%d-T%d-it%d' % ((np.dtype(dtype).name,) + r)))
    return out


def _inputs(B, K, W, F, T, seed, own_D=False):
    """Positive signals [B,T,F], unit-norm positive atoms [K,W,F] (or [B,K,W,F]) and initial coefficients [B,T,K]."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(0.5, 1.5, (B, T, F))
    D = rs.uniform(0.5, 1.5, ((B,) if own_D else ()) + (K, W, F))
    D /= np.sqrt(np.sum(np.square(D), axis=(-2, -1), keepdims=True))
    A0 = rs.uniform(1.0, 2.0, (B, T, K))
    return x, D, A0


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def _close(got, ref64, ref32, what):
    """float64: relative error <= 1e-10.  float32: within 4x the restatement's own float32 spread + 1e-6 max|ref|."""
    scale = float(np.max(np.abs(ref64)))
    err = _err(got, ref64)
    if ref32 is None:
        assert err <= 1e-10 * scale, (what, err / scale)
    else:
        spread = _err(ref32, ref64)
        assert err <= 4.0 * spread + 1e-6 * scale, (what, err, spread, scale)


def _check_coder(x, D, A0, iters, coef, resid, st, b):
    """Signal b of a computeCoefficientsBatch call against the restatement (x, D, A0 already in the run's dtype)."""
    r64 = rst.nmf(x.astype(np.float64), D.astype(np.float64), A0.astype(np.float64), iters)
    r32 = rst.nmf(x, D, A0, iters, dtype=np.float32) if x.dtype == np.float32 else None
    assert coef.dtype == x.dtype and resid.dtype == x.dtype
    _close(coef, r64[0], None if r32 is None else r32[0], 'coefficients')
    _close(resid, r64[1], None if r32 is None else r32[1], 'residual')
    assert int(st.iterations[b]) == r64[2] == iters
    assert int(st.stop[b]) == r64[3] == rst.STOP_MAX_ITERATIONS


def _check_learner(x, D0, A0, iters, D, st, b):
    r64 = lrst.learn(x.astype(np.float64), D0.astype(np.float64), A0.astype(np.float64), iters)
    r32 = lrst.learn(x, D0, A0, iters, dtype=np.float32) if x.dtype == np.float32 else None
    assert D.dtype == x.dtype
    _close(D, r64[0], None if r32 is None else r32[0], 'D')
    assert int(st.iterations[b]) == r64[1] == iters
    assert int(st.stop[b]) == r64[2] == rst.STOP_MAX_ITERATIONS


# ------------------------------------------------------------------------------------------------ limits (CPU)
@pytest.mark.parametrize('fits', [coder_fits, learner_fits], ids=['coder', 'learner'])
def test_lds_limits(fits):
    """The limits the restated plan gives (W at F = 1, F at W = 2): the learner's kernels add no tighter bound."""
    assert (first_unsupported_W(fits, 4), first_unsupported_W(fits, 8)) == (354, 370)
    assert (first_unsupported_F(fits, 4), first_unsupported_F(fits, 8)) == (89, 47)
    # at F = 88 (f32) and F = 46 (f64), W = 2, the plan fills 65 536 bytes exactly
    for itemsize, F in ((4, 88), (8, 46)):
        RB, CB = TILE[itemsize]
        assert ROWS * F * itemsize + (ROWS + 1 + RB - 1) // RB * RB * CB * itemsize == LDS_BYTES



@pytest.mark.gpu
# ------------------------------------------------------------------------------------------------ coder
@pytest.mark.parametrize('dtype,K,W,F,T,iters', _rows(coder_fits))
def test_coder_matches_restatement(dtype, K, W, F, T, iters):
    from hsc_amd.modeling import ConvolutionalNMF
    x, D, A0 = (a.astype(dtype) for a in _inputs(1, K, W, F, T, seed=K * 1000 + W * 10 + F))
    coef, resid, st = ConvolutionalNMF().computeCoefficientsBatch(x, D, nbMaxIterations=iters, initialCoefficients=A0)
    _check_coder(x[0], D, A0[0], iters, coef[0], resid[0], st, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_coder_chunked_batch_matches_restatement(dtype):
    """Five signals in chunks of two (the memory budget of uniform_alloc for two signals): uploads at an offset, a
    chunk of two signals on blockIdx.y, and a last chunk of one."""
    from hsc_amd.modeling import ConvolutionalNMF
    B, K, W, F, T, iters = 5, 9, 33, 2, 300, 2
    x, D, A0 = (a.astype(dtype) for a in _inputs(B, K, W, F, T, seed=11))
    s, L, ntt = np.dtype(dtype).itemsize, T - W + 1, (T + ROWS - 1) // ROWS
    per = (2 * L * K + 2 * T * F) * s + ntt * 2 * 8 + 3 * 8 + 3 * 4
    coef, resid, st = ConvolutionalNMF(memoryBudget=2 * per + 1).computeCoefficientsBatch(
        x, D, nbMaxIterations=iters, initialCoefficients=A0)
    assert st.timing_ms[3] == 3
    for b in range(B):
        _check_coder(x[b], D, A0[b], iters, coef[b], resid[b], st, b)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_coder_first_unsupported_shapes_raise(dtype):
    from hsc_amd.modeling import ConvolutionalNMF
    s = np.dtype(dtype).itemsize
    for W, F in ((first_unsupported_W(coder_fits, s), 1), (2, first_unsupported_F(coder_fits, s))):
        x, D, A0 = (a.astype(dtype) for a in _inputs(1, 3, W, F, W + 20, seed=1))
        with pytest.raises(_native.HscmpError) as ei:
            ConvolutionalNMF().computeCoefficientsBatch(x, D, nbMaxIterations=1, initialCoefficients=A0)
        assert ei.value.code == _native.ERR_UNSUPPORTED, (W, F, str(ei.value))


@pytest.mark.gpu
# ------------------------------------------------------------------------------------------------ learner
@pytest.mark.parametrize('dtype,K,W,F,T,iters', _rows(learner_fits))
def test_learner_matches_restatement(dtype, K, W, F, T, iters):
    from hsc_amd.nmf import ConvolutionalNMFLearner
    x, D0, A0 = (a.astype(dtype) for a in _inputs(1, K, W, F, T, seed=K * 1000 + W * 10 + F, own_D=True))
    D, st = ConvolutionalNMFLearner(K, W).trainBatch(x, nbMaxIterations=iters, initialDictionaries=D0,
                                                     initialCoefficients=A0)
    _check_learner(x[0], D0[0], A0[0], iters, D[0], st, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_learner_chunked_batch_matches_restatement(dtype):
    """Five learners in chunks of two, each with a dictionary of its own, K = 33 and W*F = 66 (several K and column
    blocks of nmf_dpart_kernel per learner)."""
    from hsc_amd.nmf import ConvolutionalNMFLearner
    B, K, W, F, T, iters = 5, 33, 33, 2, 300, 2
    x, D0, A0 = (a.astype(dtype) for a in _inputs(B, K, W, F, T, seed=12, own_D=True))
    s, L, ntt, NW = np.dtype(dtype).itemsize, T - W + 1, (T + ROWS - 1) // ROWS, W * F
    ntl = (L + ROWS - 1) // ROWS
    per = (2 * L * K + 2 * T * F + K * NW + ntl * K * (NW + 1)) * s + ntt * 2 * 8 + 3 * 8 + 3 * 4
    D, st = ConvolutionalNMFLearner(K, W, memoryBudget=2 * per + 1).trainBatch(
        x, nbMaxIterations=iters, initialDictionaries=D0, initialCoefficients=A0)
    assert st.timing_ms[3] == 3
    for b in range(B):
        _check_learner(x[b], D0[b], A0[b], iters, D[b], st, b)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_learner_first_unsupported_shapes_raise(dtype):
    from hsc_amd.nmf import ConvolutionalNMFLearner
    s = np.dtype(dtype).itemsize
    for W, F in ((first_unsupported_W(learner_fits, s), 1), (2, first_unsupported_F(learner_fits, s))):
        x, D0, A0 = (a.astype(dtype) for a in _inputs(1, 3, W, F, W + 20, seed=2, own_D=True))
        with pytest.raises(_native.HscmpError) as ei:
            ConvolutionalNMFLearner(3, W).trainBatch(x, nbMaxIterations=1, initialDictionaries=D0, initialCoefficients=A0)
        assert ei.value.code == _native.ERR_UNSUPPORTED, (W, F, str(ei.value))
