"""Convolutional NMF coefficients on MI355X: the reference's ConvolutionalNMF (hsc/modeling.py:662-747)
through libhscnmf.so (include/hscnmf.h).  DESIGN.md section 10.  ConvolutionalNMFLearner: the reference's NMF
dictionary learner (ConvolutionalDictionaryLearner(algorithm='nmf'), hsc/modeling.py:330-417), DESIGN.md section 12.

Reference behaviour kept:
  * the initial coefficients are np.random.random((T, K)).astype(sequence.dtype) + 2.0 from numpy's global
    generator, one draw per signal, in batch order;
  * one iteration is W multiplicative steps, then the additive residual; the stop rules are checked in the
    order nbMaxIterations, toleranceResidualScale, toleranceSnr, and nbMaxIterations=None stops after the
    first iteration (Python 2: `int >= None` is true);
  * the coefficients returned are the centred [T,K] array (rows (W-1)//2 .. (W-1)//2+T-W, zero elsewhere),
    the residual is squeezed to [T] for a [K,W] dictionary or a [T] signal.

Added: computeCoefficientsBatch (signals [B,T(,F)] sharing D), ConvolutionalNMFLearner.trainBatch (one dictionary
per signal).  There is no CPU path: without libhscnmf.so or a visible GPU the calls raise hsc_amd._native.HscmpError.
"""
import ctypes
import logging
import os

import numpy as np

from . import _native
from .modeling import SparseApproximator, _compute_dtype

logger = logging.getLogger(__name__)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'nmf', 'libhscnmf.so')
EXPORTS = ['hscnmf_version', 'hscnmf_create', 'hscnmf_destroy', 'hscnmf_last_error', 'hscnmf_compute', 'hscnmf_learn']
STOP_NAMES = {0: 'running', 1: 'max_iterations', 2: 'residual_scale', 3: 'snr'}


class HscnmfParams(ctypes.Structure):
    _fields_ = [('max_iterations', ctypes.c_int32), ('has_residual_scale', ctypes.c_int32), ('has_snr', ctypes.c_int32),
                ('reserved', ctypes.c_int32), ('tolerance_residual_scale', ctypes.c_double),
                ('tolerance_snr', ctypes.c_double), ('memory_budget', ctypes.c_uint64)]


_lib = None


def load_library():
    """Load libhscnmf.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        vp, ci = ctypes.c_void_p, ctypes.c_int
        head = [vp, ci, vp, ci, ci, ci, vp, ci, ci, vp, vp, ctypes.POINTER(HscnmfParams)]
        _lib = _native.load_satellite(LIB_PATH, 'hscnmf', {'hscnmf_compute': head + [vp] * 7, 'hscnmf_learn': head + [vp] * 6})
    return _lib


_contexts = {}


def _context(device):
    if device not in _contexts:
        _contexts[device] = _native.LibraryContext(load_library(), 'hscnmf', device)
    return _contexts[device]


def check_shapes(T, W):
    """The reference fails for these shapes (an empty slice, a zero-width pad); raise a clear error instead."""
    if W < 2:
        raise Exception('ConvolutionalNMF: the filter width must be at least 2 (got W = %d)' % W)
    if T < W:
        raise Exception('ConvolutionalNMF: the signal (length %d) is shorter than the filter width %d' % (T, W))


def draw_initial_coefficients(T, K, dtype):
    """hsc/modeling.py:684, from numpy's global generator."""
    return np.random.random((T, K)).astype(dtype) + 2.0


def _params(nbMaxIterations, toleranceResidualScale, toleranceSnr, memoryBudget):
    params = HscnmfParams()
    params.max_iterations = 1 if nbMaxIterations is None else int(nbMaxIterations)
    if params.max_iterations < 1:
        params.max_iterations = 1         # (the reference checks the count after the first iteration)
    params.has_residual_scale = toleranceResidualScale is not None
    params.tolerance_residual_scale = 0.0 if toleranceResidualScale is None else float(toleranceResidualScale)
    params.has_snr = toleranceSnr is not None
    params.tolerance_snr = 0.0 if toleranceSnr is None else float(toleranceSnr)
    params.memory_budget = 0 if memoryBudget is None else int(memoryBudget)
    return params


class NMFStats(object):
    """Per-signal outcome of computeCoefficientsBatch (per-learner outcome of ConvolutionalNMFLearner.trainBatch)."""

    def __init__(self, iterations, stop, snr, residual_scale, timing_ms):
        self.iterations = iterations              # int32 [B]
        self.stop = stop                          # int32 [B], include/hscnmf.h HSCNMF_STOP_*
        self.snr = snr                            # float64 [B], dB, of the returned residual
        self.residual_scale = residual_scale      # float64 [B], max |residual|
        self.timing_ms = timing_ms                # upload, iterations, download (HIP events), chunks, iterations run

    def stop_reasons(self):
        return [STOP_NAMES.get(int(s), int(s)) for s in self.stop]


class ConvolutionalNMF(SparseApproximator):
    """hsc/modeling.py:662-747, on the GPU."""

    def __init__(self, device=0, memoryBudget=None):
        self.device = device
        self.memoryBudget = memoryBudget          # device bytes per chunk of signals (None: 60% of the free memory)
        self.lastStats = None

    def computeCoefficientsBatch(self, sequences, D, nbMaxIterations=None, toleranceResidualScale=None, toleranceSnr=None,
                                 initialCoefficients=None):
        """`sequences` [B,T] or [B,T,F], D [K,W] or [K,W,F].  Returns (coefficients [B,T,K], residuals [B,T(,F)], NMFStats).
        initialCoefficients [B,T,K]: used instead of the reference's draw from the global generator."""
        sequences = np.asarray(sequences)
        assert sequences.ndim == 2 or sequences.ndim == 3
        assert D.ndim == 2 or D.ndim == 3
        B, T = sequences.shape[0], sequences.shape[1]
        K, W = D.shape[0], D.shape[1]
        check_shapes(T, W)
        dt = _compute_dtype(sequences.dtype, D.dtype)
        x = np.ascontiguousarray(sequences.reshape((B, T, -1)), dtype=dt)
        D3 = np.ascontiguousarray(D.reshape((K, W, -1)), dtype=dt)
        F = D3.shape[2]
        assert x.shape[2] == F
        if initialCoefficients is None:
            a0 = np.empty((B, T, K), dtype=dt)
            for b in range(B):
                a0[b] = draw_initial_coefficients(T, K, sequences.dtype)
        else:
            a0 = np.ascontiguousarray(initialCoefficients, dtype=dt)
            assert a0.shape == (B, T, K)
        energy = np.array([np.sum(np.square(x[b])) for b in range(B)], dtype=np.float64)       # modeling.py:681

        params = _params(nbMaxIterations, toleranceResidualScale, toleranceSnr, self.memoryBudget)

        ctx = _context(self.device)
        coef = np.empty((B, T, K), dtype=dt)
        resid = np.empty((B, T, F), dtype=dt)
        iters = np.zeros((B,), dtype=np.int32)
        stop = np.zeros((B,), dtype=np.int32)
        snr = np.zeros((B,), dtype=np.float64)
        rscale = np.zeros((B,), dtype=np.float64)
        timing = np.zeros((5,), dtype=np.float64)
        p = _native._ptr
        ctx.call('compute', _native.dtype_code(dt), p(x), B, T, F, p(D3), K, W, p(a0), p(energy), ctypes.byref(params), p(coef),
                 p(resid), p(iters), p(stop), p(snr), p(rscale), p(timing))
        if sequences.ndim == 2 or D.ndim == 2:
            resid = np.squeeze(resid, axis=2)                                                  # modeling.py:744-745
        if np.issubdtype(sequences.dtype, np.floating) and resid.dtype != sequences.dtype:
            coef, resid = coef.astype(sequences.dtype), resid.astype(sequences.dtype)
        stats = NMFStats(iters, stop, snr, rscale, timing)
        self.lastStats = stats
        for b in range(B):
            logger.debug('signal %d: SNR of %f dB after %d iterations, stop: %s' % (
                b, snr[b], iters[b], STOP_NAMES.get(int(stop[b]))))
        return coef, resid, stats

    def computeCoefficients(self, sequence, D, nbMaxIterations=None, toleranceResidualScale=None, toleranceSnr=None):
        """hsc/modeling.py:667-747.  Returns (coefficients [T,K] dense, residual [T] or [T,F])."""
        sequence = np.asarray(sequence)
        assert sequence.ndim == 1 or sequence.ndim == 2
        assert D.ndim == 2 or D.ndim == 3
        coef, resid, _ = self.computeCoefficientsBatch(sequence[np.newaxis], D, nbMaxIterations, toleranceResidualScale,
                                                       toleranceSnr)
        return coef[0], resid[0]


def _call_learn(device, dt, x, D0, a0, energy, params):
    """hscnmf_learn on x [B,T,F], D0 [B,K,W,F], a0 [B,T,K] (all of dtype dt).  Returns (D [B,K,W,F], NMFStats)."""
    B, T, F = x.shape
    K, W = D0.shape[1], D0.shape[2]
    ctx = _context(device)
    D = np.empty((B, K, W, F), dtype=dt)
    iters = np.zeros((B,), dtype=np.int32)
    stop = np.zeros((B,), dtype=np.int32)
    snr = np.zeros((B,), dtype=np.float64)
    rscale = np.zeros((B,), dtype=np.float64)
    timing = np.zeros((5,), dtype=np.float64)
    p = _native._ptr
    ctx.call('learn', _native.dtype_code(dt), p(x), B, T, F, p(D0), K, W, p(a0), p(energy), ctypes.byref(params), p(D),
             p(iters), p(stop), p(snr), p(rscale), p(timing))
    return D, NMFStats(iters, stop, snr, rscale, timing)


class ConvolutionalNMFLearner(object):
    """The reference's convolutional NMF dictionary learner (ConvolutionalDictionaryLearner._train_nmf,
    hsc/modeling.py:330-417) on the GPU, and a batch of independent learners (one dictionary per signal).

    Reference behaviour kept: per learner, the initial dictionary is drawn first (`randint` windows for
    'random_samples', `uniform` for 'noise', hsc/modeling.py:308-328), then the initial coefficients
    np.random.random((T, K)).astype(data.dtype) + 2.0; draws come from `rng` when given, numpy's global generator
    otherwise.  The computation runs in _compute_dtype(data, D_init) (float64 for float32 data with 'noise', whose
    dictionary is float64) and D is returned in the initial dictionary's dtype, as the reference returns it."""

    def __init__(self, k, windowSize, device=0, rng=None, memoryBudget=None):
        self.k = int(k)
        self.windowSize = int(windowSize)
        self.device = device
        self.rng = rng
        self.memoryBudget = memoryBudget          # device bytes per chunk of learners (None: 60% of the free memory)
        self.lastStats = None

    def _check_shapes(self, T, initMethod, drawD):
        W = self.windowSize
        if W < 2:
            raise Exception('ConvolutionalNMFLearner: the filter width must be at least 2 (got W = %d)' % W)
        if T < W:
            raise Exception('ConvolutionalNMFLearner: the signal (length %d) is shorter than the filter width %d' % (T, W))
        if drawD and initMethod == 'random_samples' and T <= W:
            raise Exception("ConvolutionalNMFLearner: initMethod='random_samples' needs a signal longer than the filter "
                            "width (length %d, filter width %d)" % (T, W))
        if drawD and initMethod not in ('random_samples', 'noise'):
            raise Exception('Unsupported initialization method: %s' % (initMethod))

    def trainBatch(self, sequences, initMethod='random_samples', nbMaxIterations=None, toleranceResidualScale=None,
                   toleranceSnr=None, initialDictionaries=None, initialCoefficients=None):
        """`sequences` [B,T] or [B,T,F].  Returns (D [B,K,W] or [B,K,W,F], NMFStats).
        initialDictionaries [B,K,W(,F)] / initialCoefficients [B,T,K]: used instead of the reference's draws."""
        from .learning import ConvolutionalDictionaryLearner
        sequences = np.asarray(sequences)
        assert sequences.ndim == 2 or sequences.ndim == 3
        B, T = sequences.shape[0], sequences.shape[1]
        K, W = self.k, self.windowSize
        self._check_shapes(T, initMethod, initialDictionaries is None)
        seqs = sequences.reshape((B, T, -1))
        F = seqs.shape[2]
        rng = np.random if self.rng is None else self.rng
        init = ConvolutionalDictionaryLearner(K, W, algorithm='nmf', rng=self.rng)
        D0s, a0s = [], []
        for b in range(B):                        # per learner, in batch order: D_init, then the coefficients
            if initialDictionaries is None:
                D0s.append(init._init_D(seqs[b], initMethod))
            if initialCoefficients is None:                                                     # modeling.py:344
                a0s.append(rng.random_sample((T, K)).astype(sequences.dtype) + 2.0)
        D0 = np.stack(D0s) if initialDictionaries is None else np.asarray(initialDictionaries)
        assert D0.shape[:3] == (B, K, W) and D0.ndim in (3, 4)
        dt = _compute_dtype(sequences.dtype, D0.dtype)
        x = np.ascontiguousarray(seqs, dtype=dt)
        D3 = np.ascontiguousarray(D0.reshape((B, K, W, -1)), dtype=dt)
        assert D3.shape[3] == F
        a0 = np.ascontiguousarray(np.stack(a0s) if initialCoefficients is None else initialCoefficients, dtype=dt)
        assert a0.shape == (B, T, K)
        energy = np.array([np.sum(np.square(x[b])) for b in range(B)], dtype=np.float64)       # modeling.py:341
        params = _params(nbMaxIterations, toleranceResidualScale, toleranceSnr, self.memoryBudget)
        D, stats = _call_learn(self.device, dt, x, D3, a0, energy, params)
        if np.issubdtype(D0.dtype, np.floating) and D.dtype != D0.dtype:
            D = D.astype(D0.dtype)
        if sequences.ndim == 2:
            D = np.squeeze(D, axis=3)                                                           # modeling.py:414-415
        self.lastStats = stats
        for b in range(B):
            logger.debug('learner %d: SNR of %f dB after %d iterations, stop: %s' % (
                b, stats.snr[b], stats.iterations[b], STOP_NAMES.get(int(stats.stop[b]))))
        return D, stats

    def train(self, X, initMethod='random_samples', nbMaxIterations=None, toleranceResidualScale=None, toleranceSnr=None):
        """hsc/modeling.py:330-417 (`_train_nmf`).  X [T] or [T,F]; returns D [K,W] or [K,W,F]."""
        X = np.asarray(X)
        assert X.ndim == 1 or X.ndim == 2
        D, _ = self.trainBatch(X[np.newaxis], initMethod, nbMaxIterations, toleranceResidualScale, toleranceSnr)
        return D[0]
