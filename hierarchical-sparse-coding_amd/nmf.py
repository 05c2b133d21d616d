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

Added: computeCoefficientsBatch (signals [B,T(,F)] sharing D), computeCoefficientsRaggedBatch (signals of different
lengths sharing D), ConvolutionalNMFLearner.trainBatch (one dictionary per signal) and trainCorpus
(ONE dictionary from many signals, ragged corpora included).
There is no CPU path: without libhscnmf.so or a visible GPU the calls raise hsc_amd._native.HscmpError.
"""
import ctypes
import logging
import os

import numpy as np

from . import _native
from .modeling import SparseApproximator, _compute_dtype

logger = logging.getLogger(__name__)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'nmf', 'libhscnmf.so')
EXPORTS = ['hscnmf_version', 'hscnmf_create', 'hscnmf_destroy', 'hscnmf_last_error', 'hscnmf_compute', 'hscnmf_learn',
           'hscnmf_learn_corpus', 'hscnmf_compute_ragged']
PLAN_EXPORTS = ['hscnmf_ragged_plan']     # include/hscnmf_plan.h: host arithmetic, no context
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
        corpus = [vp, ci, vp, vp, ci, ci, vp, ci, ci, vp, vp, ctypes.POINTER(HscnmfParams)] + [vp] * 8
        ragged = [vp, ci, vp, vp, ci, ci, vp, ci, ci, vp, vp, ctypes.POINTER(HscnmfParams)] + [vp] * 7
        plan = [ci, vp, ci, ci, ci, ci, ctypes.c_uint64, vp, vp, vp]
        _lib = _native.load_satellite(LIB_PATH, 'hscnmf', {'hscnmf_compute': head + [vp] * 7, 'hscnmf_learn': head + [vp] * 6,
                                                           'hscnmf_learn_corpus': corpus, 'hscnmf_compute_ragged': ragged,
                                                           'hscnmf_ragged_plan': plan})
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


def ragged_plan(dtype, lengths, F, K, W, budget):
    """The chunks computeCoefficientsRaggedBatch forms for signals of `lengths` under `budget` device bytes per chunk
    (hscnmf_ragged_plan of include/hscnmf_plan.h: host arithmetic, no device).  Returns (chunk_first int32 [n_chunks + 1], the bytes of the largest
    chunk): chunk c is the signals chunk_first[c] .. chunk_first[c + 1] - 1.  A refusal raises HscmpError with its code."""
    lib = load_library()
    lens = np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int64)
    first = np.zeros((lens.shape[0] + 1,), dtype=np.int32)
    n = np.zeros((1,), dtype=np.int32)
    most = np.zeros((1,), dtype=np.uint64)
    budget = int(budget)
    if budget < 0 or budget >= 1 << 64:
        raise ValueError('ragged_plan: the budget must be in [0, 2^64) bytes (got %d)' % budget)
    p = _native._ptr
    rc = lib.hscnmf_ragged_plan(_native.dtype_code(dtype), p(lens), int(lens.shape[0]), int(F), int(K), int(W), budget, p(first),
                                p(n), p(most))
    if rc != 0:
        ex = _native.HscmpError('hscnmf_ragged_plan failed (%d): %s' % (rc, lib.hscnmf_last_error(None).decode()))
        ex.code = int(rc)
        raise ex
    return first[:int(n[0]) + 1].copy(), int(most[0])


def _call_compute_ragged(device, dt, x, lengths, D3, a0, energy, params):
    """hscnmf_compute_ragged on the stack x [rows,F], lengths [B] int64, D3 [K,W,F], the stacked coefficients a0 [sum L_b,K]
    (all of dtype dt).  Returns (coefficients [rows,K], residual [rows,F], NMFStats per signal)."""
    B, F = lengths.shape[0], x.shape[1]
    K, W = D3.shape[0], D3.shape[1]
    ctx = _context(device)
    coef = np.empty((x.shape[0], K), dtype=dt)
    resid = np.empty((x.shape[0], F), dtype=dt)
    iters = np.zeros((B,), dtype=np.int32)
    stop = np.zeros((B,), dtype=np.int32)
    snr = np.zeros((B,), dtype=np.float64)
    rscale = np.zeros((B,), dtype=np.float64)
    timing = np.zeros((5,), dtype=np.float64)
    p = _native._ptr
    ctx.call('compute_ragged', _native.dtype_code(dt), p(x), p(lengths), B, F, p(D3), K, W, p(a0), p(energy), ctypes.byref(params),
             p(coef), p(resid), p(iters), p(stop), p(snr), p(rscale), p(timing))
    return coef, resid, NMFStats(iters, stop, snr, rscale, timing)


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

    def _prepare_ragged(self, sequences, D, lengths, initialCoefficients):
        """The checks and draws of computeCoefficientsRaggedBatch, before any device call.  Returns (dt, x [rows,F],
        lengths [B] int64, D3 [K,W,F], a0 [sum L_b,K], energy [B], the signals as given)."""
        from .kmeans import corpus_signals
        who = 'ConvolutionalNMF'
        seqs = corpus_signals(sequences, lengths, who)
        D = np.asarray(D)
        if D.ndim not in (2, 3):
            raise ValueError('%s: the dictionary must be [K,W] or [K,W,F] (got %d dimensions)' % (who, D.ndim))
        K, W = D.shape[0], D.shape[1]
        B = len(seqs)
        F = 1 if seqs[0].ndim == 1 else seqs[0].shape[1]
        if K < 1 or F < 1 or D.size != K * W * F:
            raise ValueError('%s: a dictionary %s does not go with signals of %d features' % (who, D.shape, F))
        for b, q in enumerate(seqs):
            try:
                check_shapes(q.shape[0], W)
            except Exception as e:
                raise type(e)('signal %d: %s' % (b, e))
        if initialCoefficients is not None and len(initialCoefficients) != B:
            raise ValueError('%s: %d initial coefficient arrays for %d signals' % (who, len(initialCoefficients), B))
        lens = np.array([q.shape[0] for q in seqs], dtype=np.int64)
        dt = _compute_dtype(seqs[0].dtype, D.dtype)
        a0s = []
        for b in range(B):                                # signal by signal, in corpus order (modeling.py:684)
            if initialCoefficients is None:
                a = draw_initial_coefficients(int(lens[b]), K, seqs[0].dtype)
            else:
                a = np.asarray(initialCoefficients[b])
                if a.shape != (lens[b], K):
                    raise ValueError('%s: the initial coefficients of signal %d must be [%d,%d] (got %s)' % (who, b, lens[b], K, a.shape))
            a0s.append(np.asarray(a[:int(lens[b]) - W + 1], dtype=dt))      # rows past L_b never reach a reconstruction
        x = np.ascontiguousarray(np.concatenate(seqs).reshape((-1, F)), dtype=dt)   # the signals' own samples, no padding
        D3 = np.ascontiguousarray(D.reshape((K, W, F)), dtype=dt)
        a0 = np.ascontiguousarray(np.concatenate(a0s), dtype=dt)
        ends = np.cumsum(lens)
        energy = np.array([np.sum(np.square(x[e - n:e])) for e, n in zip(ends, lens)], dtype=np.float64)   # modeling.py:681
        return dt, x, lens, D3, a0, energy, seqs

    def computeCoefficientsRaggedBatch(self, sequences, D, nbMaxIterations=None, toleranceResidualScale=None, toleranceSnr=None,
                                       initialCoefficients=None, lengths=None):
        """computeCoefficients for B signals of different lengths sharing D [K,W] or [K,W,F], in one call: `sequences` a
        list / tuple of [T_b] or [T_b,F] arrays, a [B,T(,F)] array, or a padded array with `lengths` (its padding is never
        read and may hold NaN); one dtype, one F.  Every signal gets, bit for bit, what computeCoefficientsBatch gives it
        as a batch of one, and stops on its own; the signals are coded in chunks of whole signals within memoryBudget.
        Without initialCoefficients (a list of [T_b,K] arrays) the draws are draw_initial_coefficients(T_b, K, dtype) per
        signal in corpus order: under one numpy seed, a loop of computeCoefficients over the signals.
        Returns (coefficients: a list of [T_b,K] arrays, residuals: a list of [T_b] or [T_b,F] arrays, NMFStats per signal)."""
        dt, x, lens, D3, a0, energy, seqs = self._prepare_ragged(sequences, D, lengths, initialCoefficients)
        params = _params(nbMaxIterations, toleranceResidualScale, toleranceSnr, self.memoryBudget)
        coef, resid, stats = _call_compute_ragged(self.device, dt, x, lens, D3, a0, energy, params)
        if seqs[0].ndim == 1 or np.ndim(D) == 2:
            resid = np.squeeze(resid, axis=1)                                                  # modeling.py:744-745
        if np.issubdtype(seqs[0].dtype, np.floating) and resid.dtype != seqs[0].dtype:
            coef, resid = coef.astype(seqs[0].dtype), resid.astype(seqs[0].dtype)
        ends = np.cumsum(lens)
        self.lastStats = stats
        for b in range(len(lens)):
            logger.debug('signal %d: SNR of %f dB after %d iterations, stop: %s' % (
                b, stats.snr[b], stats.iterations[b], STOP_NAMES.get(int(stats.stop[b]))))
        return ([coef[e - n:e] for e, n in zip(ends, lens)], [resid[e - n:e] for e, n in zip(ends, lens)], stats)

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


def _call_learn_corpus(device, dt, x, lengths, D0, a0, energy, params):
    """hscnmf_learn_corpus on the stack x [rows,F], lengths [B] int64, D0 [K,W,F], the stacked coefficients a0 [sum L_b,K]
    (all of dtype dt).  Returns (D [K,W,F], NMFStats of the corpus with signal_snr and signal_residual_scale [B])."""
    B, F = lengths.shape[0], x.shape[1]
    K, W = D0.shape[0], D0.shape[1]
    ctx = _context(device)
    D = np.empty((K, W, F), dtype=dt)
    iters = np.zeros((1,), dtype=np.int32)
    stop = np.zeros((1,), dtype=np.int32)
    snr = np.zeros((1,), dtype=np.float64)
    rscale = np.zeros((1,), dtype=np.float64)
    sig_snr = np.zeros((B,), dtype=np.float64)
    sig_rscale = np.zeros((B,), dtype=np.float64)
    timing = np.zeros((5,), dtype=np.float64)
    p = _native._ptr
    ctx.call('learn_corpus', _native.dtype_code(dt), p(x), p(lengths), B, F, p(D0), K, W, p(a0), p(energy), ctypes.byref(params),
             p(D), p(iters), p(stop), p(snr), p(rscale), p(sig_snr), p(sig_rscale), p(timing))
    stats = NMFStats(iters, stop, snr, rscale, timing)
    stats.signal_snr = sig_snr                    # float64 [B], dB, of each signal at the last iteration
    stats.signal_residual_scale = sig_rscale      # float64 [B], max |residual| of each signal
    return D, stats


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

    def _prepare_corpus(self, sequences, initMethod, lengths, initialDictionary, initialCoefficients):
        """The checks and draws of trainCorpus, before any device call.  Returns (dt, x [rows,F], lengths [B] int64,
        D3 [K,W,F], a0 [sum L_b,K], energy [B], D0 the initial dictionary as drawn or given, ndim of a signal)."""
        from .kmeans import corpus_signals, corpus_windows
        from .utils import normalize
        who = 'ConvolutionalNMFLearner'
        K, W = self.k, self.windowSize
        seqs = corpus_signals(sequences, lengths, who)
        drawD = initialDictionary is None
        for b, q in enumerate(seqs):
            try:
                self._check_shapes(q.shape[0], initMethod, drawD)
            except Exception as e:
                raise type(e)('signal %d: %s' % (b, e))
        B = len(seqs)
        F = 1 if seqs[0].ndim == 1 else seqs[0].shape[1]
        if F < 1:
            raise ValueError('%s: no features' % who)
        if initialCoefficients is not None and len(initialCoefficients) != B:
            raise ValueError('%s: %d initial coefficient arrays for %d signals' % (who, len(initialCoefficients), B))
        rng = np.random if self.rng is None else self.rng
        lens = np.array([q.shape[0] for q in seqs], dtype=np.int64)
        stack = np.concatenate(seqs).reshape((-1, F))     # the signals' own samples, no padding
        if drawD:                                         # first the dictionary (_init_D over the corpus) ...
            if initMethod == 'noise':
                D0 = normalize(rng.uniform(low=np.min(stack), high=np.max(stack), size=(K, W, F)))
            else:
                ib, it = corpus_windows(seqs, K, W, rng)
                offsets = np.concatenate([[0], np.cumsum(lens)[:-1]])
                D0 = normalize(stack[(offsets[ib] + it)[:, np.newaxis] + np.arange(W)[np.newaxis, :]])
            if seqs[0].ndim == 1:
                D0 = np.squeeze(D0, axis=2)
        else:
            D0 = np.asarray(initialDictionary)
            if D0.shape[:2] != (K, W) or D0.ndim not in (2, 3) or D0.size != K * W * F:
                raise ValueError('%s: the initial dictionary must be [%d,%d] or [%d,%d,%d] (got %s)' % (who, K, W, K, W, F, D0.shape))
        a0s = []
        for b in range(B):                                # ... then the coefficients, signal by signal (modeling.py:344)
            if initialCoefficients is None:
                a = rng.random_sample((int(lens[b]), K)).astype(seqs[0].dtype) + 2.0
            else:
                a = np.asarray(initialCoefficients[b])
                if a.shape != (lens[b], K):
                    raise ValueError('%s: the initial coefficients of signal %d must be [%d,%d] (got %s)' % (who, b, lens[b], K, a.shape))
            a0s.append(a[:int(lens[b]) - W + 1])          # rows past L_b never reach a reconstruction
        dt = _compute_dtype(seqs[0].dtype, D0.dtype)
        x = np.ascontiguousarray(stack, dtype=dt)
        D3 = np.ascontiguousarray(D0.reshape((K, W, F)), dtype=dt)
        a0 = np.ascontiguousarray(np.concatenate(a0s), dtype=dt)
        ends = np.cumsum(lens)
        energy = np.array([np.sum(np.square(x[e - n:e])) for e, n in zip(ends, lens)], dtype=np.float64)   # modeling.py:341
        return dt, x, lens, D3, a0, energy, D0, seqs[0].ndim

    def trainCorpus(self, sequences, initMethod='random_samples', nbMaxIterations=None, toleranceResidualScale=None,
                    toleranceSnr=None, lengths=None, initialDictionary=None, initialCoefficients=None):
        """`train` for ONE dictionary over a corpus of B signals: `sequences` [B,T] / [B,T,F], a list / tuple of [T_b] or
        [T_b,F] arrays, or a padded array with `lengths` (its padding is never read and may hold NaN); one dtype, one F.
        Every iteration runs the coefficient steps of each signal against the shared D, sums the update's N and den over
        all signals' own rows (no atom straddles two signals) and stops on the corpus' residual scale max_b max|r_b| and
        SNR 10 log10(sum_b energy_b / sum_b sum r_b^2): the reference's _train_nmf on the concatenation with the
        straddling coefficient rows held at zero.
        Draws (from `rng` or numpy's global generator): first the dictionary ('random_samples': K windows of W samples over
        the admissible starts of all signals, kmeans.corpus_windows, every signal longer than W; 'noise': uniform between
        the smallest and largest sample of the corpus), then per signal in corpus order random_sample((T_b, K)) + 2.0 in
        the data's dtype: for one signal, `train`'s draws and, bit for bit, `train`'s result.
        initialDictionary [K,W(,F)] / initialCoefficients (a list of [T_b,K] arrays): used instead of the draws.
        Returns D [K,W] or [K,W,F] in the initial dictionary's dtype; lastStats: the corpus' NMFStats (length 1) with
        signal_snr and signal_residual_scale [B]."""
        dt, x, lens, D3, a0, energy, D0, ndim = self._prepare_corpus(sequences, initMethod, lengths, initialDictionary,
                                                                     initialCoefficients)
        params = _params(nbMaxIterations, toleranceResidualScale, toleranceSnr, self.memoryBudget)
        D, stats = _call_learn_corpus(self.device, dt, x, lens, D3, a0, energy, params)
        if np.issubdtype(D0.dtype, np.floating) and D.dtype != D0.dtype:
            D = D.astype(D0.dtype)
        if ndim == 1:
            D = np.squeeze(D, axis=2)                                                           # modeling.py:414-415
        self.lastStats = stats
        logger.debug('corpus of %d signals: SNR of %f dB after %d iterations, stop: %s' % (
            len(lens), stats.snr[0], stats.iterations[0], STOP_NAMES.get(int(stats.stop[0]))))
        return D
