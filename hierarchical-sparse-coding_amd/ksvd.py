"""Convolutional K-SVD dictionary learning on MI355X: the reference's ConvolutionalDictionaryLearner(algorithm='ksvd')
(hsc/modeling.py:528-641) with its dictionary-update stage on the GPU, through libhscksvd.so (include/hscksvd.h).
DESIGN.md section 13.

Reference behaviour kept:
  * the initial dictionary is ConvolutionalDictionaryLearner._init_D(data, 'noise'), drawn from `rng` or numpy's
    global generator;
  * the coefficient stage is the coder the host learner builds (LoCOMP() for 'locomp', ConvolutionalMatchingPursuit()
    for 'cmp') with the same arguments, so the encodes are the host learner's, bit for bit;
  * the update refits every atom, in order, to the rank-one approximation of the patches that the OTHER atoms'
    coefficients reconstruct around its occurrences (the reference's `error`, not the data minus the reconstruction);
    usePCA=True follows the reference's `pca` helper (centred patches; P / |P| for a single occurrence);
  * the loop runs while n < maxIterations and alpha = |D - D_old| > tolerance.
The one intended deviation: an updated atom's sign is chosen so that it points the way the atom pointed before the
update (LAPACK's sign cannot be reproduced).  The K-SVD trajectory is sign-equivariant (the coders select by |c|, and
c * D does not change), so only alpha differs from the reference's: alpha is the sign-aligned distance.

A corpus (B signals, one dictionary): update_corpus / ConvolutionalKSVDLearner.trainCorpus encode the whole batch in one
computeCoefficientsBatch call per iteration (ragged batches included) and update the dictionary from every signal's
occurrences with hscksvd_update_corpus; no atom reaches into a neighbouring signal.  DESIGN.md section 16.

Independent learners (B signals, B dictionaries: restarts, or a dictionary per signal): update_batch /
ConvolutionalKSVDLearner.trainBatch encode the running learners' signals against their own dictionaries in one
computeCoefficientsMultiBatch call per iteration and update the dictionaries with one hscksvd_update_batch launch, a workgroup
per learner; learner b is bit for bit `train` on signal b.  DESIGN.md section 24.

There is no CPU path: without libhscksvd.so or a visible GPU the calls raise hsc_amd._native.HscmpError.
ConvolutionalDictionaryLearner(algorithm='ksvd') keeps its host sweep and is not routed here.
"""
import ctypes
import logging
import os
import time

import numpy as np
import scipy.sparse

from . import _native

logger = logging.getLogger(__name__)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'ksvd', 'libhscksvd.so')
EXPORTS = ['hscksvd_version', 'hscksvd_create', 'hscksvd_destroy', 'hscksvd_last_error', 'hscksvd_update',
           'hscksvd_update_corpus', 'hscksvd_update_batch']
MAX_ATOM_SIZE = 64                       # W * F, include/hscksvd.h HSCKSVD_MAX_ATOM_SIZE
WIDE_FROM_OCCURRENCES = 64               # include/hscksvd.h HSCKSVD_WIDE_FROM_OCCURRENCES: what plan 'auto' decides on
PLANS = {'auto': 0, 'one': 1, 'wide': 2}
ATOM_STATS = 4                           # n_k, lambda1, lambda2, Jacobi sweeps
METHODS = ('locomp', 'cmp')

_lib = None


def load_library():
    """Load libhscksvd.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        vp, ci = ctypes.c_void_p, ctypes.c_int
        _lib = _native.load_satellite(LIB_PATH, 'hscksvd', {
            'hscksvd_update': [vp, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp],
            'hscksvd_update_corpus': [vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, ci, ci, vp, vp],
            'hscksvd_update_batch': [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp]})
    return _lib


_contexts = {}


def _context(device):
    if device not in _contexts:
        _contexts[device] = _native.LibraryContext(load_library(), 'hscksvd', device)
    return _contexts[device]


def check_update_shapes(T, W, F, usePCA):
    """The limits of the device update (raised before any device call)."""
    if W * F > MAX_ATOM_SIZE:
        raise NotImplementedError('K-SVD on the GPU: atoms of W * F = %d samples exceed the limit of %d (W * F <= %d)'
                                  % (W * F, MAX_ATOM_SIZE, MAX_ATOM_SIZE))
    if T <= W:
        raise AssertionError('K-SVD: the signal (length %d) must be longer than the window width %d' % (T, W))
    if usePCA and F > 1:
        raise ValueError('K-SVD: usePCA=True needs one feature per sample (got F = %d): the reference assigns the '
                         'W * F eigenvector to a [W, F] atom' % F)


def _dictionary_copy(D, ndim):
    """D [..,K,W] or [..,K,W,F] as the float64 C-ordered copy of `ndim` dimensions (F explicit) that the library updates."""
    return np.array(D.reshape(D.shape[:ndim - 1] + (-1,)), dtype=np.float64, order='C')


def _coefficient_copy(c):
    """A sparse [T,K] matrix as a float64 CSC copy with sorted rows: what the library's indptr / indices / data describe."""
    c = scipy.sparse.csc_matrix(c, dtype=np.float64, copy=True)
    if not c.has_sorted_indices:
        c.sort_indices()
    return c


def _sweep(device, entry, lead, D, offsets, indptr, indices, data, usePCA, plan=()):
    """The call the three updates end in: hscksvd_<entry>(*lead, K, W, F, D, *offsets, indptr, indices, data, usePCA, *plan,
    stats, timing), D from _dictionary_copy and updated in place.  Returns (the updated data, stats D.shape[:-2] + [4], timing_ms)."""
    K, W, F = D.shape[-3:]
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.float64)
    stats = np.zeros(D.shape[:-2] + (ATOM_STATS,), dtype=np.float64)
    timing = np.zeros((3,), dtype=np.float64)
    p = _native._ptr
    _context(device).call(entry, *lead, K, W, F, p(D), *offsets, p(indptr), p(indices), p(data), 1 if usePCA else 0, *plan,
                          p(stats), p(timing))
    return data, stats, timing


def update(D, coefficients, usePCA=False, device=0):
    """One sweep of the K-SVD dictionary update (hscksvd_update) on D [K,W] or [K,W,F] and the [T,K] sparse
    coefficients the coder returned.  Returns (D float64 of D's shape, csc_matrix [T,K] float64 with the updated
    values, stats [K,4] float64: n_k, lambda1, lambda2, Jacobi sweeps, timing_ms [3]: upload, sweep, download).
    The inputs are not modified."""
    D = np.asarray(D)
    assert D.ndim == 2 or D.ndim == 3
    D3 = _dictionary_copy(D, 3)
    K, W, F = D3.shape
    T = coefficients.shape[0]
    assert coefficients.shape[1] == K
    check_update_shapes(T, W, F, usePCA)
    csc = _coefficient_copy(coefficients)
    data, stats, timing = _sweep(device, 'update', (T,), D3, (), csc.indptr, csc.indices, csc.data, usePCA)
    csc.data[:] = data
    return D3.reshape(D.shape), csc, stats, timing


def update_corpus(D, coefficients, usePCA=False, device=0, plan='auto'):
    """One sweep of the K-SVD dictionary update over a corpus (hscksvd_update_corpus): D [K,W] or [K,W,F] and a list of
    B sparse [T_b,K] coefficient matrices, one per signal.  The patches of an occurrence are built from its own signal's
    coefficients alone and clipped at that signal's ends.  plan: 'auto', 'one' (one workgroup) or 'wide' (grids per
    atom); all return the same bits.  Returns (D float64 of D's shape, list of B csc_matrix [T_b,K] float64 with the
    updated values, stats [K,4] float64: n_k, lambda1, lambda2, Jacobi sweeps, timing_ms [3]: upload, sweep, download).
    The inputs are not modified."""
    D = np.asarray(D)
    assert D.ndim == 2 or D.ndim == 3
    D3 = _dictionary_copy(D, 3)
    K, W, F = D3.shape
    if plan not in PLANS:
        raise ValueError("K-SVD: plan must be 'auto', 'one' or 'wide' (got %r)" % (plan,))
    coefficients = list(coefficients)
    if len(coefficients) == 0:
        raise ValueError('K-SVD: a corpus needs at least one signal')
    for c in coefficients:
        assert c.shape[1] == K
        check_update_shapes(c.shape[0], W, F, usePCA)
    offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c in coefficients], dtype=np.int64)])
    if offsets[-1] >= 2 ** 31:
        raise NotImplementedError('K-SVD on the GPU: the corpus has %d samples in all, the limit is 2^31 - 1' % offsets[-1])
    cscs = [_coefficient_copy(c) for c in coefficients]
    # the stack in CSC: column, then signal, then time -- a stable sort by column of the signals' entries in signal order
    cols = np.concatenate([np.repeat(np.arange(K), np.diff(c.indptr)) for c in cscs])
    order = np.argsort(cols, kind='stable')
    indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=K))])
    indices = np.concatenate([c.indices + off for c, off in zip(cscs, offsets[:-1])])[order]
    row_offsets = offsets.astype(np.int32)
    data, stats, timing = _sweep(device, 'update_corpus', (len(cscs), _native._ptr(row_offsets)), D3, (), indptr, indices,
                                 np.concatenate([c.data for c in cscs])[order], usePCA, (PLANS[plan],))
    back = np.empty_like(data)
    back[order] = data
    first = 0
    for c in cscs:
        c.data[:] = back[first:first + c.nnz]
        first += c.nnz
    return D3.reshape(D.shape), cscs, stats, timing


def update_batch(Ds, coefficients, usePCA=False, device=0):
    """B independent sweeps of the K-SVD dictionary update in one launch (hscksvd_update_batch): Ds [B,K,W] or [B,K,W,F] (or a
    list of B dictionaries of one shape) and a list of B sparse [T,K] coefficient matrices, problem b being
    update(Ds[b], coefficients[b]) bit for bit.  Returns (Ds float64 of the stacked shape, list of B csc_matrix [T,K]
    float64 with the updated values, stats [B,K,4] float64: n_k, lambda1, lambda2, Jacobi sweeps, timing_ms [3]: upload,
    sweep, download).  The inputs are not modified."""
    if isinstance(Ds, (list, tuple)):
        parts = [np.asarray(d) for d in Ds]
        if len(parts) == 0 or any(d.shape != parts[0].shape for d in parts):
            raise ValueError('K-SVD: update_batch needs at least one dictionary, all of one shape')
        Ds = np.stack(parts)
    Ds = np.asarray(Ds)
    if Ds.ndim != 3 and Ds.ndim != 4:
        raise ValueError('K-SVD: the dictionaries must be [B,K,W] or [B,K,W,F] (got %d dimensions)' % Ds.ndim)
    D4 = _dictionary_copy(Ds, 4)
    B, K, W, F = D4.shape
    coefficients = list(coefficients)
    if len(coefficients) != B or B == 0:
        raise ValueError('K-SVD: %d coefficient matrices for %d dictionaries' % (len(coefficients), B))
    T = coefficients[0].shape[0]
    for c in coefficients:
        if c.shape != (T, K):
            raise ValueError('K-SVD: update_batch needs coefficient matrices of one shape [T,K] = (%d, %d) (got %s)' % (T, K, c.shape))
    check_update_shapes(T, W, F, usePCA)
    cscs = [_coefficient_copy(c) for c in coefficients]
    offsets = np.concatenate([[0], np.cumsum([c.nnz for c in cscs], dtype=np.int64)]).astype(np.int64)
    if offsets[-1] >= 2 ** 31:
        raise NotImplementedError('K-SVD on the GPU: %d stored coefficients in all, the limit is 2^31 - 1' % offsets[-1])
    data, stats, timing = _sweep(device, 'update_batch', (B, T), D4, (_native._ptr(offsets),), np.stack([c.indptr for c in cscs]),
                                 np.concatenate([c.indices for c in cscs]), np.concatenate([c.data for c in cscs]), usePCA)
    for b, c in enumerate(cscs):
        c.data[:] = data[offsets[b]:offsets[b + 1]]
    return D4.reshape(Ds.shape), cscs, stats, timing


def _corpus_signals(sequences, lengths):
    """The signals of a corpus as a list of [T_b] or [T_b,F] views: `sequences` [B,T] / [B,T,F], a list / tuple of
    arrays, or a padded array with `lengths` [B] (the forms of computeCoefficientsBatch)."""
    if isinstance(sequences, (list, tuple)):
        if lengths is not None:
            raise ValueError('lengths= goes with a padded array, not with a list of signals')
        seqs = [np.asarray(q) for q in sequences]
    else:
        seq = np.asarray(sequences)
        if seq.ndim != 2 and seq.ndim != 3:
            raise ValueError('K-SVD: the corpus must be [B,T] or [B,T,F] (got %d dimensions)' % seq.ndim)
        if lengths is None:
            seqs = list(seq)
        else:
            lens = np.asarray(lengths).astype(np.int64).reshape(-1)
            if lens.shape[0] != seq.shape[0]:
                raise ValueError('lengths has %d entries for %d signals' % (lens.shape[0], seq.shape[0]))
            if np.any(lens > seq.shape[1]) or np.any(lens < 0):
                raise ValueError('a length is outside the padded length %d' % seq.shape[1])
            seqs = [seq[b, :int(lens[b])] for b in range(seq.shape[0])]
    if len(seqs) == 0:
        raise ValueError('K-SVD: a corpus needs at least one signal')
    if seqs[0].ndim not in (1, 2) or any(q.ndim != seqs[0].ndim or q.shape[1:] != seqs[0].shape[1:] for q in seqs):
        raise ValueError('K-SVD: the signals of a corpus must all be [T_b] or all be [T_b,F] with the same F')
    return seqs


class ConvolutionalKSVDLearner(object):
    """The reference's convolutional K-SVD learner (ConvolutionalDictionaryLearner._train_ksvd, hsc/modeling.py:528-641)
    with the dictionary update on the GPU (one hscksvd_update call per iteration).

    lastStats (after train): one dict per iteration with alpha (sign-aligned), nnz (stored coefficients), encode_ms,
    update_ms (host wall clock of the update call), sweep_ms (the device sweep alone), n_k [K] and eigenvalues [K,2]
    (the top two of the Gram matrix sum_i P_i P_i^T; of the covariance for usePCA)."""

    def __init__(self, k, windowSize, device=0, rng=None):
        self.k = int(k)
        self.windowSize = int(windowSize)
        self.device = device
        self.rng = rng
        self.lastStats = None

    def _coder(self, method):
        from .modeling import ConvolutionalMatchingPursuit, LoCOMP
        if method == 'locomp':
            return LoCOMP()
        if method == 'cmp':
            return ConvolutionalMatchingPursuit()
        raise AssertionError(method)

    def _check_method(self, method):
        if method in ('mptk-mp', 'mptk-cmp'):
            raise NotImplementedError("method='%s' needs the external MPTK toolkit, which this engine does not bind; "
                                      "use method='cmp' or 'locomp'" % method)
        if method not in METHODS:
            raise Exception('Unsupported sparse coding method: %s' % (method))

    def _check(self, data, method, usePCA):
        self._check_method(method)
        if data.ndim != 1 and data.ndim != 2:
            raise ValueError('K-SVD: the data must be [T] or [T,F] (got %d dimensions)' % data.ndim)
        F = 1 if data.ndim == 1 else data.shape[1]
        check_update_shapes(data.shape[0], self.windowSize, F, usePCA)

    def _initial_D(self, data, rng):
        """The reference's initial dictionary ('noise') for data [T] or [T,F], drawn from `rng` (None: numpy's global generator)."""
        from .learning import ConvolutionalDictionaryLearner
        D = ConvolutionalDictionaryLearner(self.k, self.windowSize, rng=rng)._init_D(data, initMethod='noise')
        return np.asarray(D, dtype=np.float64)

    @staticmethod
    def _record(alpha, nnz, t0, t1, t2, timing, atoms, **more):
        """One iteration's lastStats record: encode from t0 to t1, update to t2 (seconds), the update's timing and atoms [K,4];
        `more`: trainCorpus' plan, the batch encodes' variant."""
        return dict(alpha=float(alpha), nnz=int(nnz), encode_ms=1e3 * (t1 - t0), update_ms=1e3 * (t2 - t1),
                    sweep_ms=float(timing[1]), n_k=atoms[:, 0].astype(np.int64), eigenvalues=atoms[:, 1:3].copy(), **more)

    def train(self, data, method='locomp', maxIterations=100, tolerance=0.0, nbNonzeroCoefs=None, toleranceSnr=40.0,
              usePCA=False):
        """hsc/modeling.py:528-641 (`_train_ksvd`).  data [T] or [T,F]; returns D float64 [K,W] or [K,W,F]."""
        from .modeling import ConvolutionalSparseCoder
        data = np.asarray(data)
        self._check(data, method, usePCA)
        load_library()                                       # no CPU path: fail before the first encode
        D = self._initial_D(data, self.rng)
        stats = []
        n, alpha = 0, tolerance + 1.0
        while n < maxIterations and alpha > tolerance:
            t0 = time.perf_counter()
            coefficients, _ = ConvolutionalSparseCoder(D, self._coder(method)).encode(
                data, nbNonzeroCoefs=nbNonzeroCoefs, toleranceSnr=toleranceSnr)
            t1 = time.perf_counter()
            oldD = D
            D, coefficients, atoms, timing = update(oldD, coefficients, usePCA, self.device)
            t2 = time.perf_counter()
            alpha = np.sqrt(np.sum(np.square(D - oldD)))
            stats.append(self._record(alpha, coefficients.nnz, t0, t1, t2, timing, atoms))
            logger.debug('K-SVD iteration %d: tolerance = %f, sparsity = %f' % (
                n, alpha, float(coefficients.nnz) / np.prod(coefficients.shape)))
            n += 1
        self.lastStats = stats
        return D

    def trainBatch(self, sequences, method='locomp', maxIterations=100, tolerance=0.0, nbNonzeroCoefs=None, toleranceSnr=40.0,
                   usePCA=False, rngs=None):
        """B independent learners, learner b on sequences[b] ([B,T] or [B,T,F]): restarts, or a dictionary per signal.
        rngs: a list of B generators (learner b then reproduces train() with rngs[b], bit for bit), or one generator / None
        (the learner's own rng, else numpy's global generator) shared by all: the initial dictionaries are then drawn in batch
        order.
        Each iteration is ONE computeCoefficientsMultiBatch over the learners still running (every signal against its own
        dictionary) and ONE update_batch over them (a workgroup per learner).  Each learner stops on its own
        (n < maxIterations and alpha > tolerance); a stopped learner is neither encoded nor updated.  DESIGN.md section 24.
        Returns (D float64 [B,K,W] or [B,K,W,F], per-learner lastStats lists: train's records plus variant, the encode's kernel
        variant; encode_ms and update_ms are the batch's wall clock, shared by the learners that ran in it)."""
        from .modeling import is_ragged
        self._check_method(method)
        if is_ragged(sequences):
            raise NotImplementedError('ConvolutionalKSVDLearner.trainBatch has no ragged form (signals of different lengths): '
                                      'pass a [B,T] or [B,T,F] array')
        sequences = np.asarray(sequences)
        if sequences.ndim != 2 and sequences.ndim != 3:
            raise ValueError('K-SVD: the batch must be [B,T] or [B,T,F] (got %d dimensions)' % sequences.ndim)
        B = sequences.shape[0]
        if B == 0:
            raise ValueError('K-SVD: a batch needs at least one learner')
        check_update_shapes(sequences.shape[1], self.windowSize, 1 if sequences.ndim == 2 else sequences.shape[2], usePCA)
        if isinstance(rngs, (list, tuple)):
            if len(rngs) != B:
                raise ValueError('K-SVD: %d generators for %d learners' % (len(rngs), B))
            rngs = list(rngs)
        else:
            rngs = [self.rng if rngs is None else rngs] * B
        load_library()                                       # no CPU path: fail before the first encode
        D = np.stack([self._initial_D(sequences[b], rngs[b]) for b in range(B)])
        coder = self._coder(method)
        stats = [[] for _ in range(B)]
        n = 0
        # (train's loop test before its first iteration: n = 0, alpha = tolerance + 1)
        running = np.arange(B) if (0 < maxIterations and tolerance + 1.0 > tolerance) else np.arange(0)
        while running.size > 0:
            t0 = time.perf_counter()
            res = coder.computeCoefficientsMultiBatch(sequences[running], D[running], nbNonzeroCoefs=nbNonzeroCoefs,
                                                      toleranceSnr=toleranceSnr)
            t1 = time.perf_counter()
            newD, coefficients, atoms, timing = update_batch(D[running], res.coefficients, usePCA, self.device)
            t2 = time.perf_counter()
            keep = []
            for i, b in enumerate(running):
                alpha = np.sqrt(np.sum(np.square(newD[i] - D[b])))
                D[b] = newD[i]
                stats[b].append(self._record(alpha, coefficients[i].nnz, t0, t1, t2, timing, atoms[i], variant=res.variant))
                logger.debug('K-SVD learner %d iteration %d: tolerance = %f, sparsity = %f' % (
                    b, n, alpha, float(coefficients[i].nnz) / np.prod(coefficients[i].shape)))
                if n + 1 < maxIterations and alpha > tolerance:
                    keep.append(b)
            running = np.asarray(keep, dtype=np.int64)
            n += 1
        self.lastStats = stats
        return D, stats

    def trainCorpus(self, sequences, method='locomp', maxIterations=100, tolerance=0.0, nbNonzeroCoefs=None,
                    toleranceSnr=40.0, usePCA=False, lengths=None):
        """`train` for ONE dictionary over a corpus of B signals: `sequences` [B,T] / [B,T,F], or a ragged batch (a list of
        [T_b(,F)] arrays, or a padded array with `lengths`; method='cmp' only, and within what the engine's ragged encode takes:
        DESIGN.md section 15), as computeCoefficientsBatch takes them.
        Each iteration is one encodeBatch of the whole corpus (the stop rules apply per signal) and one update_corpus.
        With method='cmp', `nbNonzeroCoefs` and `toleranceSnr` may be sequences with one value per signal (an L0 that follows
        the signal's length, say): encodeBatch then gives every signal its own stop rules in the same call.
        D is drawn as `train` draws it, with low / high over the whole corpus; a corpus of one signal gives `train`'s
        result on that signal, bit for bit.  Returns D float64 [K,W] or [K,W,F].
        lastStats: `train`'s records (nnz: the stored coefficients of all signals) plus plan (1: one workgroup, 2: wide)
        and variant (the encode's kernel variant)."""
        from .modeling import ConvolutionalSparseCoder, is_ragged, reject_ragged
        self._check_method(method)
        if method == 'locomp':
            reject_ragged(sequences, lengths, "ConvolutionalKSVDLearner.trainCorpus(method='locomp')")
        seqs = _corpus_signals(sequences, lengths)
        for q in seqs:
            check_update_shapes(q.shape[0], self.windowSize, 1 if q.ndim == 1 else q.shape[1], usePCA)
        if sum(q.shape[0] for q in seqs) >= 2 ** 31:
            raise NotImplementedError('K-SVD on the GPU: the corpus has more than 2^31 - 1 samples in all')
        load_library()                                       # no CPU path: fail before the first encode
        if not is_ragged(sequences, lengths):
            sequences = np.asarray(sequences)
        D = self._initial_D(np.concatenate(seqs), self.rng)
        stats = []
        n, alpha = 0, tolerance + 1.0
        while n < maxIterations and alpha > tolerance:
            t0 = time.perf_counter()
            res = ConvolutionalSparseCoder(D, self._coder(method)).encodeBatch(
                sequences, nbNonzeroCoefs=nbNonzeroCoefs, toleranceSnr=toleranceSnr, lengths=lengths)
            t1 = time.perf_counter()
            oldD = D
            D, coefficients, atoms, timing = update_corpus(oldD, res.coefficients, usePCA, self.device)
            t2 = time.perf_counter()
            alpha = np.sqrt(np.sum(np.square(D - oldD)))
            nnz = sum(int(c.nnz) for c in coefficients)
            stats.append(self._record(alpha, nnz, t0, t1, t2, timing, atoms,
                                      plan=2 if np.max(atoms[:, 0]) >= WIDE_FROM_OCCURRENCES else 1, variant=res.variant))
            logger.debug('K-SVD corpus iteration %d: tolerance = %f, sparsity = %f' % (
                n, alpha, float(nnz) / (sum(q.shape[0] for q in seqs) * self.k)))
            n += 1
        self.lastStats = stats
        return D
