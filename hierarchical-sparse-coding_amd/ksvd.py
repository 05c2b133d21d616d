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
EXPORTS = ['hscksvd_version', 'hscksvd_create', 'hscksvd_destroy', 'hscksvd_last_error', 'hscksvd_update']
MAX_ATOM_SIZE = 64                       # W * F, include/hscksvd.h HSCKSVD_MAX_ATOM_SIZE
ATOM_STATS = 4                           # n_k, lambda1, lambda2, Jacobi sweeps
METHODS = ('locomp', 'cmp')

_lib = None


def load_library():
    """Load libhscksvd.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        vp, ci = ctypes.c_void_p, ctypes.c_int
        _lib = _native.load_satellite(LIB_PATH, 'hscksvd', {'hscksvd_update': [vp, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp]})
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


def update(D, coefficients, usePCA=False, device=0):
    """One sweep of the K-SVD dictionary update (hscksvd_update) on D [K,W] or [K,W,F] and the [T,K] sparse
    coefficients the coder returned.  Returns (D float64 of D's shape, csc_matrix [T,K] float64 with the updated
    values, stats [K,4] float64: n_k, lambda1, lambda2, Jacobi sweeps, timing_ms [3]: upload, sweep, download).
    The inputs are not modified."""
    D = np.asarray(D)
    assert D.ndim == 2 or D.ndim == 3
    K, W = D.shape[0], D.shape[1]
    D3 = np.array(D.reshape((K, W, -1)), dtype=np.float64, order='C')
    F = D3.shape[2]
    T = coefficients.shape[0]
    assert coefficients.shape[1] == K
    check_update_shapes(T, W, F, usePCA)
    csc = scipy.sparse.csc_matrix(coefficients, dtype=np.float64, copy=True)
    if not csc.has_sorted_indices:
        csc.sort_indices()
    indptr = np.ascontiguousarray(csc.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(csc.indices, dtype=np.int32)
    data = np.ascontiguousarray(csc.data, dtype=np.float64)
    stats = np.zeros((K, ATOM_STATS), dtype=np.float64)
    timing = np.zeros((3,), dtype=np.float64)
    ctx = _context(device)
    p = _native._ptr
    ctx.call('update', T, K, W, F, p(D3), p(indptr), p(indices), p(data), 1 if usePCA else 0, p(stats), p(timing))
    out = scipy.sparse.csc_matrix((data, indices, indptr), shape=csc.shape)
    return D3.reshape(D.shape), out, stats, timing


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

    def _check(self, data, method, usePCA):
        if method in ('mptk-mp', 'mptk-cmp'):
            raise NotImplementedError("method='%s' needs the external MPTK toolkit, which this engine does not bind; "
                                      "use method='cmp' or 'locomp'" % method)
        if method not in METHODS:
            raise Exception('Unsupported sparse coding method: %s' % (method))
        if data.ndim != 1 and data.ndim != 2:
            raise ValueError('K-SVD: the data must be [T] or [T,F] (got %d dimensions)' % data.ndim)
        F = 1 if data.ndim == 1 else data.shape[1]
        check_update_shapes(data.shape[0], self.windowSize, F, usePCA)

    def train(self, data, method='locomp', maxIterations=100, tolerance=0.0, nbNonzeroCoefs=None, toleranceSnr=40.0,
              usePCA=False):
        """hsc/modeling.py:528-641 (`_train_ksvd`).  data [T] or [T,F]; returns D float64 [K,W] or [K,W,F]."""
        from .learning import ConvolutionalDictionaryLearner
        from .modeling import ConvolutionalSparseCoder
        data = np.asarray(data)
        self._check(data, method, usePCA)
        load_library()                                       # no CPU path: fail before the first encode
        D = ConvolutionalDictionaryLearner(self.k, self.windowSize, rng=self.rng)._init_D(data, initMethod='noise')
        D = np.asarray(D, dtype=np.float64)
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
            stats.append(dict(alpha=float(alpha), nnz=int(coefficients.nnz), encode_ms=1e3 * (t1 - t0),
                              update_ms=1e3 * (t2 - t1), sweep_ms=float(timing[1]), n_k=atoms[:, 0].astype(np.int64),
                              eigenvalues=atoms[:, 1:3].copy()))
            logger.debug('K-SVD iteration %d: tolerance = %f, sparsity = %f' % (
                n, alpha, float(coefficients.nnz) / np.prod(coefficients.shape)))
            n += 1
        self.lastStats = stats
        return D
