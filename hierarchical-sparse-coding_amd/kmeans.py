"""Convolutional k-means dictionary learning on MI355X: the reference's ConvolutionalDictionaryLearner(algorithm='kmean')
(hsc/modeling.py:420-524) with every iteration's data work on the GPU, through libhsckmeans.so (include/hsckmeans.h).
DESIGN.md sections 14 and 17.

The signals and the window starts go to the device once.  Each iteration makes one hsckmeans_step call (one
synchronise) for every learner still running: the assignment of every window (the arg-max of hscmp_assign_windows,
bit for bit, on the matrix cores), the membership lists and, per centroid, the sum of its members' normalised
patches in numpy's order.  The host finishes on those K x W x F sums with the reference's own expressions: the mean,
the emptiness test (the reference's np.any() of the member indices: a centroid whose only member is window 0 is
empty), the resets, the +1e-9 of zero-norm centroids, normalize() and alpha.  So the dtype rules are numpy's and the
random draws are the host learner's, in the same order: the window starts, _init_D, then per iteration the resets
in centroid order.

trainCorpus learns ONE dictionary from a collection of signals of different lengths: the reference's learner with its
window draw (extractRandomWindows) taken over the admissible starts of all signals (corpus_windows), so that no window,
initial atom or reset patch straddles two signals.  The signals go to the device as one stack without padding
(hsckmeans_set_corpus).  The centroid half of a step has two plans with the same bits (hsckmeans_set_plan): per-centroid
member tables and one thread per element, or the wide plan for corpus-sized window counts.
A corpus may also be a list of scipy.sparse matrices (the representations of a level): the library
then builds the windows' dense rows on the device from the entries they cover (hsckmeans_set_corpus_sparse), and the
result equals the dense corpus' bit for bit.

There is no CPU path: without libhsckmeans.so or a visible GPU the calls raise hsc_amd._native.HscmpError.
ConvolutionalDictionaryLearner(algorithm='kmean') keeps its host path and is not routed here.
"""
import ctypes
import logging
import os
import time

import numpy as np

from . import _native
from .utils import normalize

logger = logging.getLogger(__name__)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'kmeans', 'libhsckmeans.so')
EXPORTS = ['hsckmeans_version', 'hsckmeans_create', 'hsckmeans_destroy', 'hsckmeans_last_error', 'hsckmeans_set_data',
           'hsckmeans_set_corpus', 'hsckmeans_set_corpus_sparse', 'hsckmeans_set_plan', 'hsckmeans_step']
INIT_METHODS = ('random_samples', 'noise')
RESET_METHODS = ('random_samples', 'random_samples_average', 'noise')
MAX_WINDOW_SIZE = 255                    # include/hsckmeans.h: W + 1 positions per workgroup column set
PLAN_AUTO, PLAN_LISTS, PLAN_WIDE = 0, 1, 2   # hsckmeans_set_plan
WIDE_CHUNK_WINDOWS = 1024                # HSCKMEANS_WIDE_CHUNK_WINDOWS: windows per chunk of the wide plan's partition
WIDE_RING_ROWS = 16                      # HSCKMEANS_WIDE_RING_ROWS: rows of a 256-element tile per half of its LDS ring
WIDE_MAX_K = 1024                        # HSCKMEANS_WIDE_MAX_K
WIDE_FROM_WINDOWS = 1000                 # HSCKMEANS_WIDE_FROM_WINDOWS: auto takes the wide plan from this many windows
MAX_STACK_ELEMENTS = 2 ** 31 - 1         # sum T_b * F of a corpus; of a sparse corpus: its window stack N * 2W * F
F32, F64 = 0, 1                          # HSCKMEANS_F32 / _F64
SKIP, ASSIGN_F32, ASSIGN_F64 = 0, 1, 2   # modes of hsckmeans_step
TIMES = 4                                # upload, assignment, centroids, download

_lib = None


def load_library():
    """Load libhsckmeans.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        vp, ci = ctypes.c_void_p, ctypes.c_int
        _lib = _native.load_satellite(LIB_PATH, 'hsckmeans', {'hsckmeans_set_data': [vp, vp, ci, ci, ci, ci, vp, ci, ci],
                                                              'hsckmeans_set_corpus': [vp, vp, ci, ci, vp, ci, vp, ci, ci],
                                                              'hsckmeans_set_corpus_sparse': [vp, ci, ci, vp, ci, vp, vp, vp, vp, ci, ci],
                                                              'hsckmeans_set_plan': [vp, ci],
                                                              'hsckmeans_step': [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]})
    return _lib


class _Context(_native.LibraryContext):
    def __init__(self, device):
        super(_Context, self).__init__(load_library(), 'hsckmeans', device)

    def set_data(self, x, starts, W):
        """x [B,T,F] float32/float64 C order, starts [B,N] int64."""
        B, T, F = x.shape
        N = starts.shape[1]
        self.B, self.N, self.W, self.F, self.dtype = B, N, W, F, x.dtype
        self.call('set_data', _native._ptr(x), F32 if x.dtype == np.float32 else F64, B, T, F, _native._ptr(starts), N, W)

    def set_corpus(self, x, row_offsets, starts, W):
        """x [rows,F] float32/float64 C order: the stacked signals; row_offsets [B+1], starts [N] (stacked rows) int64.
        Afterwards the context holds one learner (B = 1)."""
        F = x.shape[1]
        N = starts.shape[0]
        self.B, self.N, self.W, self.F, self.dtype = 1, N, W, F, x.dtype
        self.call('set_corpus', _native._ptr(x), F32 if x.dtype == np.float32 else F64, row_offsets.shape[0] - 1,
                  _native._ptr(row_offsets), F, _native._ptr(starts), N, W)

    def set_corpus_sparse(self, indptr, indices, data, F, row_offsets, starts, W):
        """The stacked signals [rows,F] as CSR: indptr [rows+1] int64, indices int32 (ascending in a row), data float32 /
        float64; row_offsets [B+1], starts [N] (stacked rows) int64.  Afterwards the context holds one learner (B = 1) on
        the window stack [N * 2W, F] built on the device; a step's t stays relative to the window."""
        N = starts.shape[0]
        self.B, self.N, self.W, self.F, self.dtype = 1, N, W, F, data.dtype
        self.call('set_corpus_sparse', F32 if data.dtype == np.float32 else F64, row_offsets.shape[0] - 1, _native._ptr(row_offsets), F,
                  _native._ptr(indptr), _native._ptr(indices), _native._ptr(data), _native._ptr(starts), N, W)

    def set_plan(self, plan):
        """PLAN_AUTO, PLAN_LISTS or PLAN_WIDE for the centroid half of the later steps (the same bits either way)."""
        self.call('set_plan', int(plan))

    def step(self, D, mode):
        """D [B,K,W,F] float64, mode [B] int32.  Returns t, k [B,N], count, nonzero [B,K], sums [B,K,W*F], timing [4]."""
        B, K = D.shape[0], D.shape[1]
        t = np.zeros((B, self.N), dtype=np.int32)
        k = np.zeros((B, self.N), dtype=np.int32)
        count = np.zeros((B, K), dtype=np.int32)
        nonzero = np.zeros((B, K), dtype=np.int32)
        sums = np.zeros((B, K, self.W * self.F), dtype=self.dtype)
        timing = np.zeros((TIMES,), dtype=np.float64)
        p = _native._ptr
        self.call('step', p(D), K, p(mode), p(t), p(k), p(count), p(nonzero), p(sums), p(timing))
        return t, k, count, nonzero, sums, timing


_contexts = {}


def _context(device):
    if device not in _contexts:
        _contexts[device] = _Context(device)
    return _contexts[device]


def _rng(rng):
    return np.random if rng is None else rng


def corpus_signals(sequences, lengths=None, who='k-means'):
    """The signals of a corpus as a list of [T_b] or [T_b,F] views: `sequences` [B,T] / [B,T,F], a list / tuple of
    arrays, or a padded array with `lengths` [B] (the ragged forms of modeling.is_ragged).  The padding is not read.
    `who` heads the messages (the learner that calls)."""
    if isinstance(sequences, (list, tuple)):
        if lengths is not None:
            raise ValueError('lengths= goes with a padded array, not with a list of signals')
        seqs = [np.asarray(q) for q in sequences]
    else:
        seq = np.asarray(sequences)
        if seq.ndim != 2 and seq.ndim != 3:
            raise ValueError('%s: the corpus must be [B,T] or [B,T,F] (got %d dimensions)' % (who, seq.ndim))
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
        raise ValueError('%s: a corpus needs at least one signal' % who)
    if seqs[0].ndim not in (1, 2) or any(q.ndim != seqs[0].ndim or q.shape[1:] != seqs[0].shape[1:] for q in seqs):
        raise ValueError('%s: the signals of a corpus must all be [T_b] or all be [T_b,F] with the same F' % who)
    if any(q.dtype != seqs[0].dtype for q in seqs):
        raise ValueError('%s: the signals of a corpus must share one dtype' % who)
    return seqs


def corpus_windows(signals, nb, width, rng=None):
    """extractRandomWindows over a corpus: `nb` windows of `width` samples, drawn uniformly over the admissible starts of
    all signals in ONE randint call (signal b has A_b = T_b - width of them, 0 .. T_b - width - 1, as the reference's
    randint(low=0, high=T - width) leaves them).  Returns (signal [nb], start [nb]) int64 in draw order; for one signal
    the starts are extractRandomWindows' own."""
    A = np.array([q.shape[0] - width for q in signals], dtype=np.int64)
    if np.any(A < 1):
        raise ValueError('signal %d: %d samples leave no window of %d' % (int(np.argmax(A < 1)), signals[int(np.argmax(A < 1))].shape[0], width))
    C = np.cumsum(A)
    g = np.asarray(_rng(rng).randint(low=0, high=int(C[-1]), size=(nb,)), dtype=np.int64)
    b = np.searchsorted(C, g, side='right').astype(np.int64)
    return b, g - (C[b] - A[b])


def sparse_corpus_signals(sequences, lengths=None, who='k-means'):
    """The signals of a sparse corpus, or None when `sequences` is not one: a list / tuple whose items are all scipy.sparse
    matrices [T_b,F] of one dtype and one F.  Returns them as CSR in canonical form (sorted columns, no duplicates), so
    that their entries are the non-zeros of .toarray(); matrices already in that form are not copied."""
    import scipy.sparse
    if not isinstance(sequences, (list, tuple)) or not any(scipy.sparse.issparse(q) for q in sequences):
        return None
    if not all(scipy.sparse.issparse(q) for q in sequences):
        raise ValueError('%s: a corpus is all dense arrays or all scipy.sparse matrices, not a mix of both' % who)
    if lengths is not None:
        raise ValueError('lengths= goes with a padded array, not with a list of sparse signals')
    if any(q.ndim != 2 or q.shape[1] != sequences[0].shape[1] for q in sequences):
        raise ValueError('%s: the sparse signals of a corpus must all be [T_b,F] with the same F' % who)
    if any(q.dtype != sequences[0].dtype for q in sequences):
        raise ValueError('%s: the signals of a corpus must share one dtype' % who)
    seqs = []
    for q in sequences:
        m = q.tocsr()
        if not m.has_canonical_format:
            m = m.copy() if m is q else m
            m.sum_duplicates()
        seqs.append(m)
    return seqs


class DenseStack(object):
    """What trainCorpus reads of a corpus of dense signals stacked without padding: `host` (what the loop cuts its reset
    patches from: the stack [rows] or [rows,F]), the extremes of its elements, the initial atoms, and the upload."""

    def __init__(self, seqs, F):
        self.host = np.concatenate(seqs)                     # the signals' own samples, no padding
        self.dtype, self.F = self.host.dtype, F
        self.row_offsets = np.zeros((len(seqs) + 1,), dtype=np.int64)
        self.row_offsets[1:] = np.cumsum([q.shape[0] for q in seqs])

    def bounds(self):
        return np.min(self.host), np.max(self.host)

    def atoms(self, at, W):
        """[len(at), W, F]: the rows at[i] .. at[i] + W of the stack."""
        return self.host.reshape((-1, self.F))[at[:, np.newaxis] + np.arange(W)[np.newaxis, :]]

    def upload(self, ctx, starts, W):
        ctx.set_corpus(np.ascontiguousarray(self.host.reshape((-1, self.F))), self.row_offsets, starts, W)


class SparseStack(object):
    """DenseStack for a sparse corpus (CSR signals [T_b,F]): every value is the one the dense stack would give.  It is its
    own `host`: dtype, ndim and dense patches stack[s:e], cut from the one signal that holds the stacked rows s .. e."""
    ndim = 2

    def __init__(self, seqs):
        self.seqs = seqs
        self.host = self
        self.dtype = seqs[0].dtype
        self.F = seqs[0].shape[1]
        self.row_offsets = np.zeros((len(seqs) + 1,), dtype=np.int64)
        self.row_offsets[1:] = np.cumsum([q.shape[0] for q in seqs])

    def bounds(self):
        """(np.min, np.max) of the dense stack: the stored entries, and 0 wherever a cell holds none."""
        data = np.concatenate([q.data for q in self.seqs] + [np.zeros((0,), dtype=self.dtype)])
        if data.shape[0] < int(self.row_offsets[-1]) * self.F:
            data = np.concatenate([data, np.zeros((1,), dtype=self.dtype)])
        return np.min(data), np.max(data)

    def __getitem__(self, rows):
        s, e = int(rows.start), int(rows.stop)
        b = int(np.searchsorted(self.row_offsets, s, side='right')) - 1
        assert e <= self.row_offsets[b + 1], 'a patch lies inside one signal'
        lo = int(self.row_offsets[b])
        return self.seqs[b][s - lo:e - lo].toarray()

    def atoms(self, at, W):
        return np.stack([self[int(s):int(s) + W] for s in at])

    def upload(self, ctx, starts, W):
        indptr, indices, data = self.csr()
        ctx.set_corpus_sparse(indptr, indices, data, self.F, self.row_offsets, starts, W)

    def csr(self):
        """(indptr [rows+1] int64, indices int32, data) of the whole stack, as hsckmeans_set_corpus_sparse takes them."""
        indptr = np.zeros((int(self.row_offsets[-1]) + 1,), dtype=np.int64)
        base = 0
        for b, q in enumerate(self.seqs):
            indptr[self.row_offsets[b] + 1:self.row_offsets[b + 1] + 1] = base + q.indptr[1:].astype(np.int64)
            base += int(q.indptr[-1])
        indices = np.concatenate([q.indices.astype(np.int32, copy=False) for q in self.seqs])
        data = np.concatenate([q.data for q in self.seqs])
        return indptr, np.ascontiguousarray(indices), np.ascontiguousarray(data)


def check_corpus_arguments(k, W, seqs, nbRandomWindows, initMethod, resetMethod, sparse=False):
    """The argument checks of trainCorpus (raised before any device call): the rules of check_arguments, the length
    rule for every signal, and the element limit of the stack (sparse: of the window stack, the only dense thing)."""
    W = int(W)
    _, F = check_arguments(k, W, (2 * max(W, 0) + 1,) + seqs[0].shape[1:], seqs[0].dtype, nbRandomWindows, initMethod, resetMethod)
    for b, q in enumerate(seqs):
        if 2 * W >= q.shape[0]:
            raise ValueError('k-means: signal %d has %d samples, windows of 2 * windowSize = %d samples need a longer signal' % (
                b, q.shape[0], 2 * W))
    if sparse:
        if int(nbRandomWindows) * 2 * W * F > MAX_STACK_ELEMENTS:
            raise NotImplementedError('k-means on the GPU: the window stack of a sparse corpus has more than 2^31 - 1 elements')
    elif sum(q.shape[0] for q in seqs) * F > MAX_STACK_ELEMENTS:
        raise NotImplementedError('k-means on the GPU: the corpus has more than 2^31 - 1 elements in all')
    return F


def check_arguments(k, W, data_shape, dtype, nbRandomWindows, initMethod, resetMethod, batch=False):
    """The argument checks of train / trainBatch (raised before any device call)."""
    if initMethod not in INIT_METHODS:
        raise Exception('Unsupported initialization method: %s' % (initMethod))
    if resetMethod not in RESET_METHODS:
        raise Exception('Unsupported reset method: %s' % (resetMethod))
    lead = 1 if batch else 0
    if len(data_shape) - lead not in (1, 2):
        lead_dims = 'B,' if batch else ''
        raise ValueError('k-means: the data must be [%sT] or [%sT,F] (got %d dimensions)' % (lead_dims, lead_dims, len(data_shape)))
    if batch and data_shape[0] < 1:
        raise ValueError('k-means: trainBatch needs at least one sequence')
    if dtype not in (np.float32, np.float64):
        raise ValueError('k-means: the data must be float32 or float64 (got %s)' % dtype)
    if k < 1:
        raise ValueError('k-means: k = %d, needs k >= 1' % k)
    if W < 1 or W > MAX_WINDOW_SIZE:
        raise NotImplementedError('k-means on the GPU: windowSize = %d is outside 1 .. %d' % (W, MAX_WINDOW_SIZE))
    if nbRandomWindows < 1:
        raise ValueError('k-means: nbRandomWindows = %d, needs at least one window' % nbRandomWindows)
    T = data_shape[lead]
    F = 1 if len(data_shape) - lead == 1 else data_shape[lead + 1]
    if F < 1:
        raise ValueError('k-means: no features')
    if 2 * W >= T:
        raise ValueError('k-means: windows of 2 * windowSize = %d samples need a longer signal (T = %d)' % (2 * W, T))
    if W * F < 2:
        raise NotImplementedError('k-means on the GPU: atoms of a single sample (W * F = 1) are not supported')
    return T, F


class ConvolutionalKMeansLearner(object):
    """The reference's convolutional k-means learner (ConvolutionalDictionaryLearner._train_kmean, hsc/modeling.py:420-524)
    with each iteration on the GPU (one hsckmeans_step call), for one learner (train) or a batch (trainBatch).

    lastStats (after train): one dict per iteration with alpha, nbResets, counts [K] (members per centroid, summing to
    nbRandomWindows), step_ms (host wall clock of the synchronised call), assign_ms, centroid_ms and kernel_ms
    (device time of the assignment, of the norms + lists + sums, and of both).  After trainBatch: one such list per
    learner."""

    def __init__(self, k, windowSize, device=0, rng=None):
        self.k = int(k)
        self.windowSize = int(windowSize)
        self.device = device
        self.rng = rng
        self.lastStats = None
        self.lastWindows = None                              # after trainCorpus: (signal [N], start [N]) of the drawn windows
        self.lastSetupSeconds = None                         # after trainCorpus: wall time before the first step (draws, upload)

    def train(self, data, nbRandomWindows, maxIterations=100, tolerance=0.0, initMethod='random_samples',
              resetMethod='noise', nbAveragedPatches=8):
        """hsc/modeling.py:420-524.  data [T] or [T,F] (np.matrix included) float32 / float64; returns D [K,W] or
        [K,W,F] with the host learner's dtype.  Draws from `rng` or numpy's global generator, as the host learner."""
        data = np.asarray(data)
        check_arguments(self.k, self.windowSize, data.shape, data.dtype, nbRandomWindows, initMethod, resetMethod)
        load_library()                                       # no CPU path: fail before the first draw
        Ds, stats = self._run(data[np.newaxis], [self.rng], int(nbRandomWindows), maxIterations, tolerance, initMethod,
                              resetMethod, nbAveragedPatches)
        self.lastStats = stats[0]
        return Ds[0]

    def trainBatch(self, sequences, nbRandomWindows, maxIterations=100, tolerance=0.0, initMethod='random_samples',
                   resetMethod='noise', nbAveragedPatches=8, rngs=None):
        """B independent learners, learner b on sequences[b] ([B,T] or [B,T,F]).  rngs: a list of B generators
        (learner b then reproduces train() with rngs[b]), or one generator / None (numpy's global generator) shared
        by all: every learner's window starts then its D, in batch order, then per iteration the resets of the
        learners still running, learner by learner.  Each learner stops on its own (n < maxIterations and
        alpha > tolerance); a stopped learner is neither updated nor draws.
        Returns (D [B,K,W(,F)] in the learners' common result dtype, per-learner lastStats lists)."""
        sequences = np.asarray(sequences)
        check_arguments(self.k, self.windowSize, sequences.shape, sequences.dtype, nbRandomWindows, initMethod,
                        resetMethod, batch=True)
        B = sequences.shape[0]
        if isinstance(rngs, (list, tuple)):
            if len(rngs) != B:
                raise ValueError('k-means: %d generators for %d learners' % (len(rngs), B))
            rngs = list(rngs)
        else:
            rngs = [rngs] * B
        load_library()
        Ds, stats = self._run(sequences, rngs, int(nbRandomWindows), maxIterations, tolerance, initMethod, resetMethod,
                              nbAveragedPatches)
        self.lastStats = stats
        return np.stack(Ds), stats

    def trainCorpus(self, sequences, nbRandomWindows, maxIterations=100, tolerance=0.0, initMethod='random_samples',
                    resetMethod='noise', nbAveragedPatches=8, lengths=None):
        """`train` for ONE dictionary over a corpus of B signals: `sequences` [B,T] / [B,T,F], a list / tuple of [T_b] or
        [T_b,F] arrays, or a padded array with `lengths` (its padding is never read and may hold NaN); float32 or float64,
        one dtype and one F.  The reference's learner with its window draw taken over all signals (corpus_windows): the
        N windows of 2 * windowSize samples, then _init_D ('random_samples': k windows of windowSize samples by the same
        rule; 'noise': uniform between the smallest and largest sample of the signals), then per iteration the resets
        in centroid order, a reset's randint(0, N) naming a drawn window whose matched patch is cut from its own
        signal.  A corpus of one signal gives `train`'s result on that signal, bit for bit (values and dtype).
        A list / tuple of scipy.sparse matrices [T_b,F] is a sparse corpus (the representations of a level, DESIGN.md section
        19): the same draws and the same result as on [m.toarray() for m in sequences], bit for bit, with no dense copy of
        the corpus on the host or the device; the element limit is then that of the window stack N * 2W * F.
        Returns D [K,W] or [K,W,F]; lastStats as after train, lastWindows = (signal [N], start [N])."""
        t0 = time.perf_counter()
        seqs = sparse_corpus_signals(sequences, lengths)
        sparse = seqs is not None
        if not sparse:
            seqs = corpus_signals(sequences, lengths)
        W, K, N = self.windowSize, self.k, int(nbRandomWindows)
        F = check_corpus_arguments(K, W, seqs, nbRandomWindows, initMethod, resetMethod, sparse=sparse)
        load_library()                                       # no CPU path: fail before the first draw
        rng = _rng(self.rng)
        stack = SparseStack(seqs) if sparse else DenseStack(seqs, F)
        row_offsets = stack.row_offsets
        sig, start = corpus_windows(seqs, N, 2 * W, rng)
        if initMethod == 'noise':                            # _init_D (modeling.py:308-328) over the corpus
            low, high = stack.bounds()
            D = normalize(rng.uniform(low=low, high=high, size=(K, W, F)))
        else:
            ib, it = corpus_windows(seqs, K, W, rng)
            D = normalize(stack.atoms(row_offsets[ib] + it, W))
        if stack.host.ndim == 1:
            D = np.squeeze(D, axis=2)
        starts = (row_offsets[sig] + start)[np.newaxis]      # stacked rows (a sparse corpus: the host's, for the reset patches)
        ctx = _context(self.device)
        stack.upload(ctx, np.ascontiguousarray(starts[0]), W)
        self.lastSetupSeconds = time.perf_counter() - t0
        Ds, stats = self._loop(ctx, [stack.host], starts, [D], [self.rng], stack.dtype, F, maxIterations, tolerance, resetMethod,
                               nbAveragedPatches)
        self.lastStats = stats[0]
        self.lastWindows = (sig, start)
        return Ds[0]

    # ---- the shared loop ---------------------------------------------------------------------------
    def _run(self, seqs, rngs, N, maxIterations, tolerance, initMethod, resetMethod, nbAveragedPatches):
        from .learning import ConvolutionalDictionaryLearner
        B, T = seqs.shape[0], seqs.shape[1]
        W, K = self.windowSize, self.k
        x = np.ascontiguousarray(seqs.reshape((B, T, -1)))
        F = x.shape[2]
        starts = np.zeros((B, N), dtype=np.int64)
        Ds = []
        for b in range(B):                                   # extractRandomWindows, then _init_D (modeling.py:426-429)
            starts[b] = _rng(rngs[b]).randint(low=0, high=T - 2 * W, size=(N,))
            Ds.append(ConvolutionalDictionaryLearner(K, W, rng=rngs[b])._init_D(seqs[b], initMethod))
        ctx = _context(self.device)
        ctx.set_data(x, starts, W)
        return self._loop(ctx, seqs, starts, Ds, rngs, x.dtype, F, maxIterations, tolerance, resetMethod, nbAveragedPatches)

    def _loop(self, ctx, datas, starts, Ds, rngs, xdtype, F, maxIterations, tolerance, resetMethod, nbAveragedPatches):
        """The iterations of the B learners whose data the context holds: datas[b] the host's copy ([T] / [T,F]; a corpus:
        the stack), starts [B,N] its window starts, Ds[b] the initial dictionaries."""
        from .modeling import _compute_dtype
        B, W, K = len(Ds), self.windowSize, self.k
        pshape = (W,) if datas[0].ndim == 1 else (W, F)
        n = [0] * B
        alpha = [tolerance + 1.0] * B
        stats = [[] for _ in range(B)]
        while True:
            running = [b for b in range(B) if n[b] < maxIterations and alpha[b] > tolerance]
            if not running:
                break
            mode = np.zeros((B,), dtype=np.int32)
            D64 = np.zeros((B, K, W, F), dtype=np.float64)
            for b in running:
                mode[b] = ASSIGN_F32 if _compute_dtype(xdtype, Ds[b].dtype) == np.float32 else ASSIGN_F64
                D64[b] = Ds[b].reshape((K, W, F))
            t0 = time.perf_counter()
            at, ak, count, nonzero, sums, timing = ctx.step(D64, mode)
            step_ms = 1e3 * (time.perf_counter() - t0)
            for b in running:
                newD, nbResets = self._finish(datas[b], starts[b], at[b], count[b], nonzero[b], sums[b], Ds[b], pshape,
                                              _rng(rngs[b]), resetMethod, nbAveragedPatches)
                alpha[b] = np.sqrt(np.sum(np.square(Ds[b] - newD)))
                logger.debug('K-mean iteration %d: tolerance = %f, nb resets = %d' % (n[b], alpha[b], nbResets))
                stats[b].append(dict(alpha=float(alpha[b]), nbResets=int(nbResets), counts=count[b].astype(np.int64),
                                     step_ms=step_ms, assign_ms=float(timing[1]), centroid_ms=float(timing[2]),
                                     kernel_ms=float(timing[1] + timing[2]), assignment=(at[b].astype(np.int64), ak[b].astype(np.int64))))
                Ds[b] = newD
                n[b] += 1
        return Ds, stats

    @staticmethod
    def _finish(data, starts, t, count, nonzero, sums, D, pshape, rng, resetMethod, nbAveragedPatches):
        """The reference's computeCentroid (modeling.py:474-503) on the device's sums; resets cut their patches from
        the host's data at start + t."""
        W = pshape[0]
        N = starts.shape[0]

        def patch(i):
            s = int(starts[i]) + int(t[i])
            return data[s:s + W]

        centroids, nbResets = [], 0
        for c in range(D.shape[0]):
            if nonzero[c]:
                # np.mean(normalize(patches[members]), axis=0): the device's sequential sum over m, divided as np.mean does
                S = sums[c].reshape(pshape)
                centroid = np.empty_like(S)
                np.true_divide(S, np.intp(count[c]), out=centroid, casting='unsafe')
            else:
                nbResets += 1
                if resetMethod == 'random_samples':
                    centroid = patch(rng.randint(low=0, high=N))
                elif resetMethod == 'random_samples_average':
                    idx = rng.randint(low=0, high=N, size=(nbAveragedPatches,))
                    centroid = np.mean(np.stack([patch(i) for i in idx]), axis=0)
                else:
                    centroid = rng.uniform(low=-1.0, high=1.0, size=pshape)
            if np.sqrt(np.sum(np.square(centroid))) == 0.0:
                centroid = centroid + 1e-9
            centroids.append(centroid)
        return normalize(np.stack(centroids)), nbResets
