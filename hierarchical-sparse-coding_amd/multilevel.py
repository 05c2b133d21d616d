"""Multilevel dictionary learning from a corpus on MI355X: the level loop of the reference's headline experiment
(scripts/learn_mlcsc_dataset.py:84-116) over many signals.  DESIGN.md section 19.

Per level: convolutional k-means on the current representation (hsc_amd.kmeans.ConvolutionalKMeansLearner.trainCorpus:
ONE dictionary from all signals), the multilevel dictionary of the levels learnt so far, and one batch encode of the
corpus with it (HierarchicalConvolutionalMatchingPursuit.computeCoefficientsBatch) whose last-level coefficient
matrices are the next level's input.  Those matrices stay sparse from the encoder to the learner: the k-means library
builds its windows from their non-zeros on the device (hsckmeans_set_corpus_sparse), so no [T, K] dense representation
exists on the host or the device.

There is no CPU path: without the native libraries or a visible GPU the calls raise hsc_amd._native.HscmpError.
"""
import collections.abc
import logging
import time

import numpy as np

from .dataset import MultilevelDictionary, addSingletonBases, scalesToWindowSizes
from .kmeans import ConvolutionalKMeansLearner
from .modeling import is_ragged, ragged_signals

logger = logging.getLogger(__name__)

METHODS = ('cmp', 'locomp')


class MultilevelDictionaryLearner(object):
    """counts[l] atoms at level l, scales[l] its input-level scale (the widths are scalesToWindowSizes(scales)); `method` is
    the hierarchical coder's ('locomp', the reference's default, or 'cmp').  One generator `rng` (None: numpy's global
    one) serves the k-means learners of all levels, in level order.

    lastStats (after trainCorpus): one dict per level with kmeans (the learner's lastStats), input_shape ((B, T, F) of
    the level's input), input_nnz (its stored non-zeros; level 0: None), setup_s (k-means before its first step: draws,
    packing, upload and window build), learn_s, encode_s (wall time of the batch encode -- of the resumed one under
    resume=True; the last level: None), encode_timings (the encoder's per-level timings of that encode: a level that was
    not run again has variant 'loaded') and encode_nnz (coefficients stored in the matrices handed to the next level)."""

    def __init__(self, counts, scales, method='locomp', device=0, rng=None):
        self.counts = [int(k) for k in counts]
        self.scales = np.asarray(scales)
        self.method = method
        self.device = device
        self.rng = rng
        self.lastStats = None
        self.lastDictionaries = None                         # after trainCorpus: the learnt [K_l, W_l(, F_l)] of every level, without singleton bases

    def _check_setup(self):
        if self.method in ('mptk-mp', 'mptk-cmp'):
            raise NotImplementedError("method='%s' needs the external MPTK toolkit, which this engine does not bind; "
                                      "use method='cmp' or 'locomp'" % self.method)
        if self.method not in METHODS:
            raise Exception('Unsupported sparse coding method: %s' % (self.method))
        if len(self.counts) != len(self.scales):
            raise ValueError('multilevel learner: %d counts for %d scales' % (len(self.counts), len(self.scales)))
        if len(self.counts) < 1:
            raise ValueError('multilevel learner: needs at least one level')

    def _check(self, sequences, lengths):
        self._check_setup()
        if is_ragged(sequences, lengths):
            raise NotImplementedError('multilevel learner: signals of different lengths are not supported: the hierarchical batch encode '
                                      '(HierarchicalConvolutionalMatchingPursuit.computeCoefficientsBatch) has no ragged form; '
                                      'use trainRaggedCorpus')
        sequences = np.asarray(sequences)
        if sequences.ndim not in (2, 3):
            raise ValueError('multilevel learner: the corpus must be [B,T] or [B,T,F] (got %d dimensions)' % sequences.ndim)
        if sequences.shape[0] < 1:
            raise ValueError('multilevel learner: a corpus needs at least one signal')
        return sequences

    def train(self, sequence, nbRandomWindows, **kwargs):
        """One signal [T] or [T,F]: trainCorpus on a corpus of that signal."""
        return self.trainCorpus(np.asarray(sequence)[np.newaxis], nbRandomWindows, **kwargs)

    def trainCorpus(self, sequences, nbRandomWindows, maxIterations=100, tolerance=0.0, initMethod='random_samples',
                    resetMethod='noise', nbAveragedPatches=8, toleranceSnr=None, nbBlocks=1, singletonWeight=0.5, lengths=None,
                    resume=True):
        """`sequences` [B,T] or [B,T,F].  The k-means arguments go to every level's trainCorpus; toleranceSnr (one value,
        one per level, or -- method='cmp' -- a table [B, >= nbLevels - 1] with a target per signal and level, DESIGN.md section
        26), nbBlocks and singletonWeight to every encode.  Returns the MultilevelDictionary of all levels
        (levels >= 1 with their singleton bases, as the reference builds it).
        resume=True: from level 1 on, the hand-off encode carries on from the previous pass's coefficients
        (computeCoefficientsFromLevelBatch, as the reference's script calls encodeFromLevel) and runs the new level only;
        resume=False encodes the levels below again.  The dictionaries are the same bit for bit either way: the lower
        levels' dictionaries and parameters have not changed."""
        sequences = self._check(sequences, lengths)
        kmeans = dict(maxIterations=maxIterations, tolerance=tolerance, initMethod=initMethod, resetMethod=resetMethod, nbAveragedPatches=nbAveragedPatches)
        encode = dict(toleranceSnr=toleranceSnr, nbBlocks=nbBlocks, singletonWeight=singletonWeight, returnDistributed=False)
        return self._levels(sequences, False, nbRandomWindows, kmeans, encode, resume)

    def trainRaggedCorpus(self, sequences, nbRandomWindows, maxIterations=100, tolerance=0.0, initMethod='random_samples',
                          resetMethod='noise', nbAveragedPatches=8, toleranceSnr=None, nbBlocks=1, singletonWeight=0.5, lengths=None,
                          resume=True):
        """trainCorpus over a corpus of signals of different lengths (method='cmp'): `sequences` a list / tuple of arrays [T_b]
        or [T_b,F], or a padded array [B,T(,F)] with `lengths` [B].  The level loop is trainCorpus's: k-means takes the ragged
        list -- from level 1 the list of sparse (T_b, K) matrices --, and the hand-off encodes are
        HierarchicalConvolutionalMatchingPursuit.computeCoefficientsRaggedBatch / computeCoefficientsFromLevelRaggedBatch, so
        every signal is encoded at its own length.  A corpus whose lengths are all equal gives
        trainCorpus's dictionaries.  lastStats is as for trainCorpus, with input_shape the list of per-signal input shapes."""
        if self.method == 'locomp':
            raise NotImplementedError('multilevel learner: the LoCOMP loop has no ragged form (signals of different lengths): use method=\'cmp\'')
        self._check_setup()
        if not is_ragged(sequences, lengths):
            raise ValueError('multilevel learner: a plain array without lengths= is a uniform corpus: use trainCorpus')
        wmax = int(max(scalesToWindowSizes(self.scales)))          # (every level's k-means draws windows of its width)
        try:
            _, seqs = ragged_signals(sequences, lengths, wmax)
        except ValueError as ex:
            raise ValueError('multilevel learner: %s' % str(ex).replace('the filters (W=', 'the widest filter of the levels (W='))
        kmeans = dict(maxIterations=maxIterations, tolerance=tolerance, initMethod=initMethod, resetMethod=resetMethod, nbAveragedPatches=nbAveragedPatches)
        encode = dict(toleranceSnr=toleranceSnr, nbBlocks=nbBlocks, singletonWeight=singletonWeight, returnDistributed=False)
        return self._levels(seqs, True, nbRandomWindows, kmeans, encode, resume)

    def _levels(self, sequences, ragged, nbRandomWindows, kmeans, encode, resume):
        """The level loop of trainCorpus (`sequences` [B,T(,F)]) and trainRaggedCorpus (a list of [T_b(,F)] arrays)."""
        from .hierarchical import HierarchicalConvolutionalMatchingPursuit
        toleranceSnr = encode['toleranceSnr']
        snr_table = None
        if toleranceSnr is not None and np.ndim(toleranceSnr) == 2:
            # a target per signal and level: rows are signals, so the level count is the second axis
            snr_table = np.asarray(toleranceSnr, dtype=np.float64)
            if snr_table.shape[0] != len(sequences) or snr_table.shape[1] < len(self.counts) - 1:
                raise ValueError('multilevel learner: toleranceSnr has shape %s, the corpus %d signals and the encodes run up to level %d' % (
                    snr_table.shape, len(sequences), len(self.counts) - 2))
        elif toleranceSnr is not None and isinstance(toleranceSnr, collections.abc.Iterable) and len(toleranceSnr) < len(self.counts) - 1:
            raise ValueError('multilevel learner: toleranceSnr has %d values, the encodes run up to level %d' % (
                len(toleranceSnr), len(self.counts) - 2))
        nbLevels = len(self.counts)
        widths = scalesToWindowSizes(self.scales)
        B = len(sequences)
        hcmp = HierarchicalConvolutionalMatchingPursuit(method=self.method, device=self.device)
        encode_all = hcmp.computeCoefficientsRaggedBatch if ragged else hcmp.computeCoefficientsBatch
        encode_from = hcmp.computeCoefficientsFromLevelRaggedBatch if ragged else hcmp.computeCoefficientsFromLevelBatch
        dictionaries, stats = [], []
        inputs, mld, coefficients = sequences, None, None
        try:
            for level in range(nbLevels):
                sparse = level > 0
                t0 = time.perf_counter()
                learner = ConvolutionalKMeansLearner(self.counts[level], int(widths[level]), device=self.device, rng=self.rng)
                D = learner.trainCorpus(inputs, nbRandomWindows, **kmeans)
                t1 = time.perf_counter()
                dictionaries.append(D)
                if level > 0:
                    mld = MultilevelDictionary.fromRawDictionaries(addSingletonBases(dictionaries), self.scales[:level + 1], hasSingletonBases=True)
                else:
                    mld = MultilevelDictionary.fromRawDictionaries(dictionaries, self.scales[:1])
                t2 = time.perf_counter()
                st = dict(kmeans=learner.lastStats, learn_s=t1 - t0, setup_s=learner.lastSetupSeconds,
                          input_shape=[tuple(m.shape) for m in inputs] if ragged else (B,) + tuple(inputs[0].shape) if sparse else tuple(sequences.shape),
                          input_nnz=int(sum(m.nnz for m in inputs)) if sparse else None, encode_s=None, encode_nnz=None, encode_timings=None)
                if level < nbLevels - 1:
                    if snr_table is not None:
                        encode = dict(encode, toleranceSnr=snr_table[:, :level + 1])      # (the columns of this pass's levels)
                    if resume and level > 0:
                        # (the levels below keep the last pass's dictionaries and parameters: their coefficients are in hand)
                        coefficients, _, st['encode_timings'] = encode_from(sequences, coefficients, mld, **encode)
                    else:
                        # (resume=False: the levels below are encoded again, to the same bits)
                        coefficients, _, st['encode_timings'] = encode_all(sequences, mld, **encode)
                    inputs = [c[-1] for c in coefficients]
                    st['encode_s'] = time.perf_counter() - t2
                    st['encode_nnz'] = int(sum(m.nnz for m in inputs))
                logger.debug('level %d: dictionary %s learnt in %.2f s, encode %s' % (level, D.shape, st['learn_s'], st['encode_s']))
                stats.append(st)
        finally:
            hcmp.close()
        self.lastStats = stats
        self.lastDictionaries = dictionaries
        return mld
