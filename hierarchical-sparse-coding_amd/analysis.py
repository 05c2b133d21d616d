"""Information-rate bookkeeping (reference: hsc/analysis.py:37-159).

The closed-form rate model the signal generator depends on (bits per event x Poisson rates, redistributed down
the decomposition tree), and the empirical counters that the scale-weight experiment reports with
(tools/scale_weight_effect.py): bit/sample of a set of coefficient matrices, the same with the events handed
down level by level, and the share of every level in the coefficients.  Host functions; the plots of
hsc/analysis.py are not provided.
"""
import collections.abc

import numpy as np
import scipy.sparse


def calculateBitForDatatype(dtype):
    """Bits of one amplitude of `dtype` (hsc/analysis.py:37-44): sign + exponent + fraction, or the
    integer width."""
    dtype = np.dtype(dtype)
    if np.issubdtype(dtype, np.floating):
        info = np.finfo(dtype)
        return 1 + info.iexp + info.nmant
    if np.issubdtype(dtype, np.integer):
        return np.iinfo(dtype).bits
    raise Exception('Unsupported datatype: %s' % (str(dtype)))


def calculateBitForLevels(multilevelDict, sequenceLength, dtype=np.float32):
    """Bits of one event per level: level index + atom index + time index + amplitude
    (hsc/analysis.py:46-57)."""
    atom_bits = np.ceil(np.log(multilevelDict.counts) / np.log(2))
    level_bits = np.ceil(np.log(len(multilevelDict.scales)) / np.log(2))
    time_bits = np.ceil(np.log(sequenceLength) / np.log(2))
    return level_bits + atom_bits + time_bits + calculateBitForDatatype(dtype)


def calculateInformationRate(multilevelDict, rates, sequenceLength, dtype=np.float32):
    """Average bit/sample of independent Poisson event streams (hsc/analysis.py:59-70)."""
    assert len(rates) == multilevelDict.getNbLevels()
    bits = calculateBitForLevels(multilevelDict, sequenceLength, dtype)
    total = 0.0
    for level in range(multilevelDict.getNbLevels()):
        total += np.sum(rates[level] * bits[level])
    return total


def calculateMultilevelInformationRates(multilevelDict, rates, sequenceLength, dtype=np.float32):
    """Bit/sample when the events are expressed at level L, L-1, ..., 0: the rate of every atom of the
    top level is handed down to the atoms of its decomposition, level by level
    (hsc/analysis.py:72-101).  Returns one figure per level, index 0 = everything at the base level.
    (As in the reference, the per-event bit budget is always the float32 one.)"""
    nbLevels = multilevelDict.getNbLevels()
    assert len(rates) == nbLevels
    if not isinstance(rates[0], collections.abc.Iterable):
        rates = [rates[level] * np.ones(multilevelDict.counts[level]) for level in range(nbLevels)]
    out = []
    for level in reversed(range(nbLevels)):
        out.append(calculateInformationRate(multilevelDict, rates, sequenceLength))
        if level > 0:
            for n, (rate, entry) in enumerate(zip(rates[level], multilevelDict.decompositions[level - 1])):
                for l, i in zip(entry[0], entry[1]):
                    rates[l][i] += rate
                rates[level][n] = 0.0
            assert np.allclose(np.sum(rates[level]), 0.0)
    return np.array(out)[::-1]


def calculateEmpiricalMultilevelInformationRates(coefficients, multilevelDict):
    """Bit/sample of the coefficient matrices [T, K_l] when their events are expressed at level L, L-1, ..., 0
    (hsc/analysis.py:103-137): the signed event counts of every level are handed down to the atoms of the
    decomposition, level by level.  As in the reference, an event handed down lands in the row given by the
    decomposition's OWN time index (not shifted by the event's position), so T must exceed the largest scale.
    Returns one figure per level, index 0 = everything at the base level."""
    nbLevels = multilevelDict.getNbLevels()
    assert len(coefficients) == nbLevels
    counts = [c.conj().sign().tolil().astype(int) for c in coefficients]
    sequenceLength = coefficients[0].shape[0]
    out = []
    for level in reversed(range(nbLevels)):
        bits = calculateBitForLevels(multilevelDict, sequenceLength, dtype=coefficients[0].dtype)
        sparseBits = np.sum([counts[l].sum() * bits[l] for l in range(nbLevels)])
        out.append(float(sparseBits) / sequenceLength)
        if level > 0:
            c = counts[level].tocoo()
            for tIdx, fIdx, n in zip(c.row, c.col, c.data):
                selectedLevels, fIndices, tIndices, _ = multilevelDict.decompositions[level - 1][fIdx]
                for l, t, f in zip(selectedLevels, tIndices, fIndices):
                    counts[l][t, f] += n
                counts[level][tIdx, fIdx] -= n
            assert counts[level].sum() == 0
    return np.array(out)[::-1]


def calculateEmpiricalInformationRates(coefficients, multilevelDict):
    """Bit/sample of the events of every level (hsc/analysis.py:139-153).  coefficients[level]: a sparse matrix
    (its stored entries are the events) or a dense array of events, one per row."""
    sequenceLength = coefficients[0].shape[0]
    bits = calculateBitForLevels(multilevelDict, sequenceLength, dtype=coefficients[0].dtype)
    sparseBits = 0
    for level in range(len(coefficients)):
        if scipy.sparse.issparse(coefficients[level]):
            nbEvents = coefficients[level].nnz
        else:
            nbEvents = coefficients[level].shape[0]
        sparseBits += nbEvents * bits[level]
    return float(sparseBits) / sequenceLength


def calculateDistributionRatios(coefficients):
    """Share of every level in the stored coefficients (hsc/analysis.py:155-159)."""
    total = np.sum([c.nnz for c in coefficients])
    return np.array([float(c.nnz) / total for c in coefficients])
