"""Golden vectors of the reference's empirical information-rate functions (hsc/analysis.py:103-159)
-> tests/golden/analysis.npz.

Needs the reference next to the repository (loaded read-only through oracle/ref_loader.py); run from the
repository root:  python tools/make_golden_analysis.py

The fixture: a 3-level dictionary from the reference's MultilevelDictionaryGenerator under a fixed seed, T = 2048 (above
the largest scale: the redistribution writes to the decomposition's own time indices), events from its SignalGenerator,
turned into per-level sparse matrices by its convertEventsToSparseMatrices.  Only data is stored:
  counts, scales                   of the dictionary
  dec{l}_ptr / _levels / _findices / _tindices    the decompositions of level l >= 1, entry n in [ptr[n], ptr[n+1])
  m{l}_data / _indices / _indptr / _shape         the matrices (CSC)
  ev{l}                            the events of level l as a dense array, one row (time, index, coefficient) each
  multilevel_rates, rate, rate_dense, ratios      what the reference returned: calculateEmpiricalMultilevelInformationRates
                                   and calculateEmpiricalInformationRates on the matrices, the latter on the dense event
                                   arrays, calculateDistributionRatios on the matrices
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'analysis.npz')
T = 2048


def main():
    ref = ref_loader.load_reference()
    if ref is None:
        raise SystemExit('the reference is not available')
    np.random.seed(31)
    mld = ref.dataset.MultilevelDictionaryGenerator().generate(scales=[8, 16, 32], counts=[6, 8, 8], decompositionSize=3,
                                                               multilevelDecomposition=True, maxNbPatternsConsecutiveRejected=50)
    np.random.seed(32)
    gen = ref.dataset.SignalGenerator(mld, [0.01, 0.01, 0.01])
    events = gen.generateEvents(T)
    matrices = ref.dataset.convertEventsToSparseMatrices(events, mld.counts, T)
    out = {'counts': np.asarray(mld.counts, dtype=np.int64), 'scales': np.asarray(mld.scales, dtype=np.int64), 'T': np.int64(T)}
    for l in range(1, mld.getNbLevels()):
        dec = mld.decompositions[l - 1]
        out['dec%d_ptr' % l] = np.cumsum([0] + [len(d[0]) for d in dec]).astype(np.int64)
        out['dec%d_levels' % l] = np.concatenate([np.asarray(d[0], dtype=np.int64) for d in dec])
        out['dec%d_findices' % l] = np.concatenate([np.asarray(d[1], dtype=np.int64) for d in dec])
        out['dec%d_tindices' % l] = np.concatenate([np.asarray(d[2], dtype=np.int64) for d in dec])
    dense = []
    for l, m in enumerate(matrices):
        c = m.tocsc()
        out['m%d_data' % l], out['m%d_indices' % l], out['m%d_indptr' % l] = c.data, c.indices, c.indptr
        out['m%d_shape' % l] = np.asarray(c.shape, dtype=np.int64)
        coo = c.tocoo()
        dense.append(np.stack((coo.row.astype(c.dtype), coo.col.astype(c.dtype), coo.data), axis=1))
        out['ev%d' % l] = dense[-1]
    # (the multilevel function edits copies it makes itself: the matrices stay as stored)
    out['multilevel_rates'] = np.asarray(ref.analysis.calculateEmpiricalMultilevelInformationRates(matrices, mld))
    out['rate'] = np.asarray(ref.analysis.calculateEmpiricalInformationRates(matrices, mld))
    out['rate_dense'] = np.asarray(ref.analysis.calculateEmpiricalInformationRates(dense, mld))
    out['ratios'] = np.asarray(ref.analysis.calculateDistributionRatios(matrices))
    np.savez_compressed(OUT, **out)
    print('analysis:', [m.nnz for m in matrices], 'events;', out['multilevel_rates'], float(out['rate']), float(out['rate_dense']),
          out['ratios'], os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
