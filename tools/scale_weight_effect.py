"""The effect of the singleton weight on where a hierarchical code puts its coefficients: the loop of the reference's
scripts/scale_weight_effect_mlcsc.py:72-92 over a corpus, without its plots.

For every weight the corpus is encoded one level at a time, as the script does: encodeBatch with the first level of the
dictionary, then for every further level encodeFromLevelBatch on the coefficients in hand with the dictionary up to that
level (method 'cmp', returnDistributed=False), so no level is encoded twice.  Each stage's coefficients are then
redistributed (convertToDistributedCoefficients) and reported per weight:
  - the empirical information rate (bit/sample, hsc_amd.analysis.calculateEmpiricalInformationRates against the whole
    dictionary) per maximum level, mean over the signals;
  - the distribution ratios of the last stage (share of every level in the stored coefficients, over the corpus);
  - the coefficient energy of the last stage against the signal energy.
The optimal rates -- the generator's own events handed down level by level (calculateEmpiricalMultilevelInformationRates)
-- are printed first.  The corpus comes from tools/generate_dataset.py's generator under a seed; --synth takes planted
signals of hsc_amd.synth on a random dictionary instead (no ground-truth events: no optimal rates).

--snr-grid takes several rows of SNR targets (R x levels values, row after row) in place of --snr: per weight all rows are
encoded as ONE batch -- R copies of the corpus, copy r with row r as every signal's targets (a 2-D toleranceSnr, DESIGN.md
section 26) -- and reported row by row.

  python tools/scale_weight_effect.py [--signals 8] [--samples 16384] [--weights 0.5 0.7 0.9 1.0] [--snr 40 30 30] [--blocks 10]
  python tools/scale_weight_effect.py --snr-grid 40 30 30  30 25 25  20 15 15
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import generate_dataset as gd  # noqa: E402
from hsc_amd.analysis import (calculateDistributionRatios, calculateEmpiricalInformationRates,  # noqa: E402
                              calculateEmpiricalMultilevelInformationRates)
from hsc_amd.dataset import convertEventsToSparseMatrices  # noqa: E402
from hsc_amd.modeling import HierarchicalConvolutionalMatchingPursuit, HierarchicalConvolutionalSparseCoder  # noqa: E402


def encode_by_level(x, mld, weight, snrs, nbBlocks, hcmp):
    """coefficientsForScales of the script: [stage][signal] distributed coefficients of an encode up to level `stage`.
    snrs: one target per level, or a table [signals, levels] with a row per signal of x."""
    stages, coefficients = [], None
    for level in range(mld.getNbLevels()):
        coder = HierarchicalConvolutionalSparseCoder(mld.upToLevel(level), hcmp)
        snr = snrs[level] if np.ndim(snrs) == 1 else np.asarray(snrs)[:, :level + 1]      # (the columns of the stage's levels)
        kw = dict(toleranceSnr=snr, nbBlocks=nbBlocks, singletonWeight=weight, returnDistributed=False)
        if level == 0:
            coefficients = coder.encodeBatch(x, **kw)[0]
        else:
            coefficients = coder.encodeFromLevelBatch(x, coefficients, **kw)[0]
        stages.append([hcmp.convertToDistributedCoefficients(c) for c in coefficients])
    return stages


def report(stages, mld, x):
    full = mld.withSingletonBases() if not mld.hasSingletonBases else mld
    rates = [float(np.mean([calculateEmpiricalInformationRates(c, full) for c in stage])) for stage in stages]
    last = stages[-1]
    # the corpus as one code: the matrices of a level stacked in time
    stacked = [scipy.sparse.vstack([c[l] for c in last]).tocsr() for l in range(len(last[0]))]
    ratios = calculateDistributionRatios(stacked)
    energy = float(sum(c.multiply(c).sum() for c in stacked))
    return dict(information_rates=rates, distribution_ratios=[float(r) for r in ratios], coefficient_energy=energy,
                signal_energy=float(np.sum(np.square(np.asarray(x, dtype=np.float64)))), nnz=[int(c.nnz) for c in stacked])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scales', type=int, nargs='+', default=[32, 64, 128])
    ap.add_argument('--counts', type=int, nargs='+', default=[16, 32, 64])
    ap.add_argument('--signals', type=int, default=8)
    ap.add_argument('--samples', type=int, default=16384)
    ap.add_argument('--rate', type=float, default=2e-3)
    ap.add_argument('--weights', type=float, nargs='+', default=[0.5, 0.7, 0.9, 1.0])
    ap.add_argument('--snr', type=float, nargs='+', default=[40.0, 30.0, 30.0, 30.0], help='SNR target per level, dB')
    ap.add_argument('--snr-grid', type=float, nargs='+', default=None,
                    help='several rows of SNR targets, R x levels values row after row: all rows of a weight in one batch')
    ap.add_argument('--blocks', type=int, default=10)
    ap.add_argument('--seed', type=int, default=5)
    ap.add_argument('--synth', action='store_true', help='planted signals of hsc_amd.synth instead of the generator')
    ap.add_argument('--out', default=None, help='also write the figures to this JSON file')
    a = ap.parse_args()
    mld = gd.build(a.scales, counts=a.counts, seed=a.seed, patience=200)
    if len(a.snr) < mld.getNbLevels():
        ap.error('--snr needs one value per level')
    out = dict(scales=a.scales, counts=a.counts, signals=a.signals, samples=a.samples, snr=a.snr[:mld.getNbLevels()], blocks=a.blocks, weights=[])
    grid = None
    if a.snr_grid is not None:
        if len(a.snr_grid) % mld.getNbLevels():
            ap.error('--snr-grid needs rows of %d values, one per level' % mld.getNbLevels())
        grid = np.asarray(a.snr_grid, dtype=np.float64).reshape((-1, mld.getNbLevels()))
        out['snr'] = None
        out['snr_grid'] = grid.tolist()
    if a.synth:
        import hsc_amd.synth as synth
        x = synth.make_batch(np.asarray(mld.getBaseDictionary()), a.samples, 0, a.signals, kind='planted',
                             nb_atoms=max(8, int(a.rate * a.samples * a.counts[0])), seed=a.seed, dtype=np.float32)
    else:
        x, events = gd.signals(mld, a.signals, a.samples, rate=a.rate, compression=None, seed=a.seed)[:2]
        optimal = np.mean([calculateEmpiricalMultilevelInformationRates(convertEventsToSparseMatrices(ev, mld.counts, a.samples), mld)
                           for ev in events], axis=0)
        out['optimal_information_rates'] = [float(v) for v in optimal]
        print('optimal information rate per maximum level (bit/sample):', ' '.join('%.4f' % v for v in optimal), flush=True)
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    try:
        for weight in a.weights:
            if grid is not None:
                # all rows in one batch: copy r of the corpus with row r for every signal
                S = len(x)
                t0 = time.perf_counter()
                stages = encode_by_level(np.concatenate([x] * len(grid), axis=0), mld, weight, np.repeat(grid, S, axis=0), a.blocks, hcmp)
                seconds = time.perf_counter() - t0
                rows = []
                for r, targets in enumerate(grid):
                    rows.append(dict(snr=targets.tolist(), **report([stage[r * S:(r + 1) * S] for stage in stages], mld, x)))
                    print('weight %.2f, targets %s dB: rate per maximum level %s bit/sample; distribution %s; coefficient energy %.6g of signal '
                          'energy %.6g' % (weight, ' '.join('%g' % v for v in targets), ' '.join('%.4f' % v for v in rows[-1]['information_rates']),
                                           ' '.join('%.3f' % v for v in rows[-1]['distribution_ratios']), rows[-1]['coefficient_energy'],
                                           rows[-1]['signal_energy']), flush=True)
                out['weights'].append(dict(weight=weight, encode_s=seconds, rows=rows))
                print('weight %.2f: %d rows in one batch of %d signals (%.2f s)' % (weight, len(grid), len(grid) * S, seconds), flush=True)
                continue
            t0 = time.perf_counter()
            stages = encode_by_level(x, mld, weight, a.snr, a.blocks, hcmp)
            row = dict(weight=weight, encode_s=time.perf_counter() - t0, **report(stages, mld, x))
            out['weights'].append(row)
            print('weight %.2f: rate per maximum level %s bit/sample; distribution %s; coefficient energy %.6g of signal energy %.6g (%.2f s)' % (
                weight, ' '.join('%.4f' % v for v in row['information_rates']), ' '.join('%.3f' % v for v in row['distribution_ratios']),
                row['coefficient_energy'], row['signal_energy'], row['encode_s']), flush=True)
    finally:
        hcmp.close()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
