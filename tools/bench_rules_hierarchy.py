"""Times hierarchical batch encodes with an SNR target per signal and level (a 2-D `toleranceSnr`) against
the loop of calls they replace, on the two-level dictionary and signal shape of tools/bench_ragged_hierarchy.py (the config-4
workload of bench.py, bench_hsc.build_workload: level 0 256 atoms x 64 taps, level 1 (256 singletons + 128) atoms x 17 taps x 256
features, nbBlocks=10, singletonWeight 0.95):

  sweep   one signal of 65 536 samples encoded to 16 rows of targets (level 0: 15 .. 30 dB, level 1: 25 .. 40 dB) as ONE uniform
          batch of 16 copies with a table, against 16 calls of computeCoefficientsBatch on the signal alone;
  corpus  64 signals of 16 384 to 65 536 samples (lengths and rows drawn under a fixed seed: level 0 in 20 .. 30 dB, level 1 in
          30 .. 40 dB) as ONE ragged batch with a table, against one call of computeCoefficientsBatch per signal.

Batch and loop alternate, `--reps` times behind one warm-up of each; the figures are the median and the range of the repetitions.
Both forms feed the signals from the host and fetch residual energies only.  Every row of the batch is compared, byte for byte,
with its call of the loop: the matrices of both levels and the energy.

  python tools/bench_rules_hierarchy.py [--out profiles/rules_hierarchy_bench.json] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_hsc  # noqa: E402
from hsc_amd.hierarchical import HierarchicalConvolutionalMatchingPursuit  # noqa: E402


def _same(a, b):
    a, b = a.tocsc(), b.tocsc()
    a.sort_indices(); b.sort_indices()
    return (a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and
            a.data.tobytes() == b.data.tobytes())


def _figures(ms):
    return dict(ms_median=round(float(np.median(ms)), 2), ms_min=round(float(min(ms)), 2), ms_max=round(float(max(ms)), 2),
                ms_all=[round(float(v), 2) for v in ms])


def measure(batch, loop, reps):
    """batch() and loop() alternating; returns (last batch result, last loop results, figures of both)."""
    batch(); loop()                                        # (warm-up: workspaces, capacity hints)
    tb, tl = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        rb = batch()
        t1 = time.perf_counter()
        rl = loop()
        t2 = time.perf_counter()
        tb.append((t1 - t0) * 1e3); tl.append((t2 - t1) * 1e3)
    return rb, rl, _figures(tb), _figures(tl)


def rows_equal(rb, rl):
    """Is row b of the batch what call b of the loop returned: matrices of every level and the residual energy."""
    same = []
    for b, one in enumerate(rl):
        same.append(all(_same(a, e) for a, e in zip(rb[0][b], one[0][0])) and rb[1][b:b + 1].tobytes() == one[1].tobytes())
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--T', type=int, default=65536)
    ap.add_argument('--rows', type=int, default=16)
    ap.add_argument('--signals', type=int, default=64)
    ap.add_argument('--tmin', type=int, default=16384)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_rules_hierarchy.py measures on the GPU and found none')
    mld, xs, kw, desc = bench_hsc.build_workload(4, args.signals, args.T, 0)
    kw = dict(kw)
    kw.pop('toleranceSnr')
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    out = dict(workload=desc, reps=args.reps)

    def describe(res):
        return dict(variants=[t['variant'] for t in res[2]], chunks=[t.get('chunks', 1) for t in res[2]],
                    selections=int(sum(t['selections'] for t in res[2])))

    # one signal, N rows of targets
    N = args.rows
    table = np.stack([np.linspace(15.0, 30.0, N), np.linspace(25.0, 40.0, N)], axis=1)
    copies = np.ascontiguousarray(np.tile(xs[:1], (N, 1)))
    rb, rl, fb, fl = measure(lambda: hcmp.computeCoefficientsBatch(copies, mld, toleranceSnr=table, residuals='energy', **kw),
                             lambda: [hcmp.computeCoefficientsBatch(xs[:1], mld, toleranceSnr=list(table[r]), residuals='energy', **kw) for r in range(N)],
                             args.reps)
    same = rows_equal(rb, rl)
    out['sweep'] = dict(samples=args.T, rows=N, table=[[float(v) for v in r] for r in table], batch=dict(fb, **describe(rb)),
                        loop_of_calls=dict(fl, variants=[t['variant'] for t in rl[-1][2]], selections=int(sum(t['selections'] for one in rl for t in one[2]))),
                        loop_over_batch=round(fl['ms_median'] / fb['ms_median'], 2), rows_byte_identical=int(sum(same)), rows_compared=len(same))

    # a corpus with a row per signal
    rs = np.random.RandomState(args.seed)
    B = args.signals
    lengths = rs.randint(args.tmin, args.T + 1, size=B).astype(np.int32)
    table = np.stack([np.round(rs.uniform(20.0, 30.0, B), 1), np.round(rs.uniform(30.0, 40.0, B), 1)], axis=1)
    ragged = [xs[b, :int(n)] for b, n in enumerate(lengths)]
    rb, rl, fb, fl = measure(lambda: hcmp.computeCoefficientsRaggedBatch(ragged, mld, toleranceSnr=table, residuals='energy', **kw),
                             lambda: [hcmp.computeCoefficientsBatch(ragged[b][np.newaxis], mld, toleranceSnr=list(table[b]), residuals='energy', **kw)
                                      for b in range(B)], args.reps)
    same = rows_equal(rb, rl)
    out['corpus'] = dict(signals=B, lengths=dict(min=int(lengths.min()), max=int(lengths.max()), samples=int(lengths.sum())), seed=args.seed,
                         batch=dict(fb, **describe(rb)),
                         loop_of_calls=dict(fl, variants=[t['variant'] for t in rl[-1][2]], selections=int(sum(t['selections'] for one in rl for t in one[2]))),
                         loop_over_batch=round(fl['ms_median'] / fb['ms_median'], 2), rows_byte_identical=int(sum(same)), rows_compared=len(same))
    out['device'] = torch.cuda.get_device_name(0)
    hcmp.close()
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    if out['sweep']['rows_byte_identical'] != N or out['corpus']['rows_byte_identical'] != B:
        raise SystemExit('a row of a batch differs from its call of the loop')


if __name__ == '__main__':
    main()
