"""Times a ragged hierarchical encode (HierarchicalConvolutionalMatchingPursuit.computeCoefficientsRaggedBatch, DESIGN.md section
21) on the config-4 workload of bench.py (bench_hsc.build_workload: 2 levels, level 0 256 atoms x 64 taps, level 1 (256 singletons
+ 128) atoms x 17 taps x 256 features, toleranceSnr [30, 40], nbBlocks=10, singletonWeight 0.95, B = 1024) against, in the same
process:
  - the uniform encode of the same signals at their full length T = 65536 (what padding every signal to the longest costs);
  - one uniform encode per signal (a batch of one) on the first `--loop-signals` ragged signals, scaled up to the batch.
Signal b of the ragged batch is the first lengths[b] samples of signal b of the workload; the lengths are drawn uniformly from
[16384, 65536] under a fixed seed.  All three feed the signals from the host and fetch residual energies only.  Each signal the
per-signal loop encodes is also compared, bit for bit, with its row of the ragged batch: matrices of both levels and the energy.

  python tools/bench_ragged_hierarchy.py [--out profiles/ragged_hierarchy_bench.json] [--steps 3] [--warmup 1]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--B', type=int, default=1024)
    ap.add_argument('--tmin', type=int, default=16384)
    ap.add_argument('--tmax', type=int, default=65536)
    ap.add_argument('--loop-signals', type=int, default=32)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_ragged_hierarchy.py measures on the GPU and found none')
    B = args.B
    mld, xs, kw, desc = bench_hsc.build_workload(4, B, args.tmax, 0)
    lengths = np.random.RandomState(args.seed).randint(args.tmin, args.tmax + 1, size=B).astype(np.int32)
    ragged = [xs[b, :int(n)] for b, n in enumerate(lengths)]
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')

    def timed(step):
        for _ in range(args.warmup):
            step()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = step()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        sel = int(sum(t['selections'] for t in res[2]))
        return res, dict(ms_per_batch=round(ms, 2), selections=sel, selections_per_s=round(sel / (ms * 1e-3), 1),
                         variants=[t['variant'] for t in res[2]], chunks=[t.get('chunks', 1) for t in res[2]],
                         kernel_ms=[[round(float(v), 3) for v in t['kernel_ms']] for t in res[2]])

    out = dict(workload=desc + '; ragged lengths uniform in [%d, %d], seed %d' % (args.tmin, args.tmax, args.seed),
               lengths=dict(min=int(lengths.min()), max=int(lengths.max()), mean=float(lengths.mean()), samples=int(lengths.sum())),
               steps=args.steps, warmup=args.warmup)
    res_r, out['ragged'] = timed(lambda: hcmp.computeCoefficientsRaggedBatch(ragged, mld, residuals='energy', **kw))
    out['ragged']['samples'] = int(lengths.sum())
    _, out['uniform_T%d' % args.tmax] = timed(lambda: hcmp.computeCoefficientsBatch(xs, mld, residuals='energy', **kw))
    out['uniform_T%d' % args.tmax]['samples'] = B * args.tmax

    # one uniform encode per signal (B = 1 each), the first `loop-signals` ragged signals, scaled to the batch
    n = min(args.loop_signals, B)
    hcmp.computeCoefficientsBatch(ragged[0][np.newaxis], mld, residuals='energy', **kw)          # (warm-up)
    t0 = time.perf_counter()
    results = [hcmp.computeCoefficientsBatch(ragged[b][np.newaxis], mld, residuals='energy', **kw) for b in range(n)]
    loop_s = time.perf_counter() - t0
    same = True
    for b, one in enumerate(results):
        same = same and all(_same(a, e) for a, e in zip(res_r[0][b], one[0][0]))
        same = same and res_r[1][b:b + 1].tobytes() == one[1].tobytes()
    per_signal_ms = loop_s * 1e3 / n
    out['per_signal_loop'] = dict(signals_timed=n, ms_per_signal=round(per_signal_ms, 2), ms_per_batch_scaled=round(per_signal_ms * B, 1))
    out['output_check'] = dict(ragged_rows_equal_per_signal_encodes=bool(same), signals_compared=n)
    out['speedup_ragged_over_per_signal_loop'] = round(out['per_signal_loop']['ms_per_batch_scaled'] / out['ragged']['ms_per_batch'], 1)
    out['ragged_over_uniform_Tmax'] = round(out['ragged']['ms_per_batch'] / out['uniform_T%d' % args.tmax]['ms_per_batch'], 3)
    out['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    hcmp.close()


if __name__ == '__main__':
    main()
