"""Times the two centroid plans of libhsckmeans.so (include/hsckmeans.h: 1 = member tables and one thread per element,
2 = wide) on a corpus: 1024 signals x 16 384 samples of the level-style data tools/bench_kmeans.py synthesizes, stacked
by hsckmeans_set_corpus, with windows drawn by hsc_amd.kmeans.corpus_windows.

  level 0: K = 16, W = 32, F = 1,  float32, N = 10 000, 100 000 and 1 000 000
  level 1: K = 32, W = 33, F = 16, float64, N = 100 000
  scan:    the level-0 shape at N = 1 000 .. 1 000 000, from which HSCKMEANS_WIDE_FROM_WINDOWS is read

The dictionary is the one trainCorpus reaches after three iterations on 10 000 windows.  For every shape the two plans
alternate in one process on the same uploaded data: one unmeasured step each, then 5 measured steps each; the figures
are the device milliseconds (HIP events) of the assignment and of the centroid part (norms, membership, sums), median
of 5 with [min, max], and every step's outputs are compared byte for byte with plan 1's.  A plan that cannot run (plan
1's [K][N] table not allocated or beyond its index range) is recorded with its error instead of a time.

  python tools/bench_kmeans_corpus.py [--out profiles/kmeans_corpus_bench.json] [--signals 1024] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_kmeans import level_data  # noqa: E402
from hsc_amd import _native, kmeans  # noqa: E402
from hsc_amd.kmeans import ConvolutionalKMeansLearner  # noqa: E402

REPS = 5


def corpus(B, T, F):
    sigs = [level_data(T, F, 1000 + b) for b in range(B)]
    return sigs


def time_plans(ctx, x, ro, sigs, N, W, D, mode, seed):
    sig, start = kmeans.corpus_windows(sigs, N, 2 * W, np.random.RandomState(seed))
    ctx.set_corpus(x, ro, np.ascontiguousarray(ro[sig] + start), W)
    row = dict(N=N, K=int(D.shape[1]), W=W, F=int(x.shape[1]), dtype=str(x.dtype), auto_plan=2 if N >= kmeans.WIDE_FROM_WINDOWS else 1)
    ref, times, errors = None, {1: [], 2: []}, {}
    for rep in range(REPS + 1):                              # rep 0: buffers and first launches, not measured
        for plan in (1, 2):
            if plan in errors:
                continue
            ctx.set_plan(plan)
            try:
                out = ctx.step(D, mode)
            except _native.HscmpError as e:
                errors[plan] = str(e)
                continue
            got = [a.tobytes() for a in out[:5]]
            if ref is None:
                ref = got
                row['largest_centroid'] = int(out[2].max())
            elif got != ref:
                raise AssertionError('plan %d: outputs differ from the first step at N = %d' % (plan, N))
            if rep:
                times[plan].append((float(out[5][1]), float(out[5][2])))
    ctx.set_plan(kmeans.PLAN_AUTO)
    for plan in (1, 2):
        if plan in errors:
            row['plan%d_error' % plan] = errors[plan]
            continue
        a = np.array(times[plan])
        for j, name in enumerate(('assign', 'centroid')):
            row['plan%d_%s_ms' % (plan, name)] = float(np.median(a[:, j]))
            row['plan%d_%s_ms_range' % (plan, name)] = [float(a[:, j].min()), float(a[:, j].max())]
    row['identical'] = True
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmeans_corpus_bench.json'))
    ap.add_argument('--signals', type=int, default=1024)
    ap.add_argument('--quick', action='store_true', help='level 0 at two window counts only (a rehearsal)')
    a = ap.parse_args()
    B, T = a.signals, 16384
    ctx = kmeans._context(0)
    out = dict(signals=B, T=T, repetitions=REPS, levels=[], scan=[])
    shapes = [(0, 16, 32, 1, [10000, 100000, 1000000]), (1, 32, 33, 16, [100000])]
    if a.quick:
        shapes = [(0, 16, 32, 1, [10000, 100000])]
    for level, K, W, F, Ns in shapes:
        t0 = time.perf_counter()
        sigs = corpus(B, T, F)
        x = np.ascontiguousarray(np.concatenate(sigs).reshape((-1, F)))
        ro = np.arange(B + 1, dtype=np.int64) * T
        learner = ConvolutionalKMeansLearner(K, W, rng=np.random.RandomState(1))
        D = learner.trainCorpus(sigs, 10000, maxIterations=3, resetMethod='random_samples')
        f32 = x.dtype == np.float32 and D.dtype == np.float32
        mode = np.array([kmeans.ASSIGN_F32 if f32 else kmeans.ASSIGN_F64], dtype=np.int32)
        D64 = np.ascontiguousarray(D.reshape((1, K, W, F)).astype(np.float64))
        print('level %d: corpus and dictionary in %.1f s' % (level, time.perf_counter() - t0), flush=True)
        for N in Ns:
            row = dict(level=level, **time_plans(ctx, x, ro, sigs, N, W, D64, mode, 7))
            out['levels'].append(row)
            print(json.dumps(row), flush=True)
        if level == 0:
            for N in ([1000, 4000, 16000] if a.quick else [1000, 2000, 4000, 8000, 16000, 32000, 64000, 125000, 250000, 500000, 1000000]):
                row = time_plans(ctx, x, ro, sigs, N, W, D64, mode, 8)
                out['scan'].append(row)
                print(json.dumps(row), flush=True)
    out['wide_from_windows'] = kmeans.WIDE_FROM_WINDOWS
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
