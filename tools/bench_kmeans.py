"""Times the host k-means learner (ConvolutionalDictionaryLearner(algorithm='kmean'): assignment on the GPU through
hscmp_assign_windows, windows and centroid updates on the host) against hsc_amd.kmeans.ConvolutionalKMeansLearner
(every iteration on the GPU) in the same process, at the three level shapes of the multilevel learning script
(T = 20000, 10000 windows, 10 iterations, resetMethod='random_samples'), on synthesized level-style data: a sparse
signal at level 0, sparse coefficient streams of K_prev features above it.  Both learners run under the same seed and
must return the same dictionary.  Also times trainBatch (B = 8 learners at level 1; 64 restarts at level 0), and
reports the assignment kernel's rate from the shapes over its device time, against the f64 / f32 matrix peak.

  python tools/bench_kmeans.py [--out profiles/kmeans_bench.json] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hsc_amd.kmeans import ConvolutionalKMeansLearner  # noqa: E402
from hsc_amd.learning import ConvolutionalDictionaryLearner  # noqa: E402

PEAK_TFLOPS = {'float64': 78.6, 'float32': 157.3}      # MI355X matrix peaks (spec)
LEVELS = [(0, 16, 32, 1), (1, 32, 33, 16), (2, 64, 33, 48)]


def level_data(T, F, seed):
    """Level 0: a float32 signal of sparse planted bursts; level >= 1: a sparse float64 [T, F] coefficient stream."""
    rs = np.random.RandomState(seed)
    x = np.zeros((T, F))
    for c in rs.randint(0, T - 16, int(2e-3 * T * max(1, F // 4))):
        for _ in range(rs.randint(1, 5)):
            x[c + rs.randint(0, 16), rs.randint(F)] = rs.uniform(0.5, 2.0) * rs.choice([-1.0, 1.0])
    return x[:, 0].astype(np.float32) if F == 1 else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmeans_bench.json'))
    ap.add_argument('--quick', action='store_true', help='level 0 only, no batches (a rehearsal)')
    a = ap.parse_args()
    N, iters, T = 10000, 10, 20000
    kw = dict(nbRandomWindows=N, maxIterations=iters, tolerance=0.0, resetMethod='random_samples')
    rows = []
    # warm-up: library loads, contexts, first kernels
    ConvolutionalKMeansLearner(4, 8).train(level_data(2000, 1, 0), 100, maxIterations=2)
    ConvolutionalDictionaryLearner(4, 8, algorithm='kmean').train(level_data(2000, 1, 0), 100, maxIterations=2)
    for level, K, W, F in LEVELS[:1] if a.quick else LEVELS:
        x = level_data(T, F, 10 + level)
        np.random.seed(1)
        t0 = time.perf_counter()
        D_host = ConvolutionalDictionaryLearner(K, W, algorithm='kmean').train(x, **kw)
        t1 = time.perf_counter()
        np.random.seed(1)
        learner = ConvolutionalKMeansLearner(K, W)
        t2 = time.perf_counter()
        D_dev = learner.train(x, **kw)
        t3 = time.perf_counter()
        st = learner.lastStats
        assign = np.array([s['assign_ms'] for s in st])
        cent = np.array([s['centroid_ms'] for s in st])
        step = np.array([s['step_ms'] for s in st])
        flop = 2.0 * N * (W + 1) * K * W * F
        dt = str(np.result_type(x.dtype, D_dev.dtype)) if x.dtype == np.float32 else 'float64'
        rate = flop / (np.median(assign) * 1e-3) / 1e12
        row = dict(level=level, K=K, W=W, F=F, N=N, iterations=len(st), data_dtype=str(x.dtype), D_dtype=str(D_dev.dtype),
                   identical=bool(D_host.dtype == D_dev.dtype and np.array_equal(D_host, D_dev)),
                   host_s=t1 - t0, device_s=t3 - t2, host_ms_per_iter=1e3 * (t1 - t0) / iters,
                   device_ms_per_iter=1e3 * (t3 - t2) / len(st), speedup=(t1 - t0) / (t3 - t2),
                   step_ms_median=float(np.median(step)), assign_ms_median=float(np.median(assign)),
                   centroid_ms_median=float(np.median(cent)), assign_gflop=flop / 1e9, assign_tflops=rate,
                   assign_dtype=dt, assign_share_of_peak=rate / PEAK_TFLOPS[dt])
        rows.append(row)
        print(json.dumps(row), flush=True)
    batches = []
    if not a.quick:
        for name, level, B in (('level1_B8', 1, 8), ('level0_restarts64', 0, 64)):
            _, K, W, F = LEVELS[level]
            xs = np.stack([level_data(T, F, 10 + level)] * B) if name.endswith('restarts64') else \
                np.stack([level_data(T, F, 100 + b) for b in range(B)])
            learner = ConvolutionalKMeansLearner(K, W)
            t0 = time.perf_counter()
            learner.trainBatch(xs, rngs=[np.random.RandomState(b) for b in range(B)], **kw)
            t1 = time.perf_counter()
            st = learner.lastStats[0]
            row = dict(name=name, B=B, K=K, W=W, F=F, N=N, iterations=iters, batch_s=t1 - t0,
                       ms_per_learner_iter=1e3 * (t1 - t0) / (B * iters),
                       step_ms_median=float(np.median([s['step_ms'] for s in st])),
                       assign_ms_median=float(np.median([s['assign_ms'] for s in st])),
                       centroid_ms_median=float(np.median([s['centroid_ms'] for s in st])))
            batches.append(row)
            print(json.dumps(row), flush=True)
    out = dict(levels=rows, batches=batches, T=T, N=N, iterations=iters)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
