"""Benchmark of ConvolutionalKSVDLearner.trainBatch (B independent K-SVD learners in one batch) against
the loop of `train` over the same signals and generators: one JSON line per batch size -> profiles/ksvd_batch_bench.json.

Shape: the reference script's (K = 16, W = 32, T = 10 000, nbNonzeroCoefs = 100, toleranceSnr = 20, the default method
'locomp', 5 iterations), B = 1, 8, 64, 256 learners, learner b on signal b with generator RandomState(1000 + b).
Per batch size, --reps times, the two ways alternated (after one warm-up of each at B = 1):
  * wall clock of trainBatch and of the loop of train (median / min / max);
  * per iteration, the encode and the dictionary update of both (host wall clock; for the loop the sum over the learners),
    and the device sweep alone (HIP events: one launch of B workgroups against B launches of one);
  * whether the B dictionaries of the two ways are bit-identical.
Run on the GPU box from the repository root:  python tools/bench_ksvd_batch.py [--out profiles/ksvd_batch_bench.json]
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

from bench_ksvd import signal  # noqa: E402
from hsc_amd import ksvd  # noqa: E402

K, W, T, NNZ, SNR, ITERATIONS = 16, 32, 10000, 100, 20.0, 5
BATCHES = (1, 8, 64, 256)


def run_batch(x):
    learner = ksvd.ConvolutionalKSVDLearner(K, W)
    t0 = time.perf_counter()
    D, stats = learner.trainBatch(x, maxIterations=ITERATIONS, nbNonzeroCoefs=NNZ, toleranceSnr=SNR,
                                  rngs=[np.random.RandomState(1000 + b) for b in range(x.shape[0])])
    wall = 1e3 * (time.perf_counter() - t0)
    # (the batch's encode_ms / update_ms / sweep_ms are shared by the learners of an iteration: take them from one that ran it)
    per_iter = []
    for n in range(ITERATIONS):
        ran = [s[n] for s in stats if len(s) > n]
        per_iter.append(dict(learners=len(ran), encode_ms=ran[0]['encode_ms'] if ran else 0.0, update_ms=ran[0]['update_ms'] if ran else 0.0,
                             sweep_ms=ran[0]['sweep_ms'] if ran else 0.0))
    return D, wall, per_iter, stats[0][0]['variant'] if stats[0] else None


def run_loop(x):
    Ds, per_iter = [], [dict(learners=0, encode_ms=0.0, update_ms=0.0, sweep_ms=0.0) for _ in range(ITERATIONS)]
    t0 = time.perf_counter()
    for b in range(x.shape[0]):
        learner = ksvd.ConvolutionalKSVDLearner(K, W, rng=np.random.RandomState(1000 + b))
        Ds.append(learner.train(x[b], maxIterations=ITERATIONS, nbNonzeroCoefs=NNZ, toleranceSnr=SNR))
        for n, s in enumerate(learner.lastStats):
            per_iter[n]['learners'] += 1
            for key in ('encode_ms', 'update_ms', 'sweep_ms'):
                per_iter[n][key] += s[key]
    wall = 1e3 * (time.perf_counter() - t0)
    return np.stack(Ds), wall, per_iter


def med(rows, key):
    """median over the repetitions of the per-iteration mean of `key`"""
    return float(np.median([np.mean([it[key] for it in rep]) for rep in rows]))


def bench(B, reps):
    x = np.stack([signal(T, W, seed=b) for b in range(B)])
    walls = {'batch': [], 'loop': []}
    iters = {'batch': [], 'loop': []}
    same, variant = True, None
    for _ in range(reps):
        Db, wall_b, it_b, variant = run_batch(x)
        Dl, wall_l, it_l = run_loop(x)
        walls['batch'].append(wall_b); walls['loop'].append(wall_l)
        iters['batch'].append(it_b); iters['loop'].append(it_l)
        same = same and bool(np.array_equal(Db, Dl))
    r = dict(B=B, K=K, W=W, T=T, nbNonzeroCoefs=NNZ, toleranceSnr=SNR, method='locomp', iterations=ITERATIONS, reps=reps,
             variant=variant, dictionaries_bit_identical=same)
    for way in ('batch', 'loop'):
        r['%s_wall_ms' % way] = float(np.median(walls[way]))
        r['%s_wall_ms_min_max' % way] = [float(np.min(walls[way])), float(np.max(walls[way]))]
        for key in ('encode_ms', 'update_ms', 'sweep_ms'):
            r['%s_%s_per_iteration' % (way, key)] = med(iters[way], key)
    r['speedup'] = r['loop_wall_ms'] / r['batch_wall_ms']
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ksvd_batch_bench.json'))
    ap.add_argument('--batches', default=','.join(str(b) for b in BATCHES))
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    warm = np.stack([signal(T, W, seed=0)])
    run_batch(warm)
    run_loop(warm)
    lines = []
    for B in [int(b) for b in args.batches.split(',')]:
        r = bench(B, args.reps)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
