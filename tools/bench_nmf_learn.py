"""Benchmark of ConvolutionalNMFLearner (hsc_amd.nmf) on one MI355X; prints one JSON line.

Cases (float32 unless stated):
  script:  K=16, W=32, T=10000, 100 iterations, one learner (the reference's scripts/learn_csc_dataset.py shape)
  long:    K=64, W=32, T=2^20, 10 iterations, one learner, float32 and float64
  batch64: 64 learners at the script shape, 100 iterations
Per case: ms per iteration from HIP events, and the dictionary update's share of it: one minus the ratio of the
coder's ms per iteration (ConvolutionalNMF on the same signals, initial coefficients and the first learner's initial
dictionary: the same W steps, residual and decision) to the learner's.  `update_flop_per_iteration` is the useful
matrix work of the update (2 L K W F per learner: the partial products N); the kernel times that give its rate come
from `rocprofv3 --kernel-trace --stats` in a run of its own.
--ref-cpu times the reference's learner on the CPU instead (script shape, a few iterations); it needs the reference
next to the repository and is skipped otherwise.

  python tools/bench_nmf_learn.py [--cases script,long,batch64] [--ref-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = {'float32': 157.3e12, 'float64': 78.6e12}
CASES = {
    'script': [dict(K=16, W=32, T=10000, B=1, iterations=100, dtype='float32')],
    'long': [dict(K=64, W=32, T=1 << 20, B=1, iterations=10, dtype='float32'),
             dict(K=64, W=32, T=1 << 20, B=1, iterations=10, dtype='float64')],
    'batch64': [dict(K=16, W=32, T=10000, B=64, iterations=100, dtype='float32')],
}


def bench_gpu(name, cfg):
    from hsc_amd.nmf import ConvolutionalNMF, ConvolutionalNMFLearner
    K, W, T, B, its, dt = cfg['K'], cfg['W'], cfg['T'], cfg['B'], cfg['iterations'], cfg['dtype']
    X = np.random.RandomState(0).random_sample((B, T)).astype(dt)
    learner = ConvolutionalNMFLearner(K, W, rng=np.random.RandomState(1))
    learner.trainBatch(X[:1, :max(4 * W, 256)], nbMaxIterations=1)                             # warm-up (code objects)
    t0 = time.perf_counter()
    from hsc_amd.learning import ConvolutionalDictionaryLearner
    init = ConvolutionalDictionaryLearner(K, W, algorithm='nmf', rng=np.random.RandomState(2))
    D0 = np.stack([init._init_D(X[b], 'random_samples') for b in range(B)])
    A0 = (np.random.RandomState(3).random_sample((B, T, K)).astype(dt) + 2.0)
    draw_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    D, st = learner.trainBatch(X, nbMaxIterations=its, initialDictionaries=D0, initialCoefficients=A0)
    wall = time.perf_counter() - t0
    up, it_ms, down, chunks, ran = [float(v) for v in st.timing_ms]
    cnmf = ConvolutionalNMF()
    cnmf.computeCoefficientsBatch(X, D0[0], nbMaxIterations=its, initialCoefficients=A0)
    code_ms = float(cnmf.lastStats.timing_ms[1])
    L = T - W + 1
    upd_flop = 2.0 * L * K * W * B
    return {'case': name, 'config': {'K': K, 'W': W, 'T': T, 'B': B}, 'dtype': dt, 'iterations': its, 'chunks': int(chunks),
            'ms_per_iteration': round(it_ms / its, 4), 'coder_ms_per_iteration': round(code_ms / its, 4),
            'update_share': round(1.0 - code_ms / it_ms, 3), 'launches_per_iteration': W + 5,
            'us_per_launch': round(1e3 * it_ms / its / (W + 5), 2),
            'update_flop_per_iteration': upd_flop,
            'update_tflops_lower_bound': round(upd_flop * its / max(1e-9, (it_ms - code_ms) * 1e-3) / 1e12, 3),
            'upload_ms': round(up, 2), 'download_ms': round(down, 2), 'host_draw_s': round(draw_s, 2), 'wall_s': round(wall, 2),
            'snr_mean_db': round(float(np.mean(st.snr)), 4), 'd_checksum': float(np.sum(np.abs(D.astype(np.float64))))}


def bench_ref_cpu(iterations=3):
    from oracle import ref_loader
    ns = ref_loader.load_reference()
    if ns is None:
        return None
    x = np.random.RandomState(0).random_sample(10000).astype(np.float32)
    cdl = ns.modeling.ConvolutionalDictionaryLearner(k=16, windowSize=32, algorithm='nmf')
    np.random.seed(0)
    t0 = time.perf_counter()
    cdl.train(x, initMethod='noise', nbMaxIterations=iterations)
    s = time.perf_counter() - t0
    return {'case': 'script', 'config': {'K': 16, 'W': 32, 'T': 10000}, 'initMethod': 'noise', 'iterations': iterations,
            'seconds': round(s, 2), 'ms_per_iteration': round(1e3 * s / iterations, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='script,long,batch64')
    ap.add_argument('--ref-cpu', action='store_true')
    a = ap.parse_args()
    out = {'bench': 'convolutional_nmf_learner', 'gpu': [], 'ref_cpu': []}
    if a.ref_cpu:
        r = bench_ref_cpu()
        if r is not None:
            out['ref_cpu'].append(r)
    else:
        for name in a.cases.split(','):
            for cfg in CASES[name]:
                out['gpu'].append(bench_gpu(name, cfg))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
