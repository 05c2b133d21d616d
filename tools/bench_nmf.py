"""Benchmark of ConvolutionalNMF (hsc_amd.nmf) on one MI355X; prints one JSON line.

Shapes: the config-1 dictionary (K=32, W=32, T=4096, B=1024) and the config-2 dictionary (K=256, W=64, T=65536,
B=32), float32 and float64, a fixed number of iterations.  Per shape: ms per iteration from HIP events (the
upload of the initial coefficients and the host draw timed separately), the matrix FLOP rate of the P = A.D
products against the fp32 (157.3 TF) / fp64 (78.6 TF) matrix peak, and the A traffic per step against 6.3 TB/s.
--ref-cpu also times the reference on the CPU for one signal (all iterations at config 1, one at config 2); it
needs the reference next to the repository and is skipped otherwise.

  python tools/bench_nmf.py [--iterations 10] [--configs 1,2] [--dtypes float32,float64] [--ref-cpu]
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
HBM = 6.3e12
CONFIGS = {1: dict(K=32, W=32, T=4096, B=1024), 2: dict(K=256, W=64, T=65536, B=32)}
ROWS = 128          # A rows per workgroup (csrc/nmf/hscnmf.hip kRows)


def bench_gpu(cfg, dtype, iterations):
    from hsc_amd.nmf import ConvolutionalNMF
    K, W, T, B = cfg['K'], cfg['W'], cfg['T'], cfg['B']
    rs = np.random.RandomState(0)
    D = rs.random_sample((K, W))
    D = (D / np.sqrt(np.sum(np.square(D), axis=1, keepdims=True))).astype(dtype)
    X = rs.random_sample((B, T)).astype(dtype)
    t0 = time.perf_counter()
    np.random.seed(0)
    A0 = np.empty((B, T, K), dtype=dtype)
    for b in range(B):                                   # the reference's draw, signal after signal
        A0[b] = np.random.random((T, K)).astype(dtype) + 2.0
    draw_s = time.perf_counter() - t0
    cnmf = ConvolutionalNMF()
    cnmf.computeCoefficientsBatch(X[:1], D, nbMaxIterations=1, initialCoefficients=A0[:1])    # warm-up (code objects)
    t0 = time.perf_counter()
    coef, resid, st = cnmf.computeCoefficientsBatch(X, D, nbMaxIterations=iterations, initialCoefficients=A0)
    wall = time.perf_counter() - t0
    up, it_ms, down, chunks, its = [float(v) for v in st.timing_ms]
    L = T - W + 1
    PR = -(-(ROWS + W - 1) // (32 if dtype == 'float32' else 16)) * (32 if dtype == 'float32' else 16)
    useful = 2.0 * L * K * W * B * W * iterations                    # P = A.D, L rows, W steps per iteration
    executed = useful * PR / ROWS                                    # with the recomputed halo rows
    steps = W * iterations
    ms_iter = it_ms / iterations
    a_bytes = 2.0 * L * K * np.dtype(dtype).itemsize * B             # read A, write A' per step (halo re-reads hit L2)
    e_ref = float(np.mean(np.sum(np.square(resid.astype(np.float64).reshape(B, -1)), axis=1)))
    return {'config': cfg, 'dtype': dtype, 'iterations': iterations, 'chunks': int(chunks),
            'ms_per_iteration': round(ms_iter, 3), 'ms_per_step': round(it_ms / steps, 4),
            'upload_ms': round(up, 1), 'download_ms': round(down, 1), 'host_draw_s': round(draw_s, 2), 'wall_s': round(wall, 2),
            'tflops_useful': round(useful / (it_ms * 1e-3) / 1e12, 2), 'tflops_executed': round(executed / (it_ms * 1e-3) / 1e12, 2),
            'frac_matrix_peak': round(executed / (it_ms * 1e-3) / PEAK[dtype], 3),
            'a_bytes_per_step': int(a_bytes), 'frac_hbm_a_traffic': round(a_bytes / (it_ms * 1e-3 / steps) / HBM, 3),
            'snr_mean_db': round(float(np.mean(st.snr)), 4), 'residual_energy_mean': e_ref}


def bench_ref_cpu(cfg, dtype, iterations):
    from oracle import ref_loader
    ns = ref_loader.load_reference()
    if ns is None:
        return None
    K, W, T = cfg['K'], cfg['W'], cfg['T']
    rs = np.random.RandomState(0)
    D = rs.random_sample((K, W))
    D = (D / np.sqrt(np.sum(np.square(D), axis=1, keepdims=True))).astype(dtype)
    x = rs.random_sample(T).astype(dtype)
    np.random.seed(0)
    t0 = time.perf_counter()
    ns.modeling.ConvolutionalNMF().computeCoefficients(x, D, nbMaxIterations=iterations)
    return {'config': cfg, 'dtype': dtype, 'iterations': iterations, 'seconds_one_signal': round(time.perf_counter() - t0, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=10)
    ap.add_argument('--configs', default='1,2')
    ap.add_argument('--dtypes', default='float32,float64')
    ap.add_argument('--ref-cpu', action='store_true')
    a = ap.parse_args()
    out = {'bench': 'convolutional_nmf', 'gpu': [], 'ref_cpu': []}
    for c in [int(v) for v in a.configs.split(',')]:
        for dt in a.dtypes.split(','):
            if a.ref_cpu:
                r = bench_ref_cpu(CONFIGS[c], dt, a.iterations if c == 1 else 1)
                if r is not None:
                    out['ref_cpu'].append(r)
            else:
                out['gpu'].append(bench_gpu(CONFIGS[c], dt, a.iterations))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
