"""Benchmark of hsc_amd.ksvd.ConvolutionalKSVDLearner: one JSON line per shape -> profiles/ksvd_bench.json.

  script:  T = 10 000, K = 64, W = 32, nbNonzeroCoefs = 100, toleranceSnr = 20, 'locomp' (scripts/learn_csc_dataset.py)
  large:   T = 2^20,   K = 64, W = 32, nbNonzeroCoefs = 20 000, 'cmp'

Per shape: the learner's encode and update ms per iteration (median over the iterations run), the device sweep alone
(HIP events), and the host sweep of ConvolutionalDictionaryLearner._train_ksvd (the same loop body, on the same D and
coefficients as the first device update, with libhscmp.so's overlap-add) with the ratio host / device.
Run on the GPU box from the repository root:  python tools/bench_ksvd.py [--out profiles/ksvd_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hsc_amd import ksvd  # noqa: E402
from hsc_amd.learning import ConvolutionalDictionaryLearner, extractWindows  # noqa: E402
from hsc_amd.modeling import ConvolutionalSparseCoder, reconstructSignal  # noqa: E402

SHAPES = [
    ('script', 10000, 64, 32, 100, 20.0, 'locomp', 4),
    ('large', 1 << 20, 64, 32, 20000, 20.0, 'cmp', 2),
]


def signal(T, W, seed=0):
    """A planted float64 signal: 16 random unit atoms at T / 100 random positions, plus white noise."""
    rs = np.random.RandomState(seed)
    atoms = rs.randn(16, W)
    atoms /= np.linalg.norm(atoms, axis=1, keepdims=True)
    x = 0.01 * rs.randn(T)
    nb = max(1, T // 100)
    for t, k, a in zip(rs.randint(0, T - W, nb), rs.randint(0, 16, nb), rs.randn(nb)):
        x[t:t + W] += (2.0 + abs(a)) * np.sign(a) * atoms[k]
    return x


def host_sweep(D, coefficients):
    """The dictionary update of ConvolutionalDictionaryLearner._train_ksvd (learning.py), on copies."""
    D = np.copy(D)
    coefficients = coefficients.tolil()
    W = D.shape[1]
    for k in range(D.shape[0]):
        indices = coefficients[:, k].nonzero()[0]
        if len(indices) == 0:
            continue
        coefficients[indices, k * np.ones_like(indices)] = 0.0
        error = reconstructSignal(coefficients.tocsc(), D)
        padded = np.pad(error, [(W // 2, W // 2)] + [(0, 0)] * (error.ndim - 1), mode='constant')
        patches = extractWindows(padded, W // 2 + indices, width=W, centered=True)
        patches = patches.reshape((patches.shape[0], -1))
        U, s, Vh = scipy.linalg.svd(patches.T, full_matrices=False)
        D[k, :] = U[:, 0].reshape(D.shape[1:])
        coefficients[indices, k * np.ones_like(indices)] = Vh.T[:, 0] * s[0]
    return D


def bench(name, T, K, W, nnz, snr, method, iterations):
    x = signal(T, W)
    np.random.seed(7)
    learner = ksvd.ConvolutionalKSVDLearner(K, W)
    learner.train(x, method=method, maxIterations=iterations, nbNonzeroCoefs=nnz, toleranceSnr=snr)
    st = learner.lastStats
    # the first iteration's inputs again: the device update alone and the host sweep on them
    np.random.seed(7)
    D0 = ConvolutionalDictionaryLearner(K, W, algorithm='ksvd')._init_D(x, initMethod='noise')
    coefficients, _ = ConvolutionalSparseCoder(D0, learner._coder(method)).encode(x, nbNonzeroCoefs=nnz, toleranceSnr=snr)
    ksvd.update(D0, coefficients)                                           # warm
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        D_dev, _, atoms, timing = ksvd.update(D0, coefficients)
        reps.append((1e3 * (time.perf_counter() - t0), timing[1]))
    t0 = time.perf_counter()
    D_host = host_sweep(D0, coefficients)
    host_ms = 1e3 * (time.perf_counter() - t0)
    a, b = D_dev.reshape(K, -1), D_host.reshape(K, -1)
    diff = float(np.max(np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1))))
    update_ms = float(np.median([r[0] for r in reps]))
    sweep_ms = float(np.median([r[1] for r in reps]))
    return dict(shape=name, T=T, K=K, W=W, nbNonzeroCoefs=nnz, toleranceSnr=snr, method=method,
                iterations=len(st), nnz=int(coefficients.nnz), max_occurrences=int(np.max(atoms[:, 0])),
                encode_ms_per_iteration=float(np.median([s['encode_ms'] for s in st])),
                update_ms_per_iteration=float(np.median([s['update_ms'] for s in st])),
                update_ms=update_ms, sweep_kernel_ms=sweep_ms, host_sweep_ms=host_ms,
                host_over_device=host_ms / update_ms, kernel_launches_per_sweep=1, copies_per_sweep=9,
                max_jacobi_sweeps=int(np.max(atoms[:, 3])), host_vs_device_D_diff_up_to_sign=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ksvd_bench.json'))
    ap.add_argument('--shapes', default='script,large')
    args = ap.parse_args()
    want = args.shapes.split(',')
    lines = []
    for s in SHAPES:
        if s[0] in want:
            r = bench(*s)
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
