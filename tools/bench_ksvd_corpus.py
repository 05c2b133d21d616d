"""Benchmark of the corpus form of the K-SVD learner (hsc_amd.ksvd.update_corpus / trainCorpus): one JSON line per
shape -> profiles/ksvd_corpus_bench.json.

  script, large:  the two shapes of tools/bench_ksvd.py, as corpora of one signal
  corpus:         1024 signals x 16 384 samples, K = 64, W = 32, nbNonzeroCoefs = 64, 'cmp'
  corpus_ragged:  the same with lengths uniform in [4096, 16 384]

Per shape, on the first iteration's inputs (D drawn as trainCorpus draws it, one encodeBatch of the whole corpus):
  * the device sweep (HIP events) under plan 1 (one workgroup) and plan 2 (wide), the plans alternated, median / min /
    max of 5 each, whether the two returned the same bits, and the plan 'auto' takes;
  * the encode of one iteration (one encodeBatch call, the second of two);
  * the per-signal way: `encode` signal by signal on 32 sampled signals, scaled to B.
Run on the GPU box from the repository root:  python tools/bench_ksvd_corpus.py [--out profiles/ksvd_corpus_bench.json]
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
from hsc_amd.learning import ConvolutionalDictionaryLearner  # noqa: E402
from hsc_amd.modeling import ConvolutionalSparseCoder  # noqa: E402

REPS = 5
SAMPLED = 32


def lengths_of(name):
    if name == 'script':
        return [10000]
    if name == 'large':
        return [1 << 20]
    if name == 'corpus':
        return [16384] * 1024
    if name == 'corpus_ragged':
        return [int(t) for t in np.random.RandomState(1).randint(4096, 16384 + 1, 1024)]
    raise ValueError(name)


# (name, K, W, nbNonzeroCoefs per signal, toleranceSnr, method)
SHAPES = [
    ('script', 64, 32, 100, 20.0, 'locomp'),
    ('large', 64, 32, 20000, 20.0, 'cmp'),
    ('corpus', 64, 32, 64, 40.0, 'cmp'),
    ('corpus_ragged', 64, 32, 64, 40.0, 'cmp'),
]


def same_bits(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
                and all(np.array_equal(x.data, y.data) for x, y in zip(a[1], b[1])))


def bench(name, K, W, nnz, snr, method):
    lengths = lengths_of(name)
    B = len(lengths)
    xs = [signal(T, W, seed=b) for b, T in enumerate(lengths)]
    ragged = len(set(lengths)) > 1
    sequences = xs if ragged else np.stack(xs)
    learner = ksvd.ConvolutionalKSVDLearner(K, W)
    np.random.seed(7)
    D0 = ConvolutionalDictionaryLearner(K, W, algorithm='ksvd')._init_D(np.concatenate(xs), initMethod='noise')
    D0 = np.asarray(D0, dtype=np.float64)
    encode_ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        res = ConvolutionalSparseCoder(D0, learner._coder(method)).encodeBatch(sequences, nbNonzeroCoefs=nnz, toleranceSnr=snr)
        encode_ms.append(1e3 * (time.perf_counter() - t0))
    coefficients = res.coefficients
    picks = np.random.RandomState(2).choice(B, min(SAMPLED, B), replace=False)
    ConvolutionalSparseCoder(D0, learner._coder(method)).encode(xs[picks[0]], nbNonzeroCoefs=nnz, toleranceSnr=snr)     # warm
    t0 = time.perf_counter()
    for b in picks:
        ConvolutionalSparseCoder(D0, learner._coder(method)).encode(xs[b], nbNonzeroCoefs=nnz, toleranceSnr=snr)
    per_signal_ms = 1e3 * (time.perf_counter() - t0) * B / len(picks)
    plans = ('one', 'wide')
    out = {p: ksvd.update_corpus(D0, coefficients, plan=p) for p in plans}                                              # warm
    sweeps = {p: [] for p in plans}
    walls = {p: [] for p in plans}
    for _ in range(REPS):
        for p in plans:
            t0 = time.perf_counter()
            timing = ksvd.update_corpus(D0, coefficients, plan=p)[3]
            walls[p].append(1e3 * (time.perf_counter() - t0))
            sweeps[p].append(float(timing[1]))
    atoms = out['one'][2]
    max_m = int(np.max(atoms[:, 0]))
    r = dict(shape=name, B=B, T_min=min(lengths), T_max=max(lengths), samples=int(sum(lengths)), K=K, W=W,
             nbNonzeroCoefs=nnz, toleranceSnr=snr, method=method, variant=res.variant,
             nnz=int(sum(c.nnz for c in coefficients)), max_occurrences=max_m, atoms_updated=int(np.sum(atoms[:, 0] > 0)),
             max_jacobi_sweeps=int(np.max(atoms[:, 3])), plans_bit_identical=same_bits(out['one'], out['wide']),
             auto_plan=2 if max_m >= ksvd.WIDE_FROM_OCCURRENCES else 1,
             encode_ms_per_iteration=encode_ms[1], per_signal_encode_ms_scaled=per_signal_ms, sampled_signals=int(len(picks)))
    for i, p in enumerate(plans):
        r['sweep_ms_plan%d' % (i + 1)] = float(np.median(sweeps[p]))
        r['sweep_ms_plan%d_min_max' % (i + 1)] = [float(np.min(sweeps[p])), float(np.max(sweeps[p]))]
        r['update_ms_plan%d' % (i + 1)] = float(np.median(walls[p]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ksvd_corpus_bench.json'))
    ap.add_argument('--shapes', default=','.join(s[0] for s in SHAPES))
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
