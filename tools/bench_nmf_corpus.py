"""Benchmark of ConvolutionalNMFLearner.trainCorpus (hscnmf_learn_corpus) on one MI355X; writes
profiles/nmf_corpus_bench.json and prints the same JSON.

  uniform: the corpus shape of the K-SVD and k-means corpus benches, 1024 signals x 16 384 samples, K = 16, W = 32, float32.
           ms per iteration of trainCorpus (ONE dictionary) and of trainBatch (1024 dictionaries) on the same signals and
           initial coefficients, the two alternating in one process, from the HIP events around each call's iterations
           (timing_ms[1] of include/hscnmf.h over the iterations run).
  ragged:  256 signals of 16 384 .. 65 536 samples (lengths from a seed), same K, W and dtype: trainCorpus only, there is
           no batch call for signals of different lengths.
Both calls run the same W step launches over the same tiles; the corpus replaces the per-learner update (K x B workgroups
summing 128 tiles each) by the per-signal sums and one update of K workgroups summing over the B signals.
Kernel times come from `rocprofv3 --kernel-trace --stats -- python tools/bench_nmf_corpus.py --small` in a run of its own.

  python tools/bench_nmf_corpus.py [--repetitions 5] [--iterations 3] [--small] [--out profiles/nmf_corpus_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _summary(values):
    v = sorted(values)
    return {'median': round(v[len(v) // 2], 4), 'min': round(v[0], 4), 'max': round(v[-1], 4)}


def _inputs(lengths, K, W, dtype, seed):
    rs = np.random.RandomState(seed)
    sigs = [rs.random_sample((T,)).astype(dtype) for T in lengths]
    D0 = rs.random_sample((K, W)).astype(dtype)
    D0 /= np.sqrt(np.sum(np.square(D0), axis=1, keepdims=True))
    A0s = [rs.random_sample((T, K)).astype(dtype) + 2.0 for T in lengths]
    return sigs, D0.astype(dtype), A0s


def bench(lengths, K, W, dtype, iterations, repetitions, with_batch):
    from hsc_amd.nmf import ConvolutionalNMFLearner
    sigs, D0, A0s = _inputs(lengths, K, W, dtype, 0)
    B, samples = len(lengths), int(np.sum(lengths))
    learner = ConvolutionalNMFLearner(K, W)
    kw = dict(nbMaxIterations=iterations)
    # warm-up: every kernel of both calls, at a small size
    learner.trainCorpus([q[:4 * W] for q in sigs[:2]], initialDictionary=D0, initialCoefficients=[a[:4 * W] for a in A0s[:2]], **kw)
    if with_batch:
        X, A0, D0s = np.stack(sigs), np.stack(A0s), np.broadcast_to(D0, (B, K, W)).copy()
        learner.trainBatch(X[:2, :4 * W], initialDictionaries=D0s[:2], initialCoefficients=A0[:2, :4 * W], **kw)
    corpus, batch, wall = [], [], []
    checksum = None
    for _ in range(repetitions):
        t0 = time.perf_counter()
        D = learner.trainCorpus(sigs, initialDictionary=D0, initialCoefficients=A0s, **kw)
        wall.append(time.perf_counter() - t0)
        st = learner.lastStats
        assert int(st.iterations[0]) == iterations and np.all(np.isfinite(D))
        corpus.append(float(st.timing_ms[1]) / iterations)
        c = float(np.sum(np.abs(D.astype(np.float64))))
        assert checksum in (None, c), 'two identical calls differ'
        checksum = c
        if with_batch:
            _, sb = learner.trainBatch(X, initialDictionaries=D0s, initialCoefficients=A0, **kw)
            assert int(sb.timing_ms[3]) == 1, 'the batch ran in more than one chunk'
            batch.append(float(sb.timing_ms[1]) / iterations)
    out = {'signals': B, 'samples': samples, 'lengths': [int(min(lengths)), int(max(lengths))], 'K': K, 'W': W, 'F': 1,
           'dtype': np.dtype(dtype).name, 'iterations': iterations, 'repetitions': repetitions,
           'launches_per_iteration': W + 7, 'corpus_ms_per_iteration': _summary(corpus),
           'corpus_ns_per_sample_iteration': round(1e6 * _summary(corpus)['median'] / samples, 4),
           'corpus_wall_s_per_call': _summary(wall), 'corpus_snr_db': round(float(st.snr[0]), 4), 'd_checksum': checksum}
    if with_batch:
        out['batch_ms_per_iteration'] = _summary(batch)
        out['corpus_over_batch'] = round(_summary(corpus)['median'] / _summary(batch)['median'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repetitions', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='64 signals (uniform) and 16 (ragged): for a profiler run')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nmf_corpus_bench.json'))
    a = ap.parse_args()
    K, W = 16, 32
    nu, nr = (64, 16) if a.small else (1024, 256)
    ragged = np.random.RandomState(1).randint(16384, 65536 + 1, size=nr).tolist()
    out = {'bench': 'convolutional_nmf_corpus', 'small': bool(a.small),
           'uniform': bench([16384] * nu, K, W, np.float32, a.iterations, a.repetitions, True),
           'ragged': bench(ragged, K, W, np.float32, a.iterations, a.repetitions, False)}
    text = json.dumps(out, indent=1)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
