"""Benchmark of ConvolutionalNMF.computeCoefficientsRaggedBatch (hscnmf_compute_ragged) on one
MI355X; writes profiles/nmf_ragged_bench.json and prints the same JSON.

Workload: K = 16, W = 32, float32, 8 iterations, signals of 16 384 .. 65 536 samples (lengths from a seed); a corpus of 1024
signals and one of 64.  Three ways of coding a corpus alternate in one process, `--repetitions` times each:
  ragged:     one computeCoefficientsRaggedBatch call;
  per_signal: computeCoefficientsBatch on one signal at a time (what computeCoefficients does; the only exact way without
              the ragged call), timed on a sample of 32 signals and scaled to the corpus by the signal count; the sampled
              signals' coefficients and residuals are compared with the ragged call's, bit for bit;
  padded:     computeCoefficientsBatch on the signals zero-padded to 65 536 samples: NOT the same results, only what
              padding costs.
Times are timing_ms of include/hscnmf.h (HIP events around the upload, the iterations and the download, summed over
chunks and, for per_signal, over the calls); wall time is reported beside them.
A fourth row, on the large corpus: a toleranceSnr at the lower quartile of the signals' SNR after the first iteration, so
that about three quarters of them stop there; the same tolerance on the corpus cut down to the signals that go on.  The
difference is what the workgroups of stopped signals, which return at their flag, cost.

  python tools/bench_nmf_ragged.py [--repetitions 5] [--iterations 8] [--small] [--out profiles/nmf_ragged_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, W, TMIN, TMAX, SAMPLE = 16, 32, 16384, 65536, 32


def _summary(values):
    v = sorted(values)
    return {'median': round(v[len(v) // 2], 4), 'min': round(v[0], 4), 'max': round(v[-1], 4)}


def _times(stats_list):
    """upload / iterations / download ms of a list of runs, each a list of timing_ms (summed within a run)."""
    runs = [np.sum(np.array(r), axis=0) for r in stats_list]
    return {'upload_ms': _summary([float(r[0]) for r in runs]), 'iterations_ms': _summary([float(r[1]) for r in runs]),
            'download_ms': _summary([float(r[2]) for r in runs])}


def _inputs(lengths, seed):
    rs = np.random.RandomState(seed)
    sigs = [rs.random_sample((T,)).astype(np.float32) for T in lengths]
    D = rs.random_sample((K, W)).astype(np.float32)
    D /= np.sqrt(np.sum(np.square(D), axis=1, keepdims=True))
    A0s = [rs.random_sample((T, K)).astype(np.float32) + np.float32(2.0) for T in lengths]
    return sigs, D, A0s


def bench(lengths, iterations, repetitions, seed):
    from hsc_amd.nmf import ConvolutionalNMF
    sigs, D, A0s = _inputs(lengths, seed)
    B, samples = len(lengths), int(np.sum(lengths))
    cnmf = ConvolutionalNMF()
    kw = dict(nbMaxIterations=iterations)
    sample = sorted(np.random.RandomState(seed + 1).choice(B, size=min(SAMPLE, B), replace=False).tolist())
    X = np.zeros((B, TMAX), dtype=np.float32)
    A = np.full((B, TMAX, K), 2.0, dtype=np.float32)
    for b, (q, a) in enumerate(zip(sigs, A0s)):
        X[b, :q.shape[0]] = q
        A[b, :q.shape[0]] = a
    # warm-up: every kernel of the three ways, at a small size
    cnmf.computeCoefficientsRaggedBatch([q[:4 * W] for q in sigs[:2]], D, initialCoefficients=[a[:4 * W] for a in A0s[:2]], **kw)
    cnmf.computeCoefficientsBatch(X[:2, :4 * W], D, initialCoefficients=A[:2, :4 * W], **kw)
    ragged, loop, padded = [], [], []
    wall = {'ragged': [], 'per_signal_sample': [], 'padded': []}
    identical = 0
    for rep in range(repetitions):
        t0 = time.perf_counter()
        coef, resid, st = cnmf.computeCoefficientsRaggedBatch(sigs, D, initialCoefficients=A0s, **kw)
        wall['ragged'].append(time.perf_counter() - t0)
        assert np.all(st.iterations == iterations)
        ragged.append([st.timing_ms.copy()])
        chunks = int(st.timing_ms[3])
        t0 = time.perf_counter()
        one = []
        for b in sample:
            c1, r1, s1 = cnmf.computeCoefficientsBatch(sigs[b][np.newaxis], D, initialCoefficients=A0s[b][np.newaxis], **kw)
            one.append(s1.timing_ms.copy())
            if rep == 0:
                identical += int(np.array_equal(c1[0], coef[b]) and np.array_equal(r1[0], resid[b]) and
                                 s1.snr[0] == st.snr[b] and s1.residual_scale[0] == st.residual_scale[b])
        wall['per_signal_sample'].append(time.perf_counter() - t0)
        loop.append(one)
        del coef, resid
        t0 = time.perf_counter()
        _, _, sp = cnmf.computeCoefficientsBatch(X, D, initialCoefficients=A, **kw)
        wall['padded'].append(time.perf_counter() - t0)
        padded.append([sp.timing_ms.copy()])
        print('%d signals: repetition %d of %d' % (B, rep + 1, repetitions), file=sys.stderr, flush=True)
    scale = float(B) / len(sample)
    out = {'signals': B, 'samples': samples, 'lengths': [int(min(lengths)), int(max(lengths))], 'K': K, 'W': W, 'F': 1,
           'dtype': 'float32', 'iterations': iterations, 'repetitions': repetitions, 'ragged_chunks': chunks,
           'ragged': _times(ragged), 'per_signal_sample': _times(loop), 'padded': _times(padded),
           'padded_chunks': int(sp.timing_ms[3]), 'padded_samples': B * TMAX,
           'sampled_signals': len(sample), 'sampled_samples': int(sum(lengths[b] for b in sample)),
           'sampled_signals_bit_identical': identical,
           'wall_s': {k: _summary(v) for k, v in wall.items()}}
    out['per_signal_scaled'] = {k: {s: round(v * scale, 4) for s, v in d.items()} for k, d in out['per_signal_sample'].items()}
    r, l = out['ragged']['iterations_ms'], out['per_signal_scaled']['iterations_ms']
    out['ragged_ms_per_iteration'] = round(r['median'] / iterations, 4)
    out['per_signal_ms_per_iteration'] = round(l['median'] / iterations, 4)
    out['per_signal_over_ragged'] = round(l['median'] / r['median'], 3)
    out['ragged_faster_by_more_than_either_spread'] = bool(l['median'] - r['median'] > max(r['max'] - r['min'], l['max'] - l['min']))
    return out, (sigs, D, A0s)


def bench_stopped(inputs, iterations, repetitions, ms_all):
    """The large corpus under a tolerance that stops about three quarters of the signals after the first iteration,
    against the corpus cut down to the signals still running."""
    from hsc_amd.nmf import ConvolutionalNMF
    sigs, D, A0s = inputs
    cnmf = ConvolutionalNMF()
    _, _, s1 = cnmf.computeCoefficientsRaggedBatch(sigs, D, initialCoefficients=A0s, nbMaxIterations=1)
    tol = float(np.percentile(s1.snr, 25.0))
    kw = dict(nbMaxIterations=iterations, toleranceSnr=tol)
    full, cut = [], []
    for rep in range(repetitions):
        coef, resid, st = cnmf.computeCoefficientsRaggedBatch(sigs, D, initialCoefficients=A0s, **kw)
        full.append([st.timing_ms.copy()])
        keep = [b for b in range(len(sigs)) if st.iterations[b] > 1]
        c2, r2, s2 = cnmf.computeCoefficientsRaggedBatch([sigs[b] for b in keep], D, initialCoefficients=[A0s[b] for b in keep], **kw)
        cut.append([s2.timing_ms.copy()])
        if rep == 0:
            same = all(np.array_equal(c2[j], coef[b]) and np.array_equal(r2[j], resid[b]) for j, b in enumerate(keep))
            its_full, its_cut = int(st.timing_ms[4]), int(s2.timing_ms[4])
            hist = {int(n): int(np.sum(st.iterations == n)) for n in np.unique(st.iterations)}
        del coef, resid, c2, r2
        print('stopped signals: repetition %d of %d' % (rep + 1, repetitions), file=sys.stderr, flush=True)
    out = {'tolerance_snr_db': round(tol, 6), 'signals': len(sigs), 'signals_stopped_after_first_iteration': len(sigs) - len(keep),
           'signals_still_running': len(keep), 'samples_still_running': int(sum(sigs[b].shape[0] for b in keep)),
           'signals_per_iteration_count': hist, 'iterations_run': its_full, 'iterations_run_cut_down': its_cut,
           'cut_down_bit_identical': bool(same), 'whole_corpus': _times(full), 'cut_down_corpus': _times(cut)}
    derive_stopped(out, ms_all)
    return out


def derive_stopped(out, ms_all):
    """The whole corpus runs its first iteration on every signal (ms_all: an iteration of the run without a tolerance) and
    the later ones on the running signals plus the returning workgroups of the stopped ones; the cut-down corpus runs
    every iteration on the running signals alone."""
    f, c = out['whole_corpus']['iterations_ms']['median'], out['cut_down_corpus']['iterations_ms']['median']
    n = out['iterations_run']
    out['first_iteration_ms_all_signals'] = round(ms_all, 4)
    out['cut_down_ms_per_iteration'] = round(c / out['iterations_run_cut_down'], 4)
    if n > 1:
        out['later_iteration_ms'] = round((f - ms_all) / (n - 1), 4)
        out['returning_workgroups_ms_per_iteration'] = round(out['later_iteration_ms'] - out['cut_down_ms_per_iteration'], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repetitions', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=8)
    ap.add_argument('--small', action='store_true', help='64 and 8 signals: for a profiler run or a trial')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nmf_ragged_bench.json'))
    a = ap.parse_args()
    nl, ns = (64, 8) if a.small else (1024, 64)
    large = np.random.RandomState(1).randint(TMIN, TMAX + 1, size=nl).tolist()
    small = np.random.RandomState(2).randint(TMIN, TMAX + 1, size=ns).tolist()
    out = {'bench': 'convolutional_nmf_ragged', 'small': bool(a.small)}
    out['corpus_%d' % ns], _ = bench(small, a.iterations, a.repetitions, 20)
    out['corpus_%d' % nl], inputs = bench(large, a.iterations, a.repetitions, 10)
    out['stopped_signals'] = bench_stopped(inputs, a.iterations, a.repetitions, out['corpus_%d' % nl]['ragged_ms_per_iteration'])
    text = json.dumps(out, indent=1)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
