"""Times MultilevelDictionaryLearner (hsc_amd.multilevel): per level, the k-means learn (with its
set-up: draws, packing, upload and the window gather) and the batch encode that hands the next level its input.

  (a) the reference script's shape (scripts/learn_mlcsc_dataset.py:84-116): one signal of T = 20 000 samples, counts
      16 / 32 / 64, scales 32 / 64 / 96, 10 000 windows, 10 iterations, SNR 10 dB, 10 blocks, singleton weight 0.95,
      method 'cmp'; the data of tools/learn_mlcsc.py.  --handoff also runs tools/learn_mlcsc.py with KMEANS=device
      in a process of its own (the same work with the dense hand-off, one signal at a time) and records the times it prints.
  (b) a corpus of 64 signals x 16 384 samples at the same counts and scales, and the k-means set-up of its level 1
      (F = 16, 10 000 windows of 2 x 33 rows) both ways on the same representation: hsckmeans_set_corpus_sparse from
      the CSR matrices against hsckmeans_set_corpus of their dense stack, host wall clock of everything trainCorpus
      does before its first step, and of the library call alone; alternating, median of 5 with [min, max]; the first
      step's outputs of both are compared byte for byte.

  (a4), (b4) the same two with a fourth level (counts 16 / 32 / 64 / 64, scales 32 / 64 / 96 / 128): the shape at which the
      hand-off encodes repeat the most lower-level work.
  --resume 1 (the learner's default) hands every level from 1 on its input by a resumed encode
  (computeCoefficientsFromLevelBatch: the new level only); --resume 0 encodes the levels below again, as before.  Every
  encode row lists the encoder's own per-level kernel times, and (--resume 1) the time of Engine.load_level alone on the
  matrices handed over: packing, upload and the unpack kernel, median of 5 with [min, max].

Every figure is a host wall clock around work that ends in a device synchronise.

  python tools/bench_multilevel.py [--out profiles/multilevel_bench.json] [--shape a|b|both|a4|b4] [--resume 0|1] [--handoff] [--quick]
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import generate_dataset as gd  # noqa: E402
from hsc_amd import kmeans  # noqa: E402
from hsc_amd.dataset import MultilevelDictionary, scalesToWindowSizes  # noqa: E402
from hsc_amd.kmeans import ConvolutionalKMeansLearner, SparseStack  # noqa: E402
from hsc_amd.modeling import HierarchicalConvolutionalMatchingPursuit, MultilevelDictionaryLearner  # noqa: E402

COUNTS, SCALES = [16, 32, 64], [32, 64, 96]
COUNTS4, SCALES4 = [16, 32, 64, 64], [32, 64, 96, 128]
ENCODE = dict(toleranceSnr=10.0, nbBlocks=10, singletonWeight=0.95)
REPS = 5


def data(B, T):
    truth = gd.build([32, 64, 128], counts=COUNTS, patience=200)          # (the dictionary of tools/learn_mlcsc.py)
    return gd.signals(truth, B, T, rate=2e-3, compression=None)[0]


def learn(x, N, iterations, counts=COUNTS, scales=SCALES, resume=True):
    learner = MultilevelDictionaryLearner(counts, scales, method='cmp', rng=np.random.RandomState(1))
    t0 = time.perf_counter()
    learner.trainCorpus(x, N, maxIterations=iterations, tolerance=0.0, resetMethod='random_samples', resume=resume, **ENCODE)
    total = time.perf_counter() - t0
    levels = []
    for level, s in enumerate(learner.lastStats):
        row = dict(level=level, input_shape=list(s['input_shape']), input_nnz=s['input_nnz'], learn_s=s['learn_s'], setup_s=s['setup_s'],
                   step_ms=[it['step_ms'] for it in s['kmeans']], encode_s=s['encode_s'], encode_nnz=s['encode_nnz'])
        if s['encode_timings'] is not None:                                    # the encoder's own account, level by level
            row['encode_levels'] = [dict(level=t['level'], variant=t['variant'], kernel_ms=float(sum(t['kernel_ms']))) for t in s['encode_timings']]
        levels.append(row)
        print('level %d: input %s nnz %s, learnt in %.3f s (set-up %.3f s), encode %s s, stored %s' % (
            level, row['input_shape'], row['input_nnz'], row['learn_s'], row['setup_s'],
            'none' if row['encode_s'] is None else '%.3f' % row['encode_s'], row['encode_nnz']), flush=True)
    return dict(total_s=total, encode_total_s=float(sum(r['encode_s'] or 0.0 for r in levels)), resume=bool(resume), levels=levels,
                dictionary_sha256=[hashlib.sha256(np.ascontiguousarray(D).tobytes()).hexdigest() for D in learner.lastDictionaries])


def load_level_alone(x, N, iterations):
    """Engine.load_level on the level-0 matrices of the corpus, as a resumed encode of level 1 does it: packing, upload, kernel."""
    from hsc_amd import _native
    reps, _ = level0_representations(x, N, iterations)
    T, K = reps[0].shape
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(np.random.RandomState(0).standard_normal((K, 8)))
        x3 = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape((len(reps), T, 1)))
        times = dict(with_signals_s=[], matrices_only_s=[], pack_s=[])
        for rep in range(REPS + 1):                                        # rep 0: allocations and the first launch
            t0 = time.perf_counter()
            eng.load_level(x3, T, reps)
            t1 = time.perf_counter()
            eng.load_level(None, T, reps)
            t2 = time.perf_counter()
            _native.pack_level(reps, T, K)
            t3 = time.perf_counter()
            if rep:
                times['with_signals_s'].append(t1 - t0); times['matrices_only_s'].append(t2 - t1); times['pack_s'].append(t3 - t2)
    finally:
        eng.close()
    row = dict(signals=len(reps), T=int(T), K=int(K), nnz=int(sum(m.nnz for m in reps)), signal_bytes=int(x3.nbytes))
    row.update({k: median_range(v) for k, v in times.items()})
    return row


def dense_handoff(T):
    """tools/learn_mlcsc.py (device k-means, dense hand-off) in a fresh process; the per-level times it prints."""
    env = dict(os.environ, KMEANS='device', T=str(T))
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'learn_mlcsc.py')], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, check=True).stdout
    rows = [dict(level=int(m.group(1)), learn_s=float(m.group(2)), encode_s=float(m.group(3)), nnz=int(m.group(4)))
            for m in re.finditer(r'level (\d+): dictionary .* learnt in ([\d.]+) s .*, encode ([\d.]+) s, nnz (\d+)', out)]
    return dict(process_s=time.perf_counter() - t0, levels=rows)


def median_range(v):
    return dict(median=float(np.median(v)), range=[float(np.min(v)), float(np.max(v))])


def setup_both_ways(reps_csc, N, W, seed=7):
    """The k-means set-up of a level on `reps_csc` (the coder's last-level matrices), sparse against dense."""
    ctx = kmeans._context(0)
    F = reps_csc[0].shape[1]
    K = 32
    D = np.random.RandomState(3).standard_normal((1, K, W, F))
    D /= np.sqrt(np.sum(D ** 2, axis=(2, 3), keepdims=True))
    mode = np.array([kmeans.ASSIGN_F64], dtype=np.int32)
    times = dict(sparse_setup_s=[], sparse_call_s=[], dense_setup_s=[], dense_call_s=[])
    outs = {}
    for rep in range(REPS + 1):                                            # rep 0: first launches and allocations, not measured
        t0 = time.perf_counter()
        seqs = kmeans.sparse_corpus_signals(reps_csc)
        stack = SparseStack(seqs)
        sig, start = kmeans.corpus_windows(seqs, N, 2 * W, np.random.RandomState(seed))
        starts = np.ascontiguousarray(stack.row_offsets[sig] + start)
        indptr, indices, values = stack.csr()
        t1 = time.perf_counter()
        ctx.set_corpus_sparse(indptr, indices, values, F, stack.row_offsets, starts, W)
        t2 = time.perf_counter()
        outs['sparse'] = [a.tobytes() for a in ctx.step(D, mode)[:5]]
        t3 = time.perf_counter()
        dense = [m.toarray() for m in reps_csc]
        x = np.ascontiguousarray(np.concatenate(dense))
        sig, start = kmeans.corpus_windows(dense, N, 2 * W, np.random.RandomState(seed))
        ro = np.zeros((len(dense) + 1,), dtype=np.int64)
        ro[1:] = np.cumsum([q.shape[0] for q in dense])
        starts_d = np.ascontiguousarray(ro[sig] + start)
        t4 = time.perf_counter()
        ctx.set_corpus(x, ro, starts_d, W)
        t5 = time.perf_counter()
        outs['dense'] = [a.tobytes() for a in ctx.step(D, mode)[:5]]
        if outs['sparse'] != outs['dense']:
            raise AssertionError('the first step differs between the sparse and the dense set-up')
        if rep:
            times['sparse_setup_s'].append(t2 - t0)
            times['sparse_call_s'].append(t2 - t1)
            times['dense_setup_s'].append(t5 - t3)
            times['dense_call_s'].append(t5 - t4)
    row = dict(signals=len(reps_csc), T=int(reps_csc[0].shape[0]), F=int(F), N=N, W=W, nnz=int(sum(m.nnz for m in reps_csc)),
               dense_bytes=int(x.nbytes), window_stack_bytes=int(N * 2 * W * F * 8), identical=True)
    row.update({k: median_range(v) for k, v in times.items()})
    return row


def level0_representations(x, N, iterations):
    widths = scalesToWindowSizes(np.asarray(SCALES))
    D0 = ConvolutionalKMeansLearner(COUNTS[0], int(widths[0]), rng=np.random.RandomState(1)).trainCorpus(
        x, N, maxIterations=iterations, resetMethod='random_samples')
    mld = MultilevelDictionary.fromRawDictionaries([D0], np.asarray(SCALES)[:1])
    hcmp = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    try:
        coefficients = hcmp.computeCoefficientsBatch(x, mld, returnDistributed=False, **ENCODE)[0]
    finally:
        hcmp.close()
    return [c[-1] for c in coefficients], int(widths[1])


def save(out, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multilevel_bench.json'))
    ap.add_argument('--shape', default='both', choices=['a', 'b', 'both', 'a4', 'b4'])
    ap.add_argument('--resume', type=int, default=1, choices=[0, 1], help='1: resumed hand-off encodes (the default of trainCorpus); 0: full re-encode')
    ap.add_argument('--handoff', action='store_true', help='(a): also run tools/learn_mlcsc.py with KMEANS=device')
    ap.add_argument('--quick', action='store_true', help='a rehearsal: short signals, few windows')
    a = ap.parse_args()
    N, iterations = (500, 2) if a.quick else (10000, 10)
    four = a.shape in ('a4', 'b4')
    counts, scales = (COUNTS4, SCALES4) if four else (COUNTS, SCALES)
    resume = bool(a.resume)
    out = dict(counts=counts, scales=scales, windows=N, iterations=iterations, encode=ENCODE, method='cmp', resume=resume)
    if a.shape in ('a', 'both', 'a4'):
        T = 3000 if a.quick else 20000
        x = data(1, T)
        print('(%s) one signal of %d samples, resume=%d' % (a.shape, T, resume), flush=True)
        learn(x, N, iterations, counts, scales, resume)                    # warm-up: libraries, engines, first launches
        runs = [learn(x, N, iterations, counts, scales, resume) for _ in range(1 if a.quick else 3)]
        out['a'] = dict(B=1, T=T, runs=runs)
        if resume:
            out['a']['load_level'] = load_level_alone(x, N, 3)
            print(json.dumps(out['a']['load_level']), flush=True)
        if a.handoff:
            out['a']['dense_handoff_script'] = [dense_handoff(T) for _ in range(1 if a.quick else 2)]
            print(json.dumps(out['a']['dense_handoff_script']), flush=True)
        save(out, a.out)
    if a.shape in ('b', 'both', 'b4'):
        B, T = (4, 3000) if a.quick else (64, 16384)
        x = data(B, T)
        print('(%s) %d signals of %d samples, resume=%d' % (a.shape, B, T, resume), flush=True)
        out['b'] = dict(B=B, T=T, run=learn(x, N, iterations, counts, scales, resume))
        if resume:
            out['b']['load_level'] = load_level_alone(x, N, 3)
            print(json.dumps(out['b']['load_level']), flush=True)
        if not four:
            reps, W1 = level0_representations(x, N, 3)
            out['b']['level1_setup'] = setup_both_ways(reps, N, W1)
            print(json.dumps(out['b']['level1_setup']), flush=True)
        save(out, a.out)


if __name__ == '__main__':
    main()
