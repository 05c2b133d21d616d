"""Times batches with stop rules per signal (hscmp_encode_batch_rules_device) against what a caller had to do
without them, in the same process and on the same build:

  1. A rate-distortion sweep: ONE signal of 65536 samples (config-2 dictionary, 256 atoms x 64 taps, float32) encoded to 16
     toleranceSnr targets from 5 to 35 dB, with nbBlocks = 1 and 'auto' -- one rules batch of 16 copies against 16 calls of B = 1.
     The 16 results are compared pairwise, bit for bit.
  2. The ragged corpus of tools/bench_ragged.py (B = 1024, lengths uniform in [16384, 65536]) with nbNonzeroCoefs_b = T_b // 256
     -- one rules batch against (a) one ragged call per distinct nbNonzeroCoefs and (b) one ragged call with the largest
     nbNonzeroCoefs for every signal (not the same result: it shows the work the rules save).
  3. --regression FILES: folds `python bench.py` lines and tools/bench_ragged.py outputs measured at the parent commit and at this
     one into the report and says whether this commit's median lies inside the parent's own min-max (files named
     parent_bench_*.json, branch_bench_*.json, parent_ragged_*.json, branch_ragged_*.json).

  python tools/bench_rules.py [--out profiles/rules_bench.json] [--steps 5] [--warmup 1] [--repeats 3]
  python tools/bench_rules.py --skip rate_distortion ragged_corpus --base profiles/rules_bench.json --regression FILES... --out ...
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hsc_amd.synth as synth  # noqa: E402
from hsc_amd import _native  # noqa: E402


def _spread(values):
    v = sorted(float(x) for x in values)
    return dict(runs=[round(x, 3) for x in values], min=round(v[0], 3), median=round(float(np.median(v)), 3), max=round(v[-1], 3))


def _results(eng):
    st = eng.fetch_stats().copy()
    t, k, c = eng.fetch_events()
    return st, t.copy(), k.copy(), c.copy(), eng.fetch_residual().copy(), eng.fetch_energies().copy()


def _same_signal(a, ia, b, ib, T):
    n = int(a[0][ia, _native.STAT_EVENTS])
    return bool(np.array_equal(a[0][ia], b[0][ib]) and all(np.array_equal(a[j][ia, :n], b[j][ib, :n]) for j in (1, 2, 3)) and
                np.array_equal(a[4][ia, :T], b[4][ib, :T]) and np.array_equal(a[5][ia], b[5][ib]))


def rate_distortion(args, torch, dev, stream):
    T, targets = args.T, [float(v) for v in np.linspace(5.0, 35.0, 16)]
    D = synth.make_dictionary(args.K, args.W, seed=2, dtype=np.float32)
    x = synth.make_signal(D, T, 0, kind='planted', nb_atoms=256, seed=2)
    eps = float(np.finfo(np.float32).eps)
    eng = _native.Engine(0)
    eng.set_stream(stream.cuda_stream)
    eng.set_dictionary(D)
    x1 = torch.from_numpy(x.reshape((1, T, 1))).to(dev)
    x16 = torch.from_numpy(np.repeat(x.reshape((1, T, 1)), len(targets), axis=0).copy()).to(dev)
    out = dict(workload='one planted signal of %d samples, dictionary %d x %d float32, toleranceSnr %s dB' % (T, args.K, args.W, targets))
    for nb in (1, 'auto'):
        cap = 8192
        rules = _native.make_rules(len(targets), toleranceSnr=targets)
        params = _native.make_params(nbBlocks=nb, eps=eps, maxEvents=cap)
        singles = [_native.make_params(toleranceSnr=v, nbBlocks=nb, eps=eps, maxEvents=cap) for v in targets]

        def batch():
            eng.encode_batch_rules_device(x16.data_ptr(), len(targets), T, None, rules, params)

        def calls(keep=None):
            for i, p in enumerate(singles):
                eng.encode_batch_device(x1.data_ptr(), 1, T, p)
                if keep is not None:
                    eng.synchronize()
                    keep.append((_results(eng), eng.last_variant()))

        def timed(step):
            runs = []
            for _ in range(args.repeats):
                for _ in range(args.warmup):
                    step()
                stream.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                stream.synchronize()
                runs.append((time.perf_counter() - t0) * 1e3 / args.steps)
            return _spread(runs)

        rec = dict(rules_batch_ms=timed(batch))
        eng.synchronize()
        rec['rules_variant'] = eng.last_variant()
        got = _results(eng)
        rec['per_call_ms'] = timed(calls)
        kept = []
        calls(kept)
        rec['per_call_variants'] = sorted(set(v for _, v in kept))
        rec['selections'] = [int(n) for n in got[0][:, _native.STAT_ITERATIONS]]
        rec['stop_reasons'] = sorted(set(_native.STOP_NAMES.get(int(s)) for s in got[0][:, _native.STAT_STOP]))
        rec['all_16_bit_identical'] = all(_same_signal(got, i, one, 0, T) for i, (one, _) in enumerate(kept))
        rec['speedup'] = round(rec['per_call_ms']['median'] / rec['rules_batch_ms']['median'], 2)
        out['nbBlocks_%s' % nb] = rec
    eng.close()
    return out


def ragged_corpus(args, torch, dev, stream):
    B = args.B
    D = synth.make_dictionary(args.K, args.W, seed=2, dtype=np.float32)
    lengths = np.random.RandomState(3).randint(args.tmin, args.tmax + 1, size=B).astype(np.int32)
    l0 = (lengths // 256).astype(np.int32)
    Tmax = int(lengths.max())
    xr = np.zeros((B, Tmax, 1), dtype=np.float32)
    for b, n in enumerate(lengths):
        xr[b, :n, 0] = synth.make_signal(D, int(n), b, kind='planted', nb_atoms=256, seed=2)
    eps = float(np.finfo(np.float32).eps)
    cap = 2 * int(l0.max()) + 64
    eng = _native.Engine(0)
    eng.set_stream(stream.cuda_stream)
    eng.set_dictionary(D)
    xd = torch.from_numpy(xr).to(dev)
    rules = _native.make_rules(B, nbNonzeroCoefs=l0)
    params = _native.make_params(eps=eps, maxEvents=cap)
    groups = []
    for v in sorted(set(int(n) for n in l0)):
        idx = np.where(l0 == v)[0]
        T = int(lengths[idx].max())
        groups.append((idx, T, torch.from_numpy(np.ascontiguousarray(xr[idx, :T])).to(dev), lengths[idx].copy(),
                       _native.make_params(nbNonzeroCoefs=v, eps=eps, maxEvents=cap)))
    p_max = _native.make_params(nbNonzeroCoefs=int(l0.max()), eps=eps, maxEvents=cap)

    def timed(step):
        runs = []
        for _ in range(args.repeats):
            for _ in range(args.warmup):
                step()
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            stream.synchronize()
            runs.append((time.perf_counter() - t0) * 1e3 / args.steps)
        return _spread(runs)

    def per_l0(keep=None):
        for idx, T, xg, lens, p in groups:
            eng.encode_batch_ragged_device(xg.data_ptr(), len(idx), T, lens, p)
            if keep is not None:
                eng.synchronize()
                keep.append(_results(eng))

    out = dict(workload='config-2 dictionary (K=%d, W=%d, float32), nbBlocks=1, B=%d, ragged lengths uniform in [%d, %d] (seed 3), '
                        'nbNonzeroCoefs_b = T_b // 256: %d to %d, %d distinct' % (args.K, args.W, B, args.tmin, args.tmax, int(l0.min()),
                                                                                  int(l0.max()), len(groups)))
    out['rules_batch_ms'] = timed(lambda: eng.encode_batch_rules_device(xd.data_ptr(), B, Tmax, lengths, rules, params))
    eng.synchronize()
    out['rules_variant'] = eng.last_variant()
    got = _results(eng)
    out['selections'] = int(got[0][:, _native.STAT_ITERATIONS].sum())
    out['all_stop_nnz'] = bool(np.all(got[0][:, _native.STAT_STOP] == 2))
    out['one_call_per_distinct_l0_ms'] = timed(per_l0)
    kept = []
    per_l0(kept)
    out['rules_rows_equal_per_l0_calls'] = all(_same_signal(got, int(b), res, i, int(lengths[b]))
                                               for (idx, _, _, _, _), res in zip(groups, kept) for i, b in enumerate(idx))
    out['one_call_with_max_l0_ms'] = timed(lambda: eng.encode_batch_ragged_device(xd.data_ptr(), B, Tmax, lengths, p_max))
    eng.synchronize()
    out['max_l0_selections'] = int(eng.fetch_stats()[:, _native.STAT_ITERATIONS].sum())
    out['rules_over_per_l0_calls'] = round(out['one_call_per_distinct_l0_ms']['median'] / out['rules_batch_ms']['median'], 2)
    out['rules_over_max_l0_call'] = round(out['one_call_with_max_l0_ms']['median'] / out['rules_batch_ms']['median'], 2)
    eng.close()
    return out


def regression(files):
    """bench.py lines ('value' in atom-selections/s, 'ms_per_step') and bench_ragged.py outputs (ragged.ms_per_batch) of the parent
    commit and of this one: is this commit's median inside the parent's min-max."""
    sets = {}
    for path in files:
        name = os.path.basename(path)
        side, kind = name.split('_')[0], name.split('_')[1]
        with open(path) as fh:
            text = fh.read()
        rec = json.loads(text if kind == 'ragged' else [ln for ln in text.splitlines() if ln.startswith('{')][-1])
        value = rec['ragged']['ms_per_batch'] if kind == 'ragged' else rec['ms_per_step']
        sets.setdefault(kind, {}).setdefault(side, []).append(value)
    out = {}
    for kind, sides in sets.items():
        rec = {side: _spread(vals) for side, vals in sides.items()}
        if 'parent' in rec and 'branch' in rec:
            rec['branch_median_inside_parent_min_max'] = bool(rec['parent']['min'] <= rec['branch']['median'] <= rec['parent']['max'])
            rec['branch_median_over_parent_median'] = round(rec['branch']['median'] / rec['parent']['median'], 4)
        rec['unit'] = 'ms per batch (tools/bench_ragged.py, ragged)' if kind == 'ragged' else 'ms per step (bench.py)'
        out[kind] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--B', type=int, default=1024)
    ap.add_argument('--T', type=int, default=65536)
    ap.add_argument('--K', type=int, default=256)
    ap.add_argument('--W', type=int, default=64)
    ap.add_argument('--tmin', type=int, default=16384)
    ap.add_argument('--tmax', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3, help='timed repetitions of every measurement (their spread is reported)')
    ap.add_argument('--regression', nargs='*', default=[], metavar='FILE')
    ap.add_argument('--skip', nargs='*', default=[], choices=['rate_distortion', 'ragged_corpus'])
    ap.add_argument('--base', default=None, metavar='FILE', help='an earlier report to extend (with both sections skipped: no GPU is needed)')
    args = ap.parse_args()
    out = {}
    if args.base:
        with open(args.base) as fh:
            out = json.load(fh)
    if len(set(args.skip)) < 2:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_rules.py measures on the GPU and found none')
        dev = torch.device('cuda:0')
        stream = torch.cuda.Stream(device=dev)
        out.update(steps=args.steps, warmup=args.warmup, repeats=args.repeats, device=torch.cuda.get_device_name(0))
        if 'rate_distortion' not in args.skip:
            out['rate_distortion'] = rate_distortion(args, torch, dev, stream)
        if 'ragged_corpus' not in args.skip:
            out['ragged_corpus'] = ragged_corpus(args, torch, dev, stream)
    if args.regression:
        out['regression'] = regression(args.regression)
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
