"""The wide loop (csrc/hscmp_wide.h) against the round-parallel and the one-atom-at-a-time loops, for few
long signals.  Writes profiles/wide_bench.json.

    python tools/bench_wide.py --out profiles/wide_bench.json --parent build/parent

--parent: a checkout of the parent commit with its libhscmp.so built.  Either tree runs in child processes of its own, alternating, `--rounds`
times each; a child warms every (shape, loop) once and then times `--reps` encodes.  The loop time is hscmp_last_kernel_ms()[2]:
HIP events around the loop on the context's stream -- for the wide loop that spans the host's reads of the control blocks.
Without --parent the other loops come from this tree (HSCMP_WIDE=0), and the file says so.

The share of the loop spent in each of the four wide kernels is a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_wide.py --child --shape 128,32,1,262144,auto --loops wide
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCHES = (1, 4, 16, 64)
LENGTHS = (65536, 262144, 1048576)
DICTS = ((128, 32), (256, 64))
BLOCKS = ('auto', 10)
SNR = 20.0
LOOP_ENV = {'wide': dict(HSCMP_WIDE='1'), 'rp': dict(HSCMP_WIDE='0', HSCMP_RP='1'), 'seq': dict(HSCMP_WIDE='0', HSCMP_RP='0'),
            'default': dict()}


def shapes(max_samples):
    return [(K, W, B, T, nb) for K, W in DICTS for T in LENGTHS for B in BATCHES for nb in BLOCKS if B * T <= max_samples]


def child(args):
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)
    import numpy as np
    import hsc_amd.synth as synth
    from hsc_amd import _native
    from hsc_amd.modeling import ConvolutionalMatchingPursuit
    for spec in args.shape:
        K, W, B, T, nb = spec.split(',')
        K, W, B, T = int(K), int(W), int(B), int(T)
        nb = nb if nb == 'auto' else int(nb)
        D = synth.make_dictionary(K, W, seed=1)
        xs = synth.make_batch(D, T, 0, B, kind='planted', nb_atoms=T // 100, noise=0.03, seed=1)
        for loop in args.loops.split(','):
            for name in ('HSCMP_WIDE', 'HSCMP_RP'):
                os.environ.pop(name, None)
            os.environ.update(LOOP_ENV[loop])
            cmp = ConvolutionalMatchingPursuit()
            ms, wall, res = [], [], None
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                res = cmp.computeCoefficientsBatch(xs, D, nbBlocks=nb, toleranceSnr=SNR, maxEvents=max(4096, T // 16))
                if rep:                                         # (the first run warms the kernels and the workspace)
                    ms.append(float(res.kernel_ms[2]))
                    wall.append(1e3 * (time.perf_counter() - t0))
            h = hashlib.sha256()
            for b in range(B):
                for a in res.events[b]:
                    h.update(np.ascontiguousarray(a).tobytes())
                h.update(np.ascontiguousarray(res.residuals[b]).tobytes())
            h.update(np.ascontiguousarray(res.stats).tobytes())
            eng = _native.engine_for(0, D[:, :, None], None)
            line = dict(K=K, W=W, B=B, T=T, nbBlocks=nb, loop=loop, variant=res.variant, loop_ms=ms, wall_ms=wall,
                        rounds=[int(v) for v in res.stats[:, 2]], events=[int(v) for v in res.stats[:, 5]],
                        digest=h.hexdigest(), counters=list(eng.wide_counters()) if hasattr(eng, 'wide_counters') else None)
            print('BENCH ' + json.dumps(line), flush=True)


def run_child(lib, specs, loops, reps):
    env = dict(os.environ)
    env.pop('HSCMP_LIBRARY', None)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--loops', loops, '--reps', str(reps)]
    if lib:
        cmd += ['--root', lib]
    for s in specs:
        cmd += ['--shape', '%d,%d,%d,%d,%s' % s]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit('a child failed with exit code %d' % out.returncode)
    return [json.loads(l[6:]) for l in out.stdout.splitlines() if l.startswith('BENCH ')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wide_bench.json'))
    ap.add_argument('--parent', default=None, help="a checkout of the parent commit, built (the baseline columns)")
    ap.add_argument('--root', default=None, help='(child) the tree to import the package from')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--max-samples', type=int, default=1 << 25, help='skip shapes with more than this many samples per batch')
    ap.add_argument('--only', default=None, help='K,W of one dictionary')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--loops', default='wide')
    args = ap.parse_args()
    if args.child:
        return child(args)
    todo = shapes(args.max_samples)
    if args.only:
        K, W = (int(v) for v in args.only.split(','))
        todo = [s for s in todo if s[:2] == (K, W)]
    rows = {}
    for rnd in range(args.rounds):                               # this tree and the baseline alternating
        for who, lib, loops in (('this', None, 'wide,default'), ('base', args.parent, 'rp,seq')):
            for line in run_child(lib, todo, loops, args.reps):
                key = (line['K'], line['W'], line['B'], line['T'], str(line['nbBlocks']))
                row = rows.setdefault(key, dict(K=line['K'], W=line['W'], B=line['B'], T=line['T'], nbBlocks=line['nbBlocks'], loops={}))
                cell = row['loops'].setdefault(line['loop'], dict(variant=line['variant'], loop_ms=[], wall_ms=[], digest=line['digest'],
                                                                 rounds=line['rounds'], events=line['events'], counters=line['counters']))
                cell['loop_ms'] += line['loop_ms']
                cell['wall_ms'] += line['wall_ms']
                assert cell['digest'] == line['digest'], 'two runs of one loop differ: %r' % (key,)
    table = []
    for key in sorted(rows):
        row = rows[key]
        for cell in row['loops'].values():
            v = sorted(cell['loop_ms'])
            cell['median_ms'], cell['min_ms'], cell['max_ms'] = v[len(v) // 2], v[0], v[-1]
        digests = set(c['digest'] for c in row['loops'].values())
        row['bit_identical'] = len(digests) == 1
        rounds = max(row['loops']['wide']['rounds'])
        row['wide_ms_per_round'] = row['loops']['wide']['median_ms'] / max(1, rounds)
        c = row['loops']['wide']['counters']
        if c:
            row['steps_queued'], row['host_polls'], row['steps_with_work'], row['no_op_steps'] = c[0], c[1], c[2], c[0] * c[3] - c[2]
        table.append(row)
    doc = dict(tool='tools/bench_wide.py', snr=SNR, signals="synth.make_batch(kind='planted', nb_atoms=T // 100, noise=0.03, seed=1)",
               baseline='the parent commit built beside this tree' if args.parent else "this tree's own loops (HSCMP_WIDE=0)",
               rounds=args.rounds, reps=args.reps, max_samples=args.max_samples, rows=table)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    for row in table:
        L = row['loops']
        print('%3dx%-2d B=%-2d T=%-7d nb=%-4s wide %8.3f [%7.3f %7.3f]  rp %s  seq %8.3f [%7.3f %7.3f]  default=%s same=%s steps=%s polls=%s' % (
            row['K'], row['W'], row['B'], row['T'], row['nbBlocks'], L['wide']['median_ms'], L['wide']['min_ms'], L['wide']['max_ms'],
            ('%8.3f' % L['rp']['median_ms']) if L['rp']['variant'].endswith('_rp') else '   (seq)',
            L['seq']['median_ms'], L['seq']['min_ms'], L['seq']['max_ms'], L['default']['variant'].split('_')[-1], row['bit_identical'],
            row.get('steps_queued'), row.get('host_polls')))


if __name__ == '__main__':
    main()
