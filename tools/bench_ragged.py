"""Times a ragged batch (signals of different lengths in one call, hscmp_encode_batch_ragged_device) on the config-2 dictionary
(256 atoms x 64 taps, float32, nbNonzeroCoefs = 256, nbBlocks = 1, B = 1024) against, in the same process:
  - a uniform batch at T = 65536 (the longest length the ragged batch may hold: what zero-padding every signal would cost);
  - a uniform batch at the mean length of the ragged one (the same samples spread evenly);
  - one computeCoefficients call per signal, on 32 of the ragged signals, scaled up to the batch.
The lengths are drawn uniformly from [16384, 65536] under a fixed seed.  Each signal the per-signal loop encodes is also
compared, bit for bit, with its row of the ragged batch.

  python tools/bench_ragged.py [--out profiles/ragged_bench.json] [--steps 10] [--warmup 2]
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
from hsc_amd.modeling import ConvolutionalMatchingPursuit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--B', type=int, default=1024)
    ap.add_argument('--K', type=int, default=256)
    ap.add_argument('--W', type=int, default=64)
    ap.add_argument('--L0', type=int, default=256)
    ap.add_argument('--tmin', type=int, default=16384)
    ap.add_argument('--tmax', type=int, default=65536)
    ap.add_argument('--loop-signals', type=int, default=32)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_ragged.py measures on the GPU and found none')
    dev = torch.device('cuda:0')
    B, L0 = args.B, args.L0
    D = synth.make_dictionary(args.K, args.W, seed=2, dtype=np.float32)
    lengths = np.random.RandomState(args.seed).randint(args.tmin, args.tmax + 1, size=B).astype(np.int32)
    tmean = int(round(float(lengths.mean())))
    ragged = [synth.make_signal(D, int(n), i, kind='planted', nb_atoms=L0, seed=2) for i, n in enumerate(lengths)]
    Tmax = int(lengths.max())
    xr = np.zeros((B, Tmax, 1), dtype=np.float32)
    for b, s in enumerate(ragged):
        xr[b, :len(s), 0] = s

    stream = torch.cuda.Stream(device=dev)
    eng = _native.Engine(0)
    eng.set_stream(stream.cuda_stream)
    eng.set_dictionary(D)
    params = _native.make_params(nbNonzeroCoefs=L0, nbBlocks=1, minCoefficients=1e-16, eps=float(np.finfo(np.float32).eps),
                                 maxEvents=2 * L0 + 64)

    def timed(step):
        for _ in range(args.warmup):
            step()
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        stream.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        st = eng.fetch_stats()
        sel = int(st[:, _native.STAT_ITERATIONS].sum())
        return dict(ms_per_batch=round(ms, 3), selections=sel, selections_per_s=round(sel / (ms * 1e-3), 1),
                    variant=eng.last_variant(), all_stop_nnz=bool(np.all(st[:, _native.STAT_STOP] == 2)))

    out = dict(workload='config-2 dictionary (K=%d, W=%d, float32), nbNonzeroCoefs=%d, nbBlocks=1, B=%d; ragged lengths uniform in '
                        '[%d, %d], seed %d' % (args.K, args.W, L0, B, args.tmin, args.tmax, args.seed),
               lengths=dict(min=int(lengths.min()), max=Tmax, mean=float(lengths.mean()), samples=int(lengths.sum())),
               steps=args.steps, warmup=args.warmup)

    xd = torch.from_numpy(xr).to(dev)
    out['ragged'] = timed(lambda: eng.encode_batch_ragged_device(xd.data_ptr(), B, Tmax, lengths, params))
    st_r = eng.fetch_stats()
    t_r, k_r, c_r = eng.fetch_events()
    r_r = eng.fetch_residual()
    out['ragged_length_ordering'] = 'not built: each signal keeps its own persistent workgroup (or quarter of one), see DESIGN.md section 15'
    del xd

    for name, T in (('uniform_T%d' % args.tmax, args.tmax), ('uniform_mean_T%d' % tmean, tmean)):
        xu = torch.from_numpy(synth.make_batch(D, T, 0, B, kind='planted', nb_atoms=L0, seed=2, dtype=np.float32)).to(dev)
        out[name] = timed(lambda: eng.encode_batch_device(xu.data_ptr(), B, T, params))
        out[name]['samples'] = B * T
        del xu
    out['ragged']['samples'] = int(lengths.sum())

    # one computeCoefficients call per signal (B = 1 each), the first `loop-signals` ragged signals, scaled to the batch
    cmp = ConvolutionalMatchingPursuit()
    n = min(args.loop_signals, B)
    cmp.computeCoefficients(ragged[0], D, nbNonzeroCoefs=L0)            # (warm-up)
    same = True
    t0 = time.perf_counter()
    results = []
    for b in range(n):
        coef, residual = cmp.computeCoefficients(ragged[b], D, nbNonzeroCoefs=L0)
        results.append((cmp.lastResult.events[0], cmp.lastResult.stats[0], residual))
    loop_s = time.perf_counter() - t0
    for b, (ev, st, residual) in enumerate(results):
        ne = int(st_r[b, _native.STAT_EVENTS])
        same = same and np.array_equal(ev[0], t_r[b, :ne]) and np.array_equal(ev[1], k_r[b, :ne]) and np.array_equal(ev[2], c_r[b, :ne])
        same = same and np.array_equal(st, st_r[b]) and np.array_equal(residual, r_r[b, :len(residual), 0])
    per_signal_ms = loop_s * 1e3 / n
    out['per_signal_loop'] = dict(signals_timed=n, ms_per_signal=round(per_signal_ms, 3), ms_per_batch_scaled=round(per_signal_ms * B, 1),
                                  selections_per_s=round(L0 / (per_signal_ms * 1e-3), 1))
    out['output_check'] = dict(ragged_rows_equal_per_signal_encodes=bool(same), signals_compared=n)
    out['speedup_ragged_over_per_signal_loop'] = round(out['per_signal_loop']['ms_per_batch_scaled'] / out['ragged']['ms_per_batch'], 1)
    out['ragged_over_uniform_Tmax'] = round(out['ragged']['ms_per_batch'] / out['uniform_T%d' % args.tmax]['ms_per_batch'], 3)
    out['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    eng.close()


if __name__ == '__main__':
    main()
