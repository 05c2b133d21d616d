"""Golden vectors of the reference's convolutional NMF dictionary learner (ConvolutionalDictionaryLearner(algorithm='nmf'),
hsc/modeling.py:330-417) -> tests/golden/nmf_learn.npz.

Needs the reference next to the repository (loaded read-only through oracle/ref_loader.py); run from the
repository root:  python tools/make_golden_nmf_learn.py

Every case stores its signal x, the numpy seed under which the reference draws its initial dictionary and then its
initial coefficients (the draws themselves are not stored: tests redo them from the seed), the init method, the stop
parameters (NaN for None) and the reference's outputs: the dictionary D, the number of iterations (counted from the
reference's per-iteration debug records) and the stop reason (from its closing record).
A float32 case also stores the reference's float64 run on the same draws as D64 (x, the initial dictionary and the
initial coefficients upcast): the difference is that case's own float32 spread.  For float32 data with 'noise' the
reference's D is float64 while its coefficients stay float32 (a mixed run); D64 is then the all-float64 run.
A case stopped by a tolerance has the tolerance half way between two iterations' values, and the distance of the
nearest iteration to it (dB, or relative for the residual scale) is stored as its stop margin.
"""
import contextlib
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'nmf_learn.npz')
STOP_CODES = {'Maximum number of iterations reached': 1, 'Tolerance for residual scale (absolute value) reached': 2,
              'Tolerance for signal-to-noise ratio reached': 3}


class _Records(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self, logging.DEBUG)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


@contextlib.contextmanager
def _as_float64_of_float32(cdl):
    """The reference's float64 run on the float32 run's draws: the initial dictionary is drawn from the float32 data and
    upcast; the initial coefficients are handed over as float32(r) + 2 minus 2 (exact in float64), to which the
    reference adds 2 again."""
    orig_random, orig_init = np.random.random, cdl._init_D
    np.random.random = lambda size=None: (orig_random(size).astype(np.float32) + np.float32(2.0)).astype(np.float64) - 2.0
    cdl._init_D = lambda data, initMethod='random_samples': orig_init(data.astype(np.float32), initMethod).astype(np.float64)
    try:
        yield
    finally:
        np.random.random = orig_random
        del cdl._init_D


def run_ref(mod, x, seed, K, W, init, maxIt, tolRs, tolSnr, as64=False):
    h = _Records()
    log = logging.getLogger(mod.__name__)
    log.addHandler(h)
    old = log.level
    log.setLevel(logging.DEBUG)
    cdl = mod.ConvolutionalDictionaryLearner(k=K, windowSize=W, algorithm='nmf')
    try:
        np.random.seed(seed)
        if as64:
            with _as_float64_of_float32(cdl):
                D = cdl.train(x.astype(np.float64), initMethod=init, nbMaxIterations=maxIt, toleranceResidualScale=tolRs,
                              toleranceSnr=tolSnr)
        else:
            D = cdl.train(x, initMethod=init, nbMaxIterations=maxIt, toleranceResidualScale=tolRs, toleranceSnr=tolSnr)
    finally:
        log.removeHandler(h)
        log.setLevel(old)
    iters = sum(1 for m in h.messages if m.startswith('SNR of '))
    stop = [STOP_CODES[m] for m in h.messages if m in STOP_CODES]
    assert len(stop) == 1
    snr = float([m for m in h.messages if m.startswith('SNR of ')][-1].split()[2])
    return np.asarray(D), iters, stop[0], snr


def make_signal(seed, T, F, dtype, planted=False, K=8, W=6):
    """Uniform samples (the reference unittests' data), or (planted) a few positive atoms plus a little positive noise,
    on which the learner's residual shrinks over the iterations and the tolerances can stop."""
    rs = np.random.RandomState(seed)
    x = rs.random_sample((T, F))
    if planted:
        D = rs.random_sample((K, W, F))
        D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
        x = 0.01 * x
        for t in rs.randint(0, T - W + 1, size=max(2, T // W)):
            x[t:t + W] += (1.0 + rs.random_sample()) * D[rs.randint(K)]
    x = x[:, 0] if F == 1 else x
    return x.astype(dtype)


def pick_tolerance(mod, x, seed, K, W, init, kind, target, min_margin):
    """A tolerance that first stops the reference at an iteration >= `target`, half way between that iteration's value
    and the best one before it; returns (tolerance, margin, iteration).  The per-iteration values come from runs of
    1, 2, ... iterations: the SNR from the reference's records, the residual scale from its last reconstruction."""
    vals = []
    for i in range(1, 40):
        if kind == 'snr':
            vals.append(run_ref(mod, x, seed, K, W, init, i, None, None)[3])
        else:
            vals.append(_rs_after(mod, x, seed, K, W, init, i))
        if i < target:
            continue
        best = max(vals[:-1]) if kind == 'snr' else min(vals[:-1])
        tol = 0.5 * (best + vals[-1])
        margin = abs(vals[-1] - best) / 2 if kind == 'snr' else abs(vals[-1] - best) / 2 / tol
        if (vals[-1] > best if kind == 'snr' else vals[-1] < best) and margin >= min_margin:
            return tol, margin, i
    if kind == 'rs':                    # never below the first iteration's value: stop there, just past it
        return vals[0] * (1.0 + 1e-3), 1e-3 / (1.0 + 1e-3), 1
    raise RuntimeError('no tolerance found: %s' % vals)


def _rs_after(mod, x, seed, K, W, init, n):
    """max |residual| of the reference after n iterations: the reference's own nbMaxIterations=n run, with the
    reference's reconstruction of its last coefficients captured through its module-level reconstructSignal."""
    seen = []
    orig = mod.reconstructSignal

    def capture(coefficients, D):
        r = orig(coefficients, D)
        seen.append(r)
        return r
    mod.reconstructSignal = capture
    try:
        run_ref(mod, x, seed, K, W, init, n, None, None)
    finally:
        mod.reconstructSignal = orig
    seq = x.reshape((x.shape[0], -1)).astype(np.float64)
    return float(np.max(np.abs(seq - np.asarray(seen[-1], np.float64).reshape(seq.shape))))


# name, dtype, T, K, W, F, initMethod, nbMaxIterations, stop kind (None: iteration count), target iteration
CASES = [
    ('u1d_f64', np.float64, 256, 16, 5, 1, 'random_samples', 100, None, 0),     # the reference unittests' shapes
    ('u2d_f64', np.float64, 256, 16, 5, 4, 'random_samples', 100, None, 0),
    ('u1d_f32', np.float32, 256, 16, 5, 1, 'random_samples', 100, None, 0),
    ('u2d_f32', np.float32, 256, 16, 5, 4, 'random_samples', 100, None, 0),
    ('w2_noise', np.float64, 120, 6, 2, 1, 'noise', 8, None, 0),
    ('w6_k5_f3', np.float64, 150, 5, 6, 3, 'random_samples', 6, None, 0),
    ('w7_k11_noise', np.float64, 200, 11, 7, 1, 'noise', 6, None, 0),
    ('w2_f3_f32', np.float32, 100, 3, 2, 3, 'random_samples', 5, None, 0),
    ('t4096', np.float32, 4096, 16, 32, 1, 'random_samples', 10, None, 0),
    ('snr', np.float64, 128, 8, 6, 1, 'random_samples', 50, 'snr', 2),
    ('rs', np.float64, 128, 8, 6, 1, 'random_samples', 50, 'rs', 2),
    ('mixed_noise_f32', np.float32, 256, 16, 5, 1, 'noise', 20, None, 0),
]


def main():
    ns = ref_loader.load_reference()
    if ns is None:
        raise SystemExit('the reference is not available')
    mod = ns.modeling
    out = {'names': np.array([c[0] for c in CASES])}
    for i, (name, dt, T, K, W, F, init, maxIt, kind, target) in enumerate(CASES):
        seed = 2000 + i
        x = make_signal(seed, T, F, dt, planted=kind is not None)
        tolRs = tolSnr = None
        margin = np.nan
        if kind == 'snr':
            tolSnr, margin, target = pick_tolerance(mod, x, seed, K, W, init, 'snr', target, 1e-3)
        elif kind == 'rs':
            tolRs, margin, target = pick_tolerance(mod, x, seed, K, W, init, 'rs', target, 1e-6)
        D, iters, stop, _ = run_ref(mod, x, seed, K, W, init, maxIt, tolRs, tolSnr)
        if kind is not None:
            assert iters == target and stop == (3 if kind == 'snr' else 2), (name, iters, stop)
        p = name + '/'
        out.update({p + 'x': x, p + 'seed': np.int64(seed), p + 'K': np.int64(K), p + 'W': np.int64(W),
                    p + 'init': np.array(init), p + 'max_iterations': np.int64(maxIt),
                    p + 'tol_rs': np.float64(np.nan if tolRs is None else tolRs),
                    p + 'tol_snr': np.float64(np.nan if tolSnr is None else tolSnr), p + 'margin': np.float64(margin),
                    p + 'D': D, p + 'iterations': np.int64(iters), p + 'stop': np.int64(stop)})
        spread = 0.0
        if dt == np.float32:
            D64, it64, st64, _ = run_ref(mod, x, seed, K, W, init, maxIt, tolRs, tolSnr, as64=True)
            assert (it64, st64) == (iters, stop), (name, it64, iters)
            out[p + 'D64'] = D64
            spread = float(np.max(np.abs(D.astype(np.float64) - D64)))
        print('%-16s T=%5d K=%3d W=%2d F=%d %-14s D %s: %3d iterations, stop %d, margin %s, f32 spread %.2e' % (
            name, T, K, W, F, init, D.dtype, iters, stop, margin, spread), flush=True)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
