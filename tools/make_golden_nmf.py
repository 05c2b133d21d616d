"""Golden vectors of the reference's ConvolutionalNMF (hsc/modeling.py:662-747) -> tests/golden/nmf.npz.

Needs the reference next to the repository (loaded read-only through oracle/ref_loader.py); run from the
repository root:  python tools/make_golden_nmf.py

Every case stores its inputs (x, D), the numpy seed of the reference's draw of the initial coefficients, the
stop parameters (NaN for None) and the reference's outputs: coefficients, residual, the number of iterations
(counted from the reference's per-iteration debug records) and the stop reason (from its closing record).
A float32 case also stores the reference's float64 result on the same inputs (x, D and the float32 initial
coefficients, upcast) as coef64 / resid64: the difference is that case's own float32 spread.
A case stopped by a tolerance has the tolerance half way between two iterations' values, and the distance of
the nearest iteration to it (dB, or relative for the residual scale) is stored as its stop margin.
"""
import contextlib
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'nmf.npz')
STOP_CODES = {'Maximum number of iterations reached': 1, 'Tolerance for residual scale (absolute value) reached': 2,
              'Tolerance for signal-to-noise ratio reached': 3}


class _Records(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self, logging.DEBUG)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


@contextlib.contextmanager
def _init_as_float32():
    """The reference's float64 run on the float32 run's initial coefficients (float32(r) + 2 in float32): the draw is
    handed over as that value minus 2 (exact in float64), to which the reference adds 2 again."""
    orig = np.random.random
    np.random.random = lambda size=None: (orig(size).astype(np.float32) + np.float32(2.0)).astype(np.float64) - 2.0
    try:
        yield
    finally:
        np.random.random = orig


def run_ref(mod, x, D, seed, maxIt, tolRs, tolSnr):
    h = _Records()
    log = logging.getLogger(mod.__name__)
    log.addHandler(h)
    old = log.level
    log.setLevel(logging.DEBUG)
    try:
        np.random.seed(seed)
        coef, resid = mod.ConvolutionalNMF().computeCoefficients(x, D, nbMaxIterations=maxIt, toleranceResidualScale=tolRs,
                                                                 toleranceSnr=tolSnr)
    finally:
        log.removeHandler(h)
        log.setLevel(old)
    iters = sum(1 for m in h.messages if m.startswith('SNR of '))
    stop = [STOP_CODES[m] for m in h.messages if m in STOP_CODES]
    assert len(stop) == 1
    return np.asarray(coef), np.asarray(resid), iters, stop[0]


def make_inputs(seed, T, K, W, F, dtype, planted=False):
    """Uniform signal and atoms (the reference unittest's data), or (planted) a signal made of a few atoms of D plus a
    little positive noise, on which the residual shrinks from one iteration to the next and the tolerances can stop."""
    rs = np.random.RandomState(seed)
    x = rs.random_sample((T,) if F == 1 else (T, F))
    D = rs.random_sample((K, W) if F == 1 else (K, W, F))
    D = D / np.sqrt(np.sum(np.square(D.reshape(K, -1)), axis=1)).reshape((K,) + (1,) * (D.ndim - 1))
    if planted:
        D3 = D.reshape((K, W, -1))
        x = 0.01 * x.reshape((T, -1))
        for t in rs.randint(0, T - W + 1, size=max(2, T // W)):
            x[t:t + W] += (1.0 + rs.random_sample()) * D3[rs.randint(K)]
        x = x.reshape((T,) if F == 1 else (T, F))
    return x.astype(dtype), D.astype(dtype)


def pick_tolerance(mod, x, D, seed, kind, target, min_margin):
    """A tolerance that first stops the reference at an iteration >= `target` (SNR: not monotone in the iterations),
    half way between that iteration's value and the best one before it (target 1: just past the first iteration's
    value; on these signals the residual scale grows after the first iteration); returns (tolerance, margin, iteration)."""
    vals = []
    e = np.sum(np.square(x.astype(np.float64)))
    for i in range(1, 40):
        _, r, _, _ = run_ref(mod, x, D, seed, i, None, None)
        r = r.astype(np.float64)
        vals.append(10.0 * np.log10(e / np.sum(np.square(r))) if kind == 'snr' else float(np.max(np.abs(r))))
        if target == 1:                        # (stop at the first iteration: the tolerance just past its value)
            tol = vals[0] * (1.0 + 1e-3) if kind == 'rs' else vals[0] - 0.5
            return tol, (1e-3 / (1.0 + 1e-3) if kind == 'rs' else 0.5), 1
        if i < target:
            continue
        best = max(vals[:-1]) if kind == 'snr' else min(vals[:-1])
        tol = 0.5 * (best + vals[-1])
        margin = abs(vals[-1] - best) / 2 if kind == 'snr' else abs(vals[-1] - best) / 2 / tol
        if (vals[-1] > best if kind == 'snr' else vals[-1] < best) and margin >= min_margin:
            return tol, margin, i
    raise RuntimeError('no tolerance found: %s' % vals)


# The coefficients ([T,K] float64 per case, and twice for a float32 case) are most of the file: the shapes are kept
# small (the long cases have few atoms) so that the fixture stays a small test vector (about 0.4 MB).
CASES = [
    # name, dtype, T, K, W, F, nbMaxIterations, stop kind (None: iteration count), target iteration
    ('f64_w5', np.float64, 128, 8, 5, 1, 10, None, 0),
    ('f64_w9', np.float64, 128, 8, 9, 1, 10, None, 0),
    ('f64_w16', np.float64, 128, 8, 16, 1, 10, None, 0),
    ('f64_w2', np.float64, 100, 8, 2, 1, 6, None, 0),
    ('f64_f7_w15', np.float64, 64, 16, 15, 7, 10, None, 0),
    ('f64_f7_w4', np.float64, 80, 12, 4, 7, 4, None, 0),
    ('f64_t2048', np.float64, 2048, 4, 32, 1, 3, None, 0),
    ('f64_snr', np.float64, 128, 8, 6, 1, 50, 'snr', 2),
    ('f64_rs', np.float64, 128, 8, 7, 1, 50, 'rs', 1),
    ('f64_f7_snr', np.float64, 60, 6, 5, 7, 50, 'snr', 2),
    ('f32_w16', np.float32, 128, 8, 16, 1, 10, None, 0),
    ('f32_w5', np.float32, 128, 8, 5, 1, 10, None, 0),
    ('f32_w2', np.float32, 100, 8, 2, 1, 5, None, 0),
    ('f32_f7_w15', np.float32, 64, 16, 15, 7, 5, None, 0),
    ('f32_t2048', np.float32, 2048, 2, 32, 1, 2, None, 0),
    ('f32_snr', np.float32, 128, 8, 6, 1, 50, 'snr', 1),
    ('f32_rs', np.float32, 128, 8, 7, 3, 50, 'rs', 1),
]


def main():
    ns = ref_loader.load_reference()
    if ns is None:
        raise SystemExit('the reference is not available')
    mod = ns.modeling
    out = {'names': np.array([c[0] for c in CASES])}
    for i, (name, dt, T, K, W, F, maxIt, kind, target) in enumerate(CASES):
        seed = 1000 + i
        x, D = make_inputs(seed, T, K, W, F, dt, planted=kind is not None)
        tolRs = tolSnr = None
        margin = np.nan
        # stop margins: >= 1e-3 dB / 1e-6 relative in float64; float32 cases keep 100 times more (their spread)
        if kind == 'snr':
            tolSnr, margin, target = pick_tolerance(mod, x, D, seed, 'snr', target, 1e-3 if dt == np.float64 else 1e-1)
        elif kind == 'rs':
            tolRs, margin, target = pick_tolerance(mod, x, D, seed, 'rs', target, 1e-6 if dt == np.float64 else 1e-4)
        coef, resid, iters, stop = run_ref(mod, x, D, seed, maxIt, tolRs, tolSnr)
        if kind is not None:
            assert iters == target and stop == (3 if kind == 'snr' else 2), (name, iters, stop)
        p = name + '/'
        out.update({p + 'x': x, p + 'D': D, p + 'seed': np.int64(seed), p + 'max_iterations': np.int64(maxIt),
                    p + 'tol_rs': np.float64(np.nan if tolRs is None else tolRs),
                    p + 'tol_snr': np.float64(np.nan if tolSnr is None else tolSnr), p + 'margin': np.float64(margin),
                    p + 'coef': coef, p + 'resid': resid, p + 'iterations': np.int64(iters), p + 'stop': np.int64(stop)})
        if dt == np.float32:
            with _init_as_float32():
                c64, r64, it64, st64 = run_ref(mod, x.astype(np.float64), D.astype(np.float64), seed, maxIt, tolRs, tolSnr)
            assert (it64, st64) == (iters, stop), (name, it64, iters)
            out.update({p + 'coef64': c64, p + 'resid64': r64})
            spread = np.max(np.abs(coef - c64)) / np.max(np.abs(c64))
        else:
            spread = 0.0
        print('%-12s T=%5d K=%3d W=%2d F=%d  %2d iterations, stop %d, margin %s, f32 spread %.2e' % (
            name, T, K, W, F, iters, stop, margin, spread))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
