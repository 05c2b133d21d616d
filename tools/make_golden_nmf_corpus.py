"""Golden vectors of ConvolutionalNMFLearner.trainCorpus (ONE NMF dictionary from many signals)
-> tests/golden/nmf_corpus.npz, from the reference's own learner.

Needs the reference next to the repository (loaded read-only through oracle/ref_loader.py); run from the
repository root:  python tools/make_golden_nmf_corpus.py

The reference has no corpus learner, but its _train_nmf (hsc/modeling.py:330-417) on the CONCATENATION of the signals
computes exactly the corpus sums once the coefficient rows whose atoms would straddle a join (rows T_b-W+1 .. T_b-1 of
each signal) start at exactly zero: multiplicative updates keep a zero at zero, so the reconstruction separates per
signal, N and den become sums over the signals' own rows, and energySignal, energyResidual and max|residual| become the
corpus totals.  Per case the real _train_nmf runs on the concatenation with
  * np.random.random patched to hand over the prepared coefficients minus 2.0 (the straddling rows -2.0: exactly 0 after
    the reference's `+ 2.0`; the other rows r + 2.0 - 2.0, which the `+ 2.0` restores exactly), and
  * _init_D patched to return the stored D_init.
Stored per case: the signals stacked (x, lengths), D_init, the per-signal initial coefficients stacked (A0, [sum T_b, K],
before the zeroing), the stop parameters (NaN for None) and the reference's D, iterations (counted from its
per-iteration debug records), stop reason (its closing record) and last SNR.
A float32 case also stores the reference's float64 run on the same values upcast as D64: the difference is that case's
own float32 spread.  The mixed case is float32 data with a float64 'noise' dictionary (the reference's D is float64 while
its coefficients stay float32); D64 is then the all-float64 run.
A case stopped by a tolerance has the tolerance half way between two iterations' values (pick_tolerance, as
tools/make_golden_nmf_learn.py), and the distance of the nearest iteration to it (dB, or relative for the residual
scale) is stored as its stop margin.
"""
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from tools.make_golden_nmf_learn import STOP_CODES, _Records  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'nmf_corpus.npz')


def zero_straddling_rows(A0s, W):
    """The initial coefficients of the concatenation: every signal's rows T_b-W+1 .. T_b-1 at zero."""
    out = []
    for a in A0s:
        a = a.copy()
        a[a.shape[0] - W + 1:] = 0.0
        out.append(a)
    return np.concatenate(out)


def run_ref(mod, sigs, D_init, A0s, maxIt, tolRs, tolSnr, as64=False, seen=None):
    """The reference's _train_nmf on the concatenation.  as64: everything upcast to float64 first.  seen: a list that
    receives the reference's reconstructions (through its module-level reconstructSignal)."""
    K, W = D_init.shape[0], D_init.shape[1]
    x = np.concatenate(sigs)
    A = zero_straddling_rows(A0s, W)
    assert A.dtype == x.dtype and A.shape == (x.shape[0], K)
    if as64:
        x, D_init = x.astype(np.float64), D_init.astype(np.float64)
    h = _Records()
    log = logging.getLogger(mod.__name__)
    log.addHandler(h)
    old = log.level
    log.setLevel(logging.DEBUG)
    cdl = mod.ConvolutionalDictionaryLearner(k=K, windowSize=W, algorithm='nmf')
    cdl._init_D = lambda data, initMethod='random_samples': D_init.copy()
    orig_random, orig_recon = np.random.random, mod.reconstructSignal

    def prepared(size=None):
        assert tuple(size) == A.shape, (size, A.shape)
        return A.astype(np.float64) - 2.0

    def capture(coefficients, D):
        r = orig_recon(coefficients, D)
        seen.append(r)
        return r
    np.random.random = prepared
    if seen is not None:
        mod.reconstructSignal = capture
    try:
        D = cdl.train(x, initMethod='random_samples', nbMaxIterations=maxIt, toleranceResidualScale=tolRs, toleranceSnr=tolSnr)
    finally:
        np.random.random = orig_random
        mod.reconstructSignal = orig_recon
        log.removeHandler(h)
        log.setLevel(old)
    iters = sum(1 for m in h.messages if m.startswith('SNR of '))
    stop = [STOP_CODES[m] for m in h.messages if m in STOP_CODES]
    assert len(stop) == 1
    snr = float([m for m in h.messages if m.startswith('SNR of ')][-1].split()[2])
    return np.asarray(D), iters, stop[0], snr


def _rs_after(mod, sigs, D_init, A0s, n):
    """max |residual| of the reference after n iterations, from its last reconstruction."""
    seen = []
    run_ref(mod, sigs, D_init, A0s, n, None, None, seen=seen)
    seq = np.concatenate(sigs)
    seq = seq.reshape((seq.shape[0], -1)).astype(np.float64)
    return float(np.max(np.abs(seq - np.asarray(seen[-1], np.float64).reshape(seq.shape))))


def pick_tolerance(mod, sigs, D_init, A0s, kind, target, min_margin):
    """tools/make_golden_nmf_learn.py's pick_tolerance on the corpus: a tolerance that first stops the reference at an
    iteration >= `target`, half way between that iteration's value and the best one before it."""
    vals = []
    for i in range(1, 40):
        vals.append(run_ref(mod, sigs, D_init, A0s, i, None, None)[3] if kind == 'snr' else _rs_after(mod, sigs, D_init, A0s, i))
        if i < target:
            continue
        best = max(vals[:-1]) if kind == 'snr' else min(vals[:-1])
        tol = 0.5 * (best + vals[-1])
        margin = abs(vals[-1] - best) / 2 if kind == 'snr' else abs(vals[-1] - best) / 2 / tol
        if (vals[-1] > best if kind == 'snr' else vals[-1] < best) and margin >= min_margin:
            return tol, margin, i
    raise RuntimeError('no tolerance found: %s' % vals)


def make_corpus(seed, lengths, K, W, F, dtype, planted, init):
    """Uniform signals, or (planted) the same few positive atoms in every signal plus a little positive noise, on which
    the residual shrinks over the iterations.  D_init: 'random_samples' K windows of the signals longer than W, 'noise'
    uniform between the corpus' extremes (float64, as numpy draws it), both with unit-norm atoms.  A0: r + 2.0 per signal."""
    rs = np.random.RandomState(seed)
    atoms = rs.random_sample((K, W, F))
    atoms /= np.sqrt(np.sum(np.square(atoms), axis=(1, 2), keepdims=True))
    sigs = []
    for T in lengths:
        x = rs.random_sample((T, F))
        if planted:
            x = 0.01 * x
            for t in rs.randint(0, T - W + 1, size=max(2, T // W)):
                x[t:t + W] += (1.0 + rs.random_sample()) * atoms[rs.randint(K)]
        sigs.append((x[:, 0] if F == 1 else x).astype(dtype))
    if init == 'noise':
        stack = np.concatenate(sigs)
        D = rs.uniform(low=np.min(stack), high=np.max(stack), size=(K, W, F))
    else:
        longer = [b for b, T in enumerate(lengths) if T > W]
        D = []
        for _ in range(K):
            b = longer[rs.randint(len(longer))]
            t = rs.randint(0, lengths[b] - W)
            D.append(sigs[b][t:t + W].reshape((W, F)))
        D = np.stack(D)
    D = D / np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
    if F == 1:
        D = D[:, :, 0]
    A0s = [rs.random_sample((T, K)).astype(dtype) + 2.0 for T in lengths]
    return sigs, D, A0s


# name, seed, dtype, lengths, K, W, F, D_init kind, nbMaxIterations, stop kind (None: iteration count), target iteration
# (the seed of 'rs' is one under which the corpus' residual scale shrinks from iteration to iteration)
CASES = [
    ('ragged_f1', 3000, np.float64, [70, 37, 140, 64], 5, 5, 1, 'random_samples', 6, None, 0),
    ('ragged_f3', 3001, np.float64, [60, 130, 33, 45], 4, 6, 3, 'random_samples', 5, None, 0),
    ('length_w', 3002, np.float64, [90, 8, 60], 4, 8, 1, 'noise', 4, None, 0),                 # one signal of length W: L = 1
    ('snr', 3003, np.float64, [70, 40, 130], 6, 6, 1, 'random_samples', 50, 'snr', 2),
    ('rs', 3100, np.float64, [100, 70, 130], 6, 6, 1, 'random_samples', 50, 'rs', 3),
    ('ragged_f32', 3005, np.float32, [130, 90, 45], 5, 5, 3, 'random_samples', 8, None, 0),
    ('mixed_noise_f32', 3006, np.float32, [60, 150, 41], 5, 5, 1, 'noise', 10, None, 0),
]


def main():
    ns = ref_loader.load_reference()
    if ns is None:
        raise SystemExit('the reference is not available')
    mod = ns.modeling
    out = {'names': np.array([c[0] for c in CASES])}
    for name, seed, dt, lengths, K, W, F, init, maxIt, kind, target in CASES:
        sigs, D_init, A0s = make_corpus(seed, lengths, K, W, F, dt, kind is not None, init)
        if init != 'noise':
            D_init = D_init.astype(dt)                  # windows of the data: the data's dtype
        tolRs = tolSnr = None
        margin = np.nan
        if kind == 'snr':
            tolSnr, margin, target = pick_tolerance(mod, sigs, D_init, A0s, 'snr', target, 1e-3)
        elif kind == 'rs':
            tolRs, margin, target = pick_tolerance(mod, sigs, D_init, A0s, 'rs', target, 1e-4)
        D, iters, stop, snr = run_ref(mod, sigs, D_init, A0s, maxIt, tolRs, tolSnr)
        if kind is not None:
            assert iters == target and stop == (3 if kind == 'snr' else 2), (name, iters, stop)
        p = name + '/'
        out.update({p + 'x': np.concatenate(sigs), p + 'lengths': np.array(lengths, dtype=np.int64), p + 'D_init': D_init,
                    p + 'A0': np.concatenate(A0s), p + 'K': np.int64(K), p + 'W': np.int64(W), p + 'init': np.array(init),
                    p + 'max_iterations': np.int64(maxIt), p + 'tol_rs': np.float64(np.nan if tolRs is None else tolRs),
                    p + 'tol_snr': np.float64(np.nan if tolSnr is None else tolSnr), p + 'margin': np.float64(margin),
                    p + 'D': D, p + 'iterations': np.int64(iters), p + 'stop': np.int64(stop), p + 'snr': np.float64(snr)})
        spread = 0.0
        if dt == np.float32:
            D64, it64, st64, _ = run_ref(mod, sigs, D_init, A0s, maxIt, tolRs, tolSnr, as64=True)
            assert (it64, st64) == (iters, stop), (name, it64, iters)
            out[p + 'D64'] = D64
            spread = float(np.max(np.abs(D.astype(np.float64) - D64)))
        print('%-16s lengths=%s K=%d W=%d F=%d %-14s D %s: %3d iterations, stop %d, snr %.4f, margin %s, f32 spread %.2e' % (
            name, lengths, K, W, F, init, D.dtype, iters, stop, snr, margin, spread), flush=True)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
